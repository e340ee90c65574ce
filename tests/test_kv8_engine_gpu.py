"""GPU: SlotDecodeEngine(kv_cache="fp8") on tiny-gqa-test, every row kept, with no tolerance anywhere.

  1. after admit through each of the four paths (HIP prompt pass, module prompt pass, prefix + HIP suffix pass, prefix + module
     suffix pass) the slot's codes and scales are the rule (tests/kv8_rule.py) applied to the staging cache's rows, and every other
     byte of every slot keeps its sentinel;
  2. a request's tokens do not depend on its slot or its neighbours, and graph replay equals eager stepping;
  3. six steps of logits are the words of a second, 16-bit SlotDecodeEngine on the same weights whose caches are overwritten before
     each step with the fp8 engine's dequantised rows;
  4. the refusals (a staging batch other than 1, the keyword on the other engines) and generate.py --requests --kv_cache fp8.
"""
import json

import pytest
import torch

import kv8_cases as K
import kv8_rule as R
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.engine import DecodeEngine
from test_continuous_gpu import _all_rows, _model, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
B, MAX_SEQ = 3, 96
PREFIX = [7, 3, 400, 21, 9, 9, 130, 2, 77]
# path -> (prefix?, prompt length, the counter it moves): 2..16 tokens take the HIP passes, longer ones the module path
PATHS = {"hip prompt": (False, 5, ("admit_paths", "hip")), "module prompt": (False, 20, ("admit_paths", "module")),
         "prefix + hip suffix": (True, 4, ("prefix_paths", "hip")), "prefix + module suffix": (True, 20, ("prefix_paths", "module"))}


def _engine(dt, batch=B, max_seq=MAX_SEQ):
    m, ths = _model("tiny-gqa-test", dt, 1, max_seq)   # the model's caches: the staging cache, one sequence
    return m, SlotDecodeEngine(m, _all_rows(ths), batch, kv_cache="fp8")


def _sentinels(eng):
    for kc, vc, ks, vs in eng.kv8:
        kc.fill_(K.CODE_SENTINEL), vc.fill_(K.CODE_SENTINEL), ks.fill_(K.SCALE_SENTINEL), vs.fill_(K.SCALE_SENTINEL)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_admit_quantises_the_staging_rows(dt, path):
    with_prefix, T, (counter, key) = PATHS[path]
    m, eng = _engine(dt)
    if with_prefix:
        eng.register_prefix("p", PREFIX)
    P = len(PREFIX) if with_prefix else 0
    _sentinels(eng)
    g = torch.Generator().manual_seed(T)
    toks = torch.randint(0, m.config.vocab_size, (T,), generator=g).tolist()
    s = 1
    eng.admit(s, toks, 5, None, 17, prefix="p" if with_prefix else None)
    torch.cuda.synchronize()
    assert getattr(eng, counter)[key] == 1 and sum(eng.admit_paths.values()) + sum(eng.prefix_paths.values()) == 1
    assert eng.read_state()[SLOT_ACTIVE] == 1 << s and int(eng.pos_buf[s]) == P + T
    n = P + T
    for i, layer in enumerate(m.layers):
        kv = layer.attention.kv_cache
        for name, staging, codes, scales in (("k", kv.k_cache, eng.kv8[i][0], eng.kv8[i][2]), ("v", kv.v_cache, eng.kv8[i][1], eng.kv8[i][3])):
            assert staging.shape[0] == 1
            want_c, want_s = R.quantize(staging[0, :, :n].cpu())
            codes, scales = codes.cpu(), scales.cpu()
            assert torch.equal(codes[s, :, :n], want_c), (i, name, "codes")
            assert torch.equal(scales[s, :, :n].view(torch.int32), want_s.view(torch.int32)), (i, name, "scales")
            assert bool((codes[s, :, n:] == K.CODE_SENTINEL).all()) and bool((scales[s, :, n:] == K.SCALE_SENTINEL).all()), (i, name, "past the rows")
            for o in (0, 2):
                assert bool((codes[o] == K.CODE_SENTINEL).all()) and bool((scales[o] == K.SCALE_SENTINEL).all()), (i, name, o)
    nb = eng.kv_cache_bytes()
    cfg = m.config
    rows = 2 * len(m.layers) * cfg.n_local_heads * MAX_SEQ
    assert nb == {"staging": rows * cfg.head_dim * 2, "codes": B * rows * cfg.head_dim, "scales": B * rows * 4}


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_tokens_do_not_depend_on_slot_neighbours_or_replay(dt):
    reqs = _requests(8, 3, hi_t=30, hi_b=20)
    max_seq = max(len(r.tokens) + r.max_new_tokens for r in reqs)
    m, eng = _engine(dt, 4, max_seq)
    kw = dict(temperature=0.8, top_k=50)
    a = ContinuousBatcher(eng, sync_every=8, **kw).run(reqs)["tokens"]
    seeded = [Request(r.tokens, r.max_new_tokens, seed=1234 + i) for i, r in enumerate(reqs)]  # request i keeps stream 1234 + i
    b = ContinuousBatcher(eng, sync_every=1, **kw).run(seeded[::-1])["tokens"][::-1]           # other slots, other neighbours
    c = ContinuousBatcher(eng, sync_every=8, use_graph=False, **kw).run(reqs)["tokens"]        # eager stepping
    assert [len(t) for t in a] == [r.max_new_tokens for r in reqs]
    assert a == b and a == c
    assert ("kv fp8",) == eng._feature_key()[-1:]                                            # the graph key holds the format


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_logits_are_the_16bit_engines_on_the_dequantised_rows(dt):
    m8, e8 = _engine(dt)
    m16, ths = _model("tiny-gqa-test", dt, B, MAX_SEQ)
    e16 = SlotDecodeEngine(m16, _all_rows(ths), B)
    assert e16.kv8 is None and e16.kv_cache_bytes()["codes"] == 0 and e16.kv_cache_bytes()["scales"] == 0
    for p8, p16 in zip(m8.parameters(), m16.parameters()):
        assert torch.equal(p8, p16)
    g = torch.Generator().manual_seed(5)
    admits = {0: torch.randint(0, m8.config.vocab_size, (7,), generator=g).tolist(), 2: torch.randint(0, m8.config.vocab_size, (23,), generator=g).tolist()}
    for s, toks in admits.items():   # slot 1 stays free
        for eng in (e8, e16):
            eng.admit(s, toks, 50, None, 100 + s, temperature=0.8, top_k=50)
    assert torch.equal(e8.tok_buf, e16.tok_buf) and torch.equal(e8.pos_buf, e16.pos_buf)   # the prompt passes are both 16-bit
    for step in range(6):
        pos = e8.pos_buf.tolist()
        for i, layer in enumerate(m16.layers):
            kv = layer.attention.kv_cache
            for cache, codes, scales in ((kv.k_cache, e8.kv8[i][0], e8.kv8[i][2]), (kv.v_cache, e8.kv8[i][1], e8.kv8[i][3])):
                for s in admits:
                    dq = R.dequantize(codes[s, :, :pos[s]], scales[s, :, :pos[s]])
                    assert R.representable(dq, dt), (step, i, s)                               # the rows ARE 16-bit values
                    cache[s, :, :pos[s]] = dq.to(dt).to(DEV)
        for eng in (e8, e16):
            eng._self_step(0.8, 50)
        torch.cuda.synchronize()
        for s in admits:
            assert torch.equal(e8.logits[s].view(torch.int16), e16.logits[s].view(torch.int16)), (step, s)
        assert torch.equal(e8.tok_buf, e16.tok_buf) and torch.equal(e8.pos_buf, e16.pos_buf)
    assert e8.pos_buf.tolist()[0] == 7 + 6 and e8.read_state()[SLOT_ACTIVE] == 0b101


def test_refusals():
    m, ths = _model("tiny-gqa-test", torch.float16, B, MAX_SEQ)   # caches at batch B: no staging cache
    assert "staging cache" in SlotDecodeEngine.supports(m, kv_cache="fp8") and SlotDecodeEngine.supports(m) is None
    with pytest.raises(ValueError, match=r"staging cache.*max_batch_size=1"):
        SlotDecodeEngine(m, ths, B, kv_cache="fp8")
    assert "no admission" in BatchedDecodeEngine.supports(m, kv_cache="fp8")
    with pytest.raises(ValueError, match="no admission"):
        BatchedDecodeEngine(m, ths, B, kv_cache="fp8")
    with pytest.raises(ValueError, match="unknown kv_cache"):
        SlotDecodeEngine(m, ths, B, kv_cache="fp4")
    m1, ths1 = _model("tiny-gqa-test", torch.float16, 1, MAX_SEQ)
    assert SlotDecodeEngine.supports(m1, kv_cache="fp8") is None
    with pytest.raises(ValueError, match="no admission"):
        DecodeEngine(m1, ths1, kv_cache="fp8")
    with pytest.raises(ValueError, match="1..8"):
        SlotDecodeEngine(m1, ths1, 9, kv_cache="fp8")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_generate_requests_with_an_fp8_cache_end_to_end(precision, tmp_path):
    g = torch.Generator().manual_seed(6)
    reqs = [{"tokens": torch.randint(0, 512, (int(t),), generator=g).tolist(), "max_new_tokens": int(n)}
            for t, n in zip(torch.randint(1, 30, (7,), generator=g), torch.randint(2, 30, (7,), generator=g))]
    f = tmp_path / "reqs.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in reqs) + "\n")
    argv = ["--device", "cuda", "--synthetic", "tiny-gqa-test", "--requests", str(f), "--batch_size", "4", "--compile", "--max_new_tokens", "9",
            "--sparsity", "0.5", "--precision", precision]
    res = G.main(G.build_parser().parse_args(argv + ["--kv_cache", "fp8"]))
    assert res["decoder"] == "ContinuousBatcher" and [len(s) for s in res["sequences"]] == [r["max_new_tokens"] for r in reqs]
    nb = res["kv_cache_bytes"]
    assert nb["codes"] > 0 and nb["scales"] * 64 == nb["codes"] * 4 and nb["codes"] == 4 * nb["staging"] // 2   # hd 64; 4 slots, 1 staged
    assert res["mean_tokens_per_sec"] > 0

"""GPU: shared prompt prefixes of continuous batching (teal_kv_copy_rows, SlotVerifyPass, SlotDecodeEngine.register_prefix /
admit(prefix=), ContinuousBatcher(prefixes=), generate.py --prefixes).

  1. teal_kv_copy_rows alone: the destination rows bit-identical to the source's, every other byte keeps its sentinel, rows == 0
     changes nothing, the argument refusals;
  2. register_prefix: the store = the rows admit of the same tokens leaves in a slot, nothing else moves, refused while a slot runs;
  3. admit(prefix=): rows 0..P-1 = the store, rows P..P+T-1 and the first token = a batch-1 run of the same path, other slots untouched;
  4. the last-row logits and the suffix's K / V rows against the unshared module path (the verify pass's bounds);
  5. a request's tokens do not depend on its slot, its neighbours, sync_every or refill (every row kept), with and without prefixes;
  6. graph replay = eager stepping for a whole run with prefixes;
  7. generate.py --requests --prefixes end to end.
"""
import json

import pytest
import torch

from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from test_continuous_gpu import _all_rows, _model, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5A


def _table(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(DEV)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd", [64, 128])
def test_kv_copy_rows(hd, dt):
    L = _lib.load()
    runtime.init()
    g = torch.Generator(device=DEV).manual_seed(hd)
    rb = hd * 2
    for n_t in (4, 64):
        for n_heads in (2, 8):
            for rows in (1, 15, 16, 17, 100):
                sr, dr, gap = rows + 3, rows + 7, 64  # head strides that differ, padding rows after every head, a gap between tensors
                src = torch.randint(-32768, 32767, (n_t, n_heads * sr * hd + gap), device=DEV, generator=g, dtype=torch.int16).view(dt)
                dst = torch.full((n_t, n_heads * dr * hd + gap), SENTINEL, device=DEV, dtype=torch.int16).view(dt)
                sv = [src[t, :n_heads * sr * hd].view(n_heads, sr, hd) for t in range(n_t)]
                dv = [dst[t, :n_heads * dr * hd].view(n_heads, dr, hd) for t in range(n_t)]
                st, dtab = _table(sv), _table(dv)
                want = dst.clone()
                for t in range(n_t):
                    want[t, :n_heads * dr * hd].view(n_heads, dr, hd)[:, :rows] = sv[t][:, :rows]
                before = dst.clone()
                assert L.teal_kv_copy_rows(st.data_ptr(), dtab.data_ptr(), n_t, n_heads, 0, rb, sr * rb, dr * rb, runtime.stream_ptr()) == 0
                torch.cuda.synchronize()
                assert torch.equal(dst.view(torch.int16), before.view(torch.int16))  # rows == 0: nothing
                assert L.teal_kv_copy_rows(st.data_ptr(), dtab.data_ptr(), n_t, n_heads, rows, rb, sr * rb, dr * rb, runtime.stream_ptr()) == 0
                torch.cuda.synchronize()
                # the rows, bit for bit; rows >= `rows` of every head, the padding, the gaps and the neighbouring tensors: the sentinel
                assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), (n_t, n_heads, rows)
                for t in range(n_t):
                    assert torch.equal(dv[t][:, :rows].view(torch.int16), sv[t][:, :rows].view(torch.int16))
                    assert bool((dv[t][:, rows:].view(torch.int16) == SENTINEL).all())
    s, d, st_ = st.data_ptr(), dtab.data_ptr(), runtime.stream_ptr()
    for args, code in [((None, d, 4, 2, 1, rb, rb, rb), -1), ((s, None, 4, 2, 1, rb, rb, rb), -1), ((s, d, 0, 2, 1, rb, rb, rb), -1),
                       ((s, d, 4, 0, 1, rb, rb, rb), -1), ((s, d, 4, 2, -1, rb, rb, rb), -1), ((s, d, 4, 2, 1, 0, rb, rb), -1),
                       ((s, d, 4, 2, 1, 24, 48, 48), -4), ((s, d, 4, 2, 3, rb, 2 * rb, 3 * rb), -3), ((s, d, 4, 2, 3, rb, 3 * rb, 2 * rb), -3)]:
        assert L.teal_kv_copy_rows(*args, st_) == code, (args, code)
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))  # a refused call writes nothing


def _noise(m, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for l in m.layers:
        l.attention.kv_cache.k_cache.copy_(torch.randn(l.attention.kv_cache.k_cache.shape, device=DEV, generator=g))
        l.attention.kv_cache.v_cache.copy_(torch.randn(l.attention.kv_cache.v_cache.shape, device=DEV, generator=g))
    return g


def _snap(m):
    return [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]


def _state(eng):
    return [t.clone() for t in (eng.slot_state, eng.tok_buf, eng.pos_buf, eng.history, eng.rng_state)]


@pytest.mark.parametrize("P", [1, 2, 9, 16, 17, 40])
def test_register_prefix(P):
    B, max_seq = 4, 96
    m, ths = _model("tiny-gqa-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    g = _noise(m, P)
    toks = torch.randint(0, m.config.vocab_size, (P,), device=DEV, generator=g, dtype=torch.int32).tolist()
    before, state = _snap(m), _state(eng)
    assert eng.prefix_bytes() == 0 and not eng.has_prefix("p")
    assert eng.register_prefix("p", toks) == P
    torch.cuda.synchronize()
    store = eng.prefix_store("p")
    nkv, hd = m.config.n_local_heads, m.config.head_dim
    assert tuple(store.shape) == (2 * len(m.layers), nkv, P, hd) and eng.prefix_bytes() == store.numel() * 2
    assert eng.has_prefix("p") and eng.prefix_rows("p") == P
    assert eng.admit_paths == {"hip": 0, "module": 0} and eng.prefix_paths == {"hip": 0, "module": 0}
    assert all(torch.equal(a, b) for a, b in zip(state, _state(eng)))  # no slot state, token, position, history or rng state moved
    for l, (kb, vb) in zip(m.layers, before):
        for o in range(1, B):  # (slot 0 is where the pass ran)
            assert torch.equal(l.attention.kv_cache.k_cache[o], kb[o]) and torch.equal(l.attention.kv_cache.v_cache[o], vb[o]), o
        assert torch.equal(l.attention.kv_cache.k_cache[0, :, P:], kb[0, :, P:]) and torch.equal(l.attention.kv_cache.v_cache[0, :, P:], vb[0, :, P:])
    with pytest.raises(ValueError, match="registered already"):
        eng.register_prefix("p", toks)
    # the rows admit of the same tokens leaves in a slot (the path the engine had before prefixes)
    eng.admit(1, toks, 4, None, 1)
    torch.cuda.synchronize()
    assert eng.admit_paths == ({"hip": 1, "module": 0} if 2 <= P <= 16 else {"hip": 0, "module": 1})
    for i, l in enumerate(m.layers):
        assert torch.equal(store[2 * i], l.attention.kv_cache.k_cache[1, :, :P])
        assert torch.equal(store[2 * i + 1], l.attention.kv_cache.v_cache[1, :, :P])
    assert eng.read_state()[SLOT_ACTIVE] == 0b10
    with pytest.raises(RuntimeError, match="idle"):
        eng.register_prefix("q", toks)
    assert not eng.has_prefix("q")
    eng.drop_prefix("p")
    assert eng.prefix_bytes() == 0 and not eng.has_prefix("p")
    with pytest.raises(ValueError, match="unknown prefix"):
        eng.drop_prefix("p")


def _sample_ref(L, logits, V, code, top_k, temperature, seed, dim):
    """the sampler's draw 0 of stream `seed` on `logits` [V]"""
    rng = torch.tensor([seed, 0], dtype=torch.int64).to(DEV)
    tok, pos = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = runtime.new_workspace(dim, V)
    logits = logits.contiguous()
    _lib.check(L.teal_sample_topk_ws(logits.data_ptr(), V, code, top_k, temperature, rng.data_ptr(), tok.data_ptr(), pos.data_ptr(), None, 0,
                                     ws.data_ptr(), ws.numel() * 4, runtime.stream_ptr()), "sampler")
    torch.cuda.synchronize()
    import numpy as np
    import sampler_rule
    bits = logits.view(torch.int16).cpu().numpy().view(np.uint16)
    token, runner_up, is_open = sampler_rule.draw(bits, logits.dtype == torch.bfloat16, top_k, temperature, seed, 0)
    assert int(tok.item()) == token or (is_open and int(tok.item()) == runner_up)  # the host model of the draw (tests/sampler_rule.py)
    return int(tok.item())


@pytest.mark.parametrize("T", [1, 2, 9, 16, 17, 40])
@pytest.mark.parametrize("P", [9, 40])
def test_prefix_admit_touches_only_its_slot(P, T):
    from teal_amd.gpt_fast.speculative import VerifyPass
    B, max_seq, s, dt = 4, 96, 2, torch.float16
    m, ths = _model("tiny-gqa-test", dt, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    g = _noise(m, 100 * P + T)
    V = m.config.vocab_size
    ptoks = torch.randint(0, V, (P,), device=DEV, generator=g, dtype=torch.int32)
    suffix = torch.randint(0, V, (T,), device=DEV, generator=g, dtype=torch.int32)
    eng.register_prefix("p", ptoks.tolist())
    torch.cuda.synchronize()
    store = eng.prefix_store("p").clone()
    before = _snap(m)
    eng.admit(s, suffix.tolist(), 4, None, 7, 0.8, 50, prefix="p")
    torch.cuda.synchronize()
    assert eng.prefix_paths == ({"hip": 1, "module": 0} if T <= 16 else {"hip": 0, "module": 1})
    assert eng.admit_paths == {"hip": 0, "module": 0}
    assert int(eng.pos_buf[s]) == P + T and eng.read_state()[SLOT_ACTIVE] == 1 << s
    # the same suffix through a batch-1 model on the same path, its rows 0..P-1 set to the store's
    m1, _ = _model("tiny-gqa-test", dt, 1, max_seq)
    G.relayout_for_engine(m1)
    for i, l in enumerate(m1.layers):
        l.attention.kv_cache.k_cache[0, :, :P] = store[2 * i]
        l.attention.kv_cache.v_cache[0, :, :P] = store[2 * i + 1]
    with torch.no_grad():
        if T <= 16:
            ref = VerifyPass(m1).all_logits(suffix, P)[-1]
        else:
            m1.fused_decode = False
            ref = m1(suffix.view(1, -1), torch.arange(P, P + T, device=DEV))[0, -1]
    torch.cuda.synchronize()
    for i, (l, l1, (kb, vb)) in enumerate(zip(m.layers, m1.layers, before)):
        kc, vc = l.attention.kv_cache.k_cache, l.attention.kv_cache.v_cache
        for o in range(B):
            if o != s:
                assert torch.equal(kc[o], kb[o]) and torch.equal(vc[o], vb[o]), o
        assert torch.equal(kc[s, :, :P], store[2 * i]) and torch.equal(vc[s, :, :P], store[2 * i + 1])
        assert torch.equal(kc[s, :, P:P + T], l1.attention.kv_cache.k_cache[0, :, P:P + T])
        assert torch.equal(vc[s, :, P:P + T], l1.attention.kv_cache.v_cache[0, :, P:P + T])
        assert torch.equal(kc[s, :, P + T:], kb[s, :, P + T:]) and torch.equal(vc[s, :, P + T:], vb[s, :, P + T:])
    assert torch.equal(eng.admit_logits.view(-1), ref.view(-1))
    want = _sample_ref(eng.L, ref.view(-1), V, eng.code, 50, 0.8, 7, m.config.dim)
    assert int(eng.history[s, 0]) == want and int(eng.tok_buf[s]) == want


def test_prefix_admit_refusals():
    B, max_seq = 2, 32
    m, ths = _model("tiny-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    eng.register_prefix("p", list(range(1, 21)))
    before, state = _snap(m), _state(eng)
    with pytest.raises(ValueError, match="unknown prefix"):
        eng.admit(0, [1, 2], 4, None, 1, prefix="nope")
    with pytest.raises(ValueError, match="does not fit"):
        eng.admit(0, [], 4, None, 1, prefix="p")            # an empty suffix
    with pytest.raises(ValueError, match="does not fit"):
        eng.admit(0, [1] * 12, 4, None, 1, prefix="p")      # P + T = max_seq
    with pytest.raises(ValueError, match="does not fit"):
        eng.admit(0, [1, 2], 0, None, 1, prefix="p")        # no budget
    with pytest.raises(ValueError, match="no room"):
        eng.register_prefix("long", [1] * 31)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, _state(eng))) and eng.prefix_paths == {"hip": 0, "module": 0}
    for l, (kb, vb) in zip(m.layers, before):
        assert torch.equal(l.attention.kv_cache.k_cache, kb) and torch.equal(l.attention.kv_cache.v_cache, vb)
    eng.admit(0, [1] * 11, 4, None, 1, prefix="p")          # P + T = max_seq - 1: the last row is left for the first step
    assert int(eng.pos_buf[0]) == 31


@pytest.mark.parametrize("name,dt,n_layer", [("7B", torch.float16, 2), ("llama-3-8b", torch.bfloat16, 2), ("tiny-gqa-test", torch.float16, None)])
def test_prefix_admission_is_close_to_the_unshared_module_path(name, dt, n_layer):
    """Bounds and situation of tests/test_speculative_gpu.py::test_verify_pass_equals_module_path: the context rows come from the
    module path (a prefix of more than 16 tokens), the T suffix rows from the verify pass; the reference is the module path at
    batch 1: one pass over the P prefix tokens, one over the T suffix tokens at arange(P, P + T).  6 output ulps of the logits'
    scale on the last row; the K / V rows P..P+T-1 to atol = rtol = 2e-2 (fp16) / 1e-1 (bf16)."""
    B, max_seq, s = 2, 96, 1
    torch.manual_seed(0)
    m, ths = _model(name, dt, B, max_seq, n_layer=n_layer)
    eng = SlotDecodeEngine(m, ths, B)
    ref = G.build_synthetic_model(name, DEV, dt, n_layer=n_layer)  # the same seeded weights, unpatched: the dense module path
    ref.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    V = m.config.vocab_size
    g = torch.Generator(device=DEV).manual_seed(3)
    toks = torch.randint(0, V, (48,), device=DEV, generator=g, dtype=torch.int32)
    for P in (23, 30):
        eng.register_prefix(f"p{P}", toks[:P].tolist())
    kt = 2e-2 if dt == torch.float16 else 1e-1
    with torch.no_grad():
        for P in (23, 30):
            for T in (2, 5, 16):
                x = toks[P:P + T]
                ref(toks[:P].view(1, -1).long(), torch.arange(0, P, device=DEV))
                want = ref(x.view(1, -1).long(), torch.arange(P, P + T, device=DEV))[0, -1].float()
                eng.admit(s, x.tolist(), 1, None, 5, prefix=f"p{P}")  # (budget 1: the slot is free again for the next case)
                got = eng.admit_logits.view(-1).float()
                torch.cuda.synchronize()
                ulp = float(want.abs().max()) * (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7)
                err = float((got - want).abs().max())
                print(f"{name} P={P} T={T}: last-row logits max |err| {err:.3e}, bound {6 * ulp:.3e}")
                assert err <= 6 * ulp, (name, P, T, err, ulp)
                for l, lr in zip(m.layers, ref.layers):
                    for c, cr in ((l.attention.kv_cache.k_cache, lr.attention.kv_cache.k_cache), (l.attention.kv_cache.v_cache, lr.attention.kv_cache.v_cache)):
                        assert torch.allclose(c[s, :, P:P + T].float(), cr[0, :, P:P + T].float(), atol=kt, rtol=kt), (name, P, T)
    assert eng.prefix_paths == {"hip": 6, "module": 0} and eng.read_state()[SLOT_ACTIVE] == 0


def _prefixed_requests(n, seed, pf, vocab=512):
    """_requests with every third request on prefix A, every third on prefix B (their tokens are then the suffix)"""
    reqs = _requests(n, seed, hi_t=24, vocab=vocab)
    names = [None] + list(pf)
    return [Request(r.tokens, r.max_new_tokens, prefix=names[i % len(names)]) for i, r in enumerate(reqs)]


def _pf(vocab=512):
    g = torch.Generator().manual_seed(11)
    return {"A": torch.randint(0, vocab, (9,), generator=g).tolist(), "B": torch.randint(0, vocab, (23,), generator=g).tolist()}


def test_tokens_independent_of_batch_composition_with_prefixes():
    B, pf = 4, _pf()
    reqs = _prefixed_requests(12, 1, pf)
    assert {r.prefix for r in reqs} == {None, "A", "B"}
    max_seq = max(len(pf.get(r.prefix, [])) + len(r.tokens) + r.max_new_tokens for r in reqs)
    m, ths = _model("tiny-gqa-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, _all_rows(ths), B)
    kw = dict(temperature=0.8, top_k=50, prefixes=pf)
    ra = ContinuousBatcher(eng, sync_every=8, **kw).run(reqs)
    a = ra["tokens"]
    seeded = [Request(r.tokens, r.max_new_tokens, seed=1234 + i, prefix=r.prefix) for i, r in enumerate(reqs)]
    b = ContinuousBatcher(eng, sync_every=1, **kw).run(seeded[::-1])["tokens"][::-1]
    c = ContinuousBatcher(eng, sync_every=8, refill="all", **kw).run(reqs)["tokens"]
    assert [len(t) for t in a] == [r.max_new_tokens for r in reqs]
    assert a == b and a == c
    assert ra["prefix_admissions"] == 8 and ra["prefix_rows_reused"] == 4 * 9 + 4 * 23
    assert sum(ra["prefix_paths"].values()) == 8 and ra["prefix_paths"]["module"] == sum(r.prefix is not None and len(r.tokens) > 16 for r in reqs)


def test_graph_replay_equals_eager_with_prefixes():
    B, pf = 4, _pf()
    reqs = _prefixed_requests(10, 2, pf)
    max_seq = max(len(pf.get(r.prefix, [])) + len(r.tokens) + r.max_new_tokens for r in reqs)
    m, ths = _model("tiny-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    a = ContinuousBatcher(eng, sync_every=4, use_graph=False, prefixes=pf).run(reqs)
    b = ContinuousBatcher(eng, sync_every=4, use_graph=True, prefixes=pf).run(reqs)
    assert a["tokens"] == b["tokens"] and a["steps"] == b["steps"]
    assert [len(t) for t in a["tokens"]] == [r.max_new_tokens for r in reqs]
    assert a["prefix_admissions"] == b["prefix_admissions"] == sum(r.prefix is not None for r in reqs)


@pytest.mark.parametrize("name", ["tiny-test", "tiny-gqa-test"])
def test_generate_requests_with_prefixes_end_to_end(name, tmp_path):
    g = torch.Generator().manual_seed(4)
    pf = _pf()
    reqs = [{"tokens": torch.randint(0, 512, (int(t),), generator=g).tolist(), "max_new_tokens": int(n)}
            for t, n in zip(torch.randint(1, 30, (9,), generator=g), torch.randint(2, 40, (9,), generator=g))]
    for i, r in enumerate(reqs):
        if i % 3:
            r["prefix"] = "AB"[i % 3 - 1]
    reqs[3].pop("max_new_tokens")  # the flag's default
    budgets = [r.get("max_new_tokens", 9) for r in reqs]
    f, p = tmp_path / "reqs.jsonl", tmp_path / "prefixes.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in reqs) + "\n")
    p.write_text("\n".join(json.dumps({"id": k, "tokens": v}) for k, v in pf.items()) + "\n")
    args = G.build_parser().parse_args(["--device", "cuda", "--synthetic", name, "--requests", str(f), "--prefixes", str(p), "--batch_size", "4",
                                        "--compile", "--max_new_tokens", "9", "--sparsity", "0.5"])
    res = G.main(args)
    assert res["decoder"] == "ContinuousBatcher" and [len(s) for s in res["sequences"]] == budgets
    assert res["prefix_admissions"] == sum("prefix" in r for r in reqs) == 6
    assert res["prefix_rows_reused"] == 3 * 9 + 3 * 23 and sum(res["prefix_paths"].values()) == 6
    assert res["mean_tokens_per_sec"] > 0

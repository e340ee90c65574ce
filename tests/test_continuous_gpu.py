"""GPU: continuous batching (the slot entry points of teal_batched.hip / teal_sampler.hip, SlotDecodeEngine, ContinuousBatcher).

  1. teal_batched_sparse_gemm_slots with inactive slots = teal_batched_sparse_gemm of the compacted batch, bit for bit, with the
     same kept counts; inactive slab columns exactly 0; NaN / Inf in the inactive hand-over changes no bit;
  2. teal_batched_decode_attention_slots: active slots bit-identical to the unmasked launch, inactive caches untouched, yt 0;
  3. over 50 replays an inactive slot's state does not move; retirement on the budget, on EOS and at the cache end;
  4. admit() writes only its own slot's caches, bit-identical to a batch-1 prompt pass on the same path (HIP and module);
  5. a request's tokens do not depend on its slot, its neighbours, sync_every or refill (every row kept);
  6. teacher-forced logits of a mixed active set against per-sequence DecodeEngines;
  7. graph replay = eager stepping for a whole run;
  8. generate.py --requests end to end, and --eos_id.
"""
import ctypes
import json

import pytest
import torch

from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import (SLOT_ACTIVE, SLOT_BUDGET, SLOT_EOS, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP, SlotDecodeEngine)
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.prefill import IN_SILU_MUL, IN_XT, PrefillEngine, PrefillIn
from teal_amd.kernels.sparse_gemv import batched_segs

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float16: 0, torch.bfloat16: 1}
NINF = float("-inf")


def _wT(Z, N, dt, g, pad=64):
    buf = torch.zeros(Z, N + pad, device=DEV, dtype=dt)
    buf[:, :N] = (torch.randn(Z, N, device=DEV, generator=g) * 0.02).to(dt)
    return buf


def _launch(L, gin, sg, w0, n0, w1, n1, Z, B, dt, active=None):
    slabs = torch.full((16 * (n0 + n1) * 8,), float("nan"), device=DEV)
    cnt = torch.zeros(16 * 27, device=DEV, dtype=torch.int32)
    split = ctypes.c_int(0)
    args = (ctypes.byref(gin), ctypes.byref(sg), w0.data_ptr(), w0.stride(0), n0, w1.data_ptr() if w1 is not None else None,
            w1.stride(0) if w1 is not None else 0, n1, slabs.data_ptr(), slabs.numel() * 4, Z, B)
    if active is None:
        rc = L.teal_batched_sparse_gemm(*args, cnt.data_ptr(), CODE[dt], ctypes.byref(split), runtime.stream_ptr())
    else:
        rc = L.teal_batched_sparse_gemm_slots(*args, active.data_ptr(), cnt.data_ptr(), CODE[dt], ctypes.byref(split), runtime.stream_ptr())
    _lib.check(rc, "gemm")
    torch.cuda.synchronize()
    return slabs.view(16, n0 + n1, 8)[:split.value].clone(), cnt.view(16, 3, 9)[:split.value].sum(0).cpu()


SHAPES = {"qkv": (4096, 4096 + 2 * 1024, 0), "gateup": (4096, 11008, 11008), "down": (11008, 4096, 0), "lm_head": (4096, 32000, 0)}


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gemm_slots_equals_compacted_batch(shape, dt):
    L = _lib.load()
    runtime.init()
    Z, n0, n1 = SHAPES[shape]
    N = n0 + n1
    g = torch.Generator(device=DEV).manual_seed(N + Z)
    W0, W1 = _wT(Z, n0, dt, g), (_wT(Z, n1, dt, g) if n1 else None)
    bounds, taus = {"qkv": ([4096, 5120, N], [0.5, 0.8, 0.3]), "gateup": ([n0, N], [0.6, 0.4]), "down": ([N], [0.05]),
                    "lm_head": ([N], [NINF])}[shape]
    sg = batched_segs(bounds, taus)
    B, on = 6, [0, 2, 3, 5]  # slots 1 and 4 inactive
    active = torch.tensor([sum(1 << s for s in on)], dtype=torch.int32, device=DEV)
    if shape == "down":
        gu = (torch.randn(2, 2 * Z, 8, device=DEV, generator=g) * 0.5).float()
        gc = torch.zeros_like(gu)
        gc[..., :len(on)] = gu[..., on]
        poisoned = gu.clone()
        poisoned[..., 1], poisoned[..., 4] = float("nan"), float("inf")
        mk = lambda t: PrefillIn(mode=IN_SILU_MUL, gu_slabs=t.data_ptr(), gu_split=2)  # noqa: E731
        ins = (gu, gc, poisoned)
    else:
        xt = torch.zeros(Z, 8, device=DEV, dtype=dt)
        xt[:, :B] = torch.randn(Z, B, device=DEV, generator=g).to(dt)
        xc = torch.zeros_like(xt)
        xc[:, :len(on)] = xt[:, on]
        poisoned = xt.clone()
        poisoned[:, 1], poisoned[::2, 4], poisoned[1::2, 4] = float("nan"), float("inf"), -float("inf")
        mk = lambda t: PrefillIn(mode=IN_XT, xt=t.data_ptr())  # noqa: E731
        ins = (xt, xc, poisoned)
    full, cf = _launch(L, mk(ins[0]), sg, W0, n0, W1, n1, Z, B, dt, active)
    comp, cc = _launch(L, mk(ins[1]), sg, W0, n0, W1, n1, Z, len(on), dt)
    pois, cp = _launch(L, mk(ins[2]), sg, W0, n0, W1, n1, Z, B, dt, active)
    assert torch.equal(full[..., on].view(torch.int32), comp[..., :len(on)].view(torch.int32))
    assert bool((full[..., [1, 4]] == 0).all())
    assert torch.equal(full.view(torch.int32), pois.view(torch.int32))
    for s in range(len(bounds)):
        assert [int(cf[s, b]) for b in on] == [int(cc[s, i]) for i in range(len(on))] and int(cf[s, 8]) == int(cc[s, 8])
        assert int(cf[s, 1]) == int(cf[s, 4]) == 0 and torch.equal(cf, cp)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_attention_slots(dt):
    from teal_amd.gpt_fast.model import precompute_freqs_cis
    L = _lib.load()
    runtime.init()
    n_head, n_kv, hd, B, max_seq = 32, 8, 128, 5, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    ntot = (n_head + 2 * n_kv) * hd
    slabs = (torch.randn(2, ntot, 8, device=DEV, generator=g) * 0.5).float()
    rope = precompute_freqs_cis(max_seq, hd, 10000, dt).to(DEV).contiguous()
    pos = torch.tensor([10, 70, 0, 255, 33], dtype=torch.int32, device=DEV)
    kc0 = (torch.randn(B, n_kv, max_seq, hd, device=DEV, generator=g)).to(dt)
    vc0 = (torch.randn(B, n_kv, max_seq, hd, device=DEV, generator=g)).to(dt)
    nb = int(L.teal_batched_decode_attention_ws_bytes(B, n_head, hd))
    outs = []
    for active in (None, torch.tensor([0b10101], dtype=torch.int32, device=DEV)):
        kc, vc = kc0.clone(), vc0.clone()
        yt = torch.full((n_head * hd, 8), 7.0, device=DEV, dtype=dt)
        part = torch.zeros((nb + 3) // 4, device=DEV)
        a = (slabs.data_ptr(), 2, rope.data_ptr(), pos.data_ptr())
        b = (kc.data_ptr(), vc.data_ptr(), yt.data_ptr(), part.data_ptr(), nb, B, n_head, n_kv, hd, max_seq, CODE[dt], runtime.stream_ptr())
        rc = L.teal_batched_decode_attention(*a, *b) if active is None else L.teal_batched_decode_attention_slots(*a, active.data_ptr(), *b)
        _lib.check(rc, "attention")
        torch.cuda.synchronize()
        outs.append((kc, vc, yt))
    (k1, v1, y1), (k2, v2, y2) = outs
    for s in (0, 2, 4):
        assert torch.equal(k1[s], k2[s]) and torch.equal(v1[s], v2[s]) and torch.equal(y1[:, s], y2[:, s])
    for s in (1, 3):
        assert torch.equal(k2[s], kc0[s]) and torch.equal(v2[s], vc0[s]) and bool((y2[:, s] == 0).all())


def _model(name, dt, B, max_seq, sparsity=0.5, n_layer=None):
    m = G.build_synthetic_model(name, DEV, dt, n_layer=n_layer)
    ths = G.apply_sparsity(m, sparsity=sparsity, hist_path=None, greedy_lookup=None, synthetic=True, decode_calibration=False)
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    return m, ths


def _all_rows(ths):
    return [{k: NINF for k in t} for t in ths]


def test_inactive_slots_do_not_move_and_retirement():
    B, max_seq = 4, 64
    m, ths = _model("tiny-gqa-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, _all_rows(ths), B)  # (every row kept: slot 2 below repeats slot 1's request alone, token for token)
    eng.admit(0, [5, 6, 7], 200, None, 11)       # runs into the cache end: stops exactly on its last row
    eng.admit(1, [9, 8], 5, None, 12)            # budget
    g0 = eng.capture(0.8, 50)
    snap = lambda s: (eng.tok_buf[s].item(), eng.pos_buf[s].item(), eng.rng_state[s].tolist(), eng.history[s].tolist())  # noqa: E731
    idle = [snap(s) for s in (2, 3)]
    for _ in range(50):
        g0.replay()
    st = eng.read_state()
    assert [snap(s) for s in (2, 3)] == idle
    assert st[SLOT_ACTIVE] & 0b1111 == 1 and st[SLOT_STEP] == 50
    assert st[SLOT_PRODUCED + 1] == 5 and st[SLOT_FINISH + 1] == 3  # first token at admission, four steps
    for _ in range(20):
        g0.replay()
    st = eng.read_state()
    assert st[SLOT_ACTIVE] & 0b1111 == 0 and st[SLOT_STEP] == 70 and [snap(s) for s in (2, 3)] == idle
    # slot 0: prompt rows 0..2, then steps write rows 3..max_seq-1: max_seq - 3 steps, max_seq - 2 tokens
    assert st[SLOT_PRODUCED + 0] == max_seq - 2 and st[SLOT_FINISH + 0] == max_seq - 3 - 1
    assert int(eng.pos_buf[0]) == max_seq - 1
    # EOS: the slot stops right after the first occurrence of its EOS id
    toks = eng.read_history(1, 5)
    eng.admit(2, [9, 8], 5, toks[2], 12)
    for _ in range(8):
        g0.replay()
    st = eng.read_state()
    want = toks[:toks.index(toks[2]) + 1]
    assert eng.read_history(2, st[SLOT_PRODUCED + 2]) == want and not st[SLOT_ACTIVE] & 4
    assert st[SLOT_BUDGET + 2] == 5 - len(want) and st[SLOT_EOS + 2] == toks[2]


@pytest.mark.parametrize("T", [1, 2, 9, 16, 17, 40])
def test_admit_touches_only_its_slot(T):
    B, max_seq, s = 4, 96, 2
    m, ths = _model("tiny-gqa-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    g = torch.Generator(device=DEV).manual_seed(T)
    for l in m.layers:
        l.attention.kv_cache.k_cache.copy_(torch.randn(l.attention.kv_cache.k_cache.shape, device=DEV, generator=g))
        l.attention.kv_cache.v_cache.copy_(torch.randn(l.attention.kv_cache.v_cache.shape, device=DEV, generator=g))
    before = [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]
    prompt = torch.randint(0, m.config.vocab_size, (T,), device=DEV, generator=g, dtype=torch.int32)
    eng.admit(s, prompt.tolist(), 4, None, 1)
    torch.cuda.synchronize()
    assert eng.admit_paths == ({"hip": 1, "module": 0} if 2 <= T <= 16 else {"hip": 0, "module": 1})
    # the same prompt through a batch-1 model on the same path
    m1, _ = _model("tiny-gqa-test", torch.float16, 1, max_seq)
    G.relayout_for_engine(m1)  # the engine's weight layout, as the slot's pass ran on
    with torch.no_grad():
        if 2 <= T <= 16:
            PrefillEngine(m1)(prompt)
        else:
            m1.fused_decode = False
            m1(prompt.view(1, -1), torch.arange(T, device=DEV))
    torch.cuda.synchronize()
    for l, l1, (kb, vb) in zip(m.layers, m1.layers, before):
        kc, vc = l.attention.kv_cache.k_cache, l.attention.kv_cache.v_cache
        for o in range(B):
            if o != s:
                assert torch.equal(kc[o], kb[o]) and torch.equal(vc[o], vb[o]), o
        assert torch.equal(kc[s, :, :T], l1.attention.kv_cache.k_cache[0, :, :T])
        assert torch.equal(vc[s, :, :T], l1.attention.kv_cache.v_cache[0, :, :T])


def _requests(n, seed, lo_t=1, hi_t=40, lo_b=3, hi_b=40, vocab=512):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        T = int(torch.randint(lo_t, hi_t + 1, (1,), generator=g))
        out.append(Request(torch.randint(0, vocab, (T,), generator=g).tolist(), int(torch.randint(lo_b, hi_b + 1, (1,), generator=g))))
    return out


def test_tokens_independent_of_batch_composition():
    B = 4
    reqs = _requests(12, 1)
    max_seq = max(len(r.tokens) + r.max_new_tokens for r in reqs)
    m, ths = _model("tiny-gqa-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, _all_rows(ths), B)
    kw = dict(temperature=0.8, top_k=50)
    a = ContinuousBatcher(eng, sync_every=8, **kw).run(reqs)["tokens"]
    seeded = [Request(r.tokens, r.max_new_tokens, seed=1234 + i) for i, r in enumerate(reqs)]  # request i keeps stream 1234 + i
    b = ContinuousBatcher(eng, sync_every=1, **kw).run(seeded[::-1])["tokens"][::-1]
    c = ContinuousBatcher(eng, sync_every=8, refill="all", **kw).run(reqs)["tokens"]
    assert [len(t) for t in a] == [r.max_new_tokens for r in reqs]
    assert a == b and a == c


def test_mixed_active_set_against_single_sequence_engines():
    from teal_amd.gpt_fast.engine import DecodeEngine
    B, max_seq, dt = 4, 64, torch.float16
    m, ths = _model("tiny-test", dt, B, max_seq)
    m.fused_decode = False
    eng = SlotDecodeEngine(m, ths, B)
    g = torch.Generator(device=DEV).manual_seed(9)
    prompts = {0: 5, 2: 9, 3: 3}  # slot 1 stays inactive
    singles = {}
    for s, T in prompts.items():
        p = torch.randint(0, 512, (T,), device=DEV, generator=g, dtype=torch.int32)
        eng.admit(s, p.tolist(), 60, None, s)
        m1, _ = _model("tiny-test", dt, 1, max_seq)
        with torch.no_grad():
            PrefillEngine(m1)(p)
        singles[s] = (DecodeEngine(m1, ths), T)
    toks = eng.tok_buf[:B].clone()
    for step in range(16):
        pos = eng.pos_buf[:B].clone()
        eng._step()
        lb = eng.logits.float().clone()
        for s, (d, T) in singles.items():
            ls = d(toks[s].view(1, 1), pos[s].view(1)).float().view(-1)
            cos = float(torch.nn.functional.cosine_similarity(lb[s], ls, dim=0))
            assert cos > 0.95, (step, s, cos)
        assert bool((lb[1] == 0).all())
        toks = lb.argmax(-1).int()
        eng.tok_buf[:B].copy_(toks)
        eng.pos_buf[:B].copy_(pos + 1)


def test_graph_replay_equals_eager():
    B = 4
    reqs = _requests(10, 2, hi_b=30)
    max_seq = max(len(r.tokens) + r.max_new_tokens for r in reqs)
    m, ths = _model("tiny-test", torch.float16, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    a = ContinuousBatcher(eng, sync_every=4, use_graph=False).run(reqs)
    b = ContinuousBatcher(eng, sync_every=4, use_graph=True).run(reqs)
    assert a["tokens"] == b["tokens"] and a["steps"] == b["steps"]
    assert [len(t) for t in a["tokens"]] == [r.max_new_tokens for r in reqs]


def _gen(tmp_path, name, reqs, *extra):
    f = tmp_path / "reqs.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in reqs) + "\n")
    args = G.build_parser().parse_args(["--device", "cuda", "--synthetic", name, "--requests", str(f), "--batch_size", "4", "--compile",
                                        "--max_new_tokens", "9", *extra])
    return G.main(args)


@pytest.mark.parametrize("name", ["tiny-test", "tiny-gqa-test"])
def test_generate_requests_end_to_end(name, tmp_path):
    g = torch.Generator().manual_seed(4)
    reqs = [{"tokens": torch.randint(0, 512, (int(t),), generator=g).tolist(), "max_new_tokens": int(n)}
            for t, n in zip(torch.randint(1, 30, (9,), generator=g), torch.randint(2, 40, (9,), generator=g))]
    reqs[3].pop("max_new_tokens")  # the flag's default
    budgets = [r.get("max_new_tokens", 9) for r in reqs]
    res = _gen(tmp_path, name, reqs, "--sparsity", "0.5")
    assert res["decoder"] == "ContinuousBatcher" and [len(s) for s in res["sequences"]] == budgets
    assert res["mean_tokens_per_sec"] > 0
    # --eos_id: with every row kept (sparsity 0) a request's tokens do not depend on its neighbours, so a second run must give
    # each request's first run cut right after the id's first occurrence (at 50 % the union, and with it the summation order,
    # follows the active set, which the cuts change)
    full = _gen(tmp_path, name, reqs, "--sparsity", "0")["sequences"]
    eos = next(t for s in full for t in s[1:])
    cut = _gen(tmp_path, name, reqs, "--sparsity", "0", "--eos_id", str(eos))["sequences"]
    assert any(eos in s for s in full)
    for f_, c_ in zip(full, cut):
        assert c_ == (f_[:f_.index(eos) + 1] if eos in f_ else f_)

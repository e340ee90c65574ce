"""GPU: batched decode (teal_amd/csrc/teal_batched.hip, teal_amd/gpt_fast/batched.py).

  * teal_batched_sparse_gemm against the float64 truth of W (x_b * mask_b) for B in {1, 2, 3, 5, 8}, fp16 / bf16, on the qkv
    (3 tau, MHA and GQA), gate | up (2 tau), down (silu * up producer) and lm_head (tau = -inf) shapes of 7B / 8B, with the kept
    counts per (segment, sequence) and the union's;
  * only the union is read (NaN in every other row changes no bit), identical sequences give identical rows;
  * teal_batched_decode_attention: new cache rows bit-identical to the single-sequence verify path, yt against fp32 torch,
    every other slot untouched;
  * BatchedDecodeEngine against the patched module path at batch 4 and against per-sequence DecodeEngine runs (staggered
    positions, a 32-step greedy trajectory), graph replay = eager, the sampler row by row;
  * torch.ops.teal.* at B in {2, 8, 11} against per-row calls; generate.py --batch_size 4 end to end.
"""
import ctypes

import numpy as np
import pytest
import torch

from batched_rule import kept_counts
from oracle import teal_oracle as O
from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.model import precompute_freqs_cis
from teal_amd.gpt_fast.prefill import IN_SILU_MUL, IN_XT, PrefillIn
from teal_amd.kernels.sparse_gemv import batched_segs

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float16: 0, torch.bfloat16: 1}


def _tol(truth, dt):
    return 1e-3 * np.maximum(1.0, np.abs(truth)) + O.ulp16(truth, O.F16 if dt == torch.float16 else O.BF16)


def _wT(Z, N, dt, g, pad=64):
    """a column-major [N, Z] weight (memory W^T [Z][N + pad]) as the engine lays it out"""
    buf = torch.zeros(Z, N + pad, device=DEV, dtype=dt)
    buf[:, :N] = (torch.randn(Z, N, device=DEV, generator=g) * 0.02).to(dt)
    return buf


def _gemm(L, gin, sg, w0, n0, w1, n1, Z, B, dt, counts=True):
    slabs = torch.full((16 * (n0 + n1) * 8,), float("nan"), device=DEV)
    cnt = torch.full((16 * 27,), -1, device=DEV, dtype=torch.int32) if counts else None
    split = ctypes.c_int(0)
    rc = L.teal_batched_sparse_gemm(ctypes.byref(gin), ctypes.byref(sg), w0.data_ptr(), w0.stride(0), n0,
                                    w1.data_ptr() if w1 is not None else None, w1.stride(0) if w1 is not None else 0, n1,
                                    slabs.data_ptr(), slabs.numel() * 4, Z, B, cnt.data_ptr() if counts else None, CODE[dt],
                                    ctypes.byref(split), runtime.stream_ptr())
    _lib.check(rc, "teal_batched_sparse_gemm")
    N = n0 + n1
    y = torch.empty(B, N, device=DEV, dtype=dt)
    _lib.check(L.teal_batched_round_rows(slabs.data_ptr(), split.value, N, B, y.data_ptr(), CODE[dt], runtime.stream_ptr()), "round")
    torch.cuda.synchronize()
    c = cnt.view(16, 3, 9)[:split.value].sum(0).cpu().numpy() if counts else None
    return y, c


SHAPES = {  # name: (Z, n0, n1, segment bounds (fractions of the width resolved below), producer)
    "qkv_mha_7b": (4096, 3 * 4096, 0, "qkv", 4096),
    "qkv_gqa_8b": (4096, 4096 + 2 * 1024, 0, "qkv", 1024),
    "gateup_7b": (4096, 11008, 11008, "gateup", 0),
    "down_7b": (11008, 4096, 0, "down", 0),
    "lm_head_7b": (4096, 32000, 0, "lm", 0),
}


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
def test_gemm_parity(shape, B, dt):
    L = _lib.load()
    runtime.init()
    Z, n0, n1, kind, kv = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(Z + n0 + B)
    N = n0 + n1
    W0 = _wT(Z, n0, dt, g)
    W1 = _wT(Z, n1, dt, g) if n1 else None
    if kind == "qkv":
        bounds, taus = [n0 - 2 * kv, n0 - kv, n0], [0.5, 0.8, 0.3]
    elif kind == "gateup":
        bounds, taus = [n0, N], [0.6, 0.4]
    elif kind == "lm":
        bounds, taus = [N], [float("-inf")]
    else:
        bounds, taus = [N], [0.05]
    if kind == "down":  # silu(gate) * up from random gate | up slabs (2 slices)
        gu = (torch.randn(2, 2 * Z, 8, device=DEV, generator=g) * 0.5).float()
        gin = PrefillIn(mode=IN_SILU_MUL, gu_slabs=gu.data_ptr(), gu_split=2)
        gs = (gu[0] + gu[1]).to(dt).float()
        gate, up = gs[:Z], gs[Z:]
        x = ((gate / (1 + torch.exp(-gate))).to(dt).float() * up).to(dt).float()[:, :B].t().contiguous()  # [B, Z]
    else:
        xt = torch.zeros(Z, 8, device=DEV, dtype=dt)
        xt[:, :B] = torch.randn(Z, B, device=DEV, generator=g).to(dt)
        xt[:, B:] = 7.0  # slots of absent sequences must play no role
        gin = PrefillIn(mode=IN_XT, xt=xt.data_ptr())
        x = xt[:, :B].t().float().contiguous()
    y, c = _gemm(L, gin, batched_segs(bounds, taus), W0, n0, W1, n1, Z, B, dt)
    Wfull = torch.cat([W0[:, :n0]] + ([W1[:, :n1]] if n1 else []), 1).double()  # [Z, N]
    truth = torch.zeros(B, N, dtype=torch.float64, device=DEV)
    lo = 0
    for hi, tau in zip(bounds, taus):
        xm = torch.where(x.abs() > tau, x, torch.zeros_like(x)).double()
        truth[:, lo:hi] = xm @ Wfull[:, lo:hi]
        lo = hi
    t = truth.cpu().numpy()
    got = y.float().cpu().numpy()
    bad = np.abs(got - t) > _tol(t, dt)
    assert not bad.any(), (shape, B, int(bad.sum()), float(np.abs(got - t).max()))
    want = kept_counts(x.cpu().numpy(), bounds, taus)
    for s, (per, uni) in enumerate(want):
        if kind == "down":  # (the kernel's expf and torch's exp may round a silu apart: a handful of rows either way)
            assert all(abs(int(c[s, b]) - per[b]) <= 4 for b in range(B)) and abs(int(c[s, 8]) - uni) <= 4
        else:
            assert [int(v) for v in c[s, :B]] == per and int(c[s, 8]) == uni, (s, c[s], per, uni)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_only_the_union_is_read_and_identical_rows_agree(dt):
    L = _lib.load()
    runtime.init()
    Z, N, B = 4096, 4096 + 2 * 1024, 3
    g = torch.Generator(device=DEV).manual_seed(11)
    W = _wT(Z, N, dt, g)
    xt = torch.zeros(Z, 8, device=DEV, dtype=dt)
    xt[:, :B] = torch.randn(Z, B, device=DEV, generator=g).to(dt)
    tau = 1.2
    sg = batched_segs([N], [tau])
    gin = PrefillIn(mode=IN_XT, xt=xt.data_ptr())
    clean, _ = _gemm(L, gin, sg, W, N, None, 0, Z, B, dt)
    outside = ~(xt[:, :B].float().abs() > tau).any(1)
    assert 0 < int(outside.sum()) < Z
    Wn = W.clone()
    Wn[outside] = float("nan")
    dirty, _ = _gemm(L, gin, sg, Wn, N, None, 0, Z, B, dt)
    assert torch.isfinite(dirty.float()).all()
    assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16))
    # five copies of one sequence: five bit-identical rows
    xt[:, :5] = xt[:, :1]
    same, _ = _gemm(L, gin, batched_segs([N - 2048, N - 1024, N], [0.4, 0.9, 0.1]), W, N, None, 0, Z, 5, dt)
    for b in range(1, 5):
        assert torch.equal(same[0].view(torch.int16), same[b].view(torch.int16))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n_head,n_kv,hd", [(32, 32, 128), (32, 8, 128), (8, 8, 64), (8, 2, 64)])
def test_attention(n_head, n_kv, hd, dt):
    L = _lib.load()
    runtime.init()
    B, max_seq, split = 4, 1040, 2
    g = torch.Generator(device=DEV).manual_seed(n_head + n_kv + hd)
    pos = [0, 5, 700, max_seq - 1]
    ntot = (n_head + 2 * n_kv) * hd
    slabs = (torch.randn(split, ntot, 8, device=DEV, generator=g) * 0.7).float()
    rope = precompute_freqs_cis(max_seq, hd, dtype=dt).to(DEV).contiguous()
    sentinel = -3.0
    kc = (torch.randn(B, n_kv, max_seq, hd, device=DEV, generator=g) * 0.5).to(dt)
    vc = (torch.randn(B, n_kv, max_seq, hd, device=DEV, generator=g) * 0.5).to(dt)
    for b, p in enumerate(pos):  # rows past each sequence's position hold a sentinel
        kc[b, :, p:] = sentinel
        vc[b, :, p:] = sentinel
    k0, v0 = kc.clone(), vc.clone()
    yt = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
    nb = int(L.teal_batched_decode_attention_ws_bytes(B, n_head, hd))
    part = torch.empty((nb + 3) // 4, device=DEV)
    pos_d = torch.tensor(pos, device=DEV, dtype=torch.int32)
    rc = L.teal_batched_decode_attention(slabs.data_ptr(), split, rope.data_ptr(), pos_d.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                         yt.data_ptr(), part.data_ptr(), part.numel() * 4, B, n_head, n_kv, hd, max_seq, CODE[dt],
                                         runtime.stream_ptr())
    _lib.check(rc, "teal_batched_decode_attention")
    torch.cuda.synchronize()
    assert not yt[:, B:].float().any()
    nbv = int(L.teal_verify_attention_ws_bytes(1, n_head, hd))
    vpart = torch.empty((nbv + 3) // 4, device=DEV)
    scale = 1.0 / hd ** 0.5
    tol = 2e-2 if dt == torch.float16 else 8e-2
    for b, p in enumerate(pos):
        # the single-sequence path on this sequence's slot: its cache rows must be bit-identical
        s1 = torch.zeros(split, ntot, 8, device=DEV)
        s1[:, :, 0] = slabs[:, :, b]
        k1, v1 = k0[b:b + 1].clone(), v0[b:b + 1].clone()
        y1 = torch.zeros(n_head * hd, 8, device=DEV, dtype=dt)
        p1 = torch.tensor([p], device=DEV, dtype=torch.int32)
        rc = L.teal_verify_attention(s1.data_ptr(), split, rope.data_ptr(), p1.data_ptr(), k1.data_ptr(), v1.data_ptr(), y1.data_ptr(),
                                     vpart.data_ptr(), vpart.numel() * 4, 1, n_head, n_kv, hd, max_seq, CODE[dt], runtime.stream_ptr())
        _lib.check(rc, "teal_verify_attention")
        torch.cuda.synchronize()
        assert torch.equal(kc[b, :, p].view(torch.int16), k1[0, :, p].view(torch.int16))
        assert torch.equal(vc[b, :, p].view(torch.int16), v1[0, :, p].view(torch.int16))
        # every other row of this sequence untouched (rows past p keep the sentinel)
        rows = torch.ones(max_seq, dtype=torch.bool, device=DEV)
        rows[p] = False
        assert torch.equal(kc[b][:, rows], k0[b][:, rows]) and torch.equal(vc[b][:, rows], v0[b][:, rows])
        # yt against fp32 attention over rows 0 .. p
        K = kc[b, :, :p + 1].float().repeat_interleave(n_head // n_kv, 0)
        V = vc[b, :, :p + 1].float().repeat_interleave(n_head // n_kv, 0)
        q = slabs[:, :n_head * hd, b].sum(0).to(dt).float().view(n_head, hd)
        cs = rope[p].float()  # [hd/2, 2]
        q2 = q.view(n_head, hd // 2, 2)
        qr = torch.stack([q2[..., 0] * cs[:, 0] - q2[..., 1] * cs[:, 1], q2[..., 1] * cs[:, 0] + q2[..., 0] * cs[:, 1]], -1).view(n_head, hd)
        qr = qr.to(dt).float()
        att = torch.softmax(torch.einsum("hd,hsd->hs", qr, K) * scale, -1)
        ref = torch.einsum("hs,hsd->hd", att, V).reshape(-1)
        got = yt[:, b].float()
        assert float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max())), (b, p, float((got - ref).abs().max()))


def _model(name, dt, n_layer, B, max_seq=64, sparsity=0.5):
    m = G.build_synthetic_model(name, DEV, dt, n_layer=n_layer)
    ths = G.apply_sparsity(m, sparsity=sparsity, hist_path=None, greedy_lookup=None, synthetic=True, decode_calibration=False)
    m.fused_decode = False
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)  # (after the calibration, which leaves its own short caches)
    return m, ths


def _ulps(dt, scale):
    return scale * (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7)


def _close(a, b, dt, sparsity):
    """the precedent of tests/test_engine.py: with every row kept the fused steps track each other to rounding (element-wise);
    at 50 % a few activations sit within rounding of tau and may flip between two summation orders, so compare directions"""
    if sparsity == 0.0:
        tol = (6e-3 if dt == torch.float16 else 6e-2) * max(1.0, float(b.abs().max()))  # (of the logits' scale: 7B-wide rows sum more terms)
        return bool(torch.allclose(a, b, atol=tol, rtol=0)), float((a - b).abs().max())
    cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
    return cos > 0.95, cos  # (7B-wide synthetic rows: one flipped activation moves a 2-layer model's logits by a few per cent)


@pytest.mark.parametrize("sparsity", [0.0, 0.5])
@pytest.mark.parametrize("name,dt,n_layer", [("tiny-test", torch.float16, None), ("tiny-gqa-test", torch.bfloat16, None), ("7B", torch.float16, 2)])
def test_engine_step_vs_module_path_and_decode_engine(name, dt, n_layer, sparsity):
    from teal_amd.gpt_fast.batched import BatchedDecodeEngine
    from teal_amd.gpt_fast.engine import DecodeEngine
    torch.manual_seed(0)
    B, T, max_seq = 4, 6, 64
    m, ths = _model(name, dt, n_layer, B, max_seq, sparsity)
    V = m.config.vocab_size
    g = torch.Generator(device=DEV).manual_seed(5)
    prompts = torch.randint(0, V, (B, T + 40), device=DEV, generator=g)
    # reference 1: the patched module path at batch 4, equal positions
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    with torch.no_grad():
        m(prompts[:, :T], torch.arange(0, T, device=DEV))
        saved = [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]
        want = m(prompts[:, T:T + 1], torch.tensor([T], device=DEV))[:, -1].float()
    for l, (kc, vc) in zip(m.layers, saved):
        l.attention.kv_cache.k_cache.copy_(kc)
        l.attention.kv_cache.v_cache.copy_(vc)
    eng = BatchedDecodeEngine(m, ths, B)
    got = eng(prompts[:, T].int(), torch.full((B,), T, dtype=torch.int32)).float().clone()
    for b in range(B):
        ok, how = _close(got[b], want[b], dt, sparsity)
        assert ok, (b, how)
    kf = eng.kept_fractions()
    assert set(kf) == {"q", "k", "v", "o", "gate", "up", "down"}
    assert all(0 < v["per_seq"] <= v["union"] <= 1 for v in kf.values()), kf
    if sparsity == 0.0:
        assert all(v["union"] == 1.0 for v in kf.values()), kf
    # reference 2: B separate single-sequence DecodeEngines at staggered positions, teacher-forced over 32 greedy steps
    starts = [T, T + 3, T + 9, T + 1]
    singles = []
    for b in range(B):
        mb, _ = _model(name, dt, n_layer, 1, max_seq, sparsity)
        with torch.no_grad():
            mb(prompts[b:b + 1, :starts[b]], torch.arange(0, starts[b], device=DEV))
        for l, lb in zip(m.layers, mb.layers):  # sequence b's cache slot: its own prompt, its own length
            l.attention.kv_cache.k_cache[b].copy_(lb.attention.kv_cache.k_cache[0])
            l.attention.kv_cache.v_cache[b].copy_(lb.attention.kv_cache.v_cache[0])
        singles.append(DecodeEngine(mb, ths))
    toks = torch.stack([prompts[b, starts[b]] for b in range(B)]).int()
    pos = torch.tensor(starts, dtype=torch.int32)
    for step in range(32):
        lb = eng(toks, pos).float().clone()
        for b in range(B):
            ls = singles[b](toks[b].view(1, 1), pos[b].view(1).to(DEV)).float().view(-1)
            ok, how = _close(lb[b], ls, dt, sparsity)
            assert ok, (step, b, how)
        toks = lb.argmax(-1).int()  # greedy, fed to both sides
        pos = pos + 1


def test_graph_replay_and_sampling():
    from teal_amd.gpt_fast.batched import BatchedDecodeEngine
    B, max_seq = 4, 256
    m, ths = _model("tiny-gqa-test", torch.float16, None, B, max_seq)
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    eng = BatchedDecodeEngine(m, ths, B)
    first = torch.tensor([3, 50, 77, 3], dtype=torch.int32)
    caches = [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]

    def reset():
        for l, (kc, vc) in zip(m.layers, caches):
            l.attention.kv_cache.k_cache.copy_(kc)
            l.attention.kv_cache.v_cache.copy_(vc)
    eager = eng.decode_n(first, torch.tensor([0, 1, 2, 3]), 200, temperature=0.8, top_k=50, use_graph=False)
    reset()
    graph = eng.decode_n(first, torch.tensor([0, 1, 2, 3]), 200, temperature=0.8, top_k=50, use_graph=True)
    assert torch.equal(eager, graph)
    # the sampler row by row: same logits, same rng_state -> the existing kernel's token
    L = eng.L
    rng = eng.rng_state.clone()
    eng._sample(0.8, 50)
    torch.cuda.synchronize()
    for b in range(B):
        st = rng[b].clone()
        tok = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = L.teal_sample_topk_ws(eng.logits[b].data_ptr(), m.config.vocab_size, 0, 50, 0.8, st.data_ptr(), tok.data_ptr(), None, None, 0,
                                   eng.ws.data_ptr(), eng.ws.numel() * 4, runtime.stream_ptr())
        _lib.check(rc, "teal_sample_topk_ws")
        torch.cuda.synchronize()
        assert int(tok) == int(eng.tok_buf[b])


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [2, 8, 11])
def test_ops_accept_a_batch(B, dt):
    runtime.init()
    g = torch.Generator(device=DEV).manual_seed(B)
    Z, N, kv = 4096, 6144, 1024
    W = _wT(Z, N, dt, g)[:, :N].T
    x = torch.randn(B, 1, Z, device=DEV, generator=g).to(dt)
    y = torch.ops.teal.sparse_qkv_gemv(x, W, 0.5, 0.8, 0.3, 0, kv)
    y2 = torch.ops.teal.sparse_gemv(x, W, 0.6, 0)
    assert y.shape == (B, 1, N) and y2.shape == (B, 1, N)
    for b in range(B):
        r = torch.ops.teal.sparse_qkv_gemv(x[b:b + 1], W, 0.5, 0.8, 0.3, 0, kv).float()
        r2 = torch.ops.teal.sparse_gemv(x[b:b + 1], W, 0.6, 0).float()
        for got, want in ((y[b:b + 1].float(), r), (y2[b:b + 1].float(), r2)):
            t = want.cpu().numpy()
            assert (np.abs(got.cpu().numpy() - t) <= 2 * _tol(t, dt)).all()


@pytest.mark.parametrize("name", ["tiny-test", "tiny-gqa-test"])
def test_generate_batched_end_to_end(name):
    args = G.build_parser().parse_args(["--device", "cuda", "--synthetic", name, "--batch_size", "4", "--compile", "--sparsity", "0.5",
                                        "--num_samples", "1", "--max_new_tokens", "12"])
    res = G.main(args)
    assert res["batch_size"] == 4 and res["decoder"] == "BatchedDecodeEngine"
    seqs = res["sequences"][0]
    assert len(seqs) == 4 and all(len(s) == 6 + 12 for s in seqs)
    assert res["mean_tokens_per_sec"] > 0
    args = G.build_parser().parse_args(["--device", "cuda", "--synthetic", name, "--batch_size", "4", "--sparsity", "0.5",
                                        "--num_samples", "1", "--max_new_tokens", "4"])
    assert G.main(args)["decoder"] == "module"

"""GPU: speculative decoding (teal_amd/csrc/teal_speculative.hip, teal_amd/gpt_fast/speculative.py).

  * teal_verify_attention against fp32 torch attention with a causal offset p0 (read from the device), cache rows p0 .. p0+T-1
    bit for bit against the module path's RoPE (and the prompt pass's rows at p0 = 0), every other row untouched;
  * VerifyPass against the dense module path model(x[1, T], arange(p, p+T)): every row's logits and every layer's KV rows;
  * teal_spec_accept against the numpy restatement (tests/spec_rule.py), and the first emitted token's distribution = q_0;
  * self-speculation at top_k = 1 emits the dense model's greedy continuation (sparse and dense drafts, accepted drafts required);
    same seed, same tokens; graph = eager; rounds past the end of the cache stay inside it;
  * a separate draft model (a copy, int8, a smaller model) with its fill-in step: the dense greedy continuation, full-acceptance rounds;
  * generate.main --self_speculate emits exactly max_new_tokens tokens and returns the acceptance statistics.
"""
import math

import numpy as np
import pytest
import torch

from spec_rule import accept_numpy, row_probs
from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.model import apply_rotary_emb, precompute_freqs_cis

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {0: torch.float16, 1: torch.bfloat16}


def _rope_ref(x, cs):
    """the module path's RoPE (model.apply_rotary_emb) of rounded x [T, H, D] at table rows cs [T, D/2, 2].  A product of two
    16-bit values is exact in fp32, so x0 c - x1 s rounds once to fp32 there as in the kernels' fmaf: bit-identical"""
    return apply_rotary_emb(x.unsqueeze(0), cs)[0]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n_head,n_kv,hd", [(32, 32, 128), (32, 8, 128), (8, 8, 64)])
def test_verify_attention_vs_torch(n_head, n_kv, hd, dtype):
    L = _lib.load()
    runtime.init()
    dt, max_seq, split = DT[dtype], 1040, 2
    g = torch.Generator(device=DEV).manual_seed(n_head * 7 + hd + dtype)
    rope = precompute_freqs_cis(max_seq, hd, 10000, dt).to(DEV).contiguous()
    ntot = (n_head + 2 * n_kv) * hd
    kc0 = (torch.randn(1, n_kv, max_seq, hd, device=DEV, generator=g) * 0.5).to(dt)
    vc0 = torch.randn(1, n_kv, max_seq, hd, device=DEV, generator=g).to(dt)
    yt = torch.zeros(n_head * hd, 16, device=DEV, dtype=dt)
    parts = torch.zeros(L.teal_verify_attention_ws_bytes(16, n_head, hd) // 4, device=DEV, dtype=torch.float32)
    pos = torch.zeros(1, device=DEV, dtype=torch.int32)
    scale = 1.0 / math.sqrt(hd)
    tol = 2e-2 if dtype == 0 else 6e-2
    for T in (2, 5, 8, 9, 16):
        kr = 8 if T <= 8 else 16
        slabs = torch.randn(split, ntot, kr, device=DEV, generator=g) * 0.7
        qkv = slabs.sum(0)[:, :T].t().to(dt)  # [T, ntot] rounded once
        for p0 in (0, 1, 37, 255, 256, 1000, max_seq - T):
            kc, vc = kc0.clone(), vc0.clone()
            pos.fill_(p0)
            rc = L.teal_verify_attention(slabs.data_ptr(), split, rope.data_ptr(), pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), yt.data_ptr(),
                                         parts.data_ptr(), parts.numel() * 4, T, n_head, n_kv, hd, max_seq, dtype, runtime.stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            q = qkv[:, :n_head * hd].view(T, n_head, hd)
            k = qkv[:, n_head * hd:(n_head + n_kv) * hd].view(T, n_kv, hd)
            v = qkv[:, (n_head + n_kv) * hd:].view(T, n_kv, hd)
            cs = rope[p0:p0 + T]
            qr, kr_ = _rope_ref(q, cs), _rope_ref(k, cs)
            new = slice(p0, p0 + T)
            # rows outside p0 .. p0+T-1 untouched, bit for bit
            keep = torch.ones(max_seq, dtype=torch.bool, device=DEV)
            keep[new] = False
            assert torch.equal(kc[0][:, keep], kc0[0][:, keep]) and torch.equal(vc[0][:, keep], vc0[0][:, keep])
            assert torch.equal(vc[0, :, new].transpose(0, 1), v)
            assert torch.equal(kc[0, :, new].transpose(0, 1), kr_)  # the module path's rows, bit for bit
            if p0 == 0:  # the prompt pass's rows from the same slabs: identical
                kp, vp = kc0.clone(), vc0.clone()
                yp = torch.zeros_like(yt)
                assert L.teal_prefill_attention(slabs.data_ptr(), split, rope.data_ptr(), kp.data_ptr(), vp.data_ptr(), yp.data_ptr(), T,
                                                n_head, n_kv, hd, max_seq, dtype, runtime.stream_ptr()) == 0
                torch.cuda.synchronize()
                assert torch.equal(kp[0, :, :T], kc[0, :, :T]) and torch.equal(vp[0, :, :T], vc[0, :, :T])
            # fp32 attention over the cache with the new rows, query t sees rows 0 .. p0+t
            K = kc[0].float().repeat_interleave(n_head // n_kv, 0)[:, :p0 + T]  # [H, S, D]
            V_ = vc[0].float().repeat_interleave(n_head // n_kv, 0)[:, :p0 + T]
            s = torch.einsum("thd,hsd->hts", qr.float(), K) * scale
            mask = torch.arange(p0 + T, device=DEV)[None, :] <= (p0 + torch.arange(T, device=DEV))[:, None]
            s = s.masked_fill(~mask[None], float("-inf"))
            ref = torch.einsum("hts,hsd->thd", torch.softmax(s, -1), V_)
            y2 = yt.view(-1)[:n_head * hd * kr].view(n_head * hd, kr)  # [feature][R], R = 8 or 16
            got = y2[:, :T].t().float().view(T, n_head, hd)
            err = (got - ref).abs().max().item()
            assert err <= tol * max(1.0, ref.abs().max().item()), (T, p0, err)
            assert not y2[:, T:].any()


def _tiny(name, dt, n_layer=None, max_seq=96):
    m = G.build_synthetic_model(name, DEV, dt, n_layer=n_layer)
    m.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    return m


@pytest.mark.parametrize("name,dt,n_layer", [("7B", torch.float16, 2), ("llama-3-8b", torch.bfloat16, 2), ("tiny-gqa-test", torch.float16, None)])
def test_verify_pass_equals_module_path(name, dt, n_layer):
    from teal_amd.gpt_fast.speculative import VerifyPass
    torch.manual_seed(0)
    m = _tiny(name, dt, n_layer)
    V = m.config.vocab_size
    g = torch.Generator(device=DEV).manual_seed(3)
    toks = torch.randint(0, V, (40,), device=DEV, generator=g, dtype=torch.int32)
    vp = VerifyPass(m)
    with torch.no_grad():
        for p, T in ((12, 5), (23, 16), (30, 2)):
            m(toks[:p].view(1, -1).long(), torch.arange(0, p, device=DEV))  # the context rows, module path
            saved = [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]
            x = toks[p:p + T]
            want = m(x.view(1, -1).long(), torch.arange(p, p + T, device=DEV))[0].float()
            kv_want = [(l.attention.kv_cache.k_cache[0, :, p:p + T].float().clone(), l.attention.kv_cache.v_cache[0, :, p:p + T].float().clone())
                       for l in m.layers]
            for l, (kc, vc) in zip(m.layers, saved):
                l.attention.kv_cache.k_cache.copy_(kc)
                l.attention.kv_cache.v_cache.copy_(vc)
            got = vp.all_logits(x, p).float()
            torch.cuda.synchronize()
            # the prompt pass's tolerance (tests/test_prefill.py): 6 output ulps of the logits' scale, every row
            ulp = float(want.abs().max()) * (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7)
            assert float((got - want).abs().max()) <= 6 * ulp, (name, p, T, float((got - want).abs().max()), ulp)
            for l, (kw, vw) in zip(m.layers, kv_want):
                kt = 2e-2 if dt == torch.float16 else 1e-1
                assert torch.allclose(l.attention.kv_cache.k_cache[0, :, p:p + T].float(), kw, atol=kt, rtol=kt)
                assert torch.allclose(l.attention.kv_cache.v_cache[0, :, p:p + T].float(), vw, atol=kt, rtol=kt)


def _accept_call(L, slabs, split, dlog, V, k, dtype, top_k, temp, rng, tokens, spec_pos, out_seq, cap, out_len, n_acc, scratch):
    return L.teal_spec_accept(slabs.data_ptr(), split, dlog.data_ptr(), V, k, dtype, top_k, temp, rng.data_ptr(), tokens.data_ptr(),
                              spec_pos.data_ptr(), None, out_seq.data_ptr(), cap, out_len.data_ptr(), n_acc.data_ptr(), None,
                              scratch.data_ptr(), scratch.numel() * 4, runtime.stream_ptr())


def _f32(bits: np.ndarray, dtype: int) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32) if dtype == 1 else bits.view(np.float16).astype(np.float32)


def _to16(a: np.ndarray, dtype: int) -> np.ndarray:
    """float32 -> 16-bit bits (round to nearest even), as a uint16 array"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dtype]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("V", [32000, 128256])
@pytest.mark.parametrize("k,top_k", [(1, 0), (4, 200), (15, 1), (4, 0)])
def test_spec_accept_matches_numpy(V, k, top_k, dtype):
    L = _lib.load()
    runtime.init()
    rng_np = np.random.default_rng(V + 31 * k + top_k)
    T, kr, split, temp = k + 1, 8 if k + 1 <= 8 else 16, 2, 0.8
    scratch = torch.zeros(L.teal_spec_accept_scratch_bytes(V, k) // 4 + 64, device=DEV)
    tokens = torch.zeros(16, device=DEV, dtype=torch.int32)
    spec_pos = torch.zeros(1, device=DEV, dtype=torch.int32)
    out_seq = torch.zeros(16, device=DEV, dtype=torch.int32)
    out_len = torch.zeros(1, device=DEV, dtype=torch.int32)
    n_acc = torch.zeros(1, device=DEV, dtype=torch.int32)
    rng = torch.tensor([4321, 0], device=DEV, dtype=torch.int64)
    bad = 0
    rounds = 12
    for r in range(rounds):
        base = rng_np.standard_normal((T, V)).astype(np.float32) * 3
        slabs_np = np.zeros((split, V, kr), dtype=np.float32)
        slabs_np[0, :, :T] = base.T * 0.6
        slabs_np[1, :, :T] = base.T * 0.4
        tq = _to16((slabs_np[0] + slabs_np[1])[:, :T].T, dtype)  # slice order, rounded once
        tp = _to16(_f32(tq, dtype)[:k] + rng_np.standard_normal((k, V)).astype(np.float32) * 0.3, dtype)
        q = np.stack([row_probs(x, dtype == 1, top_k, temp) for x in tq])
        p = np.stack([row_probs(x, dtype == 1, top_k, temp) for x in tp])
        drafts = np.array([rng_np.choice(V, p=p[i].astype(np.float64) / p[i].astype(np.float64).sum()) for i in range(k)])
        ctr = int(rng[1].item())
        n_np, tok_np, near = accept_numpy(q, p, drafts, 4321, ctr)
        slabs = torch.from_numpy(slabs_np).to(DEV)
        dlog = torch.from_numpy(tp.view(np.int16)).to(DEV).view(DT[dtype])
        tokens[1:k + 1].copy_(torch.from_numpy(drafts.astype(np.int32)))
        out_len.zero_()
        spec_pos.fill_(100)
        assert _accept_call(L, slabs, split, dlog, V, k, dtype, top_k, temp, rng, tokens, spec_pos, out_seq, 16, out_len, n_acc, scratch) == 0
        torch.cuda.synchronize()
        n, tok = int(n_acc.item()), int(tokens[0].item())
        assert int(rng[1].item()) == ctr + 2 and int(out_len.item()) == n + 1 and int(spec_pos.item()) == 100 + n + 1
        assert out_seq[:n].tolist() == drafts[:n].tolist() and int(out_seq[n].item()) == tok
        if (n, tok) != (n_np, tok_np):
            assert near, (r, n, tok, n_np, tok_np)
            bad += 1
    assert bad <= 1


def test_first_token_follows_the_target_distribution():
    """20 000 rounds with fixed p / q rows and fresh draws: the first emitted token is distributed as q_0 (chi-square)."""
    L = _lib.load()
    runtime.init()
    V, k, R = 32, 2, 20000
    rs = np.random.default_rng(5)
    tq = (rs.standard_normal((k + 1, V)) * 1.5).astype(np.float16)
    tp = (tq[:k].astype(np.float32) + rs.standard_normal((k, V)).astype(np.float32)).astype(np.float16)
    q0 = row_probs(tq[0].view(np.uint16), False, 0, 1.0).astype(np.float64)
    p = np.stack([row_probs(x.view(np.uint16), False, 0, 1.0) for x in tp]).astype(np.float64)
    drafts = np.stack([rs.choice(V, size=R, p=p[i] / p[i].sum()) for i in range(k)], 1).astype(np.int32)  # [R, k]
    slabs = torch.zeros(1, V, 8, device=DEV)
    slabs[0, :, :k + 1] = torch.from_numpy(tq.astype(np.float32).T).to(DEV)
    dlog = torch.from_numpy(np.ascontiguousarray(tp)).to(DEV)
    d_dev = torch.from_numpy(drafts).to(DEV)
    scratch = torch.zeros(L.teal_spec_accept_scratch_bytes(V, k) // 4 + 64, device=DEV)
    tokens = torch.zeros(16, device=DEV, dtype=torch.int32)
    spec_pos = torch.zeros(1, device=DEV, dtype=torch.int32)
    out_seq = torch.zeros(R * (k + 1), device=DEV, dtype=torch.int32)
    out_len = torch.zeros(1, device=DEV, dtype=torch.int32)
    n_acc = torch.zeros(1, device=DEV, dtype=torch.int32)
    n_log = torch.zeros(R, device=DEV, dtype=torch.int32)
    rng = torch.tensor([99, 0], device=DEV, dtype=torch.int64)
    for r in range(R):
        tokens[1:k + 1].copy_(d_dev[r])
        assert _accept_call(L, slabs, 1, dlog, V, k, 0, 0, 1.0, rng, tokens, spec_pos, out_seq, out_seq.numel(), out_len, n_acc, scratch) == 0
        n_log[r:r + 1].copy_(n_acc)
    torch.cuda.synchronize()
    starts = np.concatenate([[0], np.cumsum(n_log.cpu().numpy() + 1)[:-1]])
    first = out_seq.cpu().numpy()[starts]
    counts = np.bincount(first, minlength=V).astype(np.float64)
    exp = q0 * R
    big = exp >= 5
    obs = np.append(counts[big], counts[~big].sum())
    ex = np.append(exp[big], exp[~big].sum())
    chi2 = float((((obs - ex) ** 2) / np.maximum(ex, 1e-9)).sum())
    dof = int(big.sum())
    # 1e-4 upper quantile of chi-square(dof), Wilson-Hilferty: the seed is fixed, so this is deterministic, not flaky
    z = 3.719
    limit = dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3
    assert chi2 < limit, (chi2, limit, dof)


def _self_spec(name, dt, k, top_k, sparsity, graph, seed=1234, max_new=40, temperature=0.8, max_seq=None, draft_dense=False):
    """self-speculation on a synthetic model; draft_dense: thresholds of -1 (every activation kept: the draft IS the dense model
    through the decode step, so nearly every round accepts all k)"""
    from teal_amd.gpt_fast.prefill import FusedPrefill
    from teal_amd.gpt_fast.engine import DecodeEngine
    from teal_amd.gpt_fast.speculative import SpeculativeDecoder, VerifyPass
    m = G.build_synthetic_model(name, DEV, dt, n_layer=2 if name in ("7B", "llama-3-8b") else None)
    if draft_dense:
        ths = [{p: -1.0 for p in G.PROJS} for _ in m.layers]
    else:
        ths = G.apply_sparsity(m, sparsity=sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
    prompt = torch.randint(0, m.config.vocab_size, (6,), device=DEV, dtype=torch.int, generator=torch.Generator(device=DEV).manual_seed(7))
    m.setup_caches(max_batch_size=1, max_seq_length=max_seq or 6 + max_new + k + 1)
    G.relayout_for_engine(m)
    pre = FusedPrefill(m, graph=graph)
    eng = DecodeEngine(m, ths)
    eng.manual_seed(seed)
    spec = SpeculativeDecoder(eng, VerifyPass(m), k, temperature, top_k, fill_in=False, capacity=max_new + k + 1, graph=graph)
    seq, hist = G.speculative_generate(spec, prompt, max_new, pre, None, temperature, top_k)
    return m, prompt, seq, hist, spec


def greedy_matches_dense(m, prompt, seq):
    """seq's new tokens = the dense module path's teacher-forced argmax at every position outside near-ties"""
    T, n = prompt.numel(), seq.numel()
    with torch.no_grad():
        m.setup_caches(max_batch_size=1, max_seq_length=n)
        logits = m(seq[:-1].view(1, -1).long(), torch.arange(0, n - 1, device=DEV))[0].float()  # dense: teacher-forced module path
    top2 = logits[T - 1:].topk(2, dim=-1)
    # near-ties: a margin under 1 % of the logit scale may flip between the fused pass and the module path
    margin = 1e-2 * max(1.0, logits.abs().max().item())
    clear = (top2.values[:, 0] - top2.values[:, 1]) > margin
    want, got = top2.indices[:, 0], seq[T:].long()
    assert clear.sum() >= 0.25 * clear.numel()
    assert torch.equal(want[clear], got[clear]), (want.tolist(), got.tolist())


@pytest.mark.parametrize("name,draft", [("tiny-test", "sparse"), ("7B", "sparse"), ("tiny-test", "dense"), ("7B", "dense")])
def test_greedy_self_speculation_is_the_dense_greedy_continuation(name, draft):
    k = 4
    m, prompt, seq, hist, _ = _self_spec(name, torch.float16, k=k, top_k=1, sparsity=0.5, graph=True, max_new=60, draft_dense=draft == "dense")
    assert sum(hist[1:]) > 0, hist  # drafts were accepted: the emission and position path of accepted tokens is covered
    if draft == "dense":
        assert hist[k] > sum(hist[:k]), hist  # a dense draft agrees with the target: most rounds accept all k
    greedy_matches_dense(m, prompt, seq)


def test_round_at_the_end_of_the_cache_stays_inside_it():
    """rounds whose positions run past max_seq (a caller that sized the cache too small) are clamped into the cache: rows below
    the first round's position and the memory right after every layer's caches are untouched"""
    from teal_amd.gpt_fast.prefill import FusedPrefill
    from teal_amd.gpt_fast.engine import DecodeEngine
    from teal_amd.gpt_fast.speculative import SpeculativeDecoder, VerifyPass
    k, max_seq, pad = 4, 24, 4096
    m = G.build_synthetic_model("tiny-test", DEV, torch.float16)
    m.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    canaries = []
    for layer in m.layers:  # every cache a view at the start of a larger buffer whose tail must stay as it was
        kv = layer.attention.kv_cache
        for name in ("k_cache", "v_cache"):
            c = getattr(kv, name)
            big = torch.full((c.numel() + pad,), 7.0, device=DEV, dtype=c.dtype)
            big[:c.numel()].zero_()
            setattr(kv, name, big[:c.numel()].view(c.shape))
            canaries.append(big)
    G.relayout_for_engine(m)
    prompt = torch.randint(0, 512, (6,), device=DEV, dtype=torch.int, generator=torch.Generator(device=DEV).manual_seed(7))
    pre = FusedPrefill(m, graph=False)
    eng = DecodeEngine(m, [{p: -1.0 for p in G.PROJS} for _ in m.layers])
    spec = SpeculativeDecoder(eng, VerifyPass(m), k, 0.8, 1, fill_in=False, capacity=64, graph=True)
    logits = pre(prompt)
    first = eng.sample_first(logits[0, -1].contiguous(), 0.8, 1)
    spec.begin(first, max_seq - 8)
    spec.capture()
    before = [(l.attention.kv_cache.k_cache.clone(), l.attention.kv_cache.v_cache.clone()) for l in m.layers]
    for _ in range(5):  # 5 rounds from max_seq - 8: positions run past the end
        spec.round()
    torch.cuda.synchronize()
    start = max_seq - 8  # the first round's position: nothing below it is written
    assert int(spec.spec_pos.item()) > max_seq, "the rounds did run past the end"
    for l, (kb, vb) in zip(m.layers, before):
        assert torch.equal(l.attention.kv_cache.k_cache[:, :, :start], kb[:, :, :start])
        assert torch.equal(l.attention.kv_cache.v_cache[:, :, :start], vb[:, :, :start])
    for big in canaries:
        n = big.numel() - pad
        assert bool((big[n:] == 7.0).all()), "a launch wrote past the cache"


def test_self_speculation_is_reproducible_and_graph_equals_eager():
    _, _, a, ha, _ = _self_spec("tiny-test", torch.float16, k=3, top_k=200, sparsity=0.5, graph=True, seed=11)
    _, _, b, hb, _ = _self_spec("tiny-test", torch.float16, k=3, top_k=200, sparsity=0.5, graph=True, seed=11)
    _, _, c, hc, _ = _self_spec("tiny-test", torch.float16, k=3, top_k=200, sparsity=0.5, graph=False, seed=11)
    assert torch.equal(a, b) and ha == hb
    assert torch.equal(a, c) and ha == hc


def test_generate_main_self_speculate_emits_max_new_tokens():
    a = G.build_parser().parse_args(["--synthetic", "tiny-test", "--self_speculate", "--speculate_k", "4", "--compile", "--sparsity", "0.5",
                                     "--max_new_tokens", "25", "--num_samples", "2", "--device", DEV])
    res = G.main(a)
    assert all(len(s) == 6 + 25 for s in res["sequences"])
    assert len(res["acceptance_probs"]) == 5 and abs(sum(res["acceptance_probs"]) - 1) < 1e-6
    assert 0 <= res["mean_accepted"] <= 4 and res["speculative"] == "self"


@pytest.mark.parametrize("draft_kind", ["copy", "int8", "smaller"])
def test_separate_draft_model_greedy_is_the_dense_greedy_continuation(draft_kind, tmp_path):
    """--draft_checkpoint_path with another checkpoint: the draft has its own engine, caches and prompt pass, and a fill-in step
    writes its KV row of d_k every round.  Drafts, loaded from checkpoints by generate.load_draft_model:
      copy     the target's weights in fp16 at sparsity 0 — agrees with the target, so rounds that accept all k (the ones that need
               the fill-in row) must occur and must dominate;
      int8     the target's weights quantised to int8 (teal_amd.quantize) — the int8 engine drafts, some drafts are accepted;
      smaller  another, smaller synthetic model of the same vocabulary at 50 % — unrelated weights: acceptance is not asserted.
    Whatever the draft, the output is the dense target's greedy continuation (top_k = 1)."""
    from teal_amd.gpt_fast.prefill import FusedPrefill
    from teal_amd.quantize import quantize_model_int8
    k, max_new, dt = 4, 60, torch.float16
    target = G.build_synthetic_model("tiny-gqa-test", DEV, dt)
    if draft_kind == "smaller":
        src, name, fname, sparsity = G.build_synthetic_model("tiny-test", DEV, dt, seed=99), "tiny-test", "model.pth", 0.5
    elif draft_kind == "int8":
        src, name, fname, sparsity = quantize_model_int8(G.build_synthetic_model("tiny-gqa-test", DEV, dt)), "tiny-gqa-test", "model_int8.pth", 0.0
    else:
        src, name, fname, sparsity = target, "tiny-gqa-test", "model.pth", 0.0
    (tmp_path / name).mkdir()
    path = tmp_path / name / fname
    torch.save({n: t.detach().cpu() for n, t in src.state_dict().items()}, str(path))
    draft = G.load_draft_model(path, DEV, dt, sparsity, None, None)
    if draft_kind == "int8":
        assert draft[0].output.weight.dtype == torch.int8
    prompt = torch.randint(0, 512, (6,), device=DEV, dtype=torch.int, generator=torch.Generator(device=DEV).manual_seed(7))
    max_seq = 6 + max_new + k + 1
    target.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    G.relayout_for_engine(target)
    pre = FusedPrefill(target, graph=True)
    spec, draft_prefill = G.build_speculator(target, None, k, 0.8, 1, max_new + k + 1, max_seq, True, draft)
    assert spec.fill_in and draft_prefill is not None and spec.draft.model is draft[0]
    seq, hist = G.speculative_generate(spec, prompt, max_new, pre, draft_prefill, 0.8, 1)
    assert seq.numel() == 6 + max_new and sum(hist) > 0
    if draft_kind == "copy":
        assert hist[k] > sum(hist[:k]), hist  # full-acceptance rounds: the next round drafts from the fill-in row
    if draft_kind == "int8":
        assert sum(hist[1:]) > 0, hist
    greedy_matches_dense(target, prompt, seq)

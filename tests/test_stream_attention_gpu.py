"""GPU: the stream split-KV body (teal_batched_decode_attention_stream[_kv8], teal_amd/csrc/teal_stream_attention.h) against the
fp64 references of tests/attention_probes.py, the chunked launch's stores, the fp8 rule of tests/kv8_rule.py, and through
SlotDecodeEngine(attention="stream").  The one place that reads the kernel's dealing is _positions: U rows per workgroup round."""
import json

import pytest
import torch

import attention_probes as P
import kv8_cases as K
import kv8_rule as R
from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SlotDecodeEngine
from test_batched_gpu import _close
from test_continuous_gpu import _all_rows, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
NAN = float("nan")
_name = lambda dt: "fp16" if dt == torch.float16 else "bf16"  # noqa: E731
_bits = lambda x: x.view(torch.int16)  # noqa: E731


def _lib_ready():
    L = _lib.load()
    runtime.init()
    return L


def _plan(heads, B, S):
    """(U, nsplit) of a launch: chunked_attention_plan at a cap of 8 heads, stream_round_rows (teal_stream_attention.h)"""
    n_head, n_kv, hd = heads
    rep = n_head // n_kv
    hq = max(c for c in range(1, 9) if rep % c == 0)
    wg = n_kv * (rep // hq) * B
    nsplit = min(max(-(-2 * torch.cuda.get_device_properties(0).multi_processor_count // wg), 1), 64, -(-S // 32))
    return 4 * (64 // (hd // 8)) * (8 if hq <= 2 else 4), nsplit


def _positions(heads, B, S):
    """lists of B positions that cover the fixed positions and the dealing's edges (padded by starting over)"""
    U, nsplit = _plan(heads, B, S)
    ps = [p for p in dict.fromkeys((0, 1, 31, 32, 33, 700, 1039, U - 1, U, U + 1, nsplit * U - 1, nsplit * U + 1)) if p < S]
    ps += ps[:-len(ps) % B]
    return [ps[i:i + B] for i in range(0, len(ps), B)]


def _launch(L, entry, heads, dt, slabs, rope, pos, act, caches, y, S):
    """entry "stream" / "stream_kv8" / "chunked" (the 16-bit chunked launch with the same predication); caches: (K, V[, K scales, V scales])"""
    n_head, n_kv, hd = heads
    B = pos.numel()
    nb = int(L.teal_batched_decode_attention_ws_bytes(B, n_head, hd))
    part = torch.full(((nb + 3) // 4,), NAN, device=DEV, dtype=torch.float32)
    a = (slabs.data_ptr(), 2, rope.data_ptr(), pos.data_ptr())
    z = (*(c.data_ptr() for c in caches), y.data_ptr(), part.data_ptr(), nb, B, n_head, n_kv, hd, S, runtime.dtype_code(dt), runtime.stream_ptr())
    ap = None if act is None else act.data_ptr()
    if entry == "chunked":
        return L.teal_batched_decode_attention(*a, *z) if act is None else L.teal_batched_decode_attention_slots(*a, ap, *z)
    return getattr(L, "teal_batched_decode_attention_" + entry)(*a, ap, *z)


def _inputs(cs):
    slabs = torch.full((2, cs[0].qkv.numel(), 8), 3.0, device=DEV, dtype=torch.float32)
    for b, c in enumerate(cs):
        slabs[:, :, b] = c.qkv.float() * 0.5
    return slabs, cs[0].rope.contiguous(), torch.tensor([c.pos for c in cs], device=DEV, dtype=torch.int32)


def _run(L, heads, dt, positions, S=P.MULTI_MAX_SEQ, active=None, peaked=False, newest="background"):
    """tests/test_attention_probes_gpu.py's _run_batched through the stream entry: launch i puts sequence b's needle set i into its
    cache.  Checks yt of absent / inactive slots, and the caches against the chunked launch's from the same inputs and against
    the caches before; returns per active sequence (b, case, yt [launches, 1, H, hd], y64, emulation or None, max |V|)"""
    n_head, n_kv, hd = heads
    B = len(positions)
    cs = [P.decode_case(n_head, n_kv, hd, p, S, dt, seed=1000 * b + p + hd, peaked=peaked, newest=newest).to(DEV) for b, p in enumerate(positions)]
    kc0, vc0 = torch.stack([c.kc for c in cs]), torch.stack([c.vc for c in cs])
    kc, vc = kc0.clone(), vc0.clone()
    slabs, rope, pos = _inputs(cs)
    act = None if active is None else torch.tensor([active], device=DEV, dtype=torch.int32)
    on = [b for b in range(B) if active is None or (active >> b) & 1]
    n_launch = max(max(c.sets.shape[0] for c in cs), 1)
    Y = torch.full((n_launch, n_head * hd, 8), NAN, device=DEV, dtype=dt)
    for i in range(n_launch):
        for b, c in enumerate(cs):
            if c.sets.shape[0]:
                kc[b][:, c.sets[i % c.sets.shape[0]]] = c.kappa[:, None, :]
        assert _launch(L, "stream", heads, dt, slabs, rope, pos, act, (kc, vc), Y[i], S) == 0
        for b, c in enumerate(cs):
            if c.sets.shape[0]:
                rows = c.sets[i % c.sets.shape[0]]
                kc[b][:, rows] = c.kc[:, rows]
    kc2, vc2 = kc0.clone(), vc0.clone()
    assert _launch(L, "chunked", heads, dt, slabs, rope, pos, act, (kc2, vc2), torch.empty_like(Y[0]), S) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2)), "the stored rows are the chunked launch's"
    assert not bool(Y[:, :, B:].float().abs().sum() != 0), "slots >= B are zero"
    out = []
    for b, c in enumerate(cs):
        p = c.pos
        if b not in on:  # yt zero in every launch, the caches untouched
            assert not bool(Y[:, :, b].float().abs().sum() != 0)
            assert torch.equal(_bits(kc[b]), _bits(kc0[b])) and torch.equal(_bits(vc[b]), _bits(vc0[b]))
            continue
        keep = torch.arange(S, device=DEV) != p  # (NaN rows included: bit patterns)
        assert torch.equal(_bits(kc[b])[:, keep], _bits(kc0[b])[:, keep]) and torch.equal(_bits(vc[b])[:, keep], _bits(vc0[b])[:, keep])
        assert torch.equal(_bits(vc[b][:, p]), _bits(c.v_new)) and not torch.equal(_bits(kc[b][:, p]), _bits(kc0[b][:, p]))
        Kb, Vb = kc[b][:, :p + 1], vc[b][:, :p + 1]
        vmax = float(Vb.float().abs().max())
        emu = None
        if c.sets.shape[0]:
            y64, outside = P.sweep_reference(c.q_rot, Kb, Vb, c.kappa, c.sets, c.visible, c.scale)
            assert float(outside.max()) < P.OUTSIDE_MAX, ("precondition", heads, b, p)
            y64 = y64[torch.arange(n_launch, device=DEV) % c.sets.shape[0]]
        else:
            y64, prob = P.attend64(c.q_rot, Kb, Vb, c.visible, c.scale)
            if peaked:
                emu = P.attend_emulated(c.q_rot, Kb, Vb, c.visible, c.scale, dt)[None]
            elif newest == "needle":  # the answer is v_new
                assert float((1 - prob[..., p]).max()) < P.OUTSIDE_MAX, ("precondition", heads, b, p)
            y64 = y64[None].expand(n_launch, 1, n_head, hd)
        out.append((b, c, Y[:, :, b].reshape(n_launch, 1, n_head, hd), y64, emu, vmax))
    return out


def _needles(tag, res, dt):
    for b, c, got, y64, _, vmax in res:
        d = (got.double() - y64).abs()
        ok = d <= P.tol_needle(y64, vmax, dt)  # (a NaN fails)
        assert bool(ok.all()), (tag, b, c.pos, "launches off:", (~ok).flatten(1).any(1).nonzero().view(-1).tolist()[:8],
                                float(d.nan_to_num(1e30).max()))


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads,Bs", [((32, 32, 128), (3,)), ((32, 8, 128), (1, 3, 8)), ((8, 8, 64), (1, 8)), ((8, 2, 64), (3, 8))])
def test_stream_needles(heads, Bs, dt):
    """every cache row in turn a dominant key (guard rows behind pos: V = 100, then NaN), then the new row as the only one"""
    L = _lib_ready()
    for B in Bs:
        for ps in _positions(heads, B, P.MULTI_MAX_SEQ):
            _needles(("sweep", heads, ps), _run(L, heads, dt, ps), dt)
            _needles(("newest only", heads, ps), _run(L, heads, dt, ps, newest="needle"), dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_stream_needles_several_rounds_per_split_at_the_cap(dt):
    L = _lib_ready()
    assert _plan((8, 2, 64), 1, 8192)[1] == 64
    _needles("long", _run(L, (8, 2, 64), dt, [8191], S=8192), dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads,B,active", [((32, 8, 128), 8, 0b10110101), ((8, 2, 64), 3, 0b101), ((8, 8, 64), 8, 0b01001010), ((32, 32, 128), 3, 0b110)])
def test_stream_slots(heads, B, active, dt):
    """a mixed active mask: the inactive slots' yt zero and caches untouched, the stored rows the chunked launch's (in _run)"""
    L = _lib_ready()
    for ps in _positions(heads, B, P.MULTI_MAX_SEQ):
        res = _run(L, heads, dt, ps, active=active)
        assert len(res) == bin(active).count("1")
        _needles(("slots", heads, ps), res, dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads,B,active", [((32, 32, 128), 3, None), ((32, 8, 128), 8, 0b01111101), ((8, 2, 64), 8, None)])
def test_stream_peaked(heads, B, active, dt):
    L = _lib_ready()
    for ps in _positions(heads, B, P.MULTI_MAX_SEQ):
        for b, c, got, y64, emu, _ in _run(L, heads, dt, ps, active=active, peaked=True):
            e_k, e_e = P.err_rel(got, y64), P.err_rel(emu, y64)
            print(f"PROBE peaked stream {heads} B={B} pos {c.pos} {_name(dt)} err_kernel={e_k:.3e} err_emulation={e_e:.3e}")
            assert e_k <= P.peaked_bound(e_e, dt), (heads, b, c.pos, e_k, e_e)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads", [(32, 8, 128), (8, 8, 64)])
def test_stream_independence(heads, dt):
    """B = 8: a sequence's yt words do not depend on its slot, on its neighbours (active or not, other positions) or on the replay"""
    L = _lib_ready()
    S = P.MULTI_MAX_SEQ
    mk = lambda p, seed: P.decode_case(*heads, p, S, dt, seed=seed, peaked=True).to(DEV)  # noqa: E731
    x, near, far = mk(700, 7), [mk(p, 50 + p) for p in (5, 1039, 33, 0, 200, 64, 999)], [mk(p, 90 + p) for p in (1000, 2, 31, 640, 1, 129, 257)]

    def yt(slot, others, active):
        cs = others[:slot] + [x] + others[slot:]
        slabs, rope, pos = _inputs(cs)
        act = None if active is None else torch.tensor([active], device=DEV, dtype=torch.int32)
        y = torch.full((heads[0] * heads[2], 8), NAN, device=DEV, dtype=dt)
        caches = (torch.stack([c.kc for c in cs]), torch.stack([c.vc for c in cs]))
        assert _launch(L, "stream", heads, dt, slabs, rope, pos, act, caches, y, S) == 0
        torch.cuda.synchronize()
        return _bits(y[:, slot]).clone()

    ref = yt(2, near, None)
    assert not bool(torch.isnan(ref.view(dt).float()).any())
    assert torch.equal(ref, yt(2, near, None)), "replay"
    assert torch.equal(ref, yt(5, near, None)), "slot"
    assert torch.equal(ref, yt(2, near, 0b00100100)) and torch.equal(ref, yt(5, near, 0b10100001)), "inactive neighbours"
    assert torch.equal(ref, yt(2, far, 0xFF)) and torch.equal(ref, yt(5, far, None)), "neighbours at other positions"


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("heads", [(8, 2, 64), (4, 4, 128)])
def test_stream_kv8_is_the_16bit_stream_launch_on_the_dequantised_cache(heads, dtype):
    L = _lib_ready()
    dt, S, B, mask = getattr(torch, dtype), P.MULTI_MAX_SEQ, 8, 0b10110101
    act = torch.tensor([mask], device=DEV, dtype=torch.int32)
    for ps in _positions(heads, B, S):
        host = K.attention_case(f"stream-kv8-{heads}-{ps}", heads, dtype, B, ps, S)
        assert host["k_exact"] and host["v_exact"]
        c = {k: v.to(DEV) for k, v in host.items() if isinstance(v, torch.Tensor)}
        pos = torch.tensor(ps, device=DEV, dtype=torch.int32)
        y16, y8 = (torch.full((heads[0] * heads[2], 8), 5.0, device=DEV, dtype=dt) for _ in range(2))
        assert _launch(L, "stream", heads, dt, c["slabs"], c["rope"], pos, act, (c["k_dq"], c["v_dq"]), y16, S) == 0
        caches8 = (c["k_codes"], c["v_codes"], c["k_scales"], c["v_scales"])
        assert _launch(L, "stream_kv8", heads, dt, c["slabs"], c["rope"], pos, act, caches8, y8, S) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(y8), _bits(y16)), ps
        on = [b for b in range(B) if (mask >> b) & 1]
        assert not y8[:, [b for b in range(8) if b not in on]].float().any() and all(bool(y8[:, b].float().any()) for b in on)
        for name in ("k", "v"):
            codes, scales, new16 = c[name + "_codes"].cpu(), c[name + "_scales"].cpu(), c[name + "_dq"].cpu()
            for b, p in enumerate(ps):
                keep = torch.ones(S, dtype=torch.bool)
                if b in on:  # the appended row: the rule applied to the row the 16-bit launch appended
                    keep[p] = False
                    want_c, want_s = R.quantize(new16[b, :, p])
                    assert torch.equal(codes[b, :, p], want_c) and torch.equal(scales[b, :, p].view(torch.int32), want_s.view(torch.int32)), (name, b, p)
                assert torch.equal(codes[b][:, keep], host[name + "_codes"][b][:, keep]), (name, b, "codes outside the new row")
                assert torch.equal(scales[b][:, keep].view(torch.int32), host[name + "_scales"][b][:, keep].view(torch.int32)), (name, b)


@pytest.mark.parametrize("kv", [None, "fp8"])
@pytest.mark.parametrize("name,dt", [("tiny-test", torch.float16), ("tiny-gqa-test", torch.bfloat16)], ids=["tiny-fp16", "gqa-bf16"])
def test_engine_graph_replay_is_eager_stepping_and_tracks_the_chunked_engine(name, dt, kv):
    B, max_seq = 3, 64

    def engine(attention):
        m, ths = _model(name, dt, B if kv is None else 1, max_seq)
        eng = SlotDecodeEngine(m, _all_rows(ths), B, kv_cache=kv, attention=attention)
        g = torch.Generator().manual_seed(5)
        for s, T in ((0, 7), (2, 23)):  # slot 1 stays free
            eng.admit(s, torch.randint(0, m.config.vocab_size, (T,), generator=g).tolist(), 50, None, 100 + s, temperature=0.8, top_k=50)
        return eng

    eager, replayed, chunked = engine("stream"), engine("stream"), engine("chunked")
    assert eager.attention == "stream" and chunked.attention == "chunked" and eager._feature_key() == chunked._feature_key()
    graph = replayed.capture(0.8, 50)
    chunked._self_step(0.8, 50)
    for step in range(6):
        eager._self_step(0.8, 50)
        graph.replay()
        torch.cuda.synchronize()
        for s in (0, 2):
            assert torch.equal(_bits(eager.logits[s]), _bits(replayed.logits[s])), (step, s)
            if step == 0:
                ok, err = _close(eager.logits[s].float(), chunked.logits[s].float(), dt, 0.0)
                assert ok, (s, err)
        assert torch.equal(eager.tok_buf, replayed.tok_buf) and torch.equal(eager.pos_buf, replayed.pos_buf)
    assert eager.pos_buf.tolist()[0] == 7 + 6


@pytest.mark.parametrize("kv", ["model", "fp8"])
def test_generate_requests_with_the_stream_body_end_to_end(kv, tmp_path):
    g = torch.Generator().manual_seed(6)
    reqs = [{"tokens": torch.randint(0, 512, (int(t),), generator=g).tolist(), "max_new_tokens": int(n)}
            for t, n in zip(torch.randint(1, 30, (7,), generator=g), torch.randint(2, 30, (7,), generator=g))]
    f = tmp_path / "reqs.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in reqs) + "\n")
    argv = ["--device", "cuda", "--synthetic", "tiny-gqa-test", "--requests", str(f), "--batch_size", "4", "--compile", "--max_new_tokens", "9",
            "--sparsity", "0.5", "--precision", "bf16", "--attention", "stream", "--kv_cache", kv]
    res = G.main(G.build_parser().parse_args(argv))
    assert res["decoder"] == "ContinuousBatcher" and [len(s) for s in res["sequences"]] == [r["max_new_tokens"] for r in reqs]

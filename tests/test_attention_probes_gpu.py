"""GPU: every attention entry point against fp64 torch on inputs that show a lost row or a wrong softmax scale
(tests/attention_probes.py; their power is proven on the CPU by tests/test_attention_probes_host.py).

  * equal-needle sweeps: one launch per needle set, every cache row a needle in exactly one launch (row r: launch r mod n_sets),
    all launches compared at once at 1 ulp + 2^-20 max|V|; row pos + 1 holds the needle key with V = 100, the rows behind it NaN;
  * the appended row: `newest only` (k_new = unrope(kappa), the answer is v_new), and bit-for-bit against apply_rotary_emb;
  * multi-token launches: the staircase (query t must return v_t — the only direct check of teal_prefill_attention's yt) and
    context-row sweeps;
  * peaked random inputs: err(kernel) <= 2 err(16-bit emulation) + 2^-10 (fp16) / 2^-7 (bf16), both measured on the same inputs.

The dominance precondition (< 2^-16 of the fp64 softmax weight outside the needles) is asserted on the reference, never on a
kernel's output.  Each test prints `PROBE ...` lines with its worst error (profiles/attention_probes.txt is made of them).
"""
import pytest
import torch

import attention_probes as P
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.model import apply_rotary_emb

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
NAN = float("nan")


def _name(dt):
    return "fp16" if dt == torch.float16 else "bf16"


def _bits(x):
    return x.view(torch.int16)


def _lib_ready():
    L = _lib.load()
    runtime.init()
    return L


def _check(tag, Y, y64, vmax, dt, sets=None):
    """Y, y64: [launches, ...].  Asserts |Y - y64| <= 1 ulp + 2^-20 vmax everywhere (a NaN fails); returns the worst error in ulps
    (of max(ulp(y64), 2^-20 vmax): where a mean of V rows cancels to ~0 the absolute term is the bound, not the ulp)"""
    d = (Y.double() - y64).abs()
    ok = d <= P.tol_needle(y64, vmax, dt)
    if not bool(ok.all()):
        bad = (~ok).flatten(1).any(1).nonzero().view(-1).tolist()
        rows = None if sets is None or not sets.numel() else [sets[i % sets.shape[0]].tolist() for i in bad[:4]]
        raise AssertionError(f"{tag}: {len(bad)} of {Y.shape[0]} launches off, first {bad[:8]}, needle rows {rows}, "
                             f"worst |err| {float(d.nan_to_num(1e30).max()):.3e}")
    return float((d / P.ulp(y64, dt).clamp(min=2.0 ** -20 * vmax)).max())


def _rows_untouched(got, want, written):
    """every cache row outside `written` bit-identical (NaN rows included)"""
    keep = torch.ones(got.shape[-2], dtype=torch.bool, device=got.device)
    keep[written] = False
    return torch.equal(_bits(got)[..., keep, :], _bits(want)[..., keep, :])


# ---- one decode token ------------------------------------------------------------------------------------------------------

def _decode_launcher(L, entry, c, nsplit):
    """-> launch(kc, vc, y_ptr): one call of the entry point on case c (tensors on DEV), and the buffers its pointers refer to (the
    caller holds them for as long as it launches)"""
    n_head, n_kv, hd, S, code, st = c.n_head, c.n_kv, c.hd, c.S, runtime.dtype_code(c.dt), runtime.stream_ptr()
    p = torch.tensor([c.pos], device=DEV, dtype=torch.int32)
    msk = torch.zeros(n_head * hd // 64, device=DEV, dtype=torch.int64)
    ws = torch.full((n_head * max(nsplit, 1) * (hd + 2),), NAN, device=DEV, dtype=torch.float32)
    qkv, rope, q = c.qkv.contiguous(), c.rope.contiguous(), c.q.contiguous()
    slabs = torch.full((qkv.numel(), 4), 7.0, device=DEV, dtype=torch.float32)  # 2 slices of x / 2; the padding lanes are ignored
    slabs[:, :2] = (qkv.float() * 0.5)[:, None]
    keep = (p, msk, ws, qkv, rope, q, slabs)
    tail = (n_head, n_kv, hd, S, nsplit, ws.data_ptr(), ws.numel() * 4, code)
    calls = {
        "decode": lambda kc, vc, y: L.teal_decode_attention(qkv.data_ptr(), rope.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), y,
                                                            n_head, n_kv, hd, S, code, st),
        "masked": lambda kc, vc, y: L.teal_decode_attention_masked(qkv.data_ptr(), rope.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                                                   y, msk.data_ptr(), 0.02, n_head, n_kv, hd, S, code, st),
        "split": lambda kc, vc, y: L.teal_decode_attention_split(qkv.data_ptr(), rope.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                                                 y, msk.data_ptr(), 0.02, *tail, st),
        "slabs": lambda kc, vc, y: L.teal_decode_attention_split_slabs(slabs.data_ptr(), 2, rope.data_ptr(), p.data_ptr(), kc.data_ptr(),
                                                                       vc.data_ptr(), y, msk.data_ptr(), 0.02, *tail, st),
        "roped": lambda kc, vc, y: L.teal_decode_attention_split_roped(q.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), y,
                                                                       msk.data_ptr(), 0.02, *tail, None, 0, st),
    }
    return calls[entry], keep


def _run_decode(L, entry, shape, dt, nsplit=0, newest="background", peaked=False):
    """all launches of one case (one per needle set, or a single one), the cache checks, and the fp64 reference over the cache as
    the kernel left it.  -> (c, Y [launches, 1, H, hd], y64, emulation or None, vmax)"""
    n_head, n_kv, hd, pos, S = shape
    appended = entry != "roped"
    c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, appended=appended, newest=newest, peaked=peaked).to(DEV)
    launch, _buffers = _decode_launcher(L, entry, c, nsplit)
    kc, vc = c.kc.clone(), c.vc.clone()
    sets = c.sets
    n_launch = max(sets.shape[0], 1)
    Y = torch.full((n_launch, n_head * hd), NAN, device=DEV, dtype=dt)
    for i in range(n_launch):
        rows = sets[i] if sets.shape[0] else sets[:0, 0]
        kc[:, rows] = c.kappa[:, None, :]
        assert launch(kc, vc, Y[i].data_ptr()) == 0
        kc[:, rows] = c.kc[:, rows]
    torch.cuda.synchronize()
    if appended:  # the appended row: the module path's RoPE, bit for bit; nothing else moved
        k_ref = apply_rotary_emb(c.k_new.view(1, 1, n_kv, hd), c.rope[pos:pos + 1]).view(n_kv, hd)
        assert torch.equal(_bits(kc[:, pos]), _bits(k_ref)) and torch.equal(_bits(k_ref), _bits(c.k_row))
        assert torch.equal(_bits(vc[:, pos]), _bits(c.v_new))
    written = [pos] if appended else []
    assert _rows_untouched(kc, c.kc, written) and _rows_untouched(vc, c.vc, written)
    n = pos + 1
    K, V = kc[:, :n], vc[:, :n]
    vmax = float(V.float().abs().max())
    emu = None
    if sets.shape[0]:
        y64, outside = P.sweep_reference(c.q_rot, K, V, c.kappa, sets, c.visible, c.scale)
        assert float(outside.max()) < P.OUTSIDE_MAX, ("precondition", shape, float(outside.max()))
    else:
        y64, prob = P.attend64(c.q_rot, K, V, c.visible, c.scale)
        y64 = y64[None]
        if peaked:
            emu = P.attend_emulated(c.q_rot, K, V, c.visible, c.scale, dt)[None]
        elif newest == "needle":
            assert float((1 - prob[..., pos]).max()) < P.OUTSIDE_MAX, ("precondition", shape)
    return c, Y.view(n_launch, 1, n_head, hd), y64, emu, vmax


def _decode_needles(L, entry, shapes, dt, newest_only=False, sweep=True):
    for shape in shapes:
        nsplit = shape[5] if len(shape) > 5 else 0
        tag = f"{entry} {shape} {_name(dt)}"
        if sweep:
            c, Y, y64, _, vmax = _run_decode(L, entry, shape[:5], dt, nsplit)
            w = _check(tag + " sweep", Y, y64, vmax, dt, c.sets)
            print(f"PROBE needles {tag} launches={Y.shape[0]} m={c.sets.shape[1]} worst_ulps={w:.3f}")
        if newest_only:
            c, Y, y64, _, vmax = _run_decode(L, entry, shape[:5], dt, nsplit, newest="needle")
            w = _check(tag + " newest only", Y, y64, vmax, dt)
            want = c.v_new.double().repeat_interleave(c.n_head // c.n_kv, 0)
            assert float((y64[0, 0] - want).abs().max()) <= 2 * P.OUTSIDE_MAX * vmax  # the answer is v_new
            print(f"PROBE newest {tag} worst_ulps={w:.3f}")


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("entry", ["decode", "masked"])
def test_single_workgroup_needles(entry, dt):
    _decode_needles(_lib_ready(), entry, P.SINGLE, dt, newest_only=True)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_split_roped_needles(dt):
    """rotated q in, every row 0 .. pos already in the cache: all of them swept, the newest included"""
    _decode_needles(_lib_ready(), "roped", P.SPLIT, dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_split_needles(dt):
    _decode_needles(_lib_ready(), "split", P.SPLIT, dt, newest_only=True)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_split_slabs_needles(dt):
    L = _lib_ready()
    _decode_needles(L, "slabs", P.SPLIT + P.GQA[:1], dt, newest_only=True, sweep=False)
    _decode_needles(L, "slabs", P.SPLIT[1:2], dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_grouped_query_needles(dt):
    _decode_needles(_lib_ready(), "split", P.GQA, dt, newest_only=True)


# ---- T tokens: teal_verify_attention, teal_prefill_attention ---------------------------------------------------------------------

def _multi_launch(L, entry, c, slabs, rope, pos, kc, vc, y, parts):
    code, st = runtime.dtype_code(c.dt), runtime.stream_ptr()
    if entry == "verify":
        return L.teal_verify_attention(slabs.data_ptr(), 2, rope.data_ptr(), pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), y,
                                       parts.data_ptr(), parts.numel() * 4, c.T, c.n_head, c.n_kv, c.hd, c.S, code, st)
    assert c.p0 == 0
    return L.teal_prefill_attention(slabs.data_ptr(), 2, rope.data_ptr(), kc.data_ptr(), vc.data_ptr(), y, c.T, c.n_head, c.n_kv, c.hd,
                                    c.S, code, st)


def _run_multi(L, entry, heads, T, p0, dt, mode, peaked=False):
    n_head, n_kv, hd = heads
    S = P.MULTI_MAX_SEQ
    c = P.multi_case(n_head, n_kv, hd, T, p0, S, dt, seed=T * 2000 + p0, mode=mode, peaked=peaked).to(DEV)
    R = 8 if T <= 8 else 16
    slabs = P.slabs_of(c.qkv, R)
    rope = c.rope.contiguous()
    kc, vc = c.kc.clone()[None], c.vc.clone()[None]                # [1, n_kv, S, hd]
    pos = torch.tensor([p0], device=DEV, dtype=torch.int32)
    parts = torch.full((L.teal_verify_attention_ws_bytes(16, n_head, hd) // 4,), NAN, device=DEV, dtype=torch.float32)
    sets = c.sets
    n_launch = max(sets.shape[0], 1)
    Y = torch.full((n_launch, n_head * hd * 16), NAN, device=DEV, dtype=dt)
    for i in range(n_launch):
        rows = sets[i] if sets.shape[0] else sets[:0, 0]
        kc[0][:, rows] = c.kappa[:, None, :]
        rc = _multi_launch(L, entry, c, slabs, rope, pos, kc, vc, Y[i].data_ptr(), parts)
        assert rc == 0
        kc[0][:, rows] = c.kc[:, rows]
    torch.cuda.synchronize()
    new = list(range(p0, p0 + T))
    k_ref = apply_rotary_emb(c.k.unsqueeze(0), c.rope[p0:p0 + T])[0]                         # [T, n_kv, hd]
    assert torch.equal(_bits(kc[0][:, new]), _bits(k_ref.transpose(0, 1))) and torch.equal(_bits(k_ref), _bits(c.k_rows))
    assert torch.equal(_bits(vc[0][:, new]), _bits(c.v.transpose(0, 1)))
    assert _rows_untouched(kc[0], c.kc, new) and _rows_untouched(vc[0], c.vc, new)
    Yv = Y[:, :n_head * hd * R].view(n_launch, n_head * hd, R)
    assert not bool(Yv[:, :, T:].float().abs().sum() != 0), "slots >= T are zero"
    got = Yv[:, :, :T].transpose(1, 2).reshape(n_launch, T, n_head, hd)
    n = p0 + T
    K, V = kc[0][:, :n], vc[0][:, :n]
    vmax = float(V.float().abs().max())
    emu = None
    if sets.shape[0]:
        y64, outside = P.sweep_reference(c.q_rot, K, V, c.kappa, sets, c.visible, c.scale)
        assert float(outside.max()) < P.OUTSIDE_MAX, ("precondition", heads, T, p0, float(outside.max()))
    else:
        y64, prob = P.attend64(c.q_rot, K, V, c.visible, c.scale)
        if peaked:
            emu = P.attend_emulated(c.q_rot, K, V, c.visible, c.scale, dt)[None]
        elif mode == "staircase":
            own = torch.stack([prob[t, :, p0 + t] for t in range(T)])
            assert float((1 - own).max()) < P.OUTSIDE_MAX, ("precondition", heads, T, p0)
            want = c.v.double().repeat_interleave(n_head // n_kv, 1)
            assert float((y64 - want).abs().max()) <= 2 * P.OUTSIDE_MAX * vmax           # query t returns v_t
        y64 = y64[None]
    return c, got, y64, emu, vmax


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads", P.MULTI_HEADS)
def test_verify_staircase(heads, dt):
    L = _lib_ready()
    worst = 0.0
    for T in P.VERIFY_T:
        for p0 in P.verify_p0(T):
            c, got, y64, _, vmax = _run_multi(L, "verify", heads, T, p0, dt, "staircase")
            worst = max(worst, _check(f"verify staircase {heads} T={T} p0={p0} {_name(dt)}", got, y64, vmax, dt))
    print(f"PROBE staircase verify {heads} {_name(dt)} worst_ulps={worst:.3f}")


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads", P.MULTI_HEADS)
def test_prefill_staircase(heads, dt):
    L = _lib_ready()
    worst = 0.0
    for T in P.PREFILL_T:
        c, got, y64, _, vmax = _run_multi(L, "prefill", heads, T, 0, dt, "staircase")
        worst = max(worst, _check(f"prefill staircase {heads} T={T} {_name(dt)}", got, y64, vmax, dt))
    print(f"PROBE staircase prefill {heads} {_name(dt)} worst_ulps={worst:.3f}")


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads", P.MULTI_HEADS)
def test_verify_context_sweeps(heads, dt):
    L = _lib_ready()
    worst, launches = 0.0, 0
    for T in P.VERIFY_SWEEP_T:
        for p0 in P.verify_p0(T)[1:]:  # (p0 = 0 has no context row to sweep)
            c, got, y64, _, vmax = _run_multi(L, "verify", heads, T, p0, dt, "sweep")
            worst = max(worst, _check(f"verify sweep {heads} T={T} p0={p0} {_name(dt)}", got, y64, vmax, dt, c.sets))
            launches += got.shape[0]
    print(f"PROBE needles verify {heads} {_name(dt)} launches={launches} worst_ulps={worst:.3f}")


# ---- B sequences, one token each: teal_batched_decode_attention[_slots] -------------------------------------------------------------

def _batched_launch(L, c, slabs, rope, pos, act, kc, vc, y, part, nb, B):
    a = (slabs.data_ptr(), 2, rope.data_ptr(), pos.data_ptr())
    z = (kc.data_ptr(), vc.data_ptr(), y, part.data_ptr(), nb, B, c.n_head, c.n_kv, c.hd, c.S, runtime.dtype_code(c.dt), runtime.stream_ptr())
    return L.teal_batched_decode_attention(*a, *z) if act is None else L.teal_batched_decode_attention_slots(*a, act.data_ptr(), *z)


def _run_batched(L, heads, B, dt, salt, active=None, peaked=False, newest="background"):
    """newest = "needle": every sequence's k_new = unrope_pos(kappa) over a background cache, one launch, the answer is its v_new"""
    n_head, n_kv, hd = heads
    S = P.MULTI_MAX_SEQ
    positions = P.batched_positions(B, salt)
    cs = [P.decode_case(n_head, n_kv, hd, p, S, dt, seed=1000 * b + p + hd, peaked=peaked, newest=newest).to(DEV) for b, p in enumerate(positions)]
    kc0, vc0 = torch.stack([c.kc for c in cs]), torch.stack([c.vc for c in cs])   # [B, n_kv, S, hd]: own rows, own V per sequence
    kc, vc = kc0.clone(), vc0.clone()
    slabs = torch.full((2, cs[0].qkv.numel(), 8), 3.0, device=DEV, dtype=torch.float32)
    for b, c in enumerate(cs):
        slabs[:, :, b] = c.qkv.float() * 0.5
    rope = cs[0].rope.contiguous()
    pos = torch.tensor(positions, device=DEV, dtype=torch.int32)
    nb = int(L.teal_batched_decode_attention_ws_bytes(B, n_head, hd))
    part = torch.full(((nb + 3) // 4,), NAN, device=DEV, dtype=torch.float32)
    act = None if active is None else torch.tensor([active], device=DEV, dtype=torch.int32)
    on = [b for b in range(B) if active is None or (active >> b) & 1]
    n_launch = max(max(c.sets.shape[0] for c in cs), 1)
    Y = torch.full((n_launch, n_head * hd, 8), NAN, device=DEV, dtype=dt)
    for i in range(n_launch):  # launch i: sequence b's needle set i mod its own number of sets
        for b, c in enumerate(cs):
            if c.sets.shape[0]:
                kc[b][:, c.sets[i % c.sets.shape[0]]] = c.kappa[:, None, :]
        rc = _batched_launch(L, cs[0], slabs, rope, pos, act, kc, vc, Y[i].data_ptr(), part, nb, B)
        assert rc == 0
        for b, c in enumerate(cs):
            if c.sets.shape[0]:
                rows = c.sets[i % c.sets.shape[0]]
                kc[b][:, rows] = c.kc[:, rows]
    torch.cuda.synchronize()
    assert not bool(Y[:, :, B:].float().abs().sum() != 0), "slots >= B are zero"
    out = []
    for b, c in enumerate(cs):
        p = c.pos
        if b not in on:  # an inactive slot: yt zero in every launch, its caches untouched
            assert not bool(Y[:, :, b].float().abs().sum() != 0)
            assert torch.equal(_bits(kc[b]), _bits(kc0[b])) and torch.equal(_bits(vc[b]), _bits(vc0[b]))
            continue
        k_ref = apply_rotary_emb(c.k_new.view(1, 1, n_kv, hd), c.rope[p:p + 1]).view(n_kv, hd)
        assert torch.equal(_bits(kc[b][:, p]), _bits(k_ref)) and torch.equal(_bits(vc[b][:, p]), _bits(c.v_new))
        assert _rows_untouched(kc[b], kc0[b], [p]) and _rows_untouched(vc[b], vc0[b], [p])
        K, V = kc[b][:, :p + 1], vc[b][:, :p + 1]
        vmax = float(V.float().abs().max())
        got = Y[:, :, b].reshape(n_launch, 1, n_head, hd)
        emu = None
        if c.sets.shape[0]:
            y64, outside = P.sweep_reference(c.q_rot, K, V, c.kappa, c.sets, c.visible, c.scale)
            assert float(outside.max()) < P.OUTSIDE_MAX, ("precondition", heads, b, p)
            y64 = y64[torch.arange(n_launch, device=DEV) % c.sets.shape[0]]
        else:
            y64, prob = P.attend64(c.q_rot, K, V, c.visible, c.scale)
            if peaked:
                emu = P.attend_emulated(c.q_rot, K, V, c.visible, c.scale, dt)[None]
            elif newest == "needle":
                assert float((1 - prob[..., p]).max()) < P.OUTSIDE_MAX, ("precondition", heads, b, p)
                want = c.v_new.double().repeat_interleave(n_head // n_kv, 0)
                assert float((y64[0] - want).abs().max()) <= 2 * P.OUTSIDE_MAX * vmax  # the answer is v_new
            y64 = y64[None].expand(n_launch, 1, n_head, hd)
        out.append((b, c, got, y64, emu, vmax))
    return out


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads,Bs", [((32, 32, 128), (3,)), ((32, 8, 128), (1, 3, 8)), ((8, 8, 64), (1, 8)), ((8, 2, 64), (3, 8))])
def test_batched_needles(heads, Bs, dt):
    L = _lib_ready()
    for B in Bs:
        worst = 0.0
        for b, c, got, y64, _, vmax in _run_batched(L, heads, B, dt, salt=B):
            worst = max(worst, _check(f"batched {heads} B={B} seq {b} pos {c.pos} {_name(dt)}", got, y64, vmax, dt, c.sets))
        print(f"PROBE needles batched {heads} B={B} {_name(dt)} worst_ulps={worst:.3f}")
        worst = 0.0  # the appended row, a probe of its own: the row each sequence builds is its only dominant key
        for b, c, got, y64, _, vmax in _run_batched(L, heads, B, dt, salt=B, newest="needle"):
            worst = max(worst, _check(f"batched newest only {heads} B={B} seq {b} pos {c.pos} {_name(dt)}", got, y64, vmax, dt))
        print(f"PROBE newest batched {heads} B={B} {_name(dt)} worst_ulps={worst:.3f}")


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads,B,active", [((32, 8, 128), 8, 0b10110101), ((8, 2, 64), 3, 0b101), ((8, 8, 64), 8, 0b01001010), ((32, 32, 128), 3, 0b110)])
def test_batched_slots_needles(heads, B, active, dt):
    """a mixed active mask: active slots at 1 ulp, inactive slots' yt zero and caches untouched (checked in _run_batched)"""
    L = _lib_ready()
    worst = 0.0
    res = _run_batched(L, heads, B, dt, salt=B + 1, active=active)
    assert len(res) == bin(active).count("1")
    for b, c, got, y64, _, vmax in res:
        worst = max(worst, _check(f"slots {heads} B={B} seq {b} pos {c.pos} {_name(dt)}", got, y64, vmax, dt, c.sets))
    print(f"PROBE needles slots {heads} B={B} active={active:#b} {_name(dt)} worst_ulps={worst:.3f}")
    worst = 0.0
    res = _run_batched(L, heads, B, dt, salt=B + 1, active=active, newest="needle")
    assert len(res) == bin(active).count("1")
    for b, c, got, y64, _, vmax in res:
        worst = max(worst, _check(f"slots newest only {heads} B={B} seq {b} pos {c.pos} {_name(dt)}", got, y64, vmax, dt))
    print(f"PROBE newest slots {heads} B={B} active={active:#b} {_name(dt)} worst_ulps={worst:.3f}")


# ---- part 2: peaked random inputs ---------------------------------------------------------------------------------------------

def _peaked(tag, got, y64, emu, dt):
    e_k, e_e = P.err_rel(got, y64), P.err_rel(emu, y64)
    bound = P.peaked_bound(e_e, dt)
    print(f"PROBE peaked {tag} {_name(dt)} err_kernel={e_k:.3e} err_emulation={e_e:.3e} bound={bound:.3e}")
    assert e_k <= bound, (tag, e_k, e_e, bound)


PEAKED_DECODE = [("decode", P.SINGLE[1]), ("decode", P.SINGLE[4]), ("masked", P.SINGLE[1]), ("masked", P.SINGLE[4]),
                 ("roped", P.SPLIT[1]), ("roped", P.SPLIT[3]), ("roped", P.SPLIT[5]),
                 ("split", P.SPLIT[1]), ("split", P.SPLIT[3]), ("split", P.SPLIT[5]),
                 ("slabs", P.SPLIT[1]), ("slabs", P.SPLIT[5]),
                 ("split", P.GQA[0]), ("split", P.GQA[1]), ("split", P.GQA[2]), ("slabs", P.GQA[2])]


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_peaked_decode(dt):
    L = _lib_ready()
    for entry, shape in PEAKED_DECODE:
        c, Y, y64, emu, _ = _run_decode(L, entry, shape[:5], dt, shape[5] if len(shape) > 5 else 0, peaked=True)
        _peaked(f"{entry} {shape}", Y, y64, emu, dt)


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_peaked_multi_token_and_batched(dt):
    L = _lib_ready()
    for heads in P.MULTI_HEADS:
        for T, p0 in ((9, 33), (16, 1000)):
            c, got, y64, emu, _ = _run_multi(L, "verify", heads, T, p0, dt, "sweep", peaked=True)
            _peaked(f"verify {heads} T={T} p0={p0}", got, y64, emu, dt)
        for T in (2, 5, 16):
            c, got, y64, emu, _ = _run_multi(L, "prefill", heads, T, 0, dt, "sweep", peaked=True)
            _peaked(f"prefill {heads} T={T}", got, y64, emu, dt)
    for heads, B, active in (((32, 8, 128), 3, None), ((8, 2, 64), 8, None), ((8, 8, 64), 8, 0b11011011), ((32, 8, 128), 8, 0b01111101),
                             ((8, 2, 64), 8, 0b10101110), ((32, 32, 128), 3, 0b111)):
        for b, c, got, y64, emu, _ in _run_batched(L, heads, B, dt, salt=2, active=active, peaked=True):
            _peaked(f"batched{'_slots' if active else ''} {heads} B={B} seq {b} pos {c.pos}", got, y64, emu, dt)

"""CPU: the attention probes' own power (tests/attention_probes.py).  Nothing is launched: fault models are applied to the fp64
reference only, and each must be REJECTED by the bound of the part meant to catch it — a later edit of the inputs cannot quietly
make the probes powerless.

  * part 1 (equal needles, 1 ulp): a dropped needle (first, middle, last), a dropped newest row, a dropped row group, a dropped
    split, a row counted twice, reading row pos + 1, the causal mask one too wide / too narrow, a query head reading the
    neighbouring KV head;
  * part 2 (peaked inputs, 2 err(emulation) + 2^-10 / 2^-7): the 64 <-> 128 scale swap, scale x 1.05, a lost eighth of the rows;
  * the 16-bit emulation (scores, probabilities, output rounded; fp32 sums) is ACCEPTED by both bounds;
  * the dominance precondition (fp64 softmax weight outside the needle set < 2^-16) for every shape the GPU tests launch.
"""
import math

import pytest
import torch

import attention_probes as P

DTS = [torch.float16, torch.bfloat16]


def _rejected(y, y64, vmax, dt):
    """what the GPU tests assert is `(|y - y64| <= tol).all()`: a NaN fails it too"""
    return not bool(((y.double() - y64).abs() <= P.tol_needle(y64, vmax, dt)).all())


def _vmax(vc, n):
    return float(vc[:, :n].float().abs().max())


def _some_sets(sets):
    n = sets.shape[0]
    return sorted({0, n // 2, n - 1})


def test_sets_partition_the_rows():
    for n in (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 255, 256, 300, 700, 1000, 1024, 1039, 2047, 4095, 4096, 4097, 5000, 5001, 16000):
        sets = P.strided_sets(n)
        n_sets, m = sets.shape
        assert m & (m - 1) == 0 and m <= 64 and n_sets <= 256 and n_sets == -(-n // m)
        assert m == (64 if n > 4096 else 16) or n < 16
        owner = torch.zeros(n, dtype=torch.long)
        for i in range(n_sets):
            rows = sets[i]
            assert len(set(rows.tolist())) == m                      # m DISTINCT needles
            own = rows[rows % n_sets == i]
            owner[own] += 1
            assert own.tolist() == list(range(i, n, n_sets))          # row r is a needle of launch r mod n_sets
        assert bool((owner == 1).all())


def test_ulp_and_tolerance():
    y = torch.tensor([1.0, 1.5, 0.75, 2.0 ** -30, 0.0, -3.0], dtype=torch.float64)
    assert P.ulp(y, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]
    assert P.ulp(y, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -37, 2.0 ** -133, 2.0 ** -6]
    for dt in DTS:  # the format's own spacing, from torch
        x = torch.tensor([0.3, 1.7, 77.0]).to(dt)
        nxt = (x.view(torch.int16) + 1).view(dt)
        assert torch.equal(P.ulp(x.double(), dt), (nxt.double() - x.double()))


@pytest.mark.parametrize("dt", DTS)
def test_dominance_decode_shapes(dt):
    """every sweep of the single-workgroup, split and grouped-query tables: weight outside ANY needle set < 2^-16, both for
    a kernel that rotates q itself (appended) and for the rotated hand-over; the newest-only probes as well"""
    for n_head, n_kv, hd, pos, S in list(P.SINGLE) + [c[:5] for c in P.SPLIT + P.GQA]:
        for appended in (True, False):
            c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, appended=appended)
            kc, _ = P.finished_cache(c)
            if c.sets.shape[0]:
                out = P.outside_upper_bound(c.q_rot, kc, c.kappa, pos + 1, c.sets.shape[1], c.scale)
                assert float(out.max()) < P.OUTSIDE_MAX, (n_head, n_kv, hd, pos, float(out.max()))
        c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, newest="needle")
        kc, vc = P.finished_cache(c)
        y64, p = P.attend64(c.q_rot, kc[:, :pos + 1], vc[:, :pos + 1], c.visible, c.scale)
        assert float((1 - p[..., pos]).max()) < P.OUTSIDE_MAX
        rep = n_head // n_kv
        assert float((y64[0] - c.v_new.double().repeat_interleave(rep, 0)).abs().max()) <= 2 * P.OUTSIDE_MAX * _vmax(vc, pos + 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n_head,n_kv,hd", P.MULTI_HEADS)
def test_dominance_multi_token_shapes(n_head, n_kv, hd, dt):
    S = P.MULTI_MAX_SEQ
    for T in sorted(set(P.VERIFY_T + P.PREFILL_T)):
        for p0 in P.verify_p0(T):
            if T in P.VERIFY_T or p0 == 0:
                c = P.multi_case(n_head, n_kv, hd, T, p0, S, dt, seed=T * 2000 + p0, mode="staircase")
                kc, vc = P.finished_multi_cache(c)
                _, p = P.attend64(c.q_rot, kc[:, :p0 + T], vc[:, :p0 + T], c.visible, c.scale)
                own = torch.stack([p[t, :, p0 + t] for t in range(T)])
                assert float((1 - own).max()) < P.OUTSIDE_MAX, (T, p0, float((1 - own).max()))
            if T in P.VERIFY_SWEEP_T and p0 > 0:
                c = P.multi_case(n_head, n_kv, hd, T, p0, S, dt, seed=T * 2000 + p0, mode="sweep")
                kc, _ = P.finished_multi_cache(c)
                out = P.outside_upper_bound(c.q_rot, kc, c.kappa, p0 + T, c.sets.shape[1], c.scale)
                assert float(out.max()) < P.OUTSIDE_MAX, (T, p0, float(out.max()))
    for B, salt in [(B, B + d) for B in P.BATCHED_B for d in (0, 1)]:  # the batched (salt B) and slot (B + 1) launches' sequences
        for b, pos in enumerate(P.batched_positions(B, salt)):
            c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=1000 * b + pos + hd)
            if c.sets.shape[0]:
                out = P.outside_upper_bound(c.q_rot, P.finished_cache(c)[0], c.kappa, pos + 1, c.sets.shape[1], c.scale)
                assert float(out.max()) < P.OUTSIDE_MAX, (B, b, pos, float(out.max()))
            c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=1000 * b + pos + hd, newest="needle")  # ... and its newest-only probe
            kc, vc = P.finished_cache(c)
            y64, p = P.attend64(c.q_rot, kc[:, :pos + 1], vc[:, :pos + 1], c.visible, c.scale)
            assert float((1 - p[..., pos]).max()) < P.OUTSIDE_MAX, (B, b, pos)
            want = c.v_new.double().repeat_interleave(n_head // n_kv, 0)
            assert float((y64[0] - want).abs().max()) <= 2 * P.OUTSIDE_MAX * _vmax(vc, pos + 1)
            w = torch.ones(pos + 1, dtype=torch.float64)
            w[pos] = 0  # a batched launch that loses the row it appended is rejected (at pos 0 it has nothing left: NaN)
            assert _rejected(P.attend64(c.q_rot, kc[:, :pos + 1], vc[:, :pos + 1], c.visible, c.scale, weights=w)[0], y64,
                             _vmax(vc, pos + 1), dt), (B, b, pos)


# ---- part 1 ----------------------------------------------------------------------------------------------------------------

NEEDLE_CASES = [(8, 2, 128, 256, 512, 16, 4),        # (n_head, n_kv, hd, pos, S, rows per group, splits): grouped heads, m = 16
                (4, 4, 64, 5000, 8192, 128, 3)]      # m = 64, ragged splits


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("appended", [True, False])
@pytest.mark.parametrize("shape", NEEDLE_CASES)
def test_needle_sweep_rejects_row_faults(shape, appended, dt):
    n_head, n_kv, hd, pos, S, step, nsplit = shape
    c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, appended=appended)
    kc, vc = P.finished_cache(c)
    n = pos + 1
    K, V, vmax = kc[:, :n], vc[:, :n], _vmax(vc, n)
    n_sets, m = c.sets.shape
    assert m == (16 if pos <= 4096 else 64)
    ones = torch.ones(n, dtype=torch.float64)
    for i in _some_sets(c.sets):
        rows = c.sets[i]
        sub = c.sets[i:i + 1]
        y64, out = P.sweep_reference(c.q_rot, K, V, c.kappa, sub, c.visible, c.scale)
        y64 = y64[0]
        assert float(out.max()) < P.OUTSIDE_MAX
        mean = V.double()[:, rows].mean(1).repeat_interleave(n_head // n_kv, 0)
        assert float((y64[0] - mean).abs().max()) <= 2 * float(out.max()) * vmax + 1e-15  # the exact answer is mean(V[R])
        # the emulation of the module path's roundings is accepted
        emu, _ = P.sweep_reference(c.q_rot, K, V, c.kappa, sub, c.visible, c.scale, fn=P.attend_emulated, dt=dt)
        assert not _rejected(emu[0], y64, vmax, dt)
        e_emu = float(((emu[0].double() - y64).abs() / P.tol_needle(y64, vmax, dt)).max())
        assert e_emu <= 0.75

        def fault(w=None, **kw):
            y, _ = P.sweep_reference(c.q_rot, kw.pop("K", K), kw.pop("V", V), c.kappa, sub, kw.pop("visible", c.visible), c.scale,
                                     weights=w, **kw)
            return _rejected(y[0], y64, vmax, dt)

        assert not fault(ones)
        for r in (rows[0], rows[m // 2], rows[-1]):              # a needle lost, a needle counted twice
            w = ones.clone()
            w[r] = 0
            assert fault(w), ("dropped needle", int(r))
            lost = P.sweep_reference(c.q_rot, K, V, c.kappa, sub, c.visible, c.scale, weights=w)[0][0]
            print(f"PROBE host needles {shape[:5]} {'appended' if appended else 'roped'} {dt} set {i} m={m} outside={float(out.max()):.1e} "
                  f"emulation/bound={e_emu:.3f} lost_needle_{int(r)}/bound={float(((lost - y64).abs() / P.tol_needle(y64, vmax, dt)).max()):.0f}")
            w[r] = 2
            assert fault(w), ("doubled needle", int(r))
        g = int(rows[m // 2]) // step                            # the row group / the split that holds a needle of this set
        w = ones.clone()
        w[g * step:(g + 1) * step] = 0
        assert fault(w), ("dropped row group", g)
        w = ones.clone()
        w[(torch.arange(n) // step) % nsplit == g % nsplit] = 0
        assert fault(w), ("dropped split", g % nsplit)
        # one row too far: the guard row pos + 1 (kappa, V = 100)
        assert fault(torch.ones(n + 1, dtype=torch.float64), K=kc[:, :n + 1], V=vc[:, :n + 1], visible=[n + 1]), "read row pos + 1"
        if n_kv > 1:
            assert fault(ones, kv_shift=1) and fault(ones, kv_shift=-1), "neighbouring KV head"
    # every row group and every split holds a needle of some launch: a lost one cannot hide
    groups = -(-pos // step)
    assert {int(r) // step for r in c.sets.view(-1)} == set(range(groups if appended else -(-n // step)))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(4, 2, 64, 0, 64), (8, 2, 128, 256, 512), (16, 4, 64, 4095, 4096)])
def test_newest_only_rejects_a_dropped_newest_row(shape, dt):
    n_head, n_kv, hd, pos, S = shape
    c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, newest="needle")
    kc, vc = P.finished_cache(c)
    n = pos + 1
    vmax = _vmax(vc, n)
    y64, _ = P.attend64(c.q_rot, kc[:, :n], vc[:, :n], c.visible, c.scale)
    emu = P.attend_emulated(c.q_rot, kc[:, :n], vc[:, :n], c.visible, c.scale, dt)
    assert not _rejected(emu, y64, vmax, dt)
    w = torch.ones(n, dtype=torch.float64)
    w[pos] = 0                                                    # `t < pos` where `t <= pos` is meant
    assert _rejected(P.attend64(c.q_rot, kc[:, :n], vc[:, :n], c.visible, c.scale, weights=w)[0], y64, vmax, dt)
    if n < S:  # (the last row of the cache has no row behind it)
        y_far, _ = P.attend64(c.q_rot, kc[:, :n + 1], vc[:, :n + 1], [n + 1], c.scale)
        assert _rejected(y_far, y64, vmax, dt), "read row pos + 1"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n_head,n_kv,hd", [(32, 8, 128), (8, 2, 64)])
def test_staircase_rejects_a_causal_mask_off_by_one(n_head, n_kv, hd, dt):
    S = P.MULTI_MAX_SEQ
    for T, p0 in ((1, 0), (2, 33), (9, 0), (16, 1000), (16, S - 16)):
        c = P.multi_case(n_head, n_kv, hd, T, p0, S, dt, seed=T * 2000 + p0, mode="staircase")
        kc, vc = P.finished_multi_cache(c)
        n = p0 + T
        vmax = _vmax(vc, n)
        y64, _ = P.attend64(c.q_rot, kc[:, :n], vc[:, :n], c.visible, c.scale)
        want = c.v.double().repeat_interleave(n_head // n_kv, 1)
        assert float((y64 - want).abs().max()) <= 2 * P.OUTSIDE_MAX * vmax     # query t returns v_t
        assert not _rejected(P.attend_emulated(c.q_rot, kc[:, :n], vc[:, :n], c.visible, c.scale, dt), y64, vmax, dt)
        n1 = min(n + 1, S)
        wide, _ = P.attend64(c.q_rot, kc[:, :n1], vc[:, :n1], [v + 1 for v in c.visible], c.scale)
        narrow, _ = P.attend64(c.q_rot, kc[:, :n], vc[:, :n], [v - 1 for v in c.visible], c.scale)
        tol = P.tol_needle(y64, vmax, dt)
        for t in range(T):  # EVERY query notices (the last one through the guard row, where the cache has one)
            if t < T - 1 or n < S:
                assert not bool(((wide[t] - y64[t]).abs() <= tol[t]).all()), ("mask one too wide", T, p0, t)
            assert not bool(((narrow[t] - y64[t]).abs() <= tol[t]).all()), ("mask one too narrow", T, p0, t)


@pytest.mark.parametrize("dt", DTS)
def test_context_sweep_of_a_multi_token_launch_rejects_a_lost_row(dt):
    n_head, n_kv, hd, T, p0, S = 8, 2, 64, 9, 1000, P.MULTI_MAX_SEQ
    c = P.multi_case(n_head, n_kv, hd, T, p0, S, dt, seed=T * 2000 + p0, mode="sweep")
    kc, vc = P.finished_multi_cache(c)
    n = p0 + T
    vmax = _vmax(vc, n)
    for i in _some_sets(c.sets):
        sub = c.sets[i:i + 1]
        y64, out = P.sweep_reference(c.q_rot, kc[:, :n], vc[:, :n], c.kappa, sub, c.visible, c.scale)
        assert float(out.max()) < P.OUTSIDE_MAX
        emu, _ = P.sweep_reference(c.q_rot, kc[:, :n], vc[:, :n], c.kappa, sub, c.visible, c.scale, fn=P.attend_emulated, dt=dt)
        assert not _rejected(emu[0], y64[0], vmax, dt)
        w = torch.ones(n, dtype=torch.float64)
        w[sub[0, 3]] = 0
        bad, _ = P.sweep_reference(c.q_rot, kc[:, :n], vc[:, :n], c.kappa, sub, c.visible, c.scale, weights=w)
        tol = P.tol_needle(y64[0], vmax, dt)
        for t in range(T):  # kappa is the same for all T queries: every one of them notices
            assert not bool(((bad[0, t] - y64[0, t]).abs() <= tol[t]).all())


# ---- part 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(4, 2, 64, 63, 64), (8, 2, 128, 256, 512), (4, 4, 64, 5000, 8192), (16, 2, 128, 2047, 2048)])
def test_peaked_inputs_reject_softmax_faults(shape, dt):
    n_head, n_kv, hd, pos, S = shape
    c = P.decode_case(n_head, n_kv, hd, pos, S, dt, seed=pos + hd, peaked=True)
    kc, vc = P.finished_cache(c)
    n = pos + 1
    K, V = kc[:, :n], vc[:, :n]
    y64, p = P.attend64(c.q_rot, K, V, c.visible, c.scale)
    e_emu = P.err_rel(P.attend_emulated(c.q_rot, K, V, c.visible, c.scale, dt), y64)
    bound = P.peaked_bound(e_emu, dt)
    assert e_emu <= bound and e_emu < (2.0 ** -7 if dt == torch.float16 else 2.0 ** -4), e_emu
    assert 0.1 < float(y64.abs().amax(-1).min()) and float(y64.abs().max()) < 4.0  # every head's output is O(0.1 .. 1), not O(1 / sqrt(pos))
    other = 1.0 / math.sqrt(192 - hd)                                                        # 64 <-> 128
    faults = {"scale swap": P.attend64(c.q_rot, K, V, c.visible, other)[0],
              "scale x 1.05": P.attend64(c.q_rot, K, V, c.visible, c.scale * 1.05)[0]}
    w = torch.ones(n, dtype=torch.float64)
    w[torch.arange(n) * 8 // n == 7] = 0
    faults["lost eighth"] = P.attend64(c.q_rot, K, V, c.visible, c.scale, weights=w)[0]
    print(f"PROBE host peaked {shape} {dt} err_emulation={e_emu:.2e} bound={bound:.2e} "
          + " ".join(f"{name.replace(' ', '_')}={P.err_rel(y, y64):.3f}" for name, y in faults.items()))
    for name, y in faults.items():
        assert P.err_rel(y, y64) > bound, (name, P.err_rel(y, y64), bound)

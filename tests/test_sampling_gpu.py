"""GPU: teal_sample_rows (teal_amd/csrc/teal_sample_rows.hip) through the C ABI against the host model (tests/sampling_rule.py).

The inputs are tests/sampling_cases.py's — the bits tests/test_sampling_rule_host.py checks the model's share of open rows on.

  1. kept_out is the model's count; on a row the model calls open, any of its legitimate counts;
  2. the token is the model's draw from the kept set that count identifies, or its runner-up where the race itself is open
     (sampler_rule's rule: at most 2 % of the draws);
  3. with top_p = 1 and min_p = 0 the tokens are teal_sample_topk_slot's over 64 consecutive draws, every one;
  4. a row's results do not depend on B, slot0, its position, its neighbours' logits or their parameters;
  5. a cleared active bit leaves token, position, counter, history and kept_out alone;
  6. the epilogue: counter, position, the history entry at the draw counter, the history guard;
  7. 50 replays of a captured launch give the tokens of 50 eager launches from the same start.
"""
import numpy as np
import pytest
import torch

import sampling_cases as SC
import sampling_rule as R
from teal_amd.gpt_fast.sampling import check_sampling, row_words

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77
POS0 = 11
N_DRAWS = 4


def _lib_rt():
    from teal_amd import _lib, runtime
    L = _lib.load()
    runtime.init()
    return L, runtime


def _upload(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).to(DEV)


def _params(rows) -> torch.Tensor:
    return torch.stack([row_words(check_sampling(*p)) for p in rows]).to(DEV)


class _Launch:
    """one teal_sample_rows call's buffers: B rows drawn n times from seed SEED + row, counter c0"""

    def __init__(self, L, runtime, bits, bf16, params, n=N_DRAWS, c0=0, slot0=0, active=None, hist_len=None, seeds=None):
        self.bits, self.bf16, self.rows, self.n, self.c0 = np.atleast_2d(bits), bf16, list(params), n, c0
        B, V = self.bits.shape
        self.B, self.V = B, V
        self.seeds = list(seeds) if seeds is not None else [SC.SEED + r for r in range(B)]
        self.hist_len = n + c0 + 1 if hist_len is None else hist_len
        self.lg = _upload(self.bits)
        self.pr = _params(self.rows)
        self.state = torch.tensor([[s, c0] for s in self.seeds], dtype=torch.int64, device=DEV)
        self.tok = torch.full((n, B), SENT, dtype=torch.int32, device=DEV)
        self.kept = torch.full((n, B), SENT, dtype=torch.int32, device=DEV)
        self.hist_all = torch.full((B * self.hist_len + 4,), SENT, dtype=torch.int32, device=DEV)  # rows history_len apart + a guard
        self.hist = self.hist_all[:B * self.hist_len].view(B, self.hist_len)
        self.pos = torch.full((B,), POS0, dtype=torch.int32, device=DEV)
        self.active = active
        code = 1 if bf16 else 0
        for j in range(n):
            rc = L.teal_sample_rows(self.lg.data_ptr(), V, V, code, B, self.pr.data_ptr(), self.state.data_ptr(),
                                    self.tok[j].data_ptr(), self.pos.data_ptr(), self.hist_all.data_ptr(), self.hist_len,
                                    self.kept[j].data_ptr(), active.data_ptr() if active is not None else None, slot0,
                                    runtime.stream_ptr())
            assert rc == 0, rc

    def read(self):
        """after a synchronize: (tokens [n][B], kept [n][B])"""
        return self.tok.cpu().numpy(), self.kept.cpu().numpy()


class _Tally:
    def __init__(self):
        self.draws = self.open = 0
        self.bad = []

    def check(self, label, run: _Launch, rows=None):
        tok, kept = run.read()
        state, pos, hist = run.state.cpu().numpy(), run.pos.cpu().numpy(), run.hist.cpu().numpy()
        for r in (range(run.B) if rows is None else rows):
            T, k, p, m = run.rows[r]
            _, count, is_open, counts = R.kept(run.bits[r], run.bf16, T, k, p, m)
            got = int(kept[0, r])
            if not (kept[:, r] == got).all() or got not in counts:
                self.bad.append((label, r, "kept", kept[:, r].tolist(), counts))
                continue
            want, ru, op = R.draws_from(run.bits[r], run.bf16, got, T, run.seeds[r], run.c0, run.n)
            self.draws += run.n
            self.open += int(op.sum())
            miss = (tok[:, r] != want) & ~(op & (tok[:, r] == ru))
            if miss.any():
                self.bad.append((label, r, "token", tok[:, r].tolist(), want.tolist(), ru.tolist(), op.tolist()))
            # the epilogue: seed kept, counter + n, position + n, the history entry at the draw counter
            wh = np.full(hist.shape[1], SENT, dtype=np.int32)
            for j in range(run.n):
                if run.c0 + j < hist.shape[1]:
                    wh[run.c0 + j] = tok[j, r]
            tail_ok = bool((run.hist_all[run.B * run.hist_len:] == SENT).all())
            if state[r].tolist() != [run.seeds[r], run.c0 + run.n] or pos[r] != POS0 + run.n or not np.array_equal(hist[r], wh) or not tail_ok:
                self.bad.append((label, r, "epilogue", state[r].tolist(), int(pos[r]), hist[r].tolist()))

    def clean(self):
        assert not self.bad, self.bad[:4]
        assert self.open <= 0.02 * self.draws, (self.open, self.draws)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("V", SC.VOCABS)
def test_rows_draw_the_models_tokens_from_the_models_kept_sets(V, dtype):
    L, runtime = _lib_rt()
    bf16 = dtype == "bf16"
    rows = SC.random_rows(V, bf16)
    runs = {"mixed": _Launch(L, runtime, rows, bf16, SC.MIXED)}
    for g in SC.GRID:
        runs[g] = _Launch(L, runtime, rows, bf16, [g] * SC.N_ROWS)
    special = SC.special_rows(V, bf16)
    for params in SC.GRID[:2] + SC.GRID[4:]:
        runs["special", params] = _Launch(L, runtime, np.stack([b for _, b in special]), bf16, [params] * len(special), c0=3)
    # the same rows one at a time (B = 1, another slot0, an active word with that bit set) and in reverse order: nothing may move
    rev = _Launch(L, runtime, rows[::-1], bf16, SC.MIXED[::-1], seeds=[SC.SEED + r for r in range(SC.N_ROWS)][::-1])
    active = torch.tensor([1 << 5], dtype=torch.int32, device=DEV)
    single = [_Launch(L, runtime, rows[r], bf16, [SC.MIXED[r]], slot0=5, active=active, seeds=[SC.SEED + r]) for r in (0, 1, 6, 7)]
    torch.cuda.synchronize()
    tally = _Tally()
    for label, run in runs.items():
        tally.check((V, dtype, label), run)
    tally.clean()
    tok, kept = runs["mixed"].read()
    rt, rk = rev.read()
    assert np.array_equal(rt[:, ::-1], tok) and np.array_equal(rk[:, ::-1], kept)
    for r, run in zip((0, 1, 6, 7), single):
        st, sk = run.read()
        assert np.array_equal(st[:, 0], tok[:, r]) and np.array_equal(sk[:, 0], kept[:, r]), r
    # the filters did something: the kept counts of the mixed rows differ, the unfiltered row kept everything
    assert kept[0, 0] == V and (V == 8 or len(set(kept[0].tolist())) > 3)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_hand_worked_rows_keep_their_counts(dtype):
    L, runtime = _lib_rt()
    bf16 = dtype == "bf16"
    bits = np.stack([SC.hand_bits(v, bf16) for _, v, _, _ in SC.HAND])
    run = _Launch(L, runtime, bits, bf16, [p for _, _, p, _ in SC.HAND], n=8)
    torch.cuda.synchronize()
    tally = _Tally()
    tally.check(dtype, run)
    tally.clean()
    tok, kept = run.read()
    assert kept[0].tolist() == [w for _, _, _, w in SC.HAND]
    x = np.array([v for _, v, _, _ in SC.HAND])
    for r, (_, v, _, want) in enumerate(SC.HAND):  # every draw comes from the `want` largest values
        assert (x[r][tok[:, r]] >= np.sort(x[r])[::-1][want - 1]).all(), r


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("V", SC.VOCABS)
def test_without_top_p_and_min_p_the_tokens_are_the_top_k_samplers(V, dtype):
    """64 consecutive draws, every one equal: bit-equal scores, not agreement outside close races"""
    L, runtime = _lib_rt()
    bf16, code, n = dtype == "bf16", int(dtype == "bf16"), 64
    row = SC.random_rows(V, bf16)[0]
    lg = _upload(row)
    active = torch.tensor([1 << 2], dtype=torch.int32, device=DEV)
    ws = runtime.new_workspace(64, 64)
    keep = []
    for T, k in ((0.8, min(200, V - 1)), (0.8, 0), (1.3, 5), (1e-6, 0)):
        run = _Launch(L, runtime, row, bf16, [(T, k, 1.0, 0.0)], n=n, slot0=2, active=active, hist_len=n + 2, seeds=[SC.SEED])
        for use_ws in (False, True):
            state = torch.tensor([SC.SEED, 0], dtype=torch.int64, device=DEV)
            tok = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
            pos = torch.full((1,), POS0, dtype=torch.int32, device=DEV)
            hist = torch.full((n + 2,), SENT, dtype=torch.int32, device=DEV)
            for j in range(n):
                assert L.teal_sample_topk_slot(lg.data_ptr(), V, code, k, T, state.data_ptr(), tok.data_ptr() + 4 * j, pos.data_ptr(),
                                               hist.data_ptr(), n + 2, ws.data_ptr() if use_ws else None, ws.numel() * 4 if use_ws else 0,
                                               active.data_ptr(), 2, runtime.stream_ptr()) == 0
            keep.append((T, k, use_ws, run, tok, hist, pos, state))
    torch.cuda.synchronize()
    for T, k, use_ws, run, tok, hist, pos, state in keep:
        got, kept = run.read()
        assert got[:, 0].tolist() == tok.tolist(), (T, k, use_ws)
        assert run.hist[0].tolist() == hist.tolist() and run.pos.tolist() == pos.tolist() and run.state[0].tolist() == state.tolist()
        assert (kept == int(R.kept(row, bf16, T, k)[1])).all()


def test_a_cleared_active_bit_leaves_the_row_alone():
    L, runtime = _lib_rt()
    V, bf16 = 8200, False
    rows = SC.random_rows(V, bf16)[:3]
    params = [SC.MIXED[1], SC.MIXED[6], SC.MIXED[7]]
    active = torch.tensor([0b101 << 4], dtype=torch.int32, device=DEV)  # slots 4 and 6 on, slot 5 off
    run = _Launch(L, runtime, rows, bf16, params, slot0=4, active=active, c0=2)
    torch.cuda.synchronize()
    tok, kept = run.read()
    assert (tok[:, 1] == SENT).all() and (kept[:, 1] == SENT).all() and run.state[1].tolist() == [SC.SEED + 1, 2]
    assert run.pos[1].item() == POS0 and (run.hist[1] == SENT).all() and int(active.item()) == 0b101 << 4
    tally = _Tally()
    tally.check("active", run, rows=(0, 2))
    tally.clean()
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    run = _Launch(L, runtime, rows, bf16, params, active=off)
    torch.cuda.synchronize()
    assert (run.tok == SENT).all() and (run.kept == SENT).all() and (run.hist == SENT).all() and (run.pos == POS0).all()
    assert run.state.tolist() == [[SC.SEED + r, 0] for r in range(3)]


def test_the_history_guard_and_optional_outputs():
    """history_len = 2: draws 2 and 3 must not write history while the counter still advances; pos, history and kept_out may be NULL"""
    L, runtime = _lib_rt()
    V, bf16 = 64, True
    rows = SC.random_rows(V, bf16)[:2]
    run = _Launch(L, runtime, rows, bf16, [SC.MIXED[1], SC.MIXED[5]], hist_len=2)
    lg, pr = _upload(rows), _params([SC.MIXED[1], SC.MIXED[5]])
    state = torch.tensor([[SC.SEED, 0], [SC.SEED + 1, 0]], dtype=torch.int64, device=DEV)
    tok = torch.full((2,), SENT, dtype=torch.int32, device=DEV)
    assert L.teal_sample_rows(lg.data_ptr(), V, V, 1, 2, pr.data_ptr(), state.data_ptr(), tok.data_ptr(), None, None, 0, None, None, 0,
                              runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    t, _ = run.read()
    # (a write past row 1's two entries would land in the guard words behind the rows; one past row 0's in row 1's entry 0)
    assert run.hist.tolist() == t[:2].T.tolist() and (run.hist_all[4:] == SENT).all()
    assert run.state[:, 1].tolist() == [N_DRAWS] * 2 and run.pos.tolist() == [POS0 + N_DRAWS] * 2
    assert tok.tolist() == t[0].tolist() and state[:, 1].tolist() == [1, 1]


def test_fifty_replays_of_a_captured_launch_are_fifty_eager_launches():
    L, runtime = _lib_rt()
    V, bf16, n = 32000, False, 50
    rows = SC.random_rows(V, bf16)
    eager = _Launch(L, runtime, rows, bf16, SC.MIXED, n=n)
    lg, pr = eager.lg, eager.pr
    state = torch.tensor([[SC.SEED + r, 0] for r in range(8)], dtype=torch.int64, device=DEV)
    tok = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
    kept = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
    hist = torch.full((8, n + 2), SENT, dtype=torch.int32, device=DEV)
    pos = torch.full((8,), POS0, dtype=torch.int32, device=DEV)

    def step():
        assert L.teal_sample_rows(lg.data_ptr(), V, V, 0, 8, pr.data_ptr(), state.data_ptr(), tok.data_ptr(), pos.data_ptr(), hist.data_ptr(),
                                  n + 2, kept.data_ptr(), None, 0, runtime.stream_ptr()) == 0

    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with runtime.graph_capture(g):
        step()
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    et, ek = eager.read()
    assert hist[:, :n].T.tolist() == et.tolist() and (hist[:, n:] == SENT).all()
    assert kept.tolist() == ek[-1].tolist() and tok.tolist() == et[-1].tolist()
    assert state.tolist() == eager.state.tolist() and pos.tolist() == [POS0 + n] * 8

"""GPU: teal_token_logprobs / teal_score_step (teal_amd/csrc/teal_logprob.hip) through the C ABI against the fp64 rule
(tests/logprob_rule.py) on the same 16-bit logits, within 4 fp32 ulps of max(1, |truth|).

  1. vocab 8 .. 128256 (one vector, exactly one round of the workgroup, one more vector than that, Llama-2's, Llama-3's), fp16 and
     bf16, B = 1 / 3 / 8, rows vocab + 8 apart with the padding at the dtype's largest finite value (an over-read changes the
     max); normal, flat, peaked and near-the-top-of-fp16 rows; token 0, V - 1, the argmax, a middle index;
  2. the alternates: exact ids for n = 1 / 5 / 8, flat rows give 0 .. n-1, a duplicated maximum lists the lower id first, and with
     the argmax as the token top_lp[0] is lp bit for bit;
  3. indexing by the draw counter (1, lp_len, and lp_len + 1 / 0, which write nothing) into NaN-filled buffers compared bitwise,
     guard words either side; predication on the active word with and without slot0;
  4. two launches give the same bits, and a row gives the same bits at B = 1 and inside B = 8;
  5. teal_score_step walks its targets and stops at the end.
"""
import math

import numpy as np
import pytest
import torch

import logprob_rule as R
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float16: 0, torch.bfloat16: 1}
GUARD = 4
LAWS = ("normal", "flat", "peaked", "top")


def _rows(law, B, V, dt, seed):
    """[B, V + 8] logits of `dt` on the device: the law in columns < V, the dtype's largest finite value in the padding"""
    g = np.random.default_rng(seed)
    if law == "normal":
        x = g.standard_normal((B, V)) * 4.0
    elif law == "flat":
        x = np.full((B, V), 1.5) + np.arange(B)[:, None]
    elif law == "peaked":  # needs the max subtraction at both ends: exp(+60000) overflows, exp(-120000) is 0
        x = np.full((B, V), -60000.0)
        x[np.arange(B), g.integers(0, V, B)] = 60000.0
    else:  # near the top of the fp16 range: exp(l) without the max subtraction is inf
        x = 65504.0 - np.abs(g.standard_normal((B, V))) * 96.0
    buf = torch.full((B, V + 8), torch.finfo(dt).max, dtype=dt, device=DEV)
    buf[:, :V] = torch.from_numpy(x).to(DEV).to(dt)
    return buf


def _tokens(rows64, V):
    """token 0, V - 1, the argmax, a middle index — cycling over the rows"""
    picks = (lambda r: 0, lambda r: V - 1, lambda r: int(np.argmax(rows64[r])), lambda r: V // 2 + (1 if V > 8 else 0))
    return [picks[r % 4](r) for r in range(len(rows64))]


class _Out:
    """lp / top_ids / top_lp for `rows` x lp_len entries, NaN-filled, GUARD words either side"""

    def __init__(self, rows, lp_len, top_n):
        self.rows, self.lp_len, self.n = rows, lp_len, top_n
        mk = lambda k: torch.full((2 * GUARD + rows * lp_len * k,), R.NAN_BITS, dtype=torch.int32, device=DEV)  # noqa: E731
        self.lp, self.ids, self.tlp = mk(1), mk(max(top_n, 1)), mk(max(top_n, 1))

    def ptrs(self):
        return self.lp.data_ptr() + 4 * GUARD, self.ids.data_ptr() + 4 * GUARD, self.tlp.data_ptr() + 4 * GUARD

    def read(self):
        torch.cuda.synchronize()
        k = max(self.n, 1)
        for t in (self.lp, self.ids, self.tlp):
            a = t.cpu().numpy()
            assert (a[:GUARD] == R.NAN_BITS).all() and (a[-GUARD:] == R.NAN_BITS).all(), "guard words overwritten"
        lp = self.lp.cpu().numpy()[GUARD:-GUARD].reshape(self.rows, self.lp_len)
        ids = self.ids.cpu().numpy()[GUARD:-GUARD].reshape(self.rows, self.lp_len, k)
        tlp = self.tlp.cpu().numpy()[GUARD:-GUARD].reshape(self.rows, self.lp_len, k)
        return lp.copy(), ids.copy(), tlp.copy()  # int32 bit patterns


def _f32(bits):
    return np.asarray(bits, dtype=np.int32).view(np.float32)


def _launch(logits, V, tokens, counters, lp_len, top_n, active=None, slot0=0, out=None, B=None):
    L = _lib.load()
    runtime.init()
    B = logits.shape[0] if B is None else B
    out = _Out(B, lp_len, top_n) if out is None else out
    tok = torch.tensor(tokens, dtype=torch.int32, device=DEV)
    rng = torch.tensor([[77, c] for c in counters], dtype=torch.int64, device=DEV)
    act = None if active is None else torch.tensor([active], dtype=torch.int32, device=DEV)
    lp, ids, tlp = out.ptrs()
    rc = L.teal_token_logprobs(logits.data_ptr(), logits.stride(0), V, CODE[logits.dtype], B, tok.data_ptr(), rng.data_ptr(), lp, lp_len,
                               top_n, ids if top_n else None, tlp if top_n else None, None if act is None else act.data_ptr(), slot0,
                               runtime.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert rng[:, 1].tolist() == list(counters) and tok.tolist() == list(tokens)  # inputs are read only
    return out


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 1024, 8192, 8200, 32000, 128256])
def test_logprobs_and_alternates_against_the_rule(V, dt, law):
    lp_len = 4
    for B, n in ((1, 1), (3, 5), (8, 8), (8, 0)):
        logits = _rows(law, B, V, dt, seed=V + B)
        rows64 = logits[:, :V].double().cpu().numpy()
        tokens = _tokens(rows64, V)
        # counters: 1 and lp_len write entries 0 and lp_len - 1; lp_len + 1 and 0 write nothing
        counters = [(1, lp_len, lp_len + 1, 2, 0, 3, 1, lp_len)[r] for r in range(B)]
        lp, ids, tlp = _launch(logits, V, tokens, counters, lp_len, n).read()
        for r in range(B):
            i = counters[r] - 1
            written = np.zeros(lp_len, bool)
            if 0 <= i < lp_len:
                written[i] = True
                truth = R.logprobs64(rows64[r])
                got = _f32(lp[r, i])
                assert R.close(got, truth[tokens[r]]), (B, r, tokens[r], float(got), truth[tokens[r]], R.worst(got, truth[tokens[r]]))
                if law == "flat":
                    assert R.close(got, -math.log(V))
                if n:
                    want = R.top_n(rows64[r], n)
                    assert ids[r, i].tolist() == want.tolist(), (B, r, ids[r, i].tolist(), want.tolist())
                    assert R.close(_f32(tlp[r, i]), truth[want]), (B, r, R.worst(_f32(tlp[r, i]), truth[want]))
                    if law == "flat":
                        assert ids[r, i].tolist() == list(range(n))
                    if tokens[r] == want[0]:
                        assert tlp[r, i, 0] == lp[r, i], "top_lp[0] and lp differ in their bits for the argmax token"
            assert (lp[r, ~written] == R.NAN_BITS).all(), (B, r, counters[r])
            if n:
                assert (ids[r, ~written] == R.NAN_BITS).all() and (tlp[r, ~written] == R.NAN_BITS).all(), (B, r, counters[r])
        if not n:
            assert (ids == R.NAN_BITS).all() and (tlp == R.NAN_BITS).all()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 8200, 128256])
def test_duplicated_maximum_and_ties_list_the_lower_id_first(V, dt):
    g = np.random.default_rng(V)
    x = np.round(g.standard_normal((2, V)) * 2.0)  # whole numbers: many equal logits
    top = [V - 1, V // 2, 3, V // 2 + 1] if V > 8 else [7, 4, 3, 5]
    x[0, top] = 40.0                               # a maximum held by four ids
    x[1, :] = np.where(np.arange(V) % 2 == 0, -0.0, 0.0)  # -0 and +0 are equal logits: ids in order
    logits = torch.full((2, V + 8), torch.finfo(dt).max, dtype=dt, device=DEV)
    logits[:, :V] = torch.from_numpy(x).to(DEV).to(dt)
    rows64 = logits[:, :V].double().cpu().numpy()
    lp, ids, tlp = _launch(logits, V, [top[2], 0], [1, 1], 1, 8).read()
    assert ids[0, 0, :4].tolist() == sorted(top)
    for r in range(2):
        assert ids[r, 0].tolist() == R.top_n(rows64[r], 8).tolist()
        assert R.close(_f32(tlp[r, 0]), R.logprobs64(rows64[r])[ids[r, 0]])
    assert ids[1, 0].tolist() == list(range(8))
    assert len(set(tlp[0, 0, :4].tolist())) == 1 and tlp[0, 0, 0] == lp[0, 0]  # equal logits, equal bits — the token's among them


def test_minus_infinity_contributes_nothing():
    V = 1024
    for dt in (torch.float16, torch.bfloat16):
        logits = _rows("normal", 2, V, dt, seed=1)
        logits[0, 5:V:3] = float("-inf")
        logits[1, 1:V] = float("-inf")  # one finite logit: lp = 0 for it, -inf for the rest
        rows64 = logits[:, :V].double().cpu().numpy()
        lp, ids, tlp = _launch(logits, V, [4, 0], [1, 1], 1, 2).read()
        truth = R.logprobs64(rows64[0])
        assert R.close(_f32(lp[0, 0]), truth[4]) and ids[0, 0].tolist() == R.top_n(rows64[0], 2).tolist()
        assert _f32(lp[1, 0]) == 0.0 and ids[1, 0].tolist() == [0, 1] and _f32(tlp[1, 0, 1]) == -np.inf
        lp2, _, _ = _launch(logits, V, [5, 7], [1, 1], 1, 0).read()
        assert _f32(lp2[0, 0]) == -np.inf and _f32(lp2[1, 0]) == -np.inf


def test_predication_on_the_active_word():
    V, dt, lp_len = 8200, torch.float16, 3
    logits = _rows("normal", 3, V, dt, seed=2)
    rows64 = logits[:, :V].double().cpu().numpy()
    tokens = [1, 2, 3]
    truth = [R.logprobs64(rows64[r])[tokens[r]] for r in range(3)]
    lp, ids, tlp = _launch(logits, V, tokens, [2, 2, 2], lp_len, 2, active=0b101).read()
    assert (lp[1] == R.NAN_BITS).all() and (ids[1] == R.NAN_BITS).all() and (tlp[1] == R.NAN_BITS).all()
    for r in (0, 2):
        assert R.close(_f32(lp[r, 1]), truth[r]) and (lp[r, [0, 2]] == R.NAN_BITS).all()
        assert ids[r, 1].tolist() == R.top_n(rows64[r], 2).tolist()
    # rows 0, 1 serve slots 2, 3
    lp, _, _ = _launch(logits[:2], V, tokens[:2], [1, 3], lp_len, 0, active=0b01100, slot0=2).read()
    assert R.close(_f32(lp[0, 0]), truth[0]) and R.close(_f32(lp[1, 2]), truth[1])
    assert (lp[0, 1:] == R.NAN_BITS).all() and (lp[1, :2] == R.NAN_BITS).all()
    lp, _, _ = _launch(logits[:2], V, tokens[:2], [1, 3], lp_len, 0, active=0b00011, slot0=2).read()
    assert (lp == R.NAN_BITS).all()  # bits 0 and 1 are other slots'
    lp, _, _ = _launch(logits[:2], V, tokens[:2], [1, 3], lp_len, 0, active=0b01000, slot0=2).read()
    assert (lp[0] == R.NAN_BITS).all() and R.close(_f32(lp[1, 2]), truth[1])


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [1024, 32000, 128256])
def test_bit_identical_across_launches_and_batch_sizes(V, dt):
    B, n = 8, 5
    logits = _rows("normal", B, V, dt, seed=3 * V)
    rows64 = logits[:, :V].double().cpu().numpy()
    tokens = _tokens(rows64, V)
    a = _launch(logits, V, tokens, [1] * B, 1, n).read()
    b = _launch(logits, V, tokens, [1] * B, 1, n).read()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for r in range(B):  # the row alone, in a launch of its own
        one = _launch(logits[r:r + 1], V, tokens[r:r + 1], [1], 1, n).read()
        for x, y in zip(a, one):
            assert np.array_equal(x[r], y[0]), r


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 32000, 128256])
def test_score_step_walks_its_targets_and_stops(V, dt):
    L = _lib.load()
    runtime.init()
    g = np.random.default_rng(V)
    targets = [int(t) for t in g.integers(0, V, 5)]
    targets[2] = V - 1
    tg = torch.tensor(targets, dtype=torch.int32, device=DEV)
    lp = torch.full((GUARD + 5 + GUARD,), R.NAN_BITS, dtype=torch.int32, device=DEV)
    tok = torch.tensor([targets[0]], dtype=torch.int32, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    truth = []
    for k in range(6):
        logits = _rows("normal", 1, V, dt, seed=V + k)  # a new row per step, as a decode step would leave
        before = (int(tok), int(pos), lp.clone())
        rc = L.teal_score_step(logits.data_ptr(), V, CODE[dt], tg.data_ptr(), 5, tok.data_ptr(), pos.data_ptr(), lp.data_ptr() + 4 * GUARD,
                               runtime.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        if k < 4:
            truth.append(R.logprobs64(logits[0, :V].double().cpu().numpy())[targets[k + 1]])
            assert int(tok) == targets[k + 1] and int(pos) == k + 1
        else:  # past the end: nothing changes
            assert (int(tok), int(pos)) == before[:2] == (targets[4], 4) and torch.equal(lp, before[2])
    a = lp.cpu().numpy()
    assert (a[:GUARD + 1] == R.NAN_BITS).all() and (a[-GUARD:] == R.NAN_BITS).all()  # guards and entry 0
    got = _f32(a[GUARD + 1:GUARD + 5])
    assert R.close(got, truth), (got, truth, R.worst(got, truth))

"""GPU: teal_logit_adjust (teal_amd/csrc/teal_logit_adjust.hip) through the C ABI against the host rule (tests/logit_rule.py),
BIT FOR BIT on `out` and on the whole state table.

  1. vocab 8 .. 128256 (one vector, part of a workgroup, exactly one workgroup, one vector more, Llama-2's, Llama-3's), fp16 and
     bf16, B = 1 / 3 / 8; logits of every finite pattern with +-0, denormals, +-MAXF and -inf planted; state words with bit 31
     only, counts only and both; the counted token at element 0, the last element of a vector, either side of the workgroup seam,
     vocab - 1 and outside the vocabulary; count_token 0 and 1; with and without a bias row; rows vocab + 8 apart with sentinels
     behind each row and guard words round the state table;
  2. predication on the active word, with and without slot0: an inactive row between two active ones keeps its sentinels;
  3. 20 replays of a captured launch move the count by exactly 20 and nothing else.
"""
import numpy as np
import pytest
import torch

import logit_rule as R
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float16: 0, torch.bfloat16: 1}
GUARD, PAD = 8, 8
OUT_FILL, PAD_FILL, STATE_GUARD = 0x5A5A, 0x1234, 0x0BADF00D
PB = -2 ** 31
PARAMS = [(1.3, 0.4, 0.1), (0.5, -0.25, 0.05), (1.0, 0.0, 0.0), (2.0, 1.5, 0.7), (0.9, 0.0, -0.3), (1.0, 0.3, 0.0), (1.7, 0.0, 0.0), (1.0, 0.0, 2.5)]


def _specials(bf16):
    maxf = 0x7F7F if bf16 else 0x7BFF
    #       +0      -0     denormals: smallest, largest, negative               +MAXF  -MAXF          -inf
    return [0x0000, 0x8000, 0x0001, 0x007F if bf16 else 0x03FF, 0x8001, 0x8040, maxf, maxf | 0x8000, 0xFF80 if bf16 else 0xFC00]


def _logit_bits(g, B, V, bf16):
    """[B][V] 16-bit patterns: every finite value is possible (NaN and +inf patterns are redrawn as ordinary ones), the specials
    planted at random places — each under every kind of state word in some row"""
    bits = g.integers(0, 1 << 16, (B, V)).astype(np.uint16)
    expo = 0x7F80 if bf16 else 0x7C00
    bad = (bits & expo) == expo
    bits[bad] = bits[bad] & np.uint16(0xBFFF)  # clear the exponent's top bit: a finite value
    sp = _specials(bf16)
    for b in range(B):
        for k in range(4 if V > 64 else 1):
            at = g.permutation(V)[:len(sp)]
            bits[b, at] = np.array(sp[:len(at)], dtype=np.uint16)
    bits[:, 0] = np.array([sp[(3 + b) % len(sp)] for b in range(B)], dtype=np.uint16)
    bits[:, V - 1] = np.array([sp[(8 + b) % len(sp)] for b in range(B)], dtype=np.uint16)  # -inf last in row 0
    return bits


def _state_words(g, B, V):
    kinds = np.array([0, 0, 0, 0, PB, 1, 2, 5, PB | 1, PB | 3, (1 << 24) + 1, 0x7FFFFFFF, -1], dtype=np.int64)
    return g.choice(kinds, (B, V)).astype(np.int32)


def _tokens(B, V, shift):
    place = [0, 7, 8191, 8192, V - 1, V, -1, V // 2 + 3, 15, 8199]
    return [place[(r + shift) % len(place)] for r in range(B)]


class _Case:
    def __init__(self, V, dt, B, seed, with_bias=True):
        g = np.random.default_rng(seed)
        self.V, self.dt, self.B, self.bf16 = V, dt, B, dt == torch.bfloat16
        self.lbits = _logit_bits(g, B, V, self.bf16)
        self.state0 = _state_words(g, B, V)
        self.params = np.array([list(PARAMS[(r + seed) % len(PARAMS)]) + [0.0] for r in range(B)], dtype=np.float32)
        self.bias_bits = R.encode((g.standard_normal((B, V)) * 8).astype(np.float32).reshape(-1), self.bf16).reshape(B, V) if with_bias else None
        if with_bias:
            self.bias_bits[:, ::5] = 0  # (+0: most entries of a real bias row)
        row = np.full((B, V + PAD), PAD_FILL, dtype=np.uint16)
        row[:, :V] = self.lbits
        self.logits = torch.from_numpy(row.view(np.int16)).to(DEV).view(dt)
        self.out = torch.from_numpy(np.full((B, V + PAD), OUT_FILL, dtype=np.uint16).view(np.int16)).to(DEV).view(dt)
        st = np.full(2 * GUARD + B * V, STATE_GUARD, dtype=np.int32)
        st[GUARD:-GUARD] = self.state0.reshape(-1)
        self.state = torch.from_numpy(st).to(DEV)
        self.par = torch.from_numpy(self.params).to(DEV)
        self.bias = torch.from_numpy(self.bias_bits.view(np.int16)).to(DEV).view(dt) if with_bias else None

    def state_ptr(self):
        return self.state.data_ptr() + 4 * GUARD

    def launch(self, tokens, count, active=None, slot0=0):
        L = _lib.load()
        runtime.init()
        self.tok = torch.tensor(tokens, dtype=torch.int32, device=DEV)
        self.act = None if active is None else torch.tensor([active], dtype=torch.int32, device=DEV)
        rc = L.teal_logit_adjust(self.logits.data_ptr(), self.logits.stride(0), self.V, CODE[self.dt], self.B, self.tok.data_ptr(), count,
                                 self.state_ptr(), self.par.data_ptr(), None if self.bias is None else self.bias.data_ptr(),
                                 self.out.data_ptr(), self.out.stride(0), None if self.act is None else self.act.data_ptr(), slot0,
                                 runtime.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()

    def read(self):
        torch.cuda.synchronize()
        out = self.out.view(torch.int16).cpu().numpy().view(np.uint16)
        st = self.state.cpu().numpy()
        assert (st[:GUARD] == STATE_GUARD).all() and (st[-GUARD:] == STATE_GUARD).all(), "guard words of the state table overwritten"
        assert (out[:, self.V:] == OUT_FILL).all(), "sentinels behind an out row overwritten"
        # the inputs are read only
        lg = self.logits.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(lg[:, :self.V], self.lbits) and (lg[:, self.V:] == PAD_FILL).all()
        assert np.array_equal(self.par.cpu().numpy(), self.params)
        if self.bias is not None:
            assert np.array_equal(self.bias.view(torch.int16).cpu().numpy().view(np.uint16), self.bias_bits)
        return out[:, :self.V].copy(), st[GUARD:-GUARD].reshape(self.B, self.V).copy()

    def expect(self, state, tokens, count, rows=None):
        """(out rows, state rows) the rule gives from `state`; rows outside `rows` keep OUT_FILL and their state"""
        want_out = np.full((self.B, self.V), OUT_FILL, dtype=np.uint16)
        want_st = state.copy()
        for r in (range(self.B) if rows is None else rows):
            if count:
                want_st[r] = R.count(state[r], tokens[r])
            th, ap, af = self.params[r, :3]
            want_out[r] = R.adjust(self.lbits[r], self.bf16, want_st[r], th, ap, af, None if self.bias_bits is None else self.bias_bits[r])
        return want_out, want_st


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 64, 512, 8192, 8200, 32000, 128256])
def test_out_and_state_match_the_rule_bit_for_bit(V, dt):
    for B, shift in ((1, 0), (3, 2), (8, 0), (8, 5), (1, 4)):
        c = _Case(V, dt, B, seed=V + 17 * B + shift)
        tokens = _tokens(B, V, shift)
        # first without counting, then — on the same buffers — with: the second launch starts from the first one's (unchanged) state
        c.launch(tokens, 0)
        out, st = c.read()
        want_out, want_st = c.expect(c.state0, tokens, 0)
        _same(st, c.state0, f"B={B} count_token=0: state")
        _same(out, want_out, f"B={B} count_token=0: out")
        c.launch(tokens, 1)
        out, st = c.read()
        want_out, want_st = c.expect(c.state0, tokens, 1)
        _same(st, want_st, f"B={B} count_token=1: state")
        _same(out, want_out, f"B={B} count_token=1: out")
        assert int((want_st != c.state0).sum()) == sum(0 <= t < V and (int(c.state0[r, t]) & 0x7FFFFFFF) != 0x7FFFFFFF for r, t in enumerate(tokens))
        assert not np.isinf(R.decode(out.reshape(-1), c.bf16)).any()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 8200, 128256])
def test_without_a_bias_row(V, dt):
    B = 3
    c = _Case(V, dt, B, seed=V + 1, with_bias=False)
    tokens = _tokens(B, V, 3)
    c.launch(tokens, 1)
    out, st = c.read()
    want_out, want_st = c.expect(c.state0, tokens, 1)
    _same(st, want_st, "state")
    _same(out, want_out, "out")
    # identity parameters and an empty state: the row's own bits, -0 and denormals included
    c = _Case(V, dt, B, seed=V + 2, with_bias=False)
    c.state[GUARD:-GUARD].zero_()
    c.state0[:] = 0
    c.par.copy_(torch.tensor([[1.0, 0.0, 0.0, 0.0]] * B))
    c.params[:] = [1.0, 0.0, 0.0, 0.0]
    c.launch([V] * B, 1)
    out, st = c.read()
    want = c.lbits.copy()
    ninf = 0xFF80 if c.bf16 else 0xFC00
    want[want == ninf] = (0x7F7F if c.bf16 else 0x7BFF) | 0x8000  # -inf leaves as -MAXF
    _same(out, want, "identity out")
    assert not st.any()


def test_predication_on_the_active_word():
    V, dt, B = 8200, torch.float16, 3
    tokens = [8191, 8192, 0]
    c = _Case(V, dt, B, seed=5)
    c.launch(tokens, 1, active=0b101)
    out, st = c.read()
    want_out, want_st = c.expect(c.state0, tokens, 1, rows=(0, 2))
    assert (want_out[1] == OUT_FILL).all() and np.array_equal(want_st[1], c.state0[1])
    _same(st, want_st, "state")
    _same(out, want_out, "out")
    # rows 0, 1 serve slots 2, 3: bit 2 set, bit 3 clear; bits 0 and 1 are other slots'
    c = _Case(V, dt, 2, seed=6)
    c.launch(tokens[:2], 1, active=0b10111, slot0=2)
    out, st = c.read()
    want_out, want_st = c.expect(c.state0, tokens, 1, rows=(0,))
    _same(st, want_st, "slot0 state")
    _same(out, want_out, "slot0 out")
    c = _Case(V, dt, 2, seed=7)
    c.launch(tokens[:2], 1, active=0b00011, slot0=2)
    out, st = c.read()
    assert (out == OUT_FILL).all() and np.array_equal(st, c.state0)


@pytest.mark.parametrize("dt,V", [(torch.float16, 32000), (torch.bfloat16, 8200)])
def test_twenty_replays_move_the_count_by_twenty_and_nothing_else(dt, V):
    B, n = 3, 20
    c = _Case(V, dt, B, seed=9)
    tokens = [8192 if V > 8192 else 17, V - 1, V]  # in range, in range, outside
    for r, t in enumerate(tokens[:2]):  # counts that have room for 20 more
        c.state0[r, t] = (PB | 4) if r else 2
    c.state[GUARD:-GUARD].copy_(torch.from_numpy(c.state0.reshape(-1)))
    c.launch(tokens, 1)  # warm-up outside capture ...
    c.state[GUARD:-GUARD].copy_(torch.from_numpy(c.state0.reshape(-1)))  # ... undone
    L = _lib.load()
    g = torch.cuda.CUDAGraph()
    with runtime.graph_capture(g):
        rc = L.teal_logit_adjust(c.logits.data_ptr(), c.logits.stride(0), V, CODE[dt], B, c.tok.data_ptr(), 1, c.state_ptr(), c.par.data_ptr(),
                                 c.bias.data_ptr(), c.out.data_ptr(), c.out.stride(0), None, 0, runtime.stream_ptr())
    assert rc == 0
    c.state[GUARD:-GUARD].copy_(torch.from_numpy(c.state0.reshape(-1)))  # (a capture runs nothing, but nothing rests on that)
    for _ in range(n):
        g.replay()
    out, st = c.read()
    want_st = c.state0.copy()
    want_st[0, tokens[0]] += n
    want_st[1, tokens[1]] += n
    _same(st, want_st, "state after 20 replays")
    assert st[0, tokens[0]] == 22 and st[1, tokens[1]] == (PB | 24)
    want_out, _ = c.expect(want_st, tokens, 0)  # the last replay adjusted with the final counts
    _same(out, want_out, "out after 20 replays")

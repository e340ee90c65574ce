"""GPU: teal_force_tokens through the ABI against the host rule (tests/force_rule.py).  No model is needed: a case is the forced
table, the length words, the draw counters, B tokens, the history rows and the active word, each buffer between sentinel words,
and after the launch EVERY word of every buffer — the sentinels and the rows the launch must leave alone included — is the rule's.

  B in {1, 3, 8} x slot0 in {0, 5} x forced_stride in {4, 37}; per case the rows run through lengths {0, 1, stride, stride + 3
  (clamped)} and counters {0, 1, len, len + 1}; history_len below and above i; history NULL; active NULL and active words with
  mixed bits; then the refusals, which must leave the buffers alone, and 20 replays of a captured launch.
"""
import itertools

import numpy as np
import pytest
import torch

import force_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8          # sentinel words in front of and behind every buffer
S_TAB, S_LEN, S_TOK, S_HIST = -7, -8, -9, -5
ERR_ARG = -1       # include/teal_hip.h: TEAL_ERR_ARG


def _lib_rt():
    from teal_amd import _lib, runtime
    L = _lib.load()
    runtime.init()
    return L, runtime


def test_the_error_code_is_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "teal_hip.h")).read()
    assert int(re.search(r"#define TEAL_ERR_ARG \((-?\d+)\)", hdr).group(1)) == ERR_ARG


class _Buf:
    """a host array between GUARD sentinel words, and its device copy"""

    def __init__(self, body, sentinel, dtype=np.int32):
        body = np.asarray(body, dtype=dtype)
        self.shape = body.shape
        g = np.full(GUARD, sentinel, dtype=dtype)
        self.host = np.concatenate([g, body.reshape(-1), g])
        tdt = torch.int32 if dtype == np.int32 else torch.int64
        self.dev = torch.from_numpy(self.host.view(np.int32 if dtype == np.int32 else np.int64).copy()).to(DEV)
        assert self.dev.dtype == tdt

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD * self.dev.element_size()

    def body(self):
        return self.host[GUARD:len(self.host) - GUARD].reshape(self.shape)

    def got(self):
        return self.dev.cpu().numpy().view(self.host.dtype)


class _Case:
    def __init__(self, B, slot0, stride, lens, counters, history_len, active, with_history=True, seed=0):
        g = np.random.default_rng(seed)
        self.B, self.slot0, self.stride, self.hl, self.active = B, slot0, stride, history_len, active
        self.forced = _Buf(g.integers(0, 50000, size=(B, stride)), S_TAB)
        self.lens = _Buf(lens, S_LEN)
        rng = np.zeros((B, 2), dtype=np.uint64)
        rng[:, 0] = g.integers(1, 1 << 40, size=B).astype(np.uint64)
        rng[:, 1] = np.asarray(counters, dtype=np.uint64)
        self.rng = _Buf(rng, 0xABCD, dtype=np.uint64)
        self.tokens = _Buf(np.full(B, S_TOK), S_TOK)
        self.history = _Buf(np.full((B, max(history_len, 1)), S_HIST)[:, :history_len], S_HIST) if with_history else None
        self.act = None if active is None else torch.tensor([active, 0x55AA], dtype=torch.int64).to(torch.int32).to(DEV)

    def launch(self, L, runtime, st=None, **kw):
        a = dict(forced=self.forced.ptr, stride=self.stride, lens=self.lens.ptr, rng=self.rng.ptr, tokens=self.tokens.ptr,
                 history=None if self.history is None else self.history.ptr, hl=self.hl, B=self.B,
                 active=None if self.act is None else self.act.data_ptr(), slot0=self.slot0,
                 stream=runtime.stream_ptr() if st is None else st)
        a.update(kw)
        return L.teal_force_tokens(*a.values())

    def unchanged(self):
        torch.cuda.synchronize()
        bufs = [self.forced, self.lens, self.rng, self.tokens] + ([self.history] if self.history is not None else [])
        return all(np.array_equal(b.got(), b.host) for b in bufs)

    def check(self, where):
        """every word of every buffer is the rule's"""
        torch.cuda.synchronize()
        tok, hist = R.force_tokens(self.forced.body(), self.lens.body(), self.rng.body(), self.tokens.body(),
                                   None if self.history is None else self.history.body(), self.active, self.slot0)
        want_tok = self.tokens.host.copy()
        want_tok[GUARD:GUARD + self.B] = tok
        assert np.array_equal(self.tokens.got(), want_tok), (where, "tokens", self.tokens.got(), want_tok)
        if self.history is not None:
            want_h = self.history.host.copy()
            want_h[GUARD:GUARD + hist.size] = hist.reshape(-1)
            assert np.array_equal(self.history.got(), want_h), (where, "history")
        for name, b in (("forced", self.forced), ("forced_len", self.lens), ("rng_state", self.rng)):
            assert np.array_equal(b.got(), b.host), (where, name)
        if self.act is not None:
            assert self.act.tolist()[1] == 0x55AA
        return tok, hist


def _rows(B, stride, shift):
    """per row a (length, counter): the lengths {0, 1, stride, stride + 3} crossed with the counters {0, 1, len, len + 1}, dealt
    to the rows starting at combination `shift`"""
    combos = []
    for ln in (0, 1, stride, stride + 3):
        for c in (0, 1, ln, ln + 1):
            combos.append((ln, c))
    picked = [combos[(shift + r) % len(combos)] for r in range(B)]
    return [p[0] for p in picked], [p[1] for p in picked]


@pytest.mark.parametrize("B,slot0,stride", list(itertools.product((1, 3, 8), (0, 5), (4, 37))))
def test_every_word_is_the_rules(B, slot0, stride):
    L, runtime = _lib_rt()
    wrote = skipped = 0
    for shift in range(0, 16, B):  # every (length, counter) combination is some row's
        lens, ctrs = _rows(B, stride, shift)
        for hl, active in ((stride + 8, None), (2, None), (stride + 8, 0xFFFFFFFF), (stride + 8, 0x5A5A5A5A & 0x7FFFFFFF),
                           (3, 0x25A5A5A5), (stride + 8, 0)):
            c = _Case(B, slot0, stride, lens, ctrs, hl, active, seed=shift)
            assert c.launch(L, runtime) == 0
            tok, hist = c.check((shift, hl, active))
            wrote += int((tok != S_TOK).sum())
            skipped += int((tok == S_TOK).sum())
        c = _Case(B, slot0, stride, lens, ctrs, 0, None, with_history=False, seed=shift)  # history NULL: only the token words
        assert c.launch(L, runtime) == 0
        c.check((shift, "no history"))
    assert wrote > 0 and skipped > 0  # both sides of the rule were seen


def test_a_counter_past_2_to_the_32_forces_nothing():
    L, runtime = _lib_rt()
    c = _Case(3, 0, 4, [4, 4, 4], [(1 << 32) + 1, 1 << 63, 2], 8, None)
    assert c.launch(L, runtime) == 0
    tok, _ = c.check("wide counters")
    assert tok.tolist()[:2] == [S_TOK, S_TOK] and tok[2] == c.forced.body()[2, 1]


def test_the_refusals_come_before_any_write():
    L, runtime = _lib_rt()
    c = _Case(3, 5, 4, [4, 4, 4], [1, 2, 3], 8, 0xFFFFFFFF)
    bad = [dict(forced=None), dict(lens=None), dict(rng=None), dict(tokens=None), dict(B=0), dict(B=9), dict(B=-1), dict(slot0=-1),
           dict(slot0=30), dict(stride=0), dict(stride=-4), dict(hl=-1)]
    for kw in bad:
        assert c.launch(L, runtime, **kw) == ERR_ARG, kw
    assert c.unchanged()
    assert c.launch(L, runtime, history=None, hl=-1) == 0  # history_len is only looked at with a history
    assert c.launch(L, runtime, slot0=29) == 0 and c.launch(L, runtime, B=3, slot0=0, active=None) == 0
    torch.cuda.synchronize()


def test_replays_of_a_captured_launch_are_bit_identical():
    L, runtime = _lib_rt()
    c = _Case(8, 0, 37, [37, 0, 5, 40, 1, 37, 2, 9], [37, 1, 5, 38, 1, 1, 3, 9], 45, 0xB7)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with runtime.graph_capture(g):
        assert c.launch(L, runtime) == 0
    seen = set()
    for _ in range(20):
        g.replay()
        torch.cuda.synchronize()
        seen.add((c.tokens.got().tobytes(), c.history.got().tobytes()))
    assert len(seen) == 1
    c.check("replays")

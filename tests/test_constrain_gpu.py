"""GPU: teal_constrain_logits (teal_amd/csrc/teal_constrain.hip) through the C ABI against the host rule (tests/constraint_rule.py),
every output word and every trace word.

  1. vocab 8 / 8192 (exactly one workgroup) / 8200 (the second workgroup holds 8 elements) / 32000 / 128256, fp16 and bf16,
     B = 1 / 3 / 8 with and without slot0; one automaton whose states put edges on tokens 0, 8191, 8192 and vocab - 1, leave a
     workgroup without any edge, hold more than 1024 edges inside one workgroup, ban exceptions of a default at the same places,
     open only the EOS id, and list vocab / 2 edges; every way the state advances (draw 0, an edge, a default, the EOS id fed, a
     banned token fed, the last trace entry); EOS in the last workgroup's tail, EOS -1;
  2. unconstrained rows are copied bit for bit (-0, +-inf, NaN payloads), inactive rows keep their `out` and trace rows, sentinels
     behind every buffer stay; two images in one arena, two slots on one image in different states;
  3. a captured chain of constrain + sample launches replayed 20 times, twice from the same state: bit-identical;
  4. every argument refusal returns its code and launches nothing;
  5. teal_sample_rows and teal_sample_topk_slot draw from the launch's output the tokens they draw from the host-masked row.
"""
import numpy as np
import pytest
import torch

import constraint_rule as R
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float16: 0, torch.bfloat16: 1}
GUARD, PAD, TL = 8, 8, 6
OUT_FILL, PAD_FILL, WORD_GUARD, TRACE_FILL = 0x5A5A, 0x1234, 0x0BADF00D, 0x0DDBA11
ARG, DTYPE, SHAPE, ALIGN = -1, -2, -3, -4
V30 = R.VIOLATION


def automaton(V):
    """five states that cover the kernel's paths at vocabulary V (tests/constraint_rule.image's form)"""
    edge = sorted({t for t in (0, 8191, 8192, V - 1) if 0 <= t < V})           # the seams of the 8192-entry workgroups
    listed = 6 if V > 8 else 3
    return [
        ([(t, 1) for t in edge], -1, False),                                     # 0: a few edges, at the seams
        (sorted([(t, -1) for t in edge] + [(listed, 3)]), 2, False),             # 1: anything but the seams; one listed edge
        ([], -1, True),                                                          # 2: accepting, no edges: only the EOS id is open
        ([(t, 3) for t in range(1, min(V, 4000), 2)], -1, True),                 # 3: up to 2000 edges in workgroup 0, none behind it
        ([(t, 4 if t % 4 else -1) for t in range(0, V, 2)], -1, False),          # 4: vocab / 2 listed edges, half of them bans
    ]


def scenarios(V):
    """(draw counter, previous trace word, fed token, EOS id): every way the state advances"""
    last, listed, odd = V - 1, 6 if V > 8 else 3, 5
    return [
        (0, TRACE_FILL, last, V - 3),                # draw 0 ignores the fed token (and there is no previous word)
        (3, 0, 8191 if V > 8191 else last, -1),      # an ordinary edge: 0 -> 1
        (2, 1, 4, V - 3),                            # a default transition: 1 -> 2, where only the EOS id — in the last tail — is open
        (1, 1, 2, 2),                                # the EOS id fed: the state stays (and 1 is not accepting: its default does not open it)
        (4, 0, 1, -1),                               # a banned token fed at the ABI level: the state stays, bit 30
        (TL - 1, 3 | V30, odd, 0),                   # the last trace entry; bit 30 of the previous word is no part of the state
        (2, 4, 2, -1),                               # vocab / 2 edges
        (1, 1, listed, V - 1),                       # a listed edge over a default: 1 -> 3; EOS on the last token
        (5, 2, 1, 0),                                # a banned token in a state without edges: stays 2, bit 30; EOS at token 0
    ]


def _bits(g, B, V, bf16):
    """[B][V] 16-bit patterns of every kind (the launch moves bits, it computes nothing): -0, +-inf and NaN payloads planted"""
    bits = g.integers(0, 1 << 16, (B, V)).astype(np.uint16)
    sp = [0x8000, 0x0000, 0x7F80 if bf16 else 0x7C00, 0xFF80 if bf16 else 0xFC00, 0x7FC1 if bf16 else 0x7E01, 0xFFFF, R.neg_maxf(bf16)]
    for b in range(B):
        at = g.permutation(V)[:len(sp)]
        bits[b, at] = np.array(sp[:len(at)], dtype=np.uint16)
    return bits


class _Case:
    """buffers with sentinels round them; `rows`: per row (image name or None, draw counter, previous word, fed token, EOS id)"""

    def __init__(self, V, dt, images, rows, seed, bits=None):
        g = np.random.default_rng(seed)
        self.V, self.dt, self.B, self.bf16, self.rows = V, dt, len(rows), dt == torch.bfloat16, rows
        B = self.B
        self.lbits = _bits(g, B, V, self.bf16) if bits is None else bits
        words, self.base = [], {}
        for name, states in images.items():
            self.base[name] = len(words)
            img = R.image(states)
            words += img + [WORD_GUARD] * (-len(img) % 4)
        self.arena0 = np.array(words, dtype=np.int32)
        self.S = {name: len(states) for name, states in images.items()}
        self.table0 = np.array([[-1, 0, 0, 0] if r[0] is None else [self.base[r[0]], self.S[r[0]], 0, 0] for r in rows], dtype=np.int32)
        self.trace0 = np.full((B, TL), TRACE_FILL, dtype=np.int32)
        for b, (_, c, prev, _, _) in enumerate(rows):
            if c:
                self.trace0[b, c - 1] = prev
        self.tokens0 = np.array([r[3] for r in rows], dtype=np.int32)
        self.eos0 = np.array([r[4] for r in rows], dtype=np.int32)
        self.rng0 = np.array([[77 + b, r[1]] for b, r in enumerate(rows)], dtype=np.int64)
        row = np.full((B, V + PAD), PAD_FILL, dtype=np.uint16)
        row[:, :V] = self.lbits
        self.logits = torch.from_numpy(row.view(np.int16)).to(DEV).view(dt)
        self.out = torch.from_numpy(np.full((B, V + PAD), OUT_FILL, dtype=np.uint16).view(np.int16)).to(DEV).view(dt)

        def guarded(a):
            w = np.full(2 * GUARD + a.size, WORD_GUARD, dtype=np.int32)
            w[GUARD:GUARD + a.size] = a.reshape(-1)
            return torch.from_numpy(w).to(DEV)
        self.arena, self.table, self.trace = guarded(self.arena0), guarded(self.table0), guarded(self.trace0)
        self.tok, self.eos = guarded(self.tokens0), guarded(self.eos0)
        self.rng = torch.from_numpy(self.rng0).to(DEV)

    @staticmethod
    def p(t):
        return t.data_ptr() + 4 * GUARD

    def launch(self, active=None, slot0=0):
        L = _lib.load()
        runtime.init()
        self.act = None if active is None else torch.from_numpy(np.array([active], dtype=np.uint32).view(np.int32)).to(DEV)
        rc = L.teal_constrain_logits(self.logits.data_ptr(), self.logits.stride(0), self.V, CODE[self.dt], self.B, self.p(self.tok), self.rng.data_ptr(),
                                     self.p(self.eos), self.p(self.table), self.p(self.arena), self.arena0.size, self.p(self.trace), TL,
                                     self.out.data_ptr(), self.out.stride(0), None if self.act is None else self.act.data_ptr(), slot0,
                                     runtime.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()

    def _inner(self, t, like):
        w = t.cpu().numpy()
        assert (w[:GUARD] == WORD_GUARD).all() and (w[GUARD + like.size:] == WORD_GUARD).all(), "guard words overwritten"
        return w[GUARD:GUARD + like.size].reshape(like.shape)

    def read(self):
        torch.cuda.synchronize()
        out = self.out.view(torch.int16).cpu().numpy().view(np.uint16)
        assert (out[:, self.V:] == OUT_FILL).all(), "sentinels behind an out row overwritten"
        lg = self.logits.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(lg[:, :self.V], self.lbits) and (lg[:, self.V:] == PAD_FILL).all()  # the inputs are read only
        for t, like in ((self.arena, self.arena0), (self.table, self.table0), (self.tok, self.tokens0), (self.eos, self.eos0)):
            assert np.array_equal(self._inner(t, like), like)
        assert np.array_equal(self.rng.cpu().numpy(), self.rng0)
        return out[:, :self.V].copy(), self._inner(self.trace, self.trace0).copy()

    def expect(self, active=None, slot0=0):
        out = np.full((self.B, self.V), OUT_FILL, dtype=np.uint16)
        trace = self.trace0.copy()
        R.launch(self.lbits, self.bf16, self.tokens0, self.rng0[:, 1], self.eos0, self.table0, self.arena0, trace, out, active, slot0)
        return out, trace


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: got {int(got[tuple(bad[0])]):#x}, "
                             f"want {int(want[tuple(bad[0])]):#x}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 8192, 8200, 32000, 128256])
def test_out_and_trace_match_the_rule_word_for_word(V, dt):
    sc = scenarios(V)
    for B, shift, slot0 in ((1, 0, 0), (3, 1, 0), (8, 0, 0), (8, 4, 0), (3, 6, 5), (1, 5, 31)):
        rows = [("a",) + sc[(r + shift) % len(sc)] for r in range(B)]
        c = _Case(V, dt, {"a": automaton(V)}, rows, seed=V + 31 * B + shift)
        active = None if not slot0 else ((1 << B) - 1) << slot0
        c.launch(active, slot0)
        out, trace = c.read()
        want_out, want_trace = c.expect(active, slot0)
        _same(trace, want_trace, f"B={B} shift={shift}: trace")
        _same(out, want_out, f"B={B} shift={shift}: out")
        assert int((trace != c.trace0).sum()) <= B  # one word per row, nothing else


def test_the_scenarios_reach_what_they_are_named_for():
    """the host rule on the scenarios: each way of advancing happens, bit 30 exactly where a banned token is fed"""
    for V in (8, 8200, 128256):
        img, sc = R.image(automaton(V)), scenarios(V)
        words = [R.state_word(img, 5, c, prev, t, e) for c, prev, t, e in sc]
        assert words == [0, 1, 2, 1, 0 | V30, 3, 4, 3, 2 | V30]
        keep = R.allowed(img, 2, V, V - 3)
        assert keep.sum() == 1 and keep[V - 3]                       # only the EOS id, in the last workgroup's tail
        assert not R.allowed(img, 1, V, 2)[2] and R.allowed(img, 1, V, -1)[2]  # a default does not open the EOS id of a non-accepting state
        assert len(R.edges(img, 3)) > 1024 or V == 8
        if V > 8192:
            assert all(t < 8192 for t, _ in R.edges(img, 3))         # workgroup 1 has none of state 3's edges
            assert {0, 8191, 8192, V - 1} <= {t for t, _ in R.edges(img, 0)}


def test_unconstrained_and_inactive_rows_and_two_images():
    V, dt = 8200, torch.float16
    other = [([(8192, 1), (8199, 0)], -1, False), ([(7, 0)], 0, True)]
    rows = [("a", 3, 0, 8191, -1), (None, 2, 7, 5, 3), ("b", 1, 0, 8192, 8199), ("a", 2, 1, 4, 8197), ("b", 4, 1, 9, 8199), (None, 0, 0, 0, -1)]
    c = _Case(V, dt, {"a": automaton(V), "b": other}, rows, seed=3)
    c.launch(0b101111)  # row 4 inactive
    out, trace = c.read()
    want_out, want_trace = c.expect(0b101111)
    _same(trace, want_trace, "trace")
    _same(out, want_out, "out")
    assert np.array_equal(out[1], c.lbits[1]) and np.array_equal(out[5], c.lbits[5])  # unconstrained: the row's own bits, NaNs included
    assert trace[1, 2] == 0 and trace[5, 0] == 0
    assert (out[4] == OUT_FILL).all() and (trace[4] == c.trace0[4]).all()            # inactive: nothing
    assert trace[0, 3] == 1 and trace[3, 2] == 2 and trace[2, 1] == 1                # two slots on image a in different states; image b


@pytest.mark.parametrize("dt,V", [(torch.float16, 32000), (torch.bfloat16, 8200)])
def test_twenty_replays_of_a_captured_chain_are_bit_identical(dt, V):
    """constrain -> teal_sample_rows, captured once: 20 replays walk the automaton 20 draws; from the restored state they do it again
    to the bit, and the whole state path is the rule's"""
    B, n = 3, 20
    g = np.random.default_rng(V)
    A = sorted(g.permutation(V)[:V // 2].tolist())
    Bset = sorted(g.permutation(V)[:V // 3].tolist())
    states = [([(t, 1) for t in A], -1, False), ([(t, -1) for t in Bset[:1000]], 0, True)]  # A, then anything but 1000 tokens, and back
    lbits = R_encode(g.standard_normal((B, V)).astype(np.float32) * 3, dt)
    c = _Case(V, dt, {"a": states}, [("a", 0, 0, 0, -1), (None, 0, 0, 0, -1), ("a", 0, 0, 0, -1)], seed=1, bits=lbits)
    L = _lib.load()
    runtime.init()
    trace = torch.zeros(B, n + 1, dtype=torch.int32, device=DEV)
    hist = torch.zeros(B, n + 1, dtype=torch.int32, device=DEV)
    tok = torch.zeros(B, dtype=torch.int32, device=DEV)
    params = torch.from_numpy(np.array([[np.float32(1.0).view(np.int32), 50, np.float32(0.9).view(np.int32), 0]] * B, dtype=np.int32)).to(DEV)
    rng = torch.tensor([[11 + b, 0] for b in range(B)], dtype=torch.int64, device=DEV)

    def chain():
        rc = L.teal_constrain_logits(c.logits.data_ptr(), c.logits.stride(0), V, CODE[dt], B, tok.data_ptr(), rng.data_ptr(), c.p(c.eos), c.p(c.table),
                                     c.p(c.arena), c.arena0.size, trace.data_ptr(), n + 1, c.out.data_ptr(), c.out.stride(0), None, 0, runtime.stream_ptr())
        assert rc == 0, rc
        rc = L.teal_sample_rows(c.out.data_ptr(), c.out.stride(0), V, CODE[dt], B, params.data_ptr(), rng.data_ptr(), tok.data_ptr(), None,
                                hist.data_ptr(), n + 1, None, None, 0, runtime.stream_ptr())
        assert rc == 0, rc

    loop = [trace, hist, tok, rng]
    saved = [t.clone() for t in loop]
    graph, _ = runtime.capture_graph(chain, loop)
    runs = []
    for _ in range(2):
        for t, s in zip(loop, saved):
            t.copy_(s)
        for _ in range(n):
            graph.replay()
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy().copy() for t in loop] + [c.out.view(torch.int16).cpu().numpy().copy()])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    tr, hs = runs[0][0], runs[0][1]
    img = R.image(states)
    for r in (0, 2):
        w = 0
        for i in range(n):
            assert tr[r, i] == w and not w & V30
            assert R.allowed(img, w, V, -1)[hs[r, i]], (r, i, int(hs[r, i]))
            w = R.state_word(img, 2, i + 1, w, int(hs[r, i]), -1)
    assert not tr[1].any()


def R_encode(x, dt):
    """fp32 -> the dtype's 16 bits, as torch rounds"""
    return torch.from_numpy(x).to(dt).view(torch.int16).numpy().view(np.uint16).copy()


def test_every_argument_refusal_returns_its_code_without_a_launch():
    V, dt = 64, torch.float16
    c = _Case(V, dt, {"a": automaton(V)}, [("a", 0, 0, 0, -1), ("a", 0, 0, 0, -1)], seed=2)
    L = _lib.load()
    runtime.init()
    good = dict(logits=c.logits.data_ptr(), ls=c.logits.stride(0), vocab=V, dtype=0, B=2, tokens=c.p(c.tok), rng=c.rng.data_ptr(), eos=c.p(c.eos),
                table=c.p(c.table), arena=c.p(c.arena), words=c.arena0.size, trace=c.p(c.trace), tl=TL, out=c.out.data_ptr(), os=c.out.stride(0),
                active=None, slot0=0)

    def call(**kw):
        a = dict(good, **kw)
        return L.teal_constrain_logits(*[a[k] for k in good], runtime.stream_ptr())

    for name in ("logits", "tokens", "rng", "eos", "table", "arena", "trace", "out"):
        assert call(**{name: None}) == ARG, name
    for kw in (dict(B=0), dict(B=9), dict(slot0=-1), dict(slot0=31), dict(tl=0), dict(tl=-3), dict(words=0)):
        assert call(**kw) == ARG, kw
    assert call(out=good["logits"]) == ARG and call(out=good["logits"] + 2 * (V + PAD)) == ARG  # `out` on, or inside, the logits rows
    for kw in (dict(dtype=2), dict(dtype=-1)):
        assert call(**kw) == DTYPE, kw
    for kw in (dict(vocab=0), dict(vocab=12), dict(vocab=131080), dict(vocab=-8)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(logits=good["logits"] + 2), dict(out=good["out"] + 8), dict(ls=V + 4), dict(os=V + 4)):
        assert call(**kw) == ALIGN, kw
    assert call(B=1, ls=V + 4, os=3) == 0  # (one row: the strides are not looked at)
    torch.cuda.synchronize()
    out, trace = c.read()
    want_out, want_trace = c.expect()
    assert np.array_equal(out[0], want_out[0]) and (out[1] == OUT_FILL).all()  # only the B = 1 launch wrote: row 0
    assert np.array_equal(trace[0], want_trace[0]) and np.array_equal(trace[1], c.trace0[1])


@pytest.mark.parametrize("V", [32000, 128256])
def test_the_samplers_draw_from_the_launch_what_they_draw_from_the_host_masked_row(V):
    """64 consecutive draws of teal_sample_rows (top_k 50, top_p 0.9) and of teal_sample_topk_slot, fed by the launch, against the
    same samplers on rows masked on the host under the same rng state: the same tokens, every one allowed"""
    dt, B, n = torch.float16, 2, 64
    g = np.random.default_rng(V + 1)
    X = sorted(g.permutation(V)[:V // 2].tolist())
    Y = sorted(g.permutation(V)[:500].tolist())
    states = [([(t, 1) for t in X], -1, False), ([(t, 0) for t in Y], -1, True)]  # draws alternate between the two sets
    img = R.image(states)
    lbits = R_encode(g.standard_normal((B, V)).astype(np.float32) * 3, dt)
    c = _Case(V, dt, {"a": states}, [("a", 0, 0, 0, -1)] * B, seed=4, bits=lbits)
    masked = [torch.from_numpy(np.stack([R.mask(lbits[r], img, s, -1, False) for r in range(B)]).view(np.int16)).to(DEV).view(dt) for s in (0, 1)]
    L = _lib.load()
    runtime.init()
    ws = runtime.new_workspace(64, V)
    act = torch.tensor([0b11], dtype=torch.int32, device=DEV)
    params = torch.from_numpy(np.array([[np.float32(0.8).view(np.int32), 50, np.float32(0.9).view(np.int32), 0]] * B, dtype=np.int32)).to(DEV)
    for sampler in ("rows", "topk_slot"):
        bufs = {}
        for side in ("device", "host"):
            bufs[side] = dict(rng=torch.tensor([[21 + b, 0] for b in range(B)], dtype=torch.int64, device=DEV),
                              tok=torch.zeros(B, dtype=torch.int32, device=DEV), hist=torch.zeros(B, n, dtype=torch.int32, device=DEV),
                              pos=torch.zeros(B, dtype=torch.int32, device=DEV))
        trace = torch.full((B, n), TRACE_FILL, dtype=torch.int32, device=DEV)

        def draw(src, b):
            if sampler == "rows":
                rc = L.teal_sample_rows(src.data_ptr(), src.stride(0), V, 0, B, params.data_ptr(), b["rng"].data_ptr(), b["tok"].data_ptr(),
                                        b["pos"].data_ptr(), b["hist"].data_ptr(), n, None, act.data_ptr(), 0, runtime.stream_ptr())
                assert rc == 0, rc
                return
            for r in range(B):
                rc = L.teal_sample_topk_slot(src[r].data_ptr(), V, 0, 50, 0.8, b["rng"][r].data_ptr(), b["tok"][r:].data_ptr(), b["pos"][r:].data_ptr(),
                                             b["hist"][r].data_ptr(), n, ws.data_ptr(), ws.numel() * 4, act.data_ptr(), r, runtime.stream_ptr())
                assert rc == 0, rc

        for i in range(n):
            d = bufs["device"]
            rc = L.teal_constrain_logits(c.logits.data_ptr(), c.logits.stride(0), V, 0, B, d["tok"].data_ptr(), d["rng"].data_ptr(), c.p(c.eos),
                                         c.p(c.table), c.p(c.arena), c.arena0.size, trace.data_ptr(), n, c.out.data_ptr(), c.out.stride(0),
                                         act.data_ptr(), 0, runtime.stream_ptr())
            assert rc == 0, rc
            draw(c.out, d)
            draw(masked[i % 2], bufs["host"])
        torch.cuda.synchronize()
        got, want = bufs["device"]["hist"].cpu().numpy(), bufs["host"]["hist"].cpu().numpy()
        assert np.array_equal(got, want), (sampler, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(trace.cpu().numpy(), np.tile(np.arange(n) % 2, (B, 1)))  # the state path; no violation bit
        keep = [R.allowed(img, s, V, -1) for s in (0, 1)]
        assert all(keep[i % 2][got[r, i]] for r in range(B) for i in range(n))
        assert len({int(t) for t in got.reshape(-1)}) > 8  # (draws, not one token over and over)

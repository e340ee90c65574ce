"""GPU: teal_batched_retire_stops through the ABI against the host model (tests/stop_rule.py).  No model is needed: every case is
a slot state, B tokens and positions, the history rows (max_seq = 32, history_stride = 40) and the stop table, and after the launch
the WHOLE buffers — slot_state, pos, stops — must be the model's.

  1. differential: 200 random states with all-zero tables leave slot_state and pos as teal_batched_retire leaves them, bit for bit,
     and touch nothing of the table but REASON and MATCH;
  2. stop ids: each of the 16 places, the id one past NIDS, NIDS = 17 read as 16;
  3. sequences: every length in every sequence slot, the 36 one-element near-misses, len == n + 1, len == n + 2 on rows a previous
     occupant filled with the sequence, length words 0 and 9;
  4. precedence; 5. min_new_tokens; 6. untouched slots; 7. all eight slots stopping in one launch; 8. 50 replays of a captured
     launch; 9. the argument checks leave the buffers alone.
"""
import random

import pytest
import torch

import stop_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_SEQ, STRIDE = 32, 40
GUARD = 8  # words in front of and behind the history rows: a read below index 0 of row 0 stays inside the allocation


def _lib_rt():
    from teal_amd import _lib, runtime
    L = _lib.load()
    runtime.init()
    return L, runtime


def _state(active=0, step=5, budget=5, produced=0, eos=-1):
    """a slot state with the same budget / produced / EOS in every slot (lists: one value per slot)"""
    st = [0] * R.SLOT_WORDS
    st[R.ACTIVE], st[R.STEP] = active, step
    for b in range(8):
        st[R.BUDGET + b] = budget[b] if isinstance(budget, list) else budget
        st[R.PRODUCED + b] = produced[b] if isinstance(produced, list) else produced
        st[R.EOS + b] = eos[b] if isinstance(eos, list) else eos
        st[R.FINISH + b] = -1
    return st


class _Case:
    """the buffers of one launch, as lists on the host and as tensors on the device"""

    def __init__(self, state, tokens, pos, history, stops, B, mask, count_step=True, hist_guard=None):
        self.B, self.mask, self.count_step = B, mask, count_step
        self.state, self.tokens, self.pos = list(state), list(tokens) + [0] * (8 - len(tokens)), list(pos) + [0] * (8 - len(pos))
        self.history = [list(h) + [-5] * (STRIDE - len(h)) for h in history] + [[-5] * STRIDE for _ in range(8 - len(history))]
        self.stops = [list(r) for r in stops] + [R.row() for _ in range(8 - len(stops))]
        guard = [-9] * GUARD if hist_guard is None else list(hist_guard)
        flat = guard + [t for h in self.history for t in h] + [-9] * GUARD
        i32 = dict(dtype=torch.int32, device=DEV)
        self.d_state, self.d_tok, self.d_pos = torch.tensor(self.state, **i32), torch.tensor(self.tokens, **i32), torch.tensor(self.pos, **i32)
        self.d_hist_all, self.d_stops = torch.tensor(flat, **i32), torch.tensor(self.stops, **i32)
        self.d_hist = self.d_hist_all[GUARD:GUARD + 8 * STRIDE]
        self.hist_flat = flat

    def launch(self, L, runtime, st=None, **kw):
        a = dict(state=self.d_state.data_ptr(), tokens=self.d_tok.data_ptr(), pos=self.d_pos.data_ptr(), history=self.d_hist.data_ptr(),
                 stride=STRIDE, stops=self.d_stops.data_ptr(), B=self.B, mask=self.mask, max_seq=MAX_SEQ, count_step=int(self.count_step),
                 stream=runtime.stream_ptr() if st is None else st)
        a.update(kw)
        return L.teal_batched_retire_stops(*a.values())

    def got(self):
        torch.cuda.synchronize()
        return self.d_state.tolist(), self.d_pos.tolist(), self.d_stops.tolist()

    def want(self):
        st, pos, stops = list(self.state), list(self.pos), [list(r) for r in self.stops]
        R.retire(st, self.tokens, pos, self.history, stops, self.B, self.mask, MAX_SEQ, self.count_step)
        return st, pos, stops

    def check(self, L, runtime, where=None):
        """launch once; the whole buffers are the model's and the inputs the launch only reads are unchanged"""
        assert self.launch(L, runtime) == 0
        got, want = self.got(), self.want()
        assert got[0] == want[0], (where, "slot_state", got[0], want[0])
        assert got[1] == want[1], (where, "pos", got[1], want[1])
        assert got[2] == want[2], (where, "stops", [(b, i, g, w) for b in range(8) for i, (g, w) in enumerate(zip(got[2][b], want[2][b])) if g != w])
        assert self.d_tok.tolist() == self.tokens and self.d_hist_all.tolist() == self.hist_flat, where
        return want


def _single(n, t, hist, b=0, budget=5, eos=-1, p=10, **kw):
    """slot b alone, n tokens produced (hist: draws 0 .. n-1), drawing t"""
    history = [[] for _ in range(b)] + [list(hist) + [t]]
    stops = [R.row() for _ in range(b)] + [R.row(**kw)]
    return _Case(_state(1 << b, budget=budget, produced=n, eos=eos), [0] * b + [t], [3] * b + [p], history, stops, max(b + 1, 1), 0xFF)


def _fired(want, b=0):
    st, _, stops = want
    return (st[R.ACTIVE] >> b) & 1 == 0, stops[b][R.REASON], stops[b][R.MATCH]


# ---- 1. differential -----------------------------------------------------------------------------------------------------------
def test_with_empty_tables_the_launch_is_teal_batched_retire():
    L, runtime = _lib_rt()
    g = random.Random(11)
    seen = set()
    for i in range(200):
        B = g.choice([1, 3, 8])
        tokens = [g.randrange(4) for _ in range(8)]
        eos = [g.choice([-1, tokens[b], (tokens[b] + 1) % 4]) for b in range(8)]
        st = _state(g.randrange(256), step=g.randrange(100), budget=[g.randint(1, 3) for _ in range(8)],
                    produced=[g.randrange(20) for _ in range(8)], eos=eos)
        pos = [g.choice([g.randint(1, MAX_SEQ - 1), MAX_SEQ - 1, MAX_SEQ]) for _ in range(8)]
        hist = [[g.randrange(4) for _ in range(STRIDE)] for _ in range(8)]
        table = [[0] * R.WORDS for _ in range(8)]  # all zero: MIN, NIDS, NSEQ and every other word
        c = _Case(st, tokens, pos, hist, table, B, g.randrange(256), count_step=bool(g.getrandbits(1)))
        plain_state, plain_pos = c.d_state.clone(), c.d_pos.clone()
        assert L.teal_batched_retire(plain_state.data_ptr(), c.d_tok.data_ptr(), plain_pos.data_ptr(), B, c.mask, MAX_SEQ, int(c.count_step),
                                     runtime.stream_ptr()) == 0
        want = c.check(L, runtime, i)
        assert torch.equal(c.d_state, plain_state) and torch.equal(c.d_pos, plain_pos), i
        for b in range(8):
            row = list(want[2][b])
            seen.add(row[R.REASON])
            row[R.REASON] = row[R.MATCH] = 0
            assert row == [0] * R.WORDS, (i, b)
    assert seen == {R.RUNNING, R.STOP_TOKEN, R.LENGTH, R.CACHE}  # the EOS word, budgets and the cache end all occurred


# ---- 2. stop ids -----------------------------------------------------------------------------------------------------------------
def test_stop_ids_in_every_place_and_not_past_the_end():
    L, runtime = _lib_rt()
    ids = list(range(100, 116))
    for i in range(16):
        want = _single(3, ids[i], [1, 2, 3], stop_token_ids=ids).check(L, runtime, ("place", i))
        assert _fired(want) == (True, R.STOP_TOKEN, ids[i])
        c = _single(3, ids[i], [1, 2, 3], stop_token_ids=ids)
        c.stops[0][R.NIDS] = i  # the id sits at index NIDS, one past the end
        c = _Case(c.state, c.tokens, c.pos, c.history, c.stops, 1, 0xFF)
        assert _fired(c.check(L, runtime, ("past", i))) == (False, R.RUNNING, -1)
    c = _single(3, ids[15], [1, 2, 3], stop_token_ids=ids)
    c.stops[0][R.NIDS] = 17
    c = _Case(c.state, c.tokens, c.pos, c.history, c.stops, 1, 0xFF)
    assert _fired(c.check(L, runtime, "17 ids")) == (True, R.STOP_TOKEN, ids[15])
    # ... read as 16: the word behind the ids (the first sequence's length) is no stop id
    c = _single(3, 5, [1, 2, 3], stop_token_ids=ids)
    c.stops[0][R.NIDS], c.stops[0][R.SEQLEN] = 17, 5
    c = _Case(c.state, c.tokens, c.pos, c.history, c.stops, 1, 0xFF)
    assert _fired(c.check(L, runtime, "word 24")) == (False, R.RUNNING, -1)
    c = _single(3, ids[2], [1, 2, 3], stop_token_ids=ids)
    c.stops[0][R.NIDS] = -4  # below 0: no id
    c = _Case(c.state, c.tokens, c.pos, c.history, c.stops, 1, 0xFF)
    assert _fired(c.check(L, runtime, "negative")) == (False, R.RUNNING, -1)


# ---- 3. sequences ----------------------------------------------------------------------------------------------------------------
def _seqs_with(q, seq):
    """eight sequences, number q being `seq` and the others a token nobody draws"""
    return [list(seq) if i == q else [900 + i] for i in range(8)]


def test_every_length_in_every_sequence_slot():
    L, runtime = _lib_rt()
    hist = [50 + i for i in range(12)]
    for ln in range(1, 9):
        seq = (hist + [7])[-ln:]
        for q in range(8):
            want = _single(12, 7, hist, b=q % 3, stop_sequences=_seqs_with(q, seq)).check(L, runtime, (ln, q))
            assert _fired(want, q % 3) == (True, R.STOP_SEQUENCE, q), (ln, q)


def test_the_36_near_misses_do_not_fire():
    L, runtime = _lib_rt()
    hist = [50 + i for i in range(12)]
    n = 0
    for ln in range(1, 9):
        for j in range(ln):
            seq = (hist + [7])[-ln:]
            seq[j] += 200  # one element wrong
            want = _single(12, 7, hist, stop_sequences=_seqs_with((ln + j) % 8, seq)).check(L, runtime, (ln, j))
            assert _fired(want) == (False, R.RUNNING, -1), (ln, j)
            n += 1
    assert n == 36


def test_a_sequence_needs_len_generated_tokens_whatever_the_rows_hold():
    L, runtime = _lib_rt()
    for ln in range(1, 9):
        seq = [60 + j for j in range(ln)]
        c = _single(ln - 1, seq[-1], seq[:-1], b=1, stop_sequences=[seq])  # len == n + 1: the request's first len tokens
        assert _fired(c.check(L, runtime, ("n + 1", ln)), 1) == (True, R.STOP_SEQUENCE, 0), ln
    for ln in range(2, 9):
        # len == n + 2: element 0 would be the entry in front of the row.  Every history word — the other rows, the guards, this row
        # past n — holds the sequence in phase, as a previous occupant would have left it
        seq, b, n = [60 + j for j in range(ln)], 1, ln - 2
        flat = [seq[(i - (GUARD + b * STRIDE - 1)) % ln] for i in range(GUARD + 8 * STRIDE + GUARD)]
        rows = [flat[GUARD + r * STRIDE:GUARD + (r + 1) * STRIDE] for r in range(8)]
        assert rows[b][:n + 1] == seq[1:] and rows[0][-1] == seq[0]
        c = _Case(_state(1 << b, produced=n), [0, seq[-1]], [3, 10], rows, [R.row(), R.row(stop_sequences=[seq])], 2, 0xFF,
                  hist_guard=flat[:GUARD])
        assert _fired(c.check(L, runtime, ("n + 2", ln)), b) == (False, R.RUNNING, -1), ln


def test_a_length_word_of_0_or_9_never_fires():
    L, runtime = _lib_rt()
    for bad in (0, 9, -1, 64):
        c = _single(12, 7, [7] * 12, stop_sequences=[[7] * 8] * 8)
        for q in range(8):
            c.stops[0][R.SEQLEN + q] = bad
        c = _Case(c.state, c.tokens, c.pos, c.history, c.stops, 1, 0xFF)
        assert _fired(c.check(L, runtime, bad)) == (False, R.RUNNING, -1), bad


# ---- 4. precedence, 5. min_new_tokens -----------------------------------------------------------------------------------------------
def test_precedence():
    L, runtime = _lib_rt()
    hist = [5, 6, 9]
    both = _single(3, 7, hist, stop_token_ids=[7], stop_sequences=[[9, 7]]).check(L, runtime, "id and sequence")
    assert _fired(both) == (True, R.STOP_TOKEN, 7)
    two = _single(3, 7, hist, stop_sequences=[[1], [6, 9, 7], [7], [9, 7]]).check(L, runtime, "two sequences")
    assert _fired(two) == (True, R.STOP_SEQUENCE, 1)
    last = _single(3, 7, hist, budget=1, stop_token_ids=[7]).check(L, runtime, "stop on the last token")
    assert _fired(last) == (True, R.STOP_TOKEN, 7) and last[0][R.BUDGET] == 0
    assert _fired(_single(3, 7, hist, budget=1, stop_sequences=[[7]]).check(L, runtime, "sequence on the last token")) == (True, R.STOP_SEQUENCE, 0)
    assert _fired(_single(3, 7, hist, budget=1, stop_token_ids=[8]).check(L, runtime, "budget")) == (True, R.LENGTH, -1)
    cache = _single(3, 7, hist, p=MAX_SEQ).check(L, runtime, "cache")
    assert _fired(cache) == (True, R.CACHE, -1) and cache[1][0] == MAX_SEQ - 1
    assert _fired(_single(3, 7, hist, budget=1, p=MAX_SEQ).check(L, runtime, "budget and cache")) == (True, R.LENGTH, -1)
    assert _fired(_single(3, 7, hist, eos=7, p=MAX_SEQ).check(L, runtime, "eos and cache")) == (True, R.STOP_TOKEN, 7)


@pytest.mark.parametrize("kw", [dict(stop_token_ids=[7]), dict(stop_sequences=[[9, 7]]), dict(eos=7)], ids=["id", "sequence", "eos"])
def test_min_new_tokens_holds_every_stop_back_but_the_budget(kw):
    L, runtime = _lib_rt()
    hist = [5, 6, 9]
    assert _fired(_single(3, 7, hist, min_new_tokens=4, **kw).check(L, runtime, "n + 1 == MIN"))[0]
    assert _fired(_single(3, 7, hist, min_new_tokens=5, **kw).check(L, runtime, "n + 1 == MIN - 1")) == (False, R.RUNNING, -1)
    assert _fired(_single(3, 7, hist, min_new_tokens=1, **kw).check(L, runtime, "MIN 1"))[0]
    assert _fired(_single(3, 7, hist, budget=1, min_new_tokens=9, **kw).check(L, runtime, "budget below MIN")) == (True, R.LENGTH, -1)
    assert _fired(_single(3, 7, hist, p=MAX_SEQ, min_new_tokens=9, **kw).check(L, runtime, "cache below MIN")) == (True, R.CACHE, -1)


# ---- 6. untouched slots, 7. all eight slots ------------------------------------------------------------------------------------------
def test_inactive_and_out_of_mask_slots_are_left_alone():
    L, runtime = _lib_rt()
    full = R.row(stop_token_ids=[7] * 16, stop_sequences=[[7]] * 8)
    hist = [[7] * STRIDE for _ in range(8)]
    st = _state(0b01100110, budget=1, produced=4, eos=7)
    for B, mask in [(8, 0b10101010), (4, 0xFF), (8, 0), (1, 0xFF)]:
        c = _Case(st, [7] * 8, [MAX_SEQ] * 8, hist, [full] * 8, B, mask)
        want = c.check(L, runtime, (B, mask))
        for b in range(8):
            served = b < B and (mask >> b) & 1 and (st[R.ACTIVE] >> b) & 1
            assert (want[2][b] != full) == bool(served) and (want[1][b] != MAX_SEQ) == bool(served), (B, mask, b)
        assert want[0][R.STEP] == st[R.STEP] + 1


def test_all_eight_slots_stop_in_one_launch_for_eight_reasons():
    L, runtime = _lib_rt()
    ids = list(range(100, 116))
    hist = [[50 + i for i in range(12)] + [t] for t in (100, 33, 115, 7, 8, 1, 2, 9)]
    stops = [R.row(stop_token_ids=ids), R.row(), R.row(stop_token_ids=ids), R.row(stop_sequences=[[7]]),
             R.row(stop_sequences=_seqs_with(7, hist[4][-8:])), R.row(stop_token_ids=ids), R.row(stop_sequences=[[44]]),
             R.row(stop_token_ids=[9], stop_sequences=[[61, 9]])]
    st = _state(0xFF, budget=[5, 5, 5, 5, 5, 1, 5, 5], produced=12, eos=[-1, 33, -1, -1, -1, -1, -1, -1])
    c = _Case(st, [h[-1] for h in hist], [20, 20, 20, 20, 20, 20, MAX_SEQ, 20], hist, stops, 8, 0xFF)
    want = c.check(L, runtime)
    assert want[0][R.ACTIVE] == 0
    assert [(r[R.REASON], r[R.MATCH]) for r in want[2]] == [(R.STOP_TOKEN, 100), (R.STOP_TOKEN, 33), (R.STOP_TOKEN, 115), (R.STOP_SEQUENCE, 0),
                                                            (R.STOP_SEQUENCE, 7), (R.LENGTH, -1), (R.CACHE, -1), (R.STOP_TOKEN, 9)]
    # ... and every other subset of them: the active word is assembled from all eight waves
    for keep in (0b00000001, 0b10000000, 0b01010101, 0b11101111):
        st2 = list(st)
        for b in range(8):
            if (keep >> b) & 1:  # this slot keeps running: nothing matches, budget and cache left
                st2[R.BUDGET + b], st2[R.EOS + b] = 5, -1
        stops2 = [R.row() if (keep >> b) & 1 else stops[b] for b in range(8)]
        pos2 = [20 if (keep >> b) & 1 else p for b, p in enumerate(c.pos)]
        assert _Case(st2, c.tokens, pos2, hist, stops2, 8, 0xFF).check(L, runtime, keep)[0][R.ACTIVE] == keep


# ---- 8. replays, 9. argument checks ---------------------------------------------------------------------------------------------
def test_fifty_replays_of_a_captured_launch_give_identical_buffers():
    L, runtime = _lib_rt()
    hist = [[50 + i for i in range(12)] + [7] for _ in range(8)]
    stops = [R.row(stop_sequences=_seqs_with(b, hist[b][-(b + 1):]), min_new_tokens=b) for b in range(8)]
    st = _state(0b11011011, budget=[3, 1, 3, 3, 3, 3, 3, 3], produced=12)
    c = _Case(st, [7] * 8, [20, 20, 20, MAX_SEQ, 20, 20, 20, 20], hist, stops, 8, 0b11110111)
    saved = [t.clone() for t in (c.d_state, c.d_pos, c.d_stops)]
    assert c.launch(L, runtime) == 0  # once outside the capture
    first = c.got()
    assert first == c.want()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with runtime.graph_capture(g):
        assert c.launch(L, runtime) == 0
    for i in range(50):
        for t, v in zip((c.d_state, c.d_pos, c.d_stops), saved):
            t.copy_(v)
        g.replay()
        assert c.got() == first, i


@pytest.mark.parametrize("kw", [dict(state=None), dict(tokens=None), dict(pos=None), dict(history=None), dict(stops=None), dict(B=0), dict(B=9),
                                dict(max_seq=0), dict(stride=7)])
def test_argument_checks_return_their_code_and_touch_nothing(kw):
    L, runtime = _lib_rt()
    c = _single(3, 7, [5, 6, 9], stop_token_ids=[7])
    assert c.launch(L, runtime, **kw) == -1  # TEAL_ERR_ARG
    assert c.got() == (c.state, c.pos, c.stops) and c.d_hist_all.tolist() == c.hist_flat

"""Host model of teal_batched_retire_stops (include/teal_hip.h): the rule restated in plain Python on lists, one slot after the
other — nothing of the kernel's lane layout, ballots or barrier.  `retire` changes its list arguments in place, as the launch
changes its buffers; `fire` is the same rule on one finished token stream, for the engine tests."""

ACTIVE, STEP, BUDGET, PRODUCED, EOS, FINISH, SLOT_WORDS = 0, 1, 8, 16, 24, 32, 40
MIN, NIDS, NSEQ, REASON, MATCH, IDS, SEQLEN, SEQ, WORDS = 0, 1, 2, 3, 4, 8, 24, 32, 96
RUNNING, STOP_TOKEN, STOP_SEQUENCE, LENGTH, CACHE = 0, 1, 2, 3, 4
NAMES = {STOP_TOKEN: "stop_token", STOP_SEQUENCE: "stop_sequence", LENGTH: "length", CACHE: "cache"}


def _hits(row, eos, hist, n, t):
    """(hit_id, lowest matching sequence or -1) for the token t of draw n, hist[c] the token of draw c < n"""
    if n + 1 < row[MIN]:
        return False, -1
    nids, nseq = min(max(row[NIDS], 0), 16), min(max(row[NSEQ], 0), 8)
    hit_id = (eos >= 0 and t == eos) or any(t == row[IDS + i] for i in range(nids))
    for q in range(nseq):
        ln = row[SEQLEN + q]
        if not 1 <= ln <= 8 or ln > n + 1:
            continue
        seq = row[SEQ + 8 * q:SEQ + 8 * q + ln]
        if seq[-1] == t and all(seq[j] == hist[n - ln + 1 + j] for j in range(ln - 1)):
            return hit_id, q
    return hit_id, -1


def retire(state, tokens, pos, history, stops, B, mask, max_seq, count_step):
    """state: SLOT_WORDS ints; tokens, pos: one int per slot; history: one list per slot; stops: 8 rows of WORDS ints"""
    act = state[ACTIVE] & 0xFFFFFFFF
    for b in range(B):
        if not ((mask >> b) & 1 and (act >> b) & 1):
            continue
        n, t, p, row = state[PRODUCED + b], tokens[b], pos[b], stops[b]
        state[BUDGET + b] -= 1
        state[PRODUCED + b] = n + 1
        hit_id, hit_seq = _hits(row, state[EOS + b], history[b], n, t)
        if hit_id:
            why, match = STOP_TOKEN, t
        elif hit_seq >= 0:
            why, match = STOP_SEQUENCE, hit_seq
        elif state[BUDGET + b] <= 0:
            why, match = LENGTH, -1
        elif p >= max_seq:
            why, match = CACHE, -1
        else:
            continue
        state[FINISH + b] = state[STEP]
        row[REASON], row[MATCH] = why, match
        state[ACTIVE] &= ~(1 << b)
        if p > max_seq - 1:
            pos[b] = max_seq - 1
    if count_step:
        state[STEP] += 1


def row(stop_token_ids=(), stop_sequences=(), min_new_tokens=0):
    """a stop row written by hand (independent of stopping.pack_row)"""
    r = [0] * WORDS
    r[MIN], r[NIDS], r[NSEQ], r[MATCH] = min_new_tokens, len(stop_token_ids), len(stop_sequences), -1
    for i in range(16):
        r[IDS + i] = stop_token_ids[i] if i < len(stop_token_ids) else -1
    for q in range(8):
        s = list(stop_sequences[q]) if q < len(stop_sequences) else []
        r[SEQLEN + q] = len(s)
        for j in range(8):
            r[SEQ + 8 * q + j] = s[j] if j < len(s) else -1
    return r


def fire(stream, budget, eos=-1, stop_token_ids=(), stop_sequences=(), min_new_tokens=0, first_pos=0, max_seq=1 << 30):
    """the rule run over `stream`, the tokens a request draws when nothing but its budget stops it: (tokens it produces, reason
    name, match).  first_pos: the position after its first draw (prompt length)."""
    state = [0] * SLOT_WORDS
    state[ACTIVE], state[BUDGET], state[EOS] = 1, budget, eos
    stops = [row(stop_token_ids, stop_sequences, min_new_tokens)] + [row() for _ in range(7)]
    hist, pos = [[]], [first_pos]
    for i, t in enumerate(stream):
        hist[0].append(t)
        retire(state, [t], pos, hist, stops, 1, 1, max_seq, True)
        if not state[ACTIVE] & 1:
            return stream[:i + 1], NAMES[stops[0][REASON]], stops[0][MATCH]
        pos[0] += 1
    raise AssertionError("the stream ended before the request did")

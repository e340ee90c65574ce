"""Host model of teal_constrain_logits (include/teal_hip.h): the rule restated in numpy on the raw words — the automaton image as
the launch reads it, a linear scan where the kernel searches, one row after the other; nothing of the kernel's bitmap, lower
bounds or workgroups.  `launch` changes `trace` and `out` in place, as the launch changes its buffers."""
import numpy as np

VIOLATION, STATE_MASK = 1 << 30, 0x3FFFFFFF


def neg_maxf(bf16: bool) -> int:
    """the 16 bits of -MAXF: the dtype's most negative finite value"""
    return 0xFF7F if bf16 else 0xFBFF


def image(states):
    """the words of an automaton given as [(edges [(token, next), ...], default, accept), ...], written by hand (independent of
    constraints.Automaton.image): S header rows {edge_begin, edge_end, default, accept}, offsets relative to the image, then the
    edges as (token, next) pairs"""
    S = len(states)
    words = [0] * (4 * S)
    for s, (edges, default, accept) in enumerate(states):
        words[4 * s:4 * s + 4] = [len(words), len(words) + 2 * len(edges), default, int(bool(accept))]
        for tok, nxt in edges:
            words += [tok, nxt]
    return words


def edges(img, s):
    b, e = img[4 * s], img[4 * s + 1]
    return [(int(img[i]), int(img[i + 1])) for i in range(b, e, 2)]


def delta(img, s, t):
    for tok, nxt in edges(img, s):
        if tok == t:
            return nxt
    return int(img[4 * s + 2])


def state_word(img, S, c, prev_word, t, e):
    """the trace word of draw c: the state, with bit 30 set on a violation"""
    if c == 0:
        return 0
    p = min(prev_word & STATE_MASK, S - 1)
    if t == e:
        return p
    d = delta(img, p, t)
    return d if d >= 0 else p | VIOLATION


def allowed(img, s, V, e):
    """bool [V]: what the mask keeps in state s for a request with EOS id e"""
    keep = np.full(V, img[4 * s + 2] >= 0)
    for tok, nxt in edges(img, s):
        keep[tok] = nxt >= 0
    if 0 <= e < V:
        keep[e] = bool(img[4 * s + 3])
    return keep


def mask(bits, img, s, e, bf16):
    return np.where(allowed(img, s, len(bits), e), bits, np.uint16(neg_maxf(bf16)))


def launch(lbits, bf16, tokens, counters, eos, table, arena, trace, out, active=None, slot0=0):
    """lbits, out: uint16 [B][V]; tokens, counters, eos: one int per row; table: [B][4]; arena: the words; trace: int [B][L]"""
    arena = np.asarray(arena)
    for r in range(lbits.shape[0]):
        if active is not None and not (active >> (slot0 + r)) & 1:
            continue
        base, S = int(table[r][0]), int(table[r][1])
        c = int(counters[r])
        if base < 0:
            out[r] = lbits[r]
            trace[r][c] = 0
            continue
        img = arena[base:]
        w = state_word(img, S, c, int(trace[r][c - 1]) if c else 0, int(tokens[r]), int(eos[r]))
        trace[r][c] = w
        out[r] = mask(lbits[r], img, w & STATE_MASK, int(eos[r]), bf16)

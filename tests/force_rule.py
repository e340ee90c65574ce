"""The forced-token rule of include/teal_hip.h (teal_force_tokens) in numpy, and what the batcher reports of a forced request.

Nothing here imports the package: the rule is restated from the header's words, so a test that compares the device (or the
batcher's Forced feature) with it compares two independent statements.
"""
import numpy as np


def force_tokens(forced, forced_len, rng_state, tokens, history, active=None, slot0=0):
    """One launch on copies of the buffers -> (tokens, history).  forced: int32 [B][forced_stride]; forced_len: int32 [B];
    rng_state: uint64 [B][2] (word 1: the draw counter the sampler has just bumped); tokens: int32 [B]; history: int32
    [B][history_len] or None; active: None or the active word (an int)."""
    forced = np.asarray(forced, dtype=np.int32)
    B, stride = forced.shape
    tokens = np.array(tokens, dtype=np.int32, copy=True)
    history = None if history is None else np.array(history, dtype=np.int32, copy=True)
    for r in range(B):
        c = int(np.asarray(rng_state, dtype=np.uint64)[r][1])
        i = c - 1
        n = min(int(forced_len[r]), stride)
        if (active is None or (int(active) >> (slot0 + r)) & 1) and 0 <= i < n:
            t = forced[r, i]
            tokens[r] = t
            if history is not None and i < history.shape[1]:
                history[r, i] = t
    return tokens, history


def expected_result(given, produced_tokens, logprobs, top_ids):
    """What the batcher reports for one request: given (its forced tokens, or None), the tokens it produced, each draw's fp32
    logprob and each draw's top-1 id -> (forced, loglikelihood, is_greedy), or (None, None, None) without forced tokens.
    forced: the forced draws it made — fewer than given if it ended first; loglikelihood: their logprobs added in draw order in
    Python floats; is_greedy: every one of those tokens was its row's top-1 id."""
    if not given:
        return None, None, None
    k = min(len(given), len(produced_tokens))
    assert list(produced_tokens[:k]) == list(given[:k]), "a forced draw yields the forced token"
    total = 0.0
    for v in logprobs[:k]:
        total += float(v)
    return k, total, all(int(top_ids[i]) == int(given[i]) for i in range(k))

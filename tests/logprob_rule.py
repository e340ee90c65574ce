"""The token-logprob rule (teal_amd/csrc/teal_logprob.hip) restated in numpy fp64 — the truth the GPU tests compare against.

    lp(t) = (l[t] - m) - log sum_v exp(l[v] - m),  m = max_v l[v]

on the row's 16-bit logits, widened exactly; the top-n are the first n of a stable sort on (-logit, id).
"""
import numpy as np

NAN_BITS = 0x7FC0DEAD  # the fill pattern of output buffers: a quiet NaN no kernel produces


def logprobs64(row) -> np.ndarray:
    """fp64 [V]: the log-softmax of one row (any float dtype; -inf contributes 0)"""
    l = np.asarray(row, dtype=np.float64)
    m = l.max()
    return (l - m) - np.log(np.exp(l - m).sum())


def top_n(row, n: int) -> np.ndarray:
    """ids of the n largest logits, by descending logit, equal logits by ascending id"""
    l = np.asarray(row, dtype=np.float64)
    return np.argsort(-l, kind="stable")[:n].astype(np.int64)


def tol(truth) -> np.ndarray:
    """4 fp32 ulps of max(1, |truth|): the subtraction rounds to 1/2 ulp, expf to 1 ulp per term, logf to 1 ulp, and the fp32
    sum (1024 strided partial sums, then a tree) stays below 1 ulp of its result"""
    t = np.maximum(1.0, np.abs(np.asarray(truth, dtype=np.float64)))
    return 4.0 * np.spacing(t.astype(np.float32)).astype(np.float64)


def close(got, truth) -> bool:
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return bool((np.abs(got - truth) <= tol(truth)).all())


def worst(got, truth) -> float:
    """the largest error in units of the tolerance (for messages)"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return float((np.abs(got - truth) / tol(truth)).max()) if got.size else 0.0

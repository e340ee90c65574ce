"""numpy restatement of TEAL's rule for a batch of sequences (tests of teal_batched.hip / BatchedDecodeEngine).

Sequence b's projection is W . (x_b * [float32(|x_b|) > float32(tau)]), each threshold segment (a column range of the
output: q / k / v, gate / up) with its own tau.  A batched launch reads the union of the rows any sequence keeps."""
import numpy as np


def keep_masks(x, tau):
    """x [B, Z] (the 16-bit activations as float32) -> bool [B, Z]"""
    return np.abs(np.asarray(x, dtype=np.float32)) > np.float32(tau)


def union_rows(masks):
    """bool [B, Z] -> bool [Z]: the rows a batched launch reads"""
    return np.asarray(masks).any(0)


def batched_gemv(W, x, bounds, taus):
    """W [N, Z], x [B, Z] -> float64 [B, N]; output columns [bounds[s-1], bounds[s]) use taus[s]"""
    W = np.asarray(W, dtype=np.float64)
    x = np.asarray(x, dtype=np.float32)
    y = np.zeros((x.shape[0], W.shape[0]))
    lo = 0
    for hi, tau in zip(bounds, taus):
        xm = np.where(keep_masks(x, tau), x, 0).astype(np.float64)
        y[:, lo:hi] = xm @ W[lo:hi].T
        lo = hi
    return y


def kept_counts(x, bounds, taus):
    """per segment: ([kept rows per sequence], union rows)"""
    out = []
    for tau in taus[:len(bounds)]:
        m = keep_masks(x, tau)
        out.append((m.sum(1).tolist(), int(union_rows(m).sum())))
    return out

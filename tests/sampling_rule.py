"""Host model of per-request sampling (teal_amd/csrc/teal_sample_rows.hip; the rule is stated in include/teal_hip.h), numpy only.

A row has four parameters {temperature, top_k, top_p, min_p}.  The filters apply in this order:

  1. temperature  inv = 1 / max(T, 1e-5), t_i = fl(fl(x_i - max) * inv) in fp32 — sampler_rule.draws' expression;
  2. top_k        sampler_rule.kept_set: every logit not below the k-th largest value, ties kept (0 < k < V; else no filter) -> K1;
  3. top_p        over K1, w_i = exp(t_i), Z = sum of w, A(v) = the mass of the members of K1 with a value strictly above v: a logit of
                  value v stays iff A(v) < top_p * Z (HF's TopPLogitsWarper on the renormalised top-k set, decided by value: equal
                  logits stay or go together, the maximum always stays); top_p >= 1: no filter;
  4. min_p        a logit stays iff exp(t_i) >= min_p; min_p == 0: no filter;
  5. the race     sampler_rule's, over what stayed.

Every filter is "value >= threshold" and the maximum passes all of them, so the kept sets are nested: with the distinct values
sorted downwards, a kept set is the first n classes for some n, and the NUMBER of logits kept identifies it.  That is how this
model hands a kept set to sampler_rule: draws(bits, top_k = kept count) keeps exactly the logits not below the count-th largest
value.

A and Z are float64 sums of float64 exp(t_i) of the exact fp32 t_i.  The device sums fp32 expf values; the model therefore calls a
row's top-p decision OPEN if some class below the maximum has |A(v) - top_p * Z| <= MARGIN * Z, and its min-p decision open if some
value has |exp(t) - min_p| <= MARGIN * min_p.  An open row has more than one legitimate kept set: each boundary class in, or out.

MARGIN = 1e-5.  Where it comes from: 1024 threads summing V / 1024 <= 128 terms each in fp32 and a tree over the partials are within
about (128 + 10 + E) * 2^-24 of exact for an expf good to E ulps — 9.5e-6 at E = 20.  The kernel accumulates 64-bit fixed-point
integers instead (trunc(expf(t) * 2^40)): its sums lose less than 2^-23 * Z to the truncation and are otherwise as good as expf,
(E + 2) * 2^-24 * Z, far inside the margin.  No bound for expf is documented by the toolchain, so the margin is not tightened to
one that would rest on a guess of E.
"""
import numpy as np

import sampler_rule as SR
from spec_rule import hash3, uniform  # noqa: F401  (the race's stream, re-exported for the tests)

MARGIN = 1e-5


def _classes(bits, bf16, temperature):
    """distinct values of the row, downwards: (class index of every logit [V], fp32 t per class, logits per class)"""
    x = SR.decode(bits, bf16)
    inv = np.float32(1.0) / max(np.float32(temperature), np.float32(1e-5))
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((x - x.max()) * inv).astype(np.float32)
    vals, inverse, counts = np.unique(-x.astype(np.float64), return_inverse=True, return_counts=True)  # (-0.0 == +0.0: one class)
    tc = np.empty(vals.size, dtype=np.float32)
    tc[inverse] = t  # equal values have equal t
    return inverse, tc, counts


def kept(bits, bf16, temperature, top_k, top_p=1.0, min_p=0.0, margin=MARGIN):
    """-> (mask [V] of the logits that enter the race, count, open, counts): `counts` is the sorted tuple of every legitimate
    kept count (just `count` unless the row is open)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    cls, t, n_in = _classes(bits, bf16, temperature)
    m = t.size
    cum = np.cumsum(n_in)                                        # logits in the first j + 1 classes
    nk = int(cls[SR.kept_set(bits, bf16, int(top_k or 0))].max()) + 1  # classes of K1 (a prefix: kept_set is a value threshold)
    w = np.exp(t.astype(np.float64))
    p_alts, m_alts = {m}, {m}
    base_p = base_m = m
    if top_p < 1.0:
        mass = (w * n_in)[:nk]
        Z = mass.sum()
        A = np.concatenate([[0.0], np.cumsum(mass)[:-1]])       # mass strictly above each class
        base_p = int((A < float(top_p) * Z).sum())               # A is non-decreasing: a prefix
        near = np.flatnonzero(np.abs(A - float(top_p) * Z) <= margin * Z)
        near = near[near > 0]                                    # the maximum always stays
        p_alts = {base_p} | {int(j) for j in near} | {int(j) + 1 for j in near}
    if min_p > 0.0:
        base_m = int((w >= float(min_p)).sum())                  # w is non-increasing over the classes: a prefix
        near = np.flatnonzero(np.abs(w - float(min_p)) <= margin * float(min_p))
        near = near[near > 0]
        m_alts = {base_m} | {int(j) for j in near} | {int(j) + 1 for j in near}
    n = min(nk, base_p, base_m)
    alts = sorted({min(nk, a, b) for a in p_alts for b in m_alts})
    counts = tuple(int(cum[a - 1]) for a in alts)
    return cls < n, int(cum[n - 1]), len(counts) > 1, counts


def draws_from(bits, bf16, count, temperature, seed, ctr0, n):
    """sampler_rule.draws over the kept set that `count` identifies -> (token [n], runner_up [n], open [n])"""
    return SR.draws(bits, bf16, int(count), temperature, seed, ctr0, n)


def draws(bits, bf16, temperature, top_k, top_p, min_p, seed, ctr0, n):
    """n consecutive draws of a row -> (token [n], runner_up [n], race open [n], kept count, kept-set open, legitimate counts)"""
    _, count, is_open, counts = kept(bits, bf16, temperature, top_k, top_p, min_p)
    tok, ru, op = draws_from(bits, bf16, count, temperature, seed, ctr0, n)
    return tok, ru, op, count, is_open, counts

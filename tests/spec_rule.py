"""numpy restatement of teal_spec_accept (include/teal_hip.h) and torch restatement of the reference's acceptance
(gpt-fast/generate.py:123-146), shared by tests/test_speculative_rule.py (CPU) and tests/test_speculative_gpu.py."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def hash3(a, b, c):
    """the fused sampler's counter-based hash (teal_common.h), vectorised over c"""
    a, b = np.uint64(a) & M32, np.uint64(b) & M32
    c = np.asarray(c, dtype=np.uint64) & M32
    h = ((a * np.uint64(0x9E3779B1)) & M32) ^ (((b + np.uint64(0x7F4A7C15)) & M32) * np.uint64(0x85EBCA77) & M32) \
        ^ (((c + np.uint64(0x165667B1)) & M32) * np.uint64(0xC2B2AE3D) & M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def uniform(h):
    return (((h >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def order_key16(bits):
    b = bits.astype(np.uint32)
    b = np.where(b == 0x8000, 0, b)  # -0.0 keys as +0.0 (teal_common.h)
    return np.where(b & 0x8000, (~b) & 0xFFFF, b | 0x8000)


def row_probs(bits: np.ndarray, bf16: bool, top_k: int, temperature: float) -> np.ndarray:
    """16-bit logits (raw bits) -> /temperature -> top-k (ties at the pivot kept) -> softmax, in fp32 like the kernel"""
    bits = bits.astype(np.uint16)
    x = (bits.astype(np.uint32) << 16).view(np.float32) if bf16 else bits.view(np.float16).astype(np.float32)
    inv = np.float32(1.0) / np.float32(max(temperature, 1e-5))
    keys = order_key16(bits)
    pivot = 0
    if 0 < top_k < x.size:
        pivot = np.sort(keys)[::-1][top_k - 1]
    w = np.exp(((x - x.max()) * inv).astype(np.float32)).astype(np.float32)
    w = np.where(keys >= pivot, w, np.float32(0))
    return (w / np.float32(w.sum(dtype=np.float32))).astype(np.float32)


def accept_numpy(q: np.ndarray, p: np.ndarray, drafts, seed: int, ctr: int, eps: float = 1e-5):
    """q [k+1][V], p [k][V] probabilities; drafts [k].  Returns (n accepted, token, near) — near: a decision within eps (u vs
    the ratio, or the race's top two scores) that fp32 rounding may flip."""
    k, V = p.shape
    u = uniform(hash3(seed, ctr, np.arange(k)))
    n, near = k, False
    for i in range(k):
        d = int(drafts[i])
        qi, pi = np.float32(q[i, d]), np.float32(p[i, d])
        ratio = np.float32(min(np.float32(1), qi / pi)) if pi > 0 else np.float32(-1)
        near |= pi > 0 and abs(float(u[i]) - float(ratio)) < eps
        if not (pi > 0 and u[i] <= ratio):
            n = i
            break
    e = (-np.log(uniform(hash3(seed, ctr + 1, np.arange(V))))).astype(np.float32)
    w = np.maximum(q[n] - p[n], 0).astype(np.float32) if n < k else q[n]
    if not (w > 0).any():
        w = q[n]
    s = (w / e).astype(np.float32)
    top2 = np.sort(s)[-2:]
    near |= bool(top2[1] > 0 and (top2[1] - top2[0]) <= eps * top2[1])
    return n, int(np.argmax(s)), near


def accept_reference_torch(q: torch.Tensor, p: torch.Tensor, drafts: torch.Tensor, u: torch.Tensor, exp_noise: torch.Tensor):
    """gpt-fast/generate.py:123-146 with its two random draws supplied: `u` (torch.rand_like of the ratios) and `exp_noise`
    (the Exp(1) draws of multinomial_sample_one_no_sync)."""
    k = p.shape[0]
    draft_probs = p[torch.arange(k), drafts]
    target_probs = q[torch.arange(k), drafts]
    accept_draft_prob = torch.minimum(torch.ones(()), target_probs / draft_probs)
    rejected = (u > accept_draft_prob).nonzero()
    if rejected.shape[0] == 0:
        return k, int(torch.argmax(q[-1] / exp_noise))
    n = int(rejected[0].item())
    new = q[n] - p[n]
    new = torch.where(new > 0, new, 0.0)
    new = new / new.sum()
    return n, int(torch.argmax(new / exp_noise))

"""Inputs and fp64 references of the attention probes, in plain torch on any device (not a test file): shared by
tests/test_attention_probes_host.py (CPU: the probes' own power) and tests/test_attention_probes_gpu.py (the HIP kernels).

Two designs:

  * equal needles (row coverage, exact).  Per KV head one key kappa = a s (s random +-1, a^2 sqrt(hd) ~ 32) is written
    bit-identically into the cache rows of a needle set R, |R| = m a power of two <= 64; every other row is background
    (std 0.5), V ~ N(0, 1), the query is unrope_pos(kappa).  The needles' scores are bit-equal whatever a kernel rounds,
    1 / m and exp(0) are exact, equal running maxima rescale by exactly 1: the answer is mean(V[R]) and the bound is
    1 ulp + 2^-20 max|V| (tol_needle).  Sweeping R over a partition of the rows (strided_sets) makes every cache row a needle
    in exactly one launch.  Row pos + 1 holds kappa with V = 100 and the rows behind it NaN: reading too far shows as well.
  * peaked random inputs (softmax numerics): q ~ N(0, 2^2), K, V ~ N(0, 1) — score std ~2, a few rows carry the weight, the
    output is O(1) — bounded by the measured error of a 16-bit emulation of the same maths (attend_emulated, peaked_bound).

Everything is drawn on the CPU from a seeded generator and then moved, so the host tests pin the very inputs the GPU sees.
"""
import math

import torch

MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -24, torch.bfloat16: -133}
NEEDLE_SCORE = 32.0           # q . kappa / sqrt(hd)
GUARD_V = 100.0               # V of the over-read guard row
OUTSIDE_MAX = 2.0 ** -16      # dominance precondition: softmax weight outside the needle set (fp64 reference)
STAIR0, STAIR_STEP = 28.0, 24.0  # multi-token staircase: score of new row t' is 28 + 24 t'


# ---- number formats --------------------------------------------------------------------------------------------------------

def ulp(y64, dt):
    """spacing of dt's numbers at |y64| (fp64 tensor in, fp64 out)"""
    _, e = torch.frexp(y64.abs().double())  # |y| = f 2^e, f in [0.5, 1)
    e = torch.where(y64 == 0, torch.full_like(e, MIN_EXP[dt]), e - 1 - MANT[dt]).clamp(min=MIN_EXP[dt])
    return torch.ldexp(torch.ones_like(y64, dtype=torch.float64), e)


def tol_needle(y64, vmax, dt):
    """part 1: one rounding to dt is 1/2 ulp, fp32 accumulation of <= 64 unit-weight terms and one division stay under
    2^-20 relative to max|V|, another 1/2 ulp for a sum that lands next to a rounding boundary"""
    return ulp(y64, dt) + 2.0 ** -20 * vmax


def err_rel(y, y64):
    """part 2: max over heads of max_d |y - y64| / max_d |y64|   (y, y64: [..., H, hd])"""
    return float(((y.double() - y64).abs().amax(-1) / y64.abs().amax(-1)).max())


def peaked_bound(err_emulation, dt):
    """kernel and emulation are two summation orders of the same roundings: independent draws of one size"""
    return 2.0 * err_emulation + (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7)


# ---- RoPE ------------------------------------------------------------------------------------------------------------------

def rope_table(S, hd, dt, base=10000.0):
    """(cos, sin) [S, hd/2, 2] in dt, the module path's table (gpt_fast/model.py precompute_freqs_cis)"""
    inv = 1.0 / (base ** (torch.arange(0, hd, 2)[: hd // 2].float() / hd))
    ang = torch.outer(torch.arange(S).float(), inv)
    return torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1).to(dt)


def rotate(x, cs, inverse=False):
    """interleaved-pair rotation of x [..., hd] by table rows cs [..., hd/2, 2], fp32 arithmetic, one rounding to x's dtype
    (a product of two 16-bit values is exact in fp32: the module path's apply_rotary_emb and the kernels' fmaf give these bits);
    inverse: by the opposite angle (unrope)"""
    xs = x.float().reshape(*x.shape[:-1], -1, 2)
    c, s = cs[..., 0].float(), cs[..., 1].float()
    if inverse:
        s = -s
    re = xs[..., 0] * c - xs[..., 1] * s
    im = xs[..., 1] * c + xs[..., 0] * s
    return torch.stack((re, im), dim=-1).flatten(-2).to(x.dtype)


# ---- needle sets -----------------------------------------------------------------------------------------------------------

def needle_m(n_rows):
    return 16 if n_rows <= 4096 else 64


def strided_sets(n_rows, m_max=None):
    """partition of rows 0 .. n_rows-1 into ceil(n_rows / m) strided sets of m rows, m the largest power of two <=
    min(m_max, n_rows): row r is a needle of set r mod n_sets.  A set short of m rows is padded with the lowest rows that are
    not its own (rows of set 0, or of set 1 for set 0).  LongTensor [n_sets, m]"""
    if n_rows <= 0:
        return torch.empty(0, 1, dtype=torch.long)
    m_max = needle_m(n_rows) if m_max is None else m_max
    m = 1 << (min(m_max, n_rows).bit_length() - 1)
    n_sets = -(-n_rows // m)
    sets = []
    for i in range(n_sets):
        own = list(range(i, n_rows, n_sets))
        r = 0
        while len(own) < m:
            if r % n_sets != i:
                own.append(r)
            r += 1
        sets.append(own)
    t = torch.tensor(sets, dtype=torch.long)
    assert t.shape == (n_sets, m) and all(len(set(s)) == m for s in sets) and int(t.max()) < n_rows
    return t


def needle_key(n_kv, hd, dt, gen, score=NEEDLE_SCORE):
    """kappa [n_kv, hd] = a s with kappa . kappa / sqrt(hd) ~ score, and the sign vectors s"""
    s = (torch.randint(0, 2, (n_kv, hd), generator=gen) * 2 - 1).float()
    return (math.sqrt(score / math.sqrt(hd)) * s).to(dt), s


# ---- references ------------------------------------------------------------------------------------------------------------

def _kv_of(n_head, n_kv, kv_shift):
    return (torch.arange(n_head) // (n_head // n_kv) + kv_shift) % n_kv


def attend64(q_rot, K, V, visible, scale, weights=None, kv_shift=0):
    """fp64 attention.  q_rot [T, H, hd] rotated queries, K / V [n_kv, N, hd] cache rows, query t sees rows 0 .. visible[t]-1.
    weights [N] or [T, N]: row multiplicities (fault models: 0 drops a row, 2 counts it twice); kv_shift: query head h reads
    KV head kvh + kv_shift (fault model).  Returns y [T, H, hd] and the probabilities [T, H, N]"""
    T, H, _ = q_rot.shape
    n_kv, N, _ = K.shape
    kv = _kv_of(H, n_kv, kv_shift).to(K.device)
    K64, V64 = K.double()[kv], V.double()[kv]                      # [H, N, hd]
    s = torch.einsum("thd,hnd->thn", q_rot.double(), K64) * scale
    vis = torch.as_tensor(visible, device=K.device).view(T, 1)
    seen = torch.arange(N, device=K.device).view(1, N) < vis     # [T, N]
    s = s.masked_fill(~seen.view(T, 1, N), float("-inf"))
    if weights is not None:
        s = s + torch.log(weights.double().to(K.device)).view(-1, 1, N)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("thn,hnd->thd", p, V64), p


def attend_emulated(q_rot, K, V, visible, scale, dt):
    """the module path's rounding points in torch: scores, probabilities and output rounded to dt, fp32 accumulation — the most
    any kernel here performs.  Same arguments as attend64; y [T, H, hd] in dt"""
    T, H, _ = q_rot.shape
    n_kv, N, _ = K.shape
    kv = _kv_of(H, n_kv, 0).to(K.device)
    s = (torch.einsum("thd,hnd->thn", q_rot.float(), K.float()[kv]) * scale).to(dt).float()
    vis = torch.as_tensor(visible, device=K.device).view(T, 1)
    seen = torch.arange(N, device=K.device).view(1, N) < vis
    s = s.masked_fill(~seen.view(T, 1, N), float("-inf"))
    p = torch.softmax(s, dim=-1).to(dt).float()
    return torch.einsum("thn,hnd->thd", p, V.float()[kv]).to(dt)


def sweep_reference(q_rot, K, V, kappa, sets, visible, scale, fn=attend64, **kw):
    """one reference per needle set: K is the cache with background in every swept row; set i's launch sees kappa in rows sets[i].
    Returns y [n_sets, T, H, hd] and outside [n_sets, T, H], the probability mass off the needle set (fn = attend64)"""
    ys, outs = [], []
    Kw = K.double() if fn is attend64 else K.clone()
    kap = kappa.to(Kw.dtype).to(Kw.device)
    for rows in sets.to(K.device):
        keep = Kw[:, rows].clone()
        Kw[:, rows] = kap[:, None, :]
        r = fn(q_rot, Kw, V, visible, scale, **kw)
        Kw[:, rows] = keep
        if fn is attend64:
            ys.append(r[0])
            outs.append(1.0 - r[1][:, :, rows].sum(-1))
        else:
            ys.append(r)
    return torch.stack(ys), (torch.stack(outs) if outs else None)


def outside_upper_bound(q_rot, K, kappa, n_rows, m, scale):
    """a cheap bound on the precondition of EVERY set of a sweep at once: sum over all rows 0 .. n_rows-1 of exp(background score -
    needle score) / m  >=  the softmax weight outside any needle set of m rows.  [T, H]"""
    T, H, _ = q_rot.shape
    kv = _kv_of(H, K.shape[0], 0).to(K.device)
    s = torch.einsum("thd,hnd->thn", q_rot.double(), K[:, :n_rows].double()[kv]) * scale
    sn = torch.einsum("thd,hd->th", q_rot.double(), kappa.double().to(K.device)[kv]) * scale
    return torch.exp(s - sn[..., None]).sum(-1) / m


# ---- cases -----------------------------------------------------------------------------------------------------------------

class Case:
    """plain record of one probe's inputs (CPU tensors; .to(device) moves every tensor)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return Case(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})


def _guarded_cache(n_kv, S, hd, dt, gen, first_free, guard_key, k_std=0.5):
    """K ~ N(0, k_std^2), V ~ N(0, 1); the guard (guard_key, V = 100) in row first_free, NaN in every row behind it"""
    kc = (torch.randn(n_kv, S, hd, generator=gen) * k_std).to(dt)
    vc = torch.randn(n_kv, S, hd, generator=gen).to(dt)
    g = first_free
    if g < S:
        kc[:, g] = guard_key
        vc[:, g] = GUARD_V
    kc[:, g + 1:] = float("nan")
    vc[:, g + 1:] = float("nan")
    return kc, vc


def decode_case(n_head, n_kv, hd, pos, S, dt, seed, appended=True, newest="background", peaked=False):
    """one decode token at position pos over a cache of S rows.

    appended: the kernel builds row pos from (k_new, v_new) with its own RoPE (rows 0 .. pos-1 are swept); otherwise the
    row is already in the cache and q arrives rotated (teal_decode_attention_split_roped: rows 0 .. pos are swept).
    newest = "needle": k_new = unrope_pos(kappa), no other needle: the answer is v_new.  peaked: part 2's input law, no needles.
    kc / vc: background, the guard in row pos + 1, NaN behind it.  qkv = q | k_new | v_new as the projection hands them over."""
    gen = torch.Generator().manual_seed(seed)
    rep = n_head // n_kv
    kappa, _ = needle_key(n_kv, hd, dt, gen)
    kc, vc = _guarded_cache(n_kv, S, hd, dt, gen, pos + 1, kappa, k_std=1.0 if peaked else 0.5)
    rope = rope_table(S, hd, dt)
    cs = rope[pos]
    k_bg = (torch.randn(n_kv, hd, generator=gen) * (1.0 if peaked else 0.5)).to(dt)
    v_new = torch.randn(n_kv, hd, generator=gen).to(dt)
    q_peaked = (torch.randn(n_head, hd, generator=gen) * 2.0).to(dt)
    target = kappa.repeat_interleave(rep, 0)                     # [H, hd]: what the rotated query should be
    if peaked:
        q = q_peaked
        q_rot = rotate(q, cs) if appended else q
    elif appended:
        q = rotate(target, cs, inverse=True)
        q_rot = rotate(q, cs)
    else:
        q = q_rot = target
    k_new = rotate(kappa, cs, inverse=True) if (newest == "needle" and not peaked) else k_bg
    n_sweep = 0 if (newest == "needle" or peaked) else (pos if appended else pos + 1)
    return Case(n_head=n_head, n_kv=n_kv, hd=hd, pos=pos, S=S, dt=dt, appended=appended, kappa=kappa, kc=kc, vc=vc, rope=rope, q=q,
                q_rot=q_rot.view(1, n_head, hd), k_new=k_new, v_new=v_new, k_row=rotate(k_new, cs), sets=strided_sets(n_sweep),
                qkv=torch.cat([q.reshape(-1), k_new.reshape(-1), v_new.reshape(-1)]), visible=[pos + 1], scale=1.0 / math.sqrt(hd))


def finished_cache(c):
    """the cache as a correct appending kernel leaves it (host side; the GPU tests use the kernel's own)"""
    kc, vc = c.kc.clone(), c.vc.clone()
    if c.appended:
        kc[:, c.pos] = c.k_row
        vc[:, c.pos] = c.v_new
    return kc, vc


def multi_case(n_head, n_kv, hd, T, p0, S, dt, seed, mode, peaked=False):
    """T new tokens at positions p0 .. p0+T-1 (teal_verify_attention; teal_prefill_attention at p0 = 0).

    mode "staircase": k_t' = unrope(a_t' s) with score 28 + 24 t' against every query unrope(2 s): query t must return v_t.
    The guard row p0 + T is the next stair up (V = 100).  mode "sweep": new rows background, q_t = unrope(kappa), rows
    0 .. p0-1 swept, the guard row holds kappa.  q, k, v: [T, heads, hd] before RoPE; k_rows: the cache rows a kernel must write."""
    gen = torch.Generator().manual_seed(seed)
    rep = n_head // n_kv
    kappa, sgn = needle_key(n_kv, hd, dt, gen)
    stair = lambda t: ((STAIR0 + STAIR_STEP * t) / (2.0 * math.sqrt(hd)) * sgn).to(dt)  # noqa: E731
    guard = stair(T) if mode == "staircase" else kappa
    kc, vc = _guarded_cache(n_kv, S, hd, dt, gen, p0 + T, guard, k_std=1.0 if peaked else 0.5)
    rope = rope_table(S, hd, dt)
    cs = rope[p0:p0 + T].unsqueeze(1)                           # [T, 1, hd/2, 2]
    k_bg = (torch.randn(T, n_kv, hd, generator=gen) * (1.0 if peaked else 0.5)).to(dt)
    v = torch.randn(T, n_kv, hd, generator=gen).to(dt)
    q_peaked = (torch.randn(T, n_head, hd, generator=gen) * 2.0).to(dt)
    if peaked:
        q, k = q_peaked, k_bg
    elif mode == "staircase":
        q = rotate((2.0 * sgn).to(dt).repeat_interleave(rep, 0).expand(T, n_head, hd), cs, inverse=True)
        k = rotate(torch.stack([stair(t) for t in range(T)]), cs, inverse=True)
    else:
        q = rotate(kappa.repeat_interleave(rep, 0).expand(T, n_head, hd), cs, inverse=True)
        k = k_bg
    n_sweep = p0 if (mode == "sweep" and not peaked) else 0
    return Case(n_head=n_head, n_kv=n_kv, hd=hd, T=T, p0=p0, S=S, dt=dt, kappa=kappa, kc=kc, vc=vc, rope=rope, q=q, k=k, v=v,
                q_rot=rotate(q, cs), k_rows=rotate(k, cs), sets=strided_sets(n_sweep), visible=[p0 + t + 1 for t in range(T)],
                qkv=torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1), scale=1.0 / math.sqrt(hd))


def finished_multi_cache(c):
    kc, vc = c.kc.clone(), c.vc.clone()
    kc[:, c.p0:c.p0 + c.T] = c.k_rows.transpose(0, 1)
    vc[:, c.p0:c.p0 + c.T] = c.v.transpose(0, 1)
    return kc, vc


def slabs_of(qkv, R, split=2):
    """the projection's fp32 split-K slabs [split][features][R] whose slice-order sum is exactly qkv [T, features] (16-bit values:
    x / split is exact for split 2); columns >= T hold 3.0, which no kernel may use"""
    T, n = qkv.shape
    assert split == 2
    s = torch.full((split, n, R), 3.0, dtype=torch.float32, device=qkv.device)
    s[:, :, :T] = (qkv.float() * 0.5).t()
    return s


# ---- the shapes: the smallest that reach each code path (teal_attention.hip: STEP, PF, RD, kGqaMinSeq*; teal_chunked_attention.h:
#      kAttnChunk = 32) ------------------------------------------------------------------------------------------------------
#          (n_head, n_kv, hd, pos, S)
SINGLE = ((4, 2, 64, 0, 64), (4, 2, 64, 255, 256),
          (8, 2, 128, 256, 512),                       # one row past the 256-row V prefetch
          (4, 4, 128, 1023, 1024), (4, 1, 64, 2047, 2048))
#          (n_head, n_kv, hd, pos, S, nsplit)
SPLIT = ((32, 32, 128, 255, 333, 4), (32, 32, 128, 300, 333, 4),   # 16-row groups: 4, then 5 per workgroup
         (8, 8, 128, 2047, 4096, 8), (8, 8, 128, 2048, 4096, 8),   # 64-row groups, the first refill
         (16, 4, 64, 4095, 4096, 4),                               # per-head kernel through the rotated hand-over only: 4 heads per
                                                                   # KV head at 4096 rows take the grouped-query kernel otherwise
         (4, 4, 64, 5000, 8192, 3),                                # ragged: 5 / 5 / 4 groups
         (8, 1, 128, 0, 512, 8))
GQA = ((16, 2, 128, 2047, 2048, 16),                               # 8 query heads per KV head
       (8, 2, 64, 4095, 4096, 16),                                 # 4 per KV head
       (64, 8, 128, 5000, 8192, 32))
MULTI_HEADS = ((32, 32, 128), (32, 8, 128), (8, 8, 64), (8, 2, 64))
MULTI_MAX_SEQ = 1040
VERIFY_T, VERIFY_SWEEP_T, PREFILL_T = (1, 2, 8, 9, 16), (1, 9, 16), (2, 5, 8, 9, 16)
BATCHED_POS = (0, 5, 31, 32, 700, 1039)
BATCHED_B = (1, 3, 8)


def verify_p0(T, max_seq=MULTI_MAX_SEQ):
    return (0, 1, 31, 32, 33, 1000, max_seq - T)


def batched_positions(B, salt):
    """B positions drawn from BATCHED_POS: a rotation, so that every position is some sequence's at B = 8"""
    return [BATCHED_POS[(salt + b) % len(BATCHED_POS)] for b in range(B)]

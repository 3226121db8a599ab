"""Plain restatements of csrc/ssd.hip for tests/test_hip_ssd.py and tests/test_ssd_host.py.  numpy on the CPU, no GPU.

* ratio_f32: r = 0 where F_forget == 0, else F_forget / F_keep -- one f32 division (0/0 -> 0, x/0 -> +inf, never a NaN).
* select: r > threshold (strict) or r >= threshold; kth_largest: the k-th largest value by the INTEGER key bits & 0x7fffffff, which
  for ratios >= 0 (and +inf) is the order of the values -- what siss_absf_select returns.
* dampen_f32: beta = lambda / r where r > lambda, else 1 (one f32 division), p' = p * beta (one f32 multiplication) on the selected;
  every other element is returned as it was.  beta_min is the min(lambda / r, 1) form of the same thing.
* stats_f64: the seven statistics of siss_ssd_dampen from the SAME f32 values, counts as integers, sums by math.fsum (exact): the
  kernel's f64 sums differ from these by their fold order alone.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
SIZES = [1027, 4_197_379]       # two blocks + a 3-float tail; 2 x (2048 x 256 x 4) + 3075: the grid-stride loop wraps twice, tail 3
STATS = ("selected", "dampened", "zeroed", "sum_beta", "sum_delta2", "sum_p2_selected", "sum_p2")


def ratio_f32(f_keep, f_forget):
    fk, ff = np.asarray(f_keep, f32), np.asarray(f_forget, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ff / fk
    assert q.dtype == f32
    return np.where(ff == 0, f32(0), q).astype(f32)


def selected(r, threshold, strict):
    r, t = np.asarray(r, f32), f32(threshold)
    return r > t if strict else r >= t


def keys(r):
    return np.ascontiguousarray(np.asarray(r, f32)).view(np.uint32) & np.uint32(0x7fffffff)


def kth_largest(r, k):
    """(threshold as f32, its key bits, count_gt, count_ge) of the k-th largest integer key, 1 <= k <= len(r)."""
    key = keys(r)
    tb = np.partition(key, len(key) - k)[len(key) - k]
    return np.array([tb], np.uint32).view(f32)[0], int(tb), int((key > tb).sum()), int((key >= tb).sum())


def beta_branch(r, lam):
    """beta = lambda / r if r > lambda else 1: the kernel's form."""
    r, lam = np.asarray(r, f32), f32(lam)
    with np.errstate(divide="ignore"):
        q = lam / r
    assert q.dtype == f32
    return np.where(r > lam, q, f32(1)).astype(f32)


def beta_min(r, lam):
    """min(lambda / r, 1): the paper's form on the materialised ratio (r > 0)."""
    r, lam = np.asarray(r, f32), f32(lam)
    with np.errstate(divide="ignore"):
        q = lam / r
    return np.minimum(q, f32(1)).astype(f32)


def dampen_f32(p, r, threshold, strict, lam):
    """(p', selected mask, beta) -- beta is 1 on the unselected, whose p is returned bit for bit."""
    p, r = np.asarray(p, f32), np.asarray(r, f32)
    sel = selected(r, threshold, strict)
    beta = np.where(sel, beta_branch(r, lam), f32(1)).astype(f32)
    q = p * beta
    assert q.dtype == f32
    return np.where(sel, q, p).astype(f32), sel, beta


def stats_f64(p, p2, sel, beta):
    """The seven statistics from the f32 p (before), p2 (after), the selection and beta."""
    p64, q64, b64 = np.asarray(p, f32).astype(f64), np.asarray(p2, f32).astype(f64), np.asarray(beta, f32).astype(f64)
    d = q64[sel] - p64[sel]
    return dict(selected=int(sel.sum()), dampened=int((sel & (beta < 1)).sum()), zeroed=int((sel & (beta == 0)).sum()),
                sum_beta=math.fsum(b64[sel]), sum_delta2=math.fsum(d * d), sum_p2_selected=math.fsum(p64[sel] * p64[sel]),
                sum_p2=math.fsum(p64 * p64))


# ------------------------------------------------------------------ seeded inputs
def importance(rng, n):
    """Squares of normals scaled into [1e-12, 1e2]: no denormals, no overflow of a ratio (at most 1e14)."""
    x = (rng.standard_normal(n) ** 2) * 10.0 ** rng.uniform(-6, 0, n)
    return np.clip(x, 1e-12, 1e2).astype(f32)


def case(n, seed, zeros=True):
    """(p, F_keep, F_forget): with planted exact zeros in either or both importances, so that +inf, 0 / x and 0 / 0 occur."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(f32)
    fk, ff = importance(rng, n), importance(rng, n)
    if zeros:
        u = rng.random(n)
        fk[u < 0.03] = 0                     # 0.00 .. 0.03: keep 0 (of these 0.02 .. 0.03: both 0)
        ff[(u >= 0.02) & (u < 0.05)] = 0     # 0.02 .. 0.05: forget 0
    return p, fk, ff


def int_case(n, seed):
    """Small integers: p in [-8, 8], ratios in {0, 1, 2, 4, 8}, lambda 1: every beta is a power of two, every product, square and sum
    of the statistics exact."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-8, 9, n).astype(f32)
    r = rng.choice(np.array([0, 1, 2, 4, 8], f32), n).astype(f32)
    return p, r

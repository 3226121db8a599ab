"""Plain restatements of csrc/ewc.hip for tests/test_hip_ewc.py; tests/test_ewc_host.py pins the f64 one to torch's own autograd,
clip_grad_norm_ and AdamW on the CPU.  numpy on the CPU, no GPU.

* The f32 RESTATEMENT of the two kernels, operation for operation, every operation rounded on its own (the file is built without
  contraction): fisher_accumulate_f32 (F + (g * g) * w) and fold_f32 (d = p - pstar, t = (strength * F) * d, gx' = gx + t), with the
  two logged sums formed in f64 from the SAME f32 d and t (penalty_f64).  Pass 1's three sums and the scalar block on (gx', ga) are
  tests/optimizer_ref.py's (norm_sums_f32 / scalars_f32): the kernel calls the same device functions.

* The f64 REFERENCE of one optimizer step with the penalty (step_f64): g_x + strength F (p - pstar) in f64, then optimizer_ref's f64
  step.  strength is the f32 value the C ABI carries, widened.
"""
import math

import numpy as np

import optimizer_ref as O

f32, f64 = np.float32, np.float64
PENALTY_SLOT, GRAD_NORM_SLOT = 12, 13
SIZES = [1027, 4_197_379]       # two blocks + a 3-float tail; 2 x (2048 x 256 x 4) + 3075: the grid-stride loop wraps twice, tail 3


def fisher_accumulate_f32(g, F, w):
    """F[i] + (g[i] * g[i]) * w: three f32 operations in that order."""
    g, F, w = np.asarray(g, f32), np.asarray(F, f32), f32(w)
    sq = g * g
    sc = sq * w
    out = F + sc
    assert sq.dtype == f32 and sc.dtype == f32 and out.dtype == f32
    return out


def fold_f32(gx, p, pstar, F, strength):
    """(gx', d, t) of the fold: d = p - pstar, t = (strength * F) * d, gx' = gx + t, each one f32 operation."""
    gx, p, pstar, F, lam = np.asarray(gx, f32), np.asarray(p, f32), np.asarray(pstar, f32), np.asarray(F, f32), f32(strength)
    d = p - pstar
    lf = lam * F
    t = lf * d
    out = gx + t
    assert d.dtype == f32 and lf.dtype == f32 and t.dtype == f32 and out.dtype == f32
    return out, d, t


def penalty_f64(F, d, t, strength):
    """(ewc_penalty, ewc_grad_norm) in f64 from the f32 F, d, t: 0.5 * strength * sum F d^2 and sqrt(sum t^2), exactly summed."""
    F, d, t = np.asarray(F, f32).astype(f64), np.asarray(d, f32).astype(f64), np.asarray(t, f32).astype(f64)
    return 0.5 * float(f32(strength)) * math.fsum(F * d * d), math.sqrt(math.fsum(t * t))


def block_f32(gx2, ga, mode, knob, max_norm, beta1, beta2, step_before):
    """Slots 0..11 of the block as pass 1 forms them on the folded gx' (optimizer_ref's construction)."""
    return O.scalars_f32(*O.norm_sums_f32(gx2, ga), mode, knob, max_norm, beta1, beta2, step_before)


def step_f64(gx, ga, p, pstar, F, strength, m, v, step, hp, mode, knob, max_norm):
    """One whole update with the penalty, in f64: ((p, m, v, g), scalars, penalty, penalty gradient norm, gx').  `step` is the count
    after it; strength None: the plain update (the negative control)."""
    gx, p64 = np.asarray(gx, f64), np.asarray(p, f64)
    if strength is None:
        t, pen = np.zeros_like(gx), 0.0
    else:
        lam, F64, d = float(f32(strength)), np.asarray(F, f64), p64 - np.asarray(pstar, f64)
        t = lam * F64 * d
        pen = 0.5 * lam * math.fsum(F64 * d * d)
    gx2 = gx + t
    out, sc = O.step_f64(gx2, ga, p, m, v, step, hp, mode, knob, max_norm)
    return out, sc, pen, math.sqrt(math.fsum(t * t)), gx2


# ------------------------------------------------------------------ seeded inputs
def case(n, seed, scale_d=1e-3):
    """(gx, ga, p, pstar, F): gaussian gradients (optimizer_ref.gauss_pair), p ~ N(0, 1), pstar = p + scale_d N(0, 1), F = g^2-like
    non-negative values with some exact zeros."""
    rng = np.random.default_rng(seed)
    gx, ga = O.gauss_pair(n, seed + 1)
    p = rng.standard_normal(n).astype(f32)
    pstar = (p.astype(f64) + scale_d * rng.standard_normal(n)).astype(f32)
    F = (rng.standard_normal(n) ** 2).astype(f32)
    F[rng.random(n) < 0.05] = 0
    return gx, ga, p, pstar, F


def int_case(n, seed):
    """Small integers everywhere (strength 1): every product and every sum of the fold and of the two logged sums is exact."""
    rng = np.random.default_rng(seed)
    gx, ga = O.int_pair(n, seed)
    F = rng.integers(0, 4, n).astype(f32)
    pstar = rng.integers(-8, 9, n).astype(f32)
    p = (pstar + rng.integers(-3, 4, n)).astype(f32)
    return gx, ga, p, pstar, F

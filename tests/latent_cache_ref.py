"""Restatements for the latent cache's tests (tests/test_latent_cache_host.py, tests/test_hip_latent_cache.py), written from the
formula alone:

    r = idx[i]
    out[i] = (mean[r] + exp(0.5 * clamp(logvar[r], -30, 20)) * eps[i]) * scaling

in numpy float32 operation by operation (each product and sum rounded on its own; numpy's expf stands in for libm's), in float64
from the same f32 inputs and the same f32 scalar, and the f32 error bound of that chain."""
import numpy as np
import torch

U = 2.0 ** -24              # f32 unit roundoff: one rounding to nearest changes a value by at most U * |value|
ULP = 2.0 ** -23            # one f32 ulp of a value v is at most ULP * |v|
EXPF_ULP = 1                # the maximum error HIP's math API documents for expf
ROUNDINGS = 5               # 0.5 * lv, expf's own result, std * eps, mean + ., . * scaling (test_latent_sample_against_f64)


def f32(v):
    """The f32 nearest to v, as a Python float (what a c_float argument carries)."""
    return float(np.float32(v))


def _split(cache):
    C = cache.shape[1] // 2
    return cache[:, :C], cache[:, C:]


def sample_f32(cache, idx, eps, scaling):
    """The expression in numpy float32, one rounded operation after the other."""
    c = np.asarray(cache, dtype=np.float32)
    e = np.asarray(eps, dtype=np.float32)
    mean, logvar = _split(c)
    r = np.asarray(idx, dtype=np.int64)
    lv = np.minimum(np.maximum(logvar[r], np.float32(-30.0)), np.float32(20.0))
    half = (np.float32(0.5) * lv).astype(np.float32)
    sd = np.exp(half).astype(np.float32)
    prod = (sd * e).astype(np.float32)
    total = (mean[r] + prod).astype(np.float32)
    return (total * np.float32(scaling)).astype(np.float32)


def sample_f64(cache, idx, eps, scaling):
    """(out [n, C, h, w] in f64, the bound's magnitudes (M, S)): M = (|mean| + |std eps|) |scaling| and S = |std eps| |scaling|, per
    element of out.  cache / eps: torch tensors (f32); idx: integers within [0, rows)."""
    c, e = cache.double().cpu(), eps.double().cpu()
    mean, logvar = _split(c)
    r = torch.as_tensor(idx, dtype=torch.int64).cpu()
    std = torch.exp(0.5 * logvar[r].clamp(-30.0, 20.0))
    s = abs(float(scaling))
    out = (mean[r] + std * e) * float(scaling)
    S = (std * e).abs() * s
    M = mean[r].abs() * s + S
    return out, M, S


def sample_bound(M, S):
    """First-order f32 error of the kernel's chain against sample_f64: each of its ROUNDINGS roundings is at most U relative to a
    result that is at most M once carried to the output, and expf is off by at most EXPF_ULP ulp, which reaches the output through
    the std term alone (S)."""
    return ROUNDINGS * U * M + EXPF_ULP * ULP * S

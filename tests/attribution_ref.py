"""Restatement of csrc/attribution.hip on the host (numpy): the sign matrix of the counter hash, the exact and the f64 projection, the
derived error bound of the kernel's f32 chunk sums, and the f64 scores of siss_amd/attribution.py's Attributor.

R[i, j] = 1 - 2 * ((w >> (i & 31)) & 1) with, in u32 arithmetic (mix = lowbias32),
    h = mix(seed ^ 0x9E3779B9);  h = mix(h ^ lo32(i >> 5));  h = mix(h ^ hi32(i >> 5) ^ 0x85EBCA6B);  w = mix(h + j * 0x9E3779B1)
"""
import numpy as np

U32 = np.uint32
U = 2.0 ** -24                                   # the unit roundoff of f32


def mix(x):
    x = np.asarray(x, dtype=U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7feb352d)
    x ^= x >> U32(15)
    x *= U32(0x846ca68b)
    x ^= x >> U32(16)
    return x


def signs(seed, i0, n, k):
    """[n, k] int8 of +1 / -1: rows i0 .. i0 + n - 1 (flat offsets, 64-bit) of R for `seed`."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64) + np.uint64(i0)
        grp = i >> np.uint64(5)
        h = mix(U32(seed) ^ U32(0x9E3779B9))
        h = mix(h ^ (grp & np.uint64(0xffffffff)).astype(U32))
        h = mix(h ^ (grp >> np.uint64(32)).astype(U32) ^ U32(0x85EBCA6B))
        w = mix(h[:, None] + np.arange(k, dtype=U32)[None, :] * U32(0x9E3779B1))
        bit = (w >> (i & np.uint64(31)).astype(U32)[:, None]) & U32(1)
    return (1 - 2 * bit.astype(np.int8)).astype(np.int8)


def _blocks(seed, g, k, dtype, keep=None, block=1 << 15):
    """sum_i R[i, j] g[i] in `dtype` arithmetic (int64: exact; float64), over all i or over those where keep[i]."""
    acc = np.zeros(k, dtype=dtype)
    for s in range(0, len(g), block):
        x = g[s:s + block].astype(dtype)
        if keep is not None:
            x = np.where(keep[s:s + block], x, 0)
        if not x.any():
            continue
        acc += x @ signs(seed, s, len(x), k).astype(dtype)
    return acc


def project_int(seed, g, k, keep=None):
    """The kernel's result for a buffer of integers small enough that every chunk sum is exact in f32: (float32)(float64(int64 sum) /
    sqrt(k))."""
    s = _blocks(seed, np.asarray(g).astype(np.int64), k, np.int64, keep)
    return (s.astype(np.float64) / np.sqrt(np.float64(k))).astype(np.float32)


def project_f64(seed, g, k, keep=None):
    """(the f64 sums per column, sum |g|): the exact value up to f64 roundoff, before the division by sqrt(k)."""
    g = np.asarray(g, dtype=np.float64)
    s = _blocks(seed, g, k, np.float64, keep)
    a = np.abs(g if keep is None else np.where(keep, g, 0)).sum()
    return s, a


def error_bound(sum_abs, exact_sum, k, chunk):
    """|out - exact / sqrt(k)| per column: a chunk's f32 sum of c terms in any fixed order is within gamma_(c-1) * sum |g| of its exact
    value (gamma_m = m u / (1 - m u), Higham 4.4), and the chunks' bounds add up to gamma_(c-1) * sum |g| over the buffer; the final
    rounding to f32 adds u |exact| / sqrt(k).  (The f64 fold and division add terms of order 2^-53: far inside the slack of a worst-case
    bound.)"""
    m = (chunk - 1) * U
    return (m / (1 - m) * sum_abs + U * np.abs(exact_sum)) / np.sqrt(k)


def keep_of(n, stretches):
    keep = np.zeros(n, dtype=bool)
    for a, b in stretches:
        keep[a:b] = True
    return keep


def table_of(stretches):
    """siss_zero_ranges' table of float stretches (multiples of 4): starts, then prefix sums, in granules."""
    starts = [a // 4 for a, _ in stretches]
    pre = [0]
    for a, b in stretches:
        assert a % 4 == 0 and b % 4 == 0 and b > a
        pre.append(pre[-1] + (b - a) // 4)
    return np.asarray(starts + pre, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the scores
def preconditioner(phi, damping):
    """(K, lambda): K = Phi^T Phi / N + lambda I in f64, lambda = damping * mean(diag(Phi^T Phi / N))."""
    phi = np.asarray(phi, dtype=np.float64)
    gram = phi.T @ phi / phi.shape[0]
    lam = damping * np.mean(np.diag(gram))
    return gram + lam * np.eye(phi.shape[1]), lam


def scores_f64(phi, queries, damping):
    """([Q, N] f64 scores, [Q, k] preconditioned queries) by a dense numpy.linalg.solve."""
    K, _ = preconditioner(phi, damping)
    v = np.linalg.solve(K, np.asarray(queries, dtype=np.float64).T).T
    return v @ np.asarray(phi, dtype=np.float64).T, v


# ---------------------------------------------------------------------------------------------------------------- the same on torch
def _mix_t(x):
    """mix on int64 tensors holding u32 values (the products wrap in int64; their low 32 bits are the u32 products)."""
    m = 0xffffffff
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & m
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & m
    return x ^ (x >> 16)


def signs_torch(seed, i0, n, k, device):
    """signs() as [n, k] f64 on a torch device, for buffers too long for numpy in a test's time; tests hold it against signs()."""
    import torch
    i = torch.arange(n, dtype=torch.int64, device=device) + int(i0)
    grp = i >> 5
    h = _mix_t(torch.tensor((int(seed) ^ 0x9E3779B9) & 0xffffffff, dtype=torch.int64, device=device))
    h = _mix_t(h ^ (grp & 0xffffffff))
    h = _mix_t(h ^ (grp >> 32) ^ 0x85EBCA6B)
    j = (torch.arange(k, dtype=torch.int64, device=device) * 0x9E3779B1) & 0xffffffff
    w = _mix_t((h[:, None] + j[None, :]) & 0xffffffff)
    bit = (w >> (i & 31)[:, None]) & 1
    return (1 - 2 * bit).to(torch.float64)


def sums_torch(seed, g, k, block=1 << 15):
    """sum_i R[i, j] g[i] per column in f64 on g's device (exact for integers whose sums stay below 2^53), as a numpy array."""
    import torch
    acc = torch.zeros(k, dtype=torch.float64, device=g.device)
    for s in range(0, g.numel(), block):
        x = g[s:s + block].double()
        acc += x @ signs_torch(seed, s, x.numel(), k, g.device)
    return acc.cpu().numpy()

"""Plain f64 restatements of siss_amd/uce.py and csrc/uce.hip for tests/test_uce_host.py and tests/test_hip_uce.py.  numpy on the CPU.

* edit_matrix: M, D and E = (D M^-1)^T in f64 by numpy's general solve (NOT the package's Cholesky path), E rounded once to f32;
  uce_form: UCE's own form (lambda W + s_e W C_t^T C_e + s_p W C_p^T C_p)(lambda I + s_e C_e^T C_e + s_p C_p^T C_p)^-1.
* chain: the f32 fmaf chain over ascending k from +0.  sscd_search_ref.chain_sims forms each step as the exact product plus the sum in
  f64, rounded to f32 -- a double rounding that differs from ONE fused rounding on a 2^-29 near-tie.  A test compares 2e8 steps bit
  for bit here, so `chain` is chain_sims with that tie resolved: the f64 sum's own rounding error (Knuth's two-sum, exact) decides
  which f32 neighbour the exact value is nearer to.  test_uce_host.py holds the two equal on its data.
* delta_ref / apply_ref: the compact delta of a job list, and f32(p + delta) over the targets' floats alone (one f32 addition).
* stats_f64: the four statistics from the SAME f32 values, sums by math.fsum (exact).
"""
import math

import numpy as np

from sscd_search_ref import chain_sims  # noqa: F401  (re-exported: the host test holds `chain` against it)

f32, f64 = np.float32, np.float64
CHUNK = 4096                    # floats of a target per row of siss_uce_apply's partials
STATS = ("sum_delta2", "sum_p2", "max_delta", "floats")


def edit_matrix(Ce, Ct, Cp, lam, s_e=1.0, s_p=1.0):
    """(E f32 [X, X], M, D, dT) with dT = D M^-1 in f64"""
    Ce, Ct = np.asarray(Ce, f64), np.asarray(Ct, f64)
    X = Ce.shape[1]
    Cp = np.zeros((0, X)) if Cp is None else np.asarray(Cp, f64).reshape(-1, X)
    M = lam * np.eye(X) + s_e * Ce.T @ Ce + s_p * Cp.T @ Cp
    D = s_e * (Ct - Ce).T @ Ce
    dT = np.linalg.solve(M.T, D.T).T
    return np.ascontiguousarray(dT.T).astype(f32), M, D, dT


def uce_form(W, Ce, Ct, Cp, lam, s_e=1.0, s_p=1.0):
    """UCE's closed form as the paper writes it, in f64: the whole weight rebuilt from a product"""
    W, Ce, Ct = np.asarray(W, f64), np.asarray(Ce, f64), np.asarray(Ct, f64)
    X = Ce.shape[1]
    Cp = np.zeros((0, X)) if Cp is None else np.asarray(Cp, f64).reshape(-1, X)
    num = lam * W + s_e * (W @ Ct.T) @ Ce + s_p * (W @ Cp.T) @ Cp
    den = lam * np.eye(X) + s_e * Ce.T @ Ce + s_p * Cp.T @ Cp
    return np.linalg.solve(den.T, num.T).T


def chain(q, g):
    """[nq, ng] f32: fmaf(q[i, k], g[j, k], s) over k = 0, 1, ... from +0, each step ONE rounding (module docstring); finite data in
    f32's normal range"""
    q, g = np.asarray(q, f32), np.asarray(g, f32)
    s = np.zeros((q.shape[0], g.shape[0]), f32)
    low, half = np.uint64((1 << 29) - 1), np.uint64(1 << 28)
    for k in range(q.shape[1]):
        a = s.astype(f64)
        b = np.outer(q[:, k].astype(f64), g[:, k].astype(f64))          # exact: 24 x 24 bits
        t = a + b
        s = t.astype(f32)
        mid = (t.view(np.uint64) & low) == half                          # t exactly midway between two f32 values: s is the even one
        if mid.any():
            i = np.nonzero(mid)
            a, b, t, r = a[i], b[i], t[i], s[i]
            bb = t - a
            err = (a - (t - bb)) + (b - bb)                              # Knuth's two-sum: t + err == a + b exactly
            d = t - r.astype(f64)                                        # (exact) t = r + d, the other neighbour is r + 2 d
            other = np.nextafter(r, np.where(d > 0, f32(np.inf), f32(-np.inf)))
            s[i] = np.where((err != 0) & ((err > 0) == (d > 0)), other, r)
    return s + f32(0)


def delta_ref(p, jobs, E):
    """{job index: [rows, X] f32} -- jobs: [(w_off, row_off, rows)]"""
    X = E.shape[0]
    return {i: chain(p[w:w + rows * X].reshape(rows, X), E) for i, (w, _, rows) in enumerate(jobs)}


def compact(deltas, jobs, X, total_rows, fill):
    """the compact delta buffer [total_rows * X] with `fill` on the rows no job names"""
    out = np.full(total_rows * X, fill, f32)
    for i, (_, r0, rows) in enumerate(jobs):
        out[r0 * X:(r0 + rows) * X] = deltas[i].reshape(-1)
    return out


def apply_ref(p, jobs, delta, X):
    """f32(p + delta) over the targets' floats only (one f32 addition each); every other float keeps its bits"""
    q = np.array(p, f32, copy=True)
    for w, r0, rows in jobs:
        n = rows * X
        q[w:w + n] = q[w:w + n] + delta[r0 * X:r0 * X + n]
    return q


def stats_f64(p, jobs, delta, X):
    """the four statistics of siss_uce_apply from the same f32 values: exact sums of the f64 squares, the exact maximum, the count"""
    d = np.concatenate([delta[r0 * X:(r0 + rows) * X] for _, r0, rows in jobs]).astype(f64)
    w = np.concatenate([p[o:o + rows * X] for o, _, rows in jobs]).astype(f64)
    return dict(sum_delta2=math.fsum(d * d), sum_p2=math.fsum(w * w), max_delta=float(np.abs(d).max()), floats=int(d.size))


def chunks(jobs, X):
    return sum(-(-rows * X // CHUNK) for _, _, rows in jobs)


def job_bytes(jobs):
    """the 64-byte rows of csrc/uce.hip's UceJob: {long w_off, row_off; int rows, pad; long reserved[5]}"""
    dt = np.dtype([("w_off", "<i8"), ("row_off", "<i8"), ("rows", "<i4"), ("pad", "<i4"), ("reserved", "<i8", (5,))])
    rec = np.zeros(len(jobs), dtype=dt)
    for i, (w, r0, rows) in enumerate(jobs):
        rec[i]["w_off"], rec[i]["row_off"], rec[i]["rows"] = w, r0, rows
    return rec.tobytes()


def residuals(W_after, W_before, Ce, Ct, Cp):
    """(edit residual, preserve drift) over a list of weights, f64 Frobenius norms over all of them"""
    Ce, Ct = np.asarray(Ce, f64), np.asarray(Ct, f64)
    ne = de = npp = dp = 0.0
    for Wa, Wb in zip(W_after, W_before):
        Wa, Wb = np.asarray(Wa, f64), np.asarray(Wb, f64)
        vt = Wb @ Ct.T
        ne += ((Wa @ Ce.T - vt) ** 2).sum()
        de += (vt ** 2).sum()
        if Cp is not None and len(Cp):
            vp = Wb @ np.asarray(Cp, f64).T
            npp += ((Wa @ np.asarray(Cp, f64).T - vp) ** 2).sum()
            dp += (vp ** 2).sum()
    return math.sqrt(ne / de), (math.sqrt(npp / dp) if dp > 0 else None)

"""Plain reference of the weight-gradient (TN) products of csrc/gemm_tn.hip -- no GPU, no HIP library: the header formula of that
file restated with numpy slices, for tests/test_hip_wgrad.py (pinned to torch.autograd by tests/test_wgrad_ref_host.py).

    dW[set][p][n][c] (+)= sum_{r in [row_begin, row_end)} Y[set*rows_per_set + r, n] * X[set*x_set_rows + r + shift_p, coff_p + c]
    dbias[set][n]    +=  sum_r Y[set*rows_per_set + r, n]                                       (dbias2 receives the same)

Operands are 2-D host arrays [rows, ld] WITH their guard rows; `y0` / `x0` is the index of the row the job's Y / X pointer addresses
(so a shifted panel may reach in front of it).  Integer operands are reduced in int64, everything else in f64; the outputs are flat
f64 buffers (exact for the integers: every value here stays far below 2^53) which may hold NaN pre-fills and sentinels.
"""
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class Job:
    """The shape arguments of siss_tn_job (include/siss_hip.h); bias_set_stride 0 = set_stride, as there."""
    N: int
    C: int
    shifts: tuple
    coffs: tuple
    nsets: int
    rows_per_set: int
    row_begin: int
    row_end: int
    x_set_rows: int
    ldy: int
    ldx: int
    set_stride: int
    bias_set_stride: int = 0

    @property
    def npanels(self):
        return len(self.shifts)

    @property
    def floats(self):
        """Floats of one set's dW: npanels * N * C."""
        return self.npanels * self.N * self.C

    @property
    def rows(self):
        return self.row_end - self.row_begin


def _sum_dtype(*arrays):
    return np.int64 if all(np.issubdtype(a.dtype, np.integer) for a in arrays) else np.float64


def _mm(ys, xs):
    """ys^T xs in the arrays' own type (torch's integer matmul: numpy's int64 one takes seconds at 8300 rows)."""
    return (torch.from_numpy(np.ascontiguousarray(ys)).T @ torch.from_numpy(np.ascontiguousarray(xs))).numpy()


def _y_rows(j, s, y0):
    return slice(y0 + s * j.rows_per_set + j.row_begin, y0 + s * j.rows_per_set + j.row_end)


def _x_rows(j, s, p, x0):
    base = x0 + s * j.x_set_rows + j.shifts[p]
    assert base + j.row_begin >= 0, "panel reaches in front of the X allocation"
    return slice(base + j.row_begin, base + j.row_end)


def products(Y, y0, X, x0, j):
    """[nsets, npanels, N, C] products and [nsets, N] column sums of Y, in int64 (integer operands) or f64."""
    assert Y.ndim == 2 and X.ndim == 2 and Y.shape[1] == j.ldy and X.shape[1] == j.ldx
    assert 0 <= j.row_begin < j.row_end <= j.rows_per_set and j.N <= j.ldy
    T = _sum_dtype(Y, X)
    dW = np.zeros((j.nsets, j.npanels, j.N, j.C), T)
    db = np.zeros((j.nsets, j.N), T)
    for s in range(j.nsets):
        ys = Y[_y_rows(j, s, y0), :j.N].astype(T)
        assert ys.shape[0] == j.rows, "Y allocation too short"
        db[s] = ys.sum(axis=0)
        for p in range(j.npanels):
            assert j.coffs[p] + j.C <= j.ldx
            xs = X[_x_rows(j, s, p, x0), j.coffs[p]:j.coffs[p] + j.C].astype(T)
            assert xs.shape[0] == j.rows, "X allocation too short"
            dW[s, p] = _mm(ys, xs)
    return dW, db


def apply(Y, y0, X, x0, j, dW, dw0, overwrite, dbias=None, b0=0, dbias2=None, b20=0):
    """What a launch leaves behind: (dW, dbias, dbias2) as NEW flat f64 buffers.  dW: the prior flat buffer, the job's dW pointer at
    index dw0; set s owns [dw0 + s * set_stride, + npanels * N * C) and is overwritten with the product (`overwrite`) or has it
    added; nothing else changes.  dbias / dbias2 (flat priors, pointers at b0 / b20; None = absent; dbias2 without dbias is ignored,
    as the launchers do): ALWAYS accumulated, under either store mode, with the set stride bias_set_stride (0 = set_stride)."""
    return store(products(Y, y0, X, x0, j), j, dW, dw0, overwrite, dbias, b0, dbias2, b20)


def store(prods, j, dW, dw0, overwrite, dbias=None, b0=0, dbias2=None, b20=0):
    """apply() from the (products, column sums) that products() returned: a test that launches one job several ways computes them once."""
    prod, colsum = prods
    assert j.set_stride >= j.floats or j.nsets == 1
    out = np.array(dW, dtype=np.float64)
    for s in range(j.nsets):
        sl = slice(dw0 + s * j.set_stride, dw0 + s * j.set_stride + j.floats)
        assert sl.stop <= out.size
        out[sl] = prod[s].reshape(-1) if overwrite else out[sl] + prod[s].reshape(-1)
    bs = j.bias_set_stride or j.set_stride
    b1 = None if dbias is None else np.array(dbias, dtype=np.float64)
    b2 = None if dbias2 is None else np.array(dbias2, dtype=np.float64)
    for b, off in ((b1, b0), (b2 if b1 is not None else None, b20)):
        if b is None:
            continue
        for s in range(j.nsets):
            assert off + s * bs + j.N <= b.size
            b[off + s * bs:off + s * bs + j.N] += colsum[s]
    return out, b1, b2


def needed_masks(j, y_shape, y0, x_shape, x0):
    """Boolean masks over the Y and X allocations of the entries the product depends on.  Y: rows [row_begin, row_end) of every set,
    columns [0, N).  X: for every set, the union over the panels of rows [row_begin + shift_p, row_end + shift_p) from the set's X
    base, columns the union of the panels' windows [coff_p, coff_p + C)."""
    my, mx = np.zeros(y_shape, bool), np.zeros(x_shape, bool)
    cols = np.zeros(x_shape[1], bool)
    for p in range(j.npanels):
        cols[j.coffs[p]:j.coffs[p] + j.C] = True
    for s in range(j.nsets):
        my[_y_rows(j, s, y0), :j.N] = True
        for p in range(j.npanels):
            r = _x_rows(j, s, p, x0)
            assert r.stop <= x_shape[0]
            mx[r, :] |= cols
    return my, mx


def overwrite_records(j, dW_address):
    """The records siss_gemm_tn_overwrite_log holds for a job that overwrote: per set (address of its first float, float count)."""
    return [(dW_address + 4 * s * j.set_stride, j.floats) for s in range(j.nsets)]

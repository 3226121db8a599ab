"""Plain reference of the panelled NT products of csrc/gemm_nt.hip, csrc/gemm_nt_c3p.hip and their shared epilogue (nt_epilogue in
csrc/nt_common.h) -- no GPU, no HIP library: the header formula of gemm_nt.hip restated with slices, for tests/test_hip_nt.py
(pinned to torch's convolutions and autograd by tests/test_nt_ref_host.py).

    acc[b][r][n] = sum_p sum_k A[b][r + shift_p][coff_p + k] * W[b][p][n][k]   (+ sum_k A2[r][k] * W2[n][k])
    v            = (acc - rowsub[b][r]) * (alpha if alpha_cols == 0 or n < alpha_cols else 1) + bias[n] + bias2[n] + rowbias[img(r)][n]
    C[b][r][n]   = bf16(bf16(v) + R[b][r][n])      (mul: bf16(bf16(v) * R));  0 at the halo rows of a pixel grid (Hp > 0)
    Cx[r][n]     = bf16(sum_k A[r][k] * Wx[n][k]), 0 at halo rows            (the second product of siss_conv3x3_dgrad_sc)

A and A2 are 2-D host arrays [rows, ld] WITH their guard rows; `a0` / `a20` is the index of the row the A / A2 pointer addresses, so
a shifted panel may reach in front of it.  W is [batch][npanels][N][Kp].  Outputs and residuals are FLAT buffers with an element index
for the pointer (`c0`, `r0`), which may hold sentinels: store() returns a new buffer in which only the stored elements changed.
Everything is accumulated in f64 (exact for the integer operands of test_hip_nt.py: asserted below 2^53); the two roundings are
torch's float32 -> bfloat16 conversion (round to nearest even) of values asserted to be exact in f32 first.
"""
from dataclasses import dataclass

import numpy as np
import torch

QS_TILE, QS_HALF = 254, 128          # kQsTileRows / kQsHalfRows of csrc/common.h: the persistent kernel's row tile and its halves


@dataclass
class Case:
    """The shape arguments of siss_gemm_nt and its relatives (include/siss_hip.h).  strideA / strideC are in elements and must be
    whole rows here; R is addressed with strideC as well, as the kernels do.  d2s: 0, or 1 + plane of a depth-to-space scatter;
    phase_p0: the five panel offsets of siss_gemm_nt_d2s_phases (then the result has one accumulator set per plane)."""
    M: int
    N: int
    Kp: int
    shifts: tuple = (0,)
    coffs: tuple = (0,)
    lda: int = 0
    ldc: int = 0
    ldr: int = 0
    ldrb: int = 0
    batch: int = 1
    strideA: int = 0
    strideC: int = 0
    rows_per_image: int = 1
    Hp: int = 0
    Wp: int = 0
    alpha: float = 1.0
    alpha_cols: int = 0
    mul: bool = False
    d2s: int = 0
    phase_p0: tuple = None
    K2: int = 0
    lda2: int = 0
    Nx: int = 0
    ldcx: int = 0

    @property
    def npanels(self):
        return len(self.shifts)

    @property
    def nimages(self):
        return (self.M - 1) // self.rows_per_image + 1


def round_bf16(v):
    """f64 / f32 array -> the bf16 value nearest to it (ties to even), as f64.  The input must be exact in f32: there is ONE rounding."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v, equal_nan=True), "value is not exact in f32: the reference would round twice"
    return torch.from_numpy(f).to(torch.bfloat16).to(torch.float64).numpy()


def _mm(a, w):
    """a [M, K] . w [N, K]^T in f64 (BLAS; exact for integers while every partial sum stays below 2^53 -- asserted by the caller)."""
    return (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) @
            torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).T).numpy()


def _a_rows(c, b, p, a0):
    assert c.strideA % c.lda == 0
    lo = a0 + b * (c.strideA // c.lda) + c.shifts[p]
    assert lo >= 0, "panel reaches in front of the A allocation"
    return slice(lo, lo + c.M)


def accumulate(c, A, a0, W, A2=None, a20=0, W2=None):
    """[batch][M][N] accumulators in f64 ([4][M][N], one set per plane, with phase_p0)."""
    assert A.ndim == 2 and A.shape[1] == c.lda and W.shape == (c.batch, c.npanels, c.N, c.Kp)
    amax = float(np.nanmax(np.abs(A))) if A.size else 0.0
    assert amax * float(np.abs(W).max()) * c.Kp * c.npanels < 2.0 ** 53
    if c.phase_p0 is None:
        sets = [(b, range(c.npanels)) for b in range(c.batch)]
    else:
        assert c.batch == 1 and c.phase_p0[0] == 0 and c.phase_p0[4] == c.npanels
        sets = [(0, range(c.phase_p0[z], c.phase_p0[z + 1])) for z in range(4)]
    acc = np.zeros((len(sets), c.M, c.N))
    for i, (b, ps) in enumerate(sets):
        for p in ps:
            assert c.coffs[p] + c.Kp <= c.lda
            a = A[_a_rows(c, b, p, a0), c.coffs[p]:c.coffs[p] + c.Kp]
            assert a.shape[0] == c.M, "A allocation too short"
            acc[i] += _mm(a, W[b, p])
    if A2 is not None:
        assert c.batch == 1 and c.phase_p0 is None and A2.shape[1] == c.lda2 and W2.shape == (c.N, c.K2)
        acc[0] += _mm(A2[a20:a20 + c.M, :c.K2], W2)
    return acc


def accumulate_x(c, A, a0, Wx):
    """[M][Nx] accumulators of the second product Cx = A . Wx^T (unshifted rows, the columns of the centre tap's window)."""
    assert Wx.shape == (c.Nx, c.Kp)
    k0 = c.coffs[4]
    return _mm(A[a0:a0 + c.M, k0:k0 + c.Kp], Wx)


def pixel(c, r):
    """(image, y, x, halo) of the flat rows r (arrays); without a pixel structure (Hp == 0) nothing is halo."""
    r = np.asarray(r)
    img = r // c.rows_per_image
    if c.Hp == 0:
        return img, np.zeros_like(r), np.zeros_like(r), np.zeros(r.shape, bool)
    assert c.Hp * c.Wp == c.rows_per_image
    rem = r - img * c.rows_per_image
    y, x = rem // c.Wp, rem % c.Wp
    return img, y, x, (y == 0) | (y == c.Hp - 1) | (x == 0) | (x == c.Wp - 1)


def out_rows(c, plane=None):
    """(rows r that are stored, the output row of each, which of them are written as zeros).  Plain rows: every r < M at its own
    place, halo rows as zeros.  Depth-to-space (plane = 2 py + px): only the non-halo rows, pixel (y, x) of the plane at pixel
    (2y - 1 + py, 2x - 1 + px) of the (2 Hp - 2) x (2 Wp - 2) grid -- halo rows are skipped, C's halo is untouched."""
    r = np.arange(c.M)
    img, y, x, halo = pixel(c, r)
    if plane is None:
        return r, r, halo
    wf = 2 * c.Wp - 2
    ro = img * (2 * c.Hp - 2) * wf + (2 * y - 1 + (plane >> 1)) * wf + (2 * x - 1 + (plane & 1))
    keep = ~halo
    return r[keep], ro[keep], np.zeros(int(keep.sum()), bool)


def pre_residual(c, acc, b, bias=None, bias2=None, rowbias=None, rowsub=None, f32=False):
    """[M][N] of one accumulator set after alpha / bias / row bias and the FIRST rounding (none with f32)."""
    n = np.arange(c.N)
    al = np.where((n < c.alpha_cols) | (c.alpha_cols == 0), c.alpha, 1.0)
    v = acc.astype(np.float64)
    if rowsub is not None:
        v = v - np.asarray(rowsub, dtype=np.float64).reshape(c.batch, c.M)[b][:, None]
    v = v * al[None, :]
    for t in (bias, bias2):
        if t is not None:
            v = v + np.asarray(t, dtype=np.float64)[None, :c.N]
    if rowbias is not None:
        rb = np.asarray(rowbias, dtype=np.float64)
        assert rb.ndim == 2 and rb.shape[0] >= c.nimages
        v = v + rb[np.arange(c.M) // c.rows_per_image, :c.N]
    if f32:
        return v
    assert float(np.abs(v).max()) < 2.0 ** 24            # a condition on the inputs: every f32 value in the kernel is exact
    return round_bf16(v)


def store(c, acc, out, c0, *, bias=None, bias2=None, rowbias=None, rowsub=None, R=None, r0=0, r_is_c=False, f32=False, ldc=None):
    """What a launch leaves in C: a NEW flat f64 buffer.  out: the prior flat buffer, the C pointer at element c0.  R: a flat
    buffer with its pointer at r0 (row stride c.ldr), or r_is_c: the residual is C itself (read before it is written).  acc: from
    accumulate() -- per batch, or per plane with phase_p0; a single plane launch has c.d2s = 1 + plane."""
    ldc = ldc or c.ldc
    out = np.array(out, dtype=np.float64)
    prior = out.copy()
    res, rbase = (prior, c0) if r_is_c else (R, r0)
    ldr = ldc if r_is_c else c.ldr
    assert not c.mul or (res is not None and c.Hp == 0)
    n = np.arange(c.N)
    for i in range(acc.shape[0]):
        b = 0 if c.phase_p0 is not None else i
        plane = i if c.phase_p0 is not None else (c.d2s - 1 if c.d2s else None)
        v = pre_residual(c, acc[i], b, bias, bias2, rowbias, rowsub, f32)
        r, ro, zero = out_rows(c, plane)
        v = v[r]
        if res is not None:
            rr = res[(rbase + b * c.strideC + ro * ldr)[:, None] + n[None, :]]
            live = ~zero
            assert np.isfinite(rr[live]).all(), "R is read where it holds no value"
            w = v[live] * rr[live] if c.mul else v[live] + rr[live]
            v[live] = w if f32 else round_bf16(w)            # bf16 + bf16 and bf16 * bf16 are exact in f32: one rounding
        v[zero] = 0.0
        idx = (c0 + b * c.strideC + ro * ldc)[:, None] + n[None, :]
        assert idx.min() >= 0 and idx.max() < out.size
        out[idx] = v
    return out


def store_x(c, accx, outx, cx0, f32=False):
    """Cx after the launch: the rounded second product at rows [0, M), columns [0, Nx), row stride ldcx; zeros at halo rows."""
    out = np.array(outx, dtype=np.float64)
    v = accx.astype(np.float64)
    if not f32:
        assert float(np.abs(v).max()) < 2.0 ** 24
        v = round_bf16(v)
    _, _, _, halo = pixel(c, np.arange(c.M))
    v[halo] = 0.0
    idx = (cx0 + np.arange(c.M) * c.ldcx)[:, None] + np.arange(c.Nx)[None, :]
    assert idx.max() < out.size
    out[idx] = v
    return out


def needed_masks(c, a_shape, a0, a2_shape=None, a20=0, r_size=0, r0=0, rb_shape=None):
    """Boolean masks of the entries a stored value may depend on: {"A", "A2", "R", "rowbias"} (the last three None when absent).
    A: per batch the union over the panels of rows [shift_p, M + shift_p) x columns [coff_p, coff_p + Kp) -- with one unshifted
    panel rows [0, M) exactly (the kernels clamp a tile's overhang rows to M - 1 + shift); for the taps of a filter, which share
    one column window, that is all of [min shift, M - 1 + max shift], halo and guard rows included: the product of a halo row is
    formed and then discarded, so a kernel may read them, and they hold values.  A2: rows [0, M) x [0, K2) (the persistent kernel also stages rows
    -1 and M of A2; no stored value depends on them).  R (flat): the non-halo rows' place, columns [0, N), per batch at strideC.
    rowbias: [0, images) x [0, N)."""
    mA = np.zeros(a_shape, bool)
    for b in range(c.batch):
        for p in range(c.npanels):
            mA[_a_rows(c, b, p, a0), c.coffs[p]:c.coffs[p] + c.Kp] = True
    mA2 = None
    if a2_shape is not None:
        mA2 = np.zeros(a2_shape, bool)
        mA2[a20:a20 + c.M, :c.K2] = True
    mR = None
    if r_size:
        mR = np.zeros(r_size, bool)
        planes = range(4) if c.phase_p0 is not None else [c.d2s - 1 if c.d2s else None]
        for plane in planes:
            _, ro, zero = out_rows(c, plane)
            ro = ro[~zero]
            for b in range(c.batch):
                mR[(r0 + b * c.strideC + ro * c.ldr)[:, None] + np.arange(c.N)[None, :]] = True
    mB = None
    if rb_shape is not None:
        mB = np.zeros(rb_shape, bool)
        mB[:c.nimages, :c.N] = True
    return {"A": mA, "A2": mA2, "R": mR, "rowbias": mB}


# ---------------------------------------------------------------- GroupNorm statistics of the persistent kernel (NTParams::qstats)
def qstats_entries(c, stored):
    """The qstats buffer [2 * row tiles][2 slots][N / 4][sum, sumsq] of a product whose stored values are `stored` [M][N]: entry
    (2 t + h, slot) covers the rows [254 t + 128 h, ...) of tile t that belong to image floor(254 t / rows_per_image) + slot."""
    M, N = stored.shape
    tiles = -(-M // QS_TILE)
    r = np.arange(M)
    t = r // QS_TILE
    h = (r - t * QS_TILE) // QS_HALF
    slot = r // c.rows_per_image - (t * QS_TILE) // c.rows_per_image
    assert slot.min() >= 0 and slot.max() <= 1
    q4 = stored.reshape(M, N // 4, 4)
    s, ss = q4.sum(axis=2), (q4 * q4).sum(axis=2)
    out = np.zeros((2 * tiles, 2, N // 4, 2))
    np.add.at(out[..., 0], (2 * t + h, slot), s)
    np.add.at(out[..., 1], (2 * t + h, slot), ss)
    return out


def qstats_fold(c, qs):
    """[images][N / 4][sum, sumsq] from the entries (the fold of tests/test_hip_gn_qstats.py::_fold_on_host / siss_groupnorm_fwd_qs)."""
    rpi = c.rows_per_image
    q = np.asarray(qs, dtype=np.float64).reshape(-1, 2, c.N // 4, 2)
    out = np.zeros((c.nimages, c.N // 4, 2))
    for i in range(c.nimages):
        t0, t1 = i * rpi // QS_TILE, min(((i + 1) * rpi - 1) // QS_TILE, q.shape[0] // 2 - 1)
        for t in range(t0, t1 + 1):
            slot = 0 if t * QS_TILE // rpi == i else 1
            out[i] += q[2 * t, slot] + q[2 * t + 1, slot]
    return out


def image_sums(c, stored):
    """[images][N / 4][sum, sumsq] of the stored values [M][N], directly."""
    M, N = stored.shape
    q4 = stored.reshape(M, N // 4, 4)
    out = np.zeros((c.nimages, N // 4, 2))
    img = np.arange(M) // c.rows_per_image
    np.add.at(out[..., 0], img, q4.sum(axis=2))
    np.add.at(out[..., 1], img, (q4 * q4).sum(axis=2))
    return out

"""tests/wgrad_ref.py (the reference of tests/test_hip_wgrad.py) against torch.autograd.grad of F.conv2d with respect to the weight,
in f64, on padded-NHWC flat rows built on the host -- the layout and panel arithmetic of siss_amd.layout without the device.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R
from siss_amd.layout import conv3x3_panels

F64 = torch.float64


def flat_rows(t, guard):
    """[B, C, H, W] -> (padded-NHWC flat rows [guard + B (H+2) (W+2) + guard, C] with a zero halo and zero guard rows, guard)."""
    B, C, H, W = t.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=F64)
    p[:, 1:-1, 1:-1] = t.permute(0, 2, 3, 1)
    z = torch.zeros(guard, C, dtype=F64)
    return torch.cat([z, p.reshape(-1, C), z]).numpy()


def conv_grads(x, dy, conv, wshape):
    """d<conv(x, w), dy>/dw and the bias gradient by autograd, f64."""
    w = torch.zeros(wshape, dtype=F64, requires_grad=True)
    (gw,) = torch.autograd.grad(conv(x, w), w, dy)
    return gw, dy.sum(dim=(0, 2, 3))


def rnd(*shape, seed):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def run(Y, y0, X, x0, j, dbias=True):
    """Accumulating launch on a zero prior with a tail behind every set: ([nsets, npanels, N, C], [nsets, N]); the tails stay zero."""
    assert j.set_stride > j.floats + j.N
    dW, b, _ = R.apply(Y, y0, X, x0, j, np.zeros(j.nsets * j.set_stride), 0, False,
                       np.zeros(j.nsets * j.set_stride) if dbias else None, j.floats)
    dW = dW.reshape(j.nsets, j.set_stride)
    assert not dW[:, j.floats:].any()
    bias = None if b is None else b.reshape(j.nsets, j.set_stride)[:, j.floats:j.floats + j.N]
    return dW[:, :j.floats].reshape(j.nsets, j.npanels, j.N, j.C), bias


def close(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))      # f64 sums of a few hundred O(1) terms


def taps_to_w(dW, k):
    """[k*k, N, C] panels (tap = ky * k + kx) -> [N, C, k, k]."""
    return torch.as_tensor(dW).reshape(k, k, dW.shape[1], dW.shape[2]).permute(2, 3, 0, 1)


@pytest.mark.parametrize("nsets,shared", [(1, True), (2, True), (2, False)])
def test_conv3x3_through_conv3x3_panels(nsets, shared):
    """3x3, pad 1: nine row-shifted panels; [row_begin, row_end) cuts off the first and last halo rows as the engine passes it; two
    cotangent sets against ONE saved activation (x_set_rows = 0) and against their own rows; the bias gradient."""
    B, Ci, Co, H, W = 2, 8, 5, 4, 6
    wp, rpi = W + 2, (H + 2) * (W + 2)
    nx = 1 if shared else nsets
    x, dy = rnd(nx * B, Ci, H, W, seed=1), rnd(nsets * B, Co, H, W, seed=2)
    g = wp + 2
    X, Y = flat_rows(x, g), flat_rows(dy, g)
    shifts, coffs = conv3x3_panels(wp, Ci)
    rps = B * rpi
    j = R.Job(N=Co, C=Ci, shifts=tuple(shifts), coffs=tuple(coffs), nsets=nsets, rows_per_set=rps, row_begin=wp + 1,
              row_end=rps - (wp + 1), x_set_rows=0 if shared else rps, ldy=Co, ldx=Ci, set_stride=9 * Co * Ci + 16)
    dW, db = run(Y, g, X, g, j)
    conv = lambda a, w: F.conv2d(a, w, padding=1)
    for s in range(nsets):
        xs = x if shared else x[s * B:(s + 1) * B]
        gw, gb = conv_grads(xs, dy[s * B:(s + 1) * B], conv, (Co, Ci, 3, 3))
        close(taps_to_w(dW[s], 3), gw)
        close(db[s], gb)


def test_conv1x1_and_absent_bias():
    B, Ci, Co, H, W = 3, 16, 7, 3, 5
    x, dy = rnd(B, Ci, H, W, seed=3), rnd(B, Co, H, W, seed=4)
    g = W + 4
    rps = B * (H + 2) * (W + 2)
    j = R.Job(N=Co, C=Ci, shifts=(0,), coffs=(0,), nsets=1, rows_per_set=rps, row_begin=W + 3, row_end=rps - (W + 3), x_set_rows=0,
              ldy=Co, ldx=Ci, set_stride=Co * Ci + 24)
    dW, db = run(flat_rows(dy, g), g, flat_rows(x, g), g, j, dbias=False)
    assert db is None
    gw, _ = conv_grads(x, dy, lambda a, w: F.conv2d(a, w), (Co, Ci, 1, 1))
    close(taps_to_w(dW[0], 1), gw)


@pytest.mark.parametrize("pad0", [True, False])
def test_stride2_conv_in_space_to_depth_panels(pad0):
    """3x3 stride 2 as the engine runs it: nine panels over a space-to-depth copy z [B, H/2, W/2, 4 C] of the input, plane (py, px) at
    channel offset (2 py + px) C, shifts dy * wp + dx in z's padded rows (UNetEngine.downsample, both paddings of Downsample2D)."""
    B, C, Co, H, W = 2, 8, 6, 6, 8
    Ho, Wo = H // 2, W // 2
    wp = Wo + 2
    x, dy = rnd(B, C, H, W, seed=5), rnd(B, Co, Ho, Wo, seed=6)
    z = torch.cat([x[:, :, py::2, px::2] for py in range(2) for px in range(2)], dim=1)          # [B, 4 C, Ho, Wo]
    shifts, coffs = [], []
    for ky in range(3):
        for kx in range(3):
            dy_, py, dx_, px = (ky >> 1, ky & 1, kx >> 1, kx & 1) if pad0 else ((ky - 1) >> 1, (ky - 1) & 1, (kx - 1) >> 1, (kx - 1) & 1)
            shifts.append(dy_ * wp + dx_)
            coffs.append((py * 2 + px) * C)
    g = wp + 2
    rps = B * (Ho + 2) * wp
    j = R.Job(N=Co, C=C, shifts=tuple(shifts), coffs=tuple(coffs), nsets=1, rows_per_set=rps, row_begin=wp + 1, row_end=rps - (wp + 1),
              x_set_rows=0, ldy=Co, ldx=4 * C, set_stride=9 * Co * C + 8)
    dW, db = run(flat_rows(dy, g), g, flat_rows(z, g), g, j)
    conv = (lambda a, w: F.conv2d(F.pad(a, (0, 1, 0, 1)), w, stride=2)) if pad0 else (lambda a, w: F.conv2d(a, w, stride=2, padding=1))
    gw, gb = conv_grads(x, dy, conv, (Co, C, 3, 3))
    close(taps_to_w(dW[0], 3), gw)
    close(db[0], gb)


def test_store_modes_strides_and_second_bias_target():
    """Overwrite replaces a NaN prior and leaves what lies between the sets; accumulate adds; dbias and dbias2 always accumulate, with
    bias_set_stride when given; dbias2 without dbias is ignored; integer operands are reduced in int64."""
    rng = np.random.default_rng(7)
    Y, X = rng.integers(-4, 5, (40, 16)), rng.integers(-4, 5, (44, 24))
    j = R.Job(N=11, C=8, shifts=(-2, 1), coffs=(8, 16), nsets=2, rows_per_set=17, row_begin=3, row_end=15, x_set_rows=5, ldy=16, ldx=24,
              set_stride=200, bias_set_stride=13)
    prod, colsum = R.products(Y, 2, X, 4, j)
    assert prod.dtype == np.int64 and colsum.dtype == np.int64
    for s in range(2):
        ys = Y[2 + 17 * s + 3:2 + 17 * s + 15, :11]
        assert (colsum[s] == ys.sum(0)).all()
        for p in range(2):
            xs = X[4 + 5 * s + j.shifts[p] + 3:4 + 5 * s + j.shifts[p] + 15, j.coffs[p]:j.coffs[p] + 8]
            assert (prod[s, p] == np.einsum("rn,rc->nc", ys, xs)).all()
    prior = np.full(3 + 2 * 200, np.nan)
    prior[3 + 176:3 + 200] = 5.0
    b1, b2 = np.full(40, 2.0), np.full(40, -1.0)
    dW, o1, o2 = R.apply(Y, 2, X, 4, j, prior, 3, True, b1, 1, b2, 0)
    assert np.isnan(dW[:3]).all() and (dW[3 + 176:3 + 200] == 5.0).all() and np.isnan(dW[3 + 376:]).all()
    for s in range(2):
        assert (dW[3 + 200 * s:3 + 200 * s + 176] == prod[s].reshape(-1)).all()
        assert (o1[1 + 13 * s:1 + 13 * s + 11] == 2.0 + colsum[s]).all() and (o2[13 * s:13 * s + 11] == -1.0 + colsum[s]).all()
    assert o1[0] == 2.0 and o1[12] == 2.0 and (o1[25:] == 2.0).all() and (o2[24:] == -1.0).all()
    acc, n1, n2 = R.apply(Y, 2, X, 4, j, np.ones(3 + 2 * 200), 3, False, None, 0, b2, 0)
    assert n1 is None and (n2 == b2).all() and (acc[3:3 + 176] == 1 + prod[0].reshape(-1)).all() and (acc[:3] == 1).all()
    assert R.overwrite_records(j, 4096) == [(4096, 176), (4096 + 800, 176)]


@pytest.mark.parametrize("shifts,coffs,x_set_rows", [((0,), (0,), 0), ((-9, -8, -7, -1, 0, 1, 7, 8, 9), (0,) * 9, 21),
                                                      ((-7, -6, -1, 0), (0, 8, 16, 24), 40), ((-5, 0, 4), (8, 8, 8), 3)])
def test_needed_masks(shifts, coffs, x_set_rows):
    """With every entry outside the needed masks set to NaN the reference's result is finite and unchanged; the masks are exactly
    (rows of the range) x (columns below N) for Y and (union of the panels' row ranges) x (union of their column windows) for X."""
    rng = np.random.default_rng(11)
    Y, X = rng.standard_normal((2 + 2 * 21 + 3, 16)), rng.standard_normal((12 + 80 + 12, 40))
    j = R.Job(N=13, C=8, shifts=shifts, coffs=coffs, nsets=2, rows_per_set=21, row_begin=2, row_end=19, x_set_rows=x_set_rows, ldy=16,
              ldx=40, set_stride=9 * 13 * 8)
    my, mx = R.needed_masks(j, Y.shape, 2, X.shape, 12)
    assert int(my.sum()) == 2 * 17 * 13 and not my[:, 13:].any() and not my[:4].any() and my[4:21, :13].all() and not my[21:25].any()
    lo, hi = 12 + 2 + min(shifts), 12 + x_set_rows + 19 + max(shifts)
    assert not mx[:lo].any() and not mx[hi:].any() and mx[lo].any() and mx[hi - 1].any()
    cols = sorted({c for o in coffs for c in range(o, o + 8)})
    assert mx.any(axis=0).nonzero()[0].tolist() == cols
    want = R.products(Y, 2, X, 12, j)
    Yn, Xn = np.where(my, Y, np.nan), np.where(mx, X, np.nan)
    got = R.products(Yn, 2, Xn, 12, j)
    for a, b in zip(got, want):
        assert np.isfinite(a).all() and (a == b).all()
    # and every needed entry matters somewhere: a NaN inside a mask shows up in the result
    for M, which in ((my, 0), (mx, 1)):
        i = tuple(np.argwhere(M)[len(np.argwhere(M)) // 2])
        A = [Y.copy(), X.copy()]
        A[which][i] = np.nan
        dW, db = R.products(A[0], 2, A[1], 12, j)
        assert np.isnan(dW).any()

"""tests/nt_ref.py (the reference of tests/test_hip_nt.py) against torch's convolutions and autograd in f64, on padded-NHWC flat rows
built on the host -- the layout and panel arithmetic of siss_amd.layout and of the UNet engine's call sites without the device.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nt_ref as R
from siss_amd.layout import conv3x3_panels

F64 = torch.float64


def rnd(*shape, seed):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def flat_rows(t, guard):
    """[B, C, H, W] -> padded-NHWC flat rows [guard + B (H+2) (W+2) + guard, C] with a zero halo and zero guard rows."""
    B, C, H, W = t.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=F64)
    p[:, 1:-1, 1:-1] = t.permute(0, 2, 3, 1)
    z = torch.zeros(guard, C, dtype=F64)
    return torch.cat([z, p.reshape(-1, C), z]).numpy()


def unflat(rows, B, H, W):
    """[B (H+2) (W+2), C] flat padded rows -> ([B, C, H, W] interior, the padded [B, H+2, W+2, C])."""
    p = torch.as_tensor(rows).reshape(B, H + 2, W + 2, -1)
    return p[:, 1:-1, 1:-1].permute(0, 3, 1, 2), p


def native(w):
    """[Co, Ci, kh, kw] -> [kh * kw][Co][Ci] (ops.conv_w_to_native)."""
    co, ci, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, co, ci)


def dgrad_copy(wn):
    """[T][Co][Ci] -> [T][Ci][Co] with the tap order reversed (siss_conv_weight_dgrad_layout)."""
    return wn.flip(0).transpose(1, 2)


def run(c, A, a0, W, fill=0.0, rows=None, **kw):
    """The product stored with f32=True (no rounding) into a buffer pre-filled with `fill`: [rows or M, ldc]."""
    rows = rows or c.batch * max(c.M, c.strideC // c.ldc if c.strideC else c.M)
    A2, a20, W2 = kw.pop("A2", None), kw.pop("a20", 0), kw.pop("W2", None)
    acc = R.accumulate(c, A, a0, np.asarray(W).reshape(c.batch, c.npanels, c.N, c.Kp), A2, a20, None if W2 is None else np.asarray(W2))
    return R.store(c, acc, np.full(rows * c.ldc, fill), 0, f32=True, **kw).reshape(rows, c.ldc)


def close(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))      # f64 sums of a few hundred O(1) terms


def halo_is(p, v):
    return bool((p[:, 0] == v).all() and (p[:, -1] == v).all() and (p[:, :, 0] == v).all() and (p[:, :, -1] == v).all())


def conv_case(B, H, W, Ci, Co, **kw):
    wp = W + 2
    shifts, coffs = conv3x3_panels(wp, Ci)
    return R.Case(M=B * (H + 2) * wp, N=Co, Kp=Ci, shifts=tuple(shifts), coffs=tuple(coffs), lda=Ci, ldc=Co + 8,
                  rows_per_image=(H + 2) * wp, Hp=H + 2, Wp=wp, **kw)


# ---------------------------------------------------------------- convolutions
def test_conv3x3_forward_with_bias_rowbias_and_residual():
    B, Ci, Co, H, W = 3, 8, 6, 4, 5
    x, w, b, rb, res = rnd(B, Ci, H, W, seed=1), rnd(Co, Ci, 3, 3, seed=2), rnd(Co, seed=3), rnd(B, Co + 2, seed=4), rnd(B, Co, H, W, seed=5)
    g = W + 4
    c = conv_case(B, H, W, Ci, Co, ldr=Co, ldrb=Co + 2)
    Rf = flat_rows(res, 0)
    Rf[R.pixel(c, np.arange(c.M))[3]] = np.nan                   # the residual is not read at halo rows
    out = run(c, flat_rows(x, g), g, native(w).numpy(), fill=7.0, bias=b.numpy(), rowbias=rb.numpy(), R=Rf.reshape(-1))
    got, p = unflat(out[:, :Co], B, H, W)
    close(got, F.conv2d(x, w, b, padding=1) + rb[:, :Co, None, None] + res)
    assert halo_is(p, 0.0) and (out[:, Co:] == 7.0).all()        # halo rows are written as zeros; nothing lands past N


def test_conv3x3_dgrad_through_the_dgrad_weight_copy():
    B, Ci, Co, H, W = 2, 5, 8, 5, 4
    w, dy = rnd(Co, Ci, 3, 3, seed=6), rnd(B, Co, H, W, seed=7)
    x = torch.zeros(B, Ci, H, W, dtype=F64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv2d(x, w, padding=1), x, dy)
    g = W + 4
    c = conv_case(B, H, W, Co, Ci)                                # the cotangent's channels are the reduction
    out = run(c, flat_rows(dy, g), g, dgrad_copy(native(w)).numpy())
    close(unflat(out[:, :Ci], B, H, W)[0], want)


def test_conv1x1_and_linear():
    B, Ci, Co, H, W = 2, 8, 4, 3, 5
    x, w, b = rnd(B, Ci, H, W, seed=8), rnd(Co, Ci, 1, 1, seed=9), rnd(Co, seed=10)
    c = R.Case(M=B * (H + 2) * (W + 2), N=Co, Kp=Ci, lda=Ci, ldc=Co, rows_per_image=(H + 2) * (W + 2), Hp=H + 2, Wp=W + 2)
    got, p = unflat(run(c, flat_rows(x, 0), 0, native(w).numpy(), bias=b.numpy()), B, H, W)
    close(got, F.conv2d(x, w, b))
    assert halo_is(p, 0.0)
    # a linear layer over rows without a pixel structure, on a column window of a wider A, batched with strides larger than the operands
    M, K, N, nb = 7, 8, 5, 3
    a, wl, bl = rnd(nb, M + 2, 2 * K, seed=11), rnd(nb, N, K, seed=12), rnd(N, seed=13)
    c = R.Case(M=M, N=N, Kp=K, coffs=(K,), lda=2 * K, ldc=N + 3, batch=nb, strideA=(M + 2) * 2 * K, strideC=(M + 1) * (N + 3), alpha=0.25)
    out = run(c, a.reshape(-1, 2 * K).numpy(), 0, wl.numpy(), fill=9.0, bias=bl.numpy()).reshape(nb, M + 1, N + 3)
    close(out[:, :M, :N], 0.25 * torch.einsum("bmk,bnk->bmn", a[:, :M, K:], wl) + bl)
    assert (out[:, M:] == 9.0).all() and (out[:, :, N:] == 9.0).all()


def s2d_panels(wp, C):
    """(shifts, coffs) of a stride-2, pad-1 3x3 convolution over the space-to-depth copy of its input (UNetEngine.downsample)."""
    shifts, coffs = [], []
    for ky in range(3):
        for kx in range(3):
            dy_, py, dx_, px = (ky - 1) >> 1, (ky - 1) & 1, (kx - 1) >> 1, (kx - 1) & 1
            shifts.append(dy_ * wp + dx_)
            coffs.append((py * 2 + px) * C)
    return shifts, coffs


@pytest.mark.parametrize("one_launch", [False, True])
def test_stride2_dgrad_through_the_four_space_to_depth_planes(one_launch):
    """Each plane's taps form one multi-panel product over the cotangent whose depth-to-space store lands on the plane's pixels of
    the full-resolution gradient and adds what is already there (R == C); the halo of C is never written."""
    B, C, Co, H, W = 2, 4, 6, 6, 4
    Ho, Wo = H // 2, W // 2
    w, dy, prior = rnd(Co, C, 3, 3, seed=14), rnd(B, Co, Ho, Wo, seed=15), rnd(B, C, H, W, seed=16)
    x = torch.zeros(B, C, H, W, dtype=F64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv2d(x, w, stride=2, padding=1), x, dy)
    wp = Wo + 2
    shifts, coffs = s2d_panels(wp, C)
    planes = {}
    for tap in range(9):
        planes.setdefault(coffs[tap] // C, []).append(tap)
    order = [tap for pl in sorted(planes) for tap in planes[pl]]
    wds = native(w)[order].transpose(1, 2).numpy()               # [9][C][Co], grouped by plane
    g = wp + 2
    A = flat_rows(dy, g)
    M, rpi = B * (Ho + 2) * wp, (Ho + 2) * wp
    full = flat_rows(prior, 0)
    full[R.pixel(R.Case(M=full.shape[0], N=C, Kp=8, rows_per_image=(H + 2) * (W + 2), Hp=H + 2, Wp=W + 2), np.arange(full.shape[0]))[3]] = 5.0
    out = full.reshape(-1)
    kw = dict(M=M, N=C, Kp=Co, lda=Co, ldc=C, ldr=C, rows_per_image=rpi, Hp=Ho + 2, Wp=wp)
    if one_launch:
        p0 = [0]
        for pl in sorted(planes):
            p0.append(p0[-1] + len(planes[pl]))
        c = R.Case(shifts=tuple(-shifts[t] for t in order), coffs=(0,) * 9, d2s=1, phase_p0=tuple(p0), **kw)
        out = R.store(c, R.accumulate(c, A, g, wds[None]), out, 0, r_is_c=True, f32=True)
    else:
        pos = 0
        for pl in sorted(planes):
            taps = planes[pl]
            c = R.Case(shifts=tuple(-shifts[t] for t in taps), coffs=(0,) * len(taps), d2s=1 + pl, **kw)
            out = R.store(c, R.accumulate(c, A, g, wds[None, pos:pos + len(taps)]), out, 0, r_is_c=True, f32=True)
            pos += len(taps)
    got, p = unflat(out.reshape(-1, C), B, H, W)
    close(got, want + prior)
    assert halo_is(p, 5.0)


def test_subpixel_upsample_phases_against_nearest_2x_then_conv():
    B, C, Co, H, W = 2, 4, 5, 3, 4
    x, w, b = rnd(B, C, H, W, seed=17), rnd(Co, C, 3, 3, seed=18), rnd(Co, seed=19)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    wp = W + 2
    taps = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # (phase bit, 2x2 tap) -> the 3x3 taps it sums
    wf = torch.zeros(4, 4, Co, C, dtype=F64)
    for plane in range(4):
        py, px = plane >> 1, plane & 1
        for a in range(2):
            for bb in range(2):
                for ky in taps[py, a]:
                    for kx in taps[px, bb]:
                        wf[plane, a * 2 + bb] += w[:, :, ky, kx]
    g = wp + 2
    A = flat_rows(x, g)
    out = np.full(B * (2 * H + 2) * (2 * W + 2) * Co, 3.0)
    kw = dict(M=B * (H + 2) * wp, N=Co, Kp=C, lda=C, ldc=Co, rows_per_image=(H + 2) * wp, Hp=H + 2, Wp=wp, coffs=(0,) * 4)
    shifts = lambda plane: tuple((a + (plane >> 1) - 1) * wp + (bb + (plane & 1) - 1) for a in range(2) for bb in range(2))
    for plane in range(4):
        c = R.Case(shifts=shifts(plane), d2s=1 + plane, **kw)
        out = R.store(c, R.accumulate(c, A, g, wf[plane][None].numpy()), out, 0, bias=b.numpy(), f32=True)
    got, p = unflat(out.reshape(-1, Co), B, 2 * H, 2 * W)
    close(got, want)
    assert halo_is(p, 3.0)
    kw["coffs"] = (0,) * 16
    c = R.Case(shifts=sum((shifts(pl) for pl in range(4)), ()), d2s=1, phase_p0=(0, 4, 8, 12, 16), **kw)
    one = R.store(c, R.accumulate(c, A, g, wf.reshape(1, 16, Co, C).numpy()), np.full(out.size, 3.0), 0, bias=b.numpy(), f32=True)
    assert np.array_equal(one, out)


def test_folded_shortcut_forward_and_its_two_data_gradients():
    B, Ci, C2, Co, H, W = 2, 8, 4, 6, 4, 4
    h, x = rnd(B, Ci, H, W, seed=20), rnd(B, C2, H, W, seed=21)
    w, w2, b, b2 = rnd(Co, Ci, 3, 3, seed=22), rnd(Co, C2, 1, 1, seed=23), rnd(Co, seed=24), rnd(Co, seed=25)
    g = W + 4
    c = conv_case(B, H, W, Ci, Co, K2=C2, lda2=C2 + 8)
    A2 = np.concatenate([flat_rows(x, g), np.full((c.M + 2 * g, 8), np.nan)], axis=1)
    out = run(c, flat_rows(h, g), g, native(w).numpy(), bias=b.numpy(), bias2=b2.numpy(), A2=A2, a20=g, W2=w2[:, :, 0, 0].numpy())
    got, p = unflat(out[:, :Co], B, H, W)
    close(got, F.conv2d(h, w, b, padding=1) + F.conv2d(x, w2, b2))
    assert halo_is(p, 0.0)
    # backward: conv2's dgrad (+ residual) and the shortcut's dgrad over the same cotangent
    dy, res = rnd(B, Co, H, W, seed=26), rnd(B, Ci, H, W, seed=27)
    hh = torch.zeros(B, Ci, H, W, dtype=F64, requires_grad=True)
    xx = torch.zeros(B, C2, H, W, dtype=F64, requires_grad=True)
    dh, dx = torch.autograd.grad(F.conv2d(hh, w, padding=1) + F.conv2d(xx, w2), (hh, xx), dy)
    cd = conv_case(B, H, W, Co, Ci, ldr=Ci, Nx=C2, ldcx=C2 + 3)
    A = flat_rows(dy, g)
    got, _ = unflat(run(cd, A, g, dgrad_copy(native(w)).numpy(), R=flat_rows(res, 0).reshape(-1))[:, :Ci], B, H, W)
    close(got, dh + res)
    ox = R.store_x(cd, R.accumulate_x(cd, A, g, w2[:, :, 0, 0].T.numpy()), np.full(cd.M * cd.ldcx, 2.0), 0, f32=True).reshape(cd.M, cd.ldcx)
    gotx, px_ = unflat(ox[:, :C2], B, H, W)
    close(gotx, dx)
    assert halo_is(px_, 0.0) and (ox[:, C2:] == 2.0).all()


def test_mulsub_is_the_softmax_backward():
    nb, M, N, K, scale = 2, 9, 7, 8, 0.125
    dO, V, P, delta = rnd(nb, M, K, seed=28), rnd(nb, N, K, seed=29), rnd(nb, M, N, seed=30).abs(), rnd(nb, M, seed=31)
    c = R.Case(M=M, N=N, Kp=K, lda=K, ldc=N + 1, ldr=N, batch=nb, strideA=M * K, strideC=M * (N + 1), alpha=scale, mul=True)
    Rf = np.zeros(nb * M * (N + 1))                               # R is addressed with C's batch stride and its own row stride
    for b in range(nb):
        Rf[b * c.strideC:b * c.strideC + M * N] = P[b].reshape(-1).numpy()
    out = run(c, dO.reshape(-1, K).numpy(), 0, V.numpy(), rowsub=delta.numpy(), R=Rf).reshape(nb, M, N + 1)
    close(out[:, :, :N], P * scale * (torch.einsum("bmk,bnk->bmn", dO, V) - delta[:, :, None]))


def test_alpha_cols_scales_the_first_columns_only():
    M, N, K = 5, 12, 8
    a, w, b = rnd(M, K, seed=32), rnd(N, K, seed=33), rnd(N, seed=34)
    full = a @ w.T
    for cols in (4, 8):
        c = R.Case(M=M, N=N, Kp=K, lda=K, ldc=N, alpha=0.5, alpha_cols=cols)
        want = torch.cat([0.5 * full[:, :cols], full[:, cols:]], dim=1) + b
        close(run(c, a.numpy(), 0, w.numpy(), bias=b.numpy()), want)


# ---------------------------------------------------------------- the two roundings
def test_round_bf16_on_ties_and_neighbours():
    got = R.round_bf16(np.array([257.0, 259.0, 258.0, 256.5, 257.5, -257.0, -259.0, 1.0, 0.5, 65537.0 * 4]))
    assert got.tolist() == [256.0, 260.0, 258.0, 256.0, 258.0, -256.0, -260.0, 1.0, 0.5, 65536.0 * 4]
    with pytest.raises(AssertionError):
        R.round_bf16(np.array([2.0 ** 24 + 1]))                   # not an f32: the reference refuses to round twice


def test_residual_is_added_after_the_first_rounding():
    """acc = 257, R = 1: bf16(257) = 256, 256 + 1 = 257 -> 256; one rounding of 258 would give 258.  mul: bf16(257) * 3 = 768
    where bf16(771) = 772.  bias rides in front of the first rounding: 255 + 2 = 257 -> 256."""
    c = R.Case(M=1, N=1, Kp=1, lda=1, ldc=1, ldr=1)
    acc = np.array([[[257.0]]])
    assert R.store(c, acc, np.zeros(1), 0, R=np.array([1.0])).tolist() == [256.0]
    assert R.store(c, acc, np.zeros(1), 0, R=np.array([1.0]), f32=True).tolist() == [258.0]
    cm = R.Case(M=1, N=1, Kp=1, lda=1, ldc=1, ldr=1, mul=True)
    assert R.store(cm, acc, np.zeros(1), 0, R=np.array([3.0])).tolist() == [768.0]
    assert R.store(c, np.array([[[255.0]]]), np.zeros(1), 0, bias=np.array([2.0])).tolist() == [256.0]
    assert R.store(c, np.array([[[513.0]]]), np.zeros(1), 0, bias=np.array([1.0]), R=np.array([2.0])).tolist() == [512.0]   # 514 -> 512, 514 -> 512; once: 516


# ---------------------------------------------------------------- needed_masks
def _int_case(kind):
    rng = np.random.default_rng(5)
    if kind == "rows":             # no pixel structure: three shifted panels with windows of their own in a wider A, two batches
        c = R.Case(M=5, N=3, Kp=2, shifts=(-2, 0, 3), coffs=(0, 4, 2), lda=8, ldc=4, ldr=5, ldrb=4, batch=2, strideA=12 * 8, strideC=6 * 4)
        a0, arows = 3, 3 + 12 + 5 + 3 + 2
    else:                          # 3x3 on two 2x1 images with a folded shortcut
        s, co = conv3x3_panels(3, 2)
        c = R.Case(M=24, N=3, Kp=2, shifts=tuple(s), coffs=tuple(co), lda=3, ldc=4, ldr=5, ldrb=4, rows_per_image=12, Hp=4, Wp=3,
                   K2=2, lda2=3)
        a0, arows = 6, 36
    A = rng.integers(1, 5, (arows, c.lda)).astype(np.float64)
    W = rng.integers(1, 4, (c.batch, c.npanels, c.N, c.Kp)).astype(np.float64)
    Rf = rng.integers(1, 5, c.batch * max(c.strideC, c.M * c.ldr) + 8).astype(np.float64)
    rb = rng.integers(1, 5, (c.nimages + 1, c.ldrb)).astype(np.float64)
    A2 = rng.integers(1, 5, (arows, 3)).astype(np.float64) if c.K2 else None
    W2 = rng.integers(1, 4, (c.N, c.K2)).astype(np.float64) if c.K2 else None
    return c, A, a0, W, Rf, rb, A2, W2


@pytest.mark.parametrize("kind", ["rows", "pixels"])
def test_needed_masks_mark_exactly_what_the_result_depends_on(kind):
    """Every operand is positive, so no two contributions cancel.  Flipping an entry outside the masks never changes the result.
    Flipping a needed entry changes it -- except, with a pixel structure, the entries only halo rows' products read: those rows are
    stored as zeros, and the masks keep them because a kernel forms (and discards) their products."""
    c, A, a0, W, Rf, rb, A2, W2 = _int_case(kind)
    use_r = A2 is None                                            # (the folded shortcut takes no residual)

    def result(A=A, Rf=Rf, rb=rb, A2=A2):
        acc = R.accumulate(c, A, a0, W, A2, a0, W2)
        return R.store(c, acc, np.zeros(c.batch * max(c.strideC, c.M * c.ldc)), 0, rowbias=rb, R=Rf if use_r else None, r0=2, f32=True)

    base = result()
    m = R.needed_masks(c, A.shape, a0, None if A2 is None else A2.shape, a0, Rf.size if use_r else 0, 2, rb.shape)
    _, _, _, halo = R.pixel(c, np.arange(c.M))
    live_rows = set((a0 + r + s) for r in np.flatnonzero(~halo) for s in c.shifts) if c.Hp else None
    for name, arr in (("A", A), ("A2", A2), ("R", Rf if use_r else None), ("rowbias", rb)):
        if arr is None:
            assert m[name] is None
            continue
        assert m[name].shape == arr.shape and m[name].any() and not m[name].all()
        for idx in np.ndindex(arr.shape):
            t = arr.copy()
            t[idx] += 1.0
            changed = not np.array_equal(result(**{{"A": "A", "A2": "A2", "R": "Rf", "rowbias": "rb"}[name]: t}), base)
            if not m[name][idx]:
                assert not changed, (name, idx)
            elif name == "A" and live_rows is not None and idx[0] not in live_rows:
                assert not changed, (name, idx)
            elif name == "A2" and c.Hp and halo[idx[0] - a0]:
                assert not changed, (name, idx)
            else:
                assert changed, (name, idx)


# ---------------------------------------------------------------- statistics entries
def test_qstats_entries_fold_to_the_image_sums():
    """Rows per image 300 against the 254-row tile: tiles that straddle an image seam use both slots; the last tile is partial."""
    rng = np.random.default_rng(6)
    c = R.Case(M=3 * 300 - 20, N=8, Kp=8, rows_per_image=300)
    stored = rng.integers(-5, 6, (c.M, c.N)).astype(np.float64)
    q = R.qstats_entries(c, stored)
    assert q.shape == (2 * 4, 2, 2, 2) and q[:, 1].any()
    assert np.array_equal(R.qstats_fold(c, q), R.image_sums(c, stored))
    assert np.array_equal(R.image_sums(c, stored)[1, 0], [stored[300:600, :4].sum(), (stored[300:600, :4] ** 2).sum()])

"""The layout, time-embedding, small-attention and conv_out launchers called DIRECTLY, against tests/small_kernels_ref.py (which
tests/test_small_kernels_host.py pins to torch's own operators on the CPU).

csrc/elementwise.hip   siss_upsample2x, siss_upsample2x_bwd, siss_concat, siss_concat_tail, siss_concat_bwd, siss_add_inplace,
                       siss_space_to_depth_ld, siss_space_to_depth, siss_depth_to_space, siss_pad_to_compact, siss_compact_add_to_pad,
                       siss_transpose_bf16, siss_im2col3x3, siss_colsum, siss_nchw_channel_sums
csrc/timeemb.hip       siss_timestep_sincos, siss_linear_small_fwd, siss_linear_small_bwd, siss_linear_multi_fwd, siss_linear_multi_bwd
csrc/attention.hip     siss_softmax_fwd, siss_softmax_bwd, siss_mha_small_fwd, siss_mha_small_bwd, siss_mha_small_takes
csrc/conv_small.hip    siss_conv_out_dgrad, siss_conv_out_wgrad (siss_conv_out_fprop: its f32 form here, the bf16 forms in
                       tests/test_hip_unet_cond.py)
csrc/f32_path.hip      every activation kernel above runs a second time under lib.f32_mode(True), which routes the call to
                       siss_upsample2x_f32, siss_upsample2x_bwd_f32, siss_concat_f32, siss_concat_tail_f32, siss_concat_bwd_f32,
                       siss_add_inplace_f32, siss_space_to_depth_ld_f32, siss_depth_to_space_f32, siss_pad_to_compact_f32,
                       siss_compact_add_to_pad_f32, siss_transpose_f32, siss_im2col3x3_f32, siss_softmax_fwd_f32, siss_softmax_bwd_f32,
                       siss_mha_small_fwd_f32, siss_mha_small_bwd_f32, siss_conv_out_fprop_f32

Every output lives in a buffer pre-filled with a sentinel, halo rows and a guard stretch on either side included, and the WHOLE
buffer is compared: what a launcher does not promise to write must come back bit-identical.  Data movement and the one-rounding
adds are bitwise; the sums through f32 atomics are made exact with small integers; the dot products carry the a-priori bound
(n + 2) 2^-24 sum |term| (plus the activation's own error, from its construction in csrc/common.h); softmax, attention and the
sinusoidal embedding are held to a multiple of the error of torch's OWN f32 evaluation of the same expression against f64 (4x, 4x
and 2x: margins set before the first measurement).  Measured values: docs/kernels.md, "Small kernels: measured precision".
"""
import math

import pytest
import torch

import small_kernels_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DT = {"bf16": BF, "f32": F32}
U = 2.0 ** -24                       # f32 unit roundoff
SENT = 77.0                          # exact in bf16
SHAPES = [(2, 4, 6), (3, 8, 8), (1, 2, 2)]
ACT_CASES = [(dt, *s, C) for dt in DT for s in SHAPES for C in (8, 24, 96, 320) + ((20,) if dt == "f32" else ())]
OTHER_C = {8: 24, 24: 8, 96: 320, 320: 96, 20: 12}                 # the second part of a concat: seams off the powers of two
GRID_CAP = (3, 64, 64, 1368)         # 3 * 4096 * 171 = 2,101,248 chunks > 8192 blocks * 256 threads: the grid-stride loop


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def launch(dt, name, *args):
    """lib.call in the bf16 or the f32 mode (which routes `name` to its `_f32` form)."""
    from siss_amd import lib
    with lib.f32_mode(dt == "f32"):
        lib.call(name, *args)
    torch.cuda.synchronize()


def refused(dt, name, *args):
    with pytest.raises(RuntimeError, match="bad argument"):
        launch(dt, name, *args)


class Buf:
    """An output tensor inside a sentinel-filled flat buffer with a guard stretch before and after it."""

    def __init__(self, shape, dtype, dev, body=None, fill=SENT):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.g = -(-max(4 * shape[-1], 64) // 8) * 8                  # guard elements: a few rows, 16-B aligned
        self.flat = torch.full((self.n + 2 * self.g,), fill, dtype=dtype)
        if body is not None:
            self.host[:] = body
        self.d = self.flat.to(dev)

    @property
    def host(self):
        return self.flat[self.g:self.g + self.n].view(self.shape)

    @property
    def t(self):
        """The device tensor handed to the launcher."""
        return self.d[self.g:self.g + self.n].view(self.shape)

    def check(self, want, what):
        """The whole device buffer against the initial fill with `want` as its body, bit for bit."""
        e = self.flat.clone()
        e[self.g:self.g + self.n] = want.reshape(-1).to(e.dtype)
        same(self.d.cpu(), e, what)

    def guards(self, what):
        """The guard stretches alone (the body is held to a tolerance elsewhere)."""
        got = self.d.cpu()
        same(got[:self.g], self.flat[:self.g], what + ": guard before")
        same(got[-self.g:], self.flat[-self.g:], what + ": guard after")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got) != bits(want)
    if bool(ne.any()):
        i = ne.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, the first at flat index {i}: "
                             f"got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}")


def rnd(shape, dtype, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=device).to(dtype)


def ints(shape, lo, hi, dtype, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).to(dtype)


def padded(N, H, W, C, dtype, seed, device="cpu"):
    """Random padded NHWC tensor; the halo is random too (a kernel that reads it where it should not is caught)."""
    return rnd((N, H + 2, W + 2, C), dtype, seed, device)


# ================================================================ csrc/elementwise.hip: data movement and one-rounding adds
@pytest.mark.parametrize("dt,N,H,W,C", ACT_CASES)
def test_upsample2x_and_backward(dev, dt, N, H, W, C):
    T = DT[dt]
    x = padded(N, H, W, C, T, 1)
    out = Buf((N, 2 * H + 2, 2 * W + 2, C), T, dev)
    launch(dt, "siss_upsample2x", x.to(dev), out.t, N, H, W, C)
    out.check(R.upsample2x(x, out.host), "upsample2x")
    dout = padded(N, 2 * H, 2 * W, C, T, 2)
    din = Buf((N, H + 2, W + 2, C), T, dev)
    launch(dt, "siss_upsample2x_bwd", dout.to(dev), din.t, N, H, W, C)
    din.check(R.upsample2x_bwd(dout, din.host), "upsample2x_bwd")


@pytest.mark.parametrize("dt,N,H,W,C", ACT_CASES)
def test_concat_family(dev, dt, N, H, W, C):
    T, Ca, Cb = DT[dt], C, OTHER_C[C]
    a, b = padded(N, H, W, Ca, T, 3), padded(N, H, W, Cb, T, 4)
    out = Buf((N, H + 2, W + 2, Ca + Cb), T, dev)
    launch(dt, "siss_concat", a.to(dev), b.to(dev), out.t, N, H, W, Ca, Cb)
    out.check(R.concat(a, b, out.host), "concat")
    tail = Buf((N, H + 2, W + 2, Ca + Cb), T, dev)                        # the first Ca columns stay the sentinel
    launch(dt, "siss_concat_tail", b.to(dev), tail.t, N, H, W, Ca, Cb)
    tail.check(R.concat_tail(b, tail.host, Ca), "concat_tail")
    dcat = padded(N, H, W, Ca + Cb, T, 5)
    pre = padded(N, H, W, Cb, T, 6)                                       # db's prior content: flag 0 overwrites it, flag 1 adds to it
    for flag in (0, 1):
        da, db = Buf((N, H + 2, W + 2, Ca), T, dev), Buf((N, H + 2, W + 2, Cb), T, dev, body=pre)
        launch(dt, "siss_concat_bwd", dcat.to(dev), da.t, db.t, flag, N, H, W, Ca, Cb)
        ea, eb = R.concat_bwd(dcat, da.host, db.host, flag)
        da.check(ea, f"concat_bwd da (accumulate_b = {flag})")
        db.check(eb, f"concat_bwd db (accumulate_b = {flag})")


@pytest.mark.parametrize("dt,N,H,W,C", ACT_CASES)
def test_add_and_compact(dev, dt, N, H, W, C):
    T = DT[dt]
    a0, b = padded(N, H, W, C, T, 7), padded(N, H, W, C, T, 8)
    a = Buf((N, H + 2, W + 2, C), T, dev, body=a0)
    launch(dt, "siss_add_inplace", a.t, b.to(dev), N, H, W, C)
    a.check(R.add_inplace(a0, b), "add_inplace")                          # a's own halo is part of what must not change
    comp = Buf((N, H * W, C), T, dev)
    launch(dt, "siss_pad_to_compact", a0.to(dev), comp.t, N, H, W, C)
    comp.check(R.pad_to_compact(a0), "pad_to_compact")
    c = rnd((N, H * W, C), T, 9)
    for res in (None, b):
        out = Buf((N, H + 2, W + 2, C), T, dev)
        launch(dt, "siss_compact_add_to_pad", c.to(dev), None if res is None else res.to(dev), out.t, N, H, W, C)
        out.check(R.compact_add_to_pad(c, res, out.host), f"compact_add_to_pad (res {'given' if res is not None else 'None'})")


@pytest.mark.parametrize("dt,N,H,W,C", ACT_CASES)
def test_space_to_depth_and_back(dev, dt, N, H, W, C):
    T = DT[dt]
    x = padded(N, H, W, C, T, 10)
    z = Buf((N, H // 2 + 2, W // 2 + 2, 4 * C), T, dev)
    launch(dt, "siss_space_to_depth_ld", x.to(dev), z.t, N, H, W, C, 0)
    want = R.space_to_depth(x, z.host)
    z.check(want, "space_to_depth_ld (ld_in = 0)")
    wide = rnd((N, H + 2, W + 2, C + 16), T, 11)                          # ld_in > C: x as columns [8, 8 + C) of a wider tensor
    wide[..., 8:8 + C] = x
    z2 = Buf(z.shape, T, dev)
    launch(dt, "siss_space_to_depth_ld", wide.to(dev)[..., 8:8 + C], z2.t, N, H, W, C, C + 16)
    z2.check(want, "space_to_depth_ld (ld_in = C + 16, column 8)")
    if dt == "bf16":                                                      # the plain entry point (no f32 form: the engine calls _ld)
        z3 = Buf(z.shape, T, dev)
        launch(dt, "siss_space_to_depth", x.to(dev), z3.t, N, H, W, C)
        z3.check(want, "space_to_depth")
    dz = padded(N, H // 2, W // 2, 4 * C, T, 12)
    pre = padded(N, H, W, C, T, 13)
    for flag in (0, 1):
        din = Buf((N, H + 2, W + 2, C), T, dev, body=pre)
        launch(dt, "siss_depth_to_space", dz.to(dev), din.t, flag, N, H, W, C)
        din.check(R.depth_to_space(dz, din.host, flag), f"depth_to_space (accumulate = {flag})")


@pytest.mark.parametrize("name", ["upsample2x_bwd", "concat", "add_inplace"])
def test_grid_stride_loop_behind_the_block_cap(dev, name):
    """The only shape whose chunk count exceeds grid_for's 8192 blocks of 256 threads.  Data and reference live on the device
    (the same index arithmetic of small_kernels_ref, on device tensors): 36-145 MB tensors."""
    N, H, W, C = GRID_CAP
    assert N * H * W * (C // 8) > 8192 * 256

    def small(shape, seed):                                               # multiples of 1 / 8 in [-8, 8): cheap to draw, sums still round
        g = torch.Generator(device=dev).manual_seed(seed)
        return (torch.randint(-64, 64, shape, generator=g, device=dev).float() / 8).to(BF)
    if name == "upsample2x_bwd":
        dout = small((N, 2 * H + 2, 2 * W + 2, C), 14)
        din = torch.full((N, H + 2, W + 2, C), SENT, dtype=BF, device=dev)
        want = R.upsample2x_bwd(dout, din)
        launch("bf16", "siss_upsample2x_bwd", dout, din, N, H, W, C)
        same(din, want, name)
    elif name == "concat":
        Ca, Cb = C - 160, 160
        a, b = small((N, H + 2, W + 2, Ca), 15), small((N, H + 2, W + 2, Cb), 16)
        out = torch.full((N, H + 2, W + 2, C), SENT, dtype=BF, device=dev)
        want = R.concat(a, b, out)
        launch("bf16", "siss_concat", a, b, out, N, H, W, Ca, Cb)
        same(out, want, name)
    else:
        a, b = small((N, H + 2, W + 2, C), 17), small((N, H + 2, W + 2, C), 18)
        want = R.add_inplace(a, b)
        launch("bf16", "siss_add_inplace", a, b, N, H, W, C)
        same(a, want, name)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("B,Rr,C", [(3, 1, 1), (2, 33, 31), (2, 64, 96), (1, 257, 40)])
def test_transpose(dev, dt, B, Rr, C):
    x = rnd((B, Rr, C), DT[dt], 19)
    out = Buf((B, C, Rr), DT[dt], dev)
    launch(dt, "siss_transpose_bf16", x.to(dev), out.t, B, Rr, C)
    out.check(R.transpose(x), "transpose")


IM2COL_FAST = [(N, Cin, H, W, 64) for (N, H, W) in [(2, 5, 7), (1, 16, 16), (1, 1, 1)] for Cin in (1, 3, 4)]
IM2COL_GENERIC = [(2, Cin, 5, 7, K) for (Cin, K) in [(2, 32), (4, 40), (3, 32), (8, 72), (5, 48)]]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("N,Cin,H,W,K", IM2COL_FAST + IM2COL_GENERIC)
def test_im2col3x3(dev, N, Cin, H, W, K, flip):
    """bf16 rows from an f32 image (rounded to nearest even) and from a bf16 image; f32 rows from an f32 image (the _f32 form).
    Halo rows and the columns at or beyond 9 Cin are ZEROS the launcher writes: nothing of the sentinel survives but the guards."""
    img = rnd((N, Cin, H, W), F32, 20)
    for dt, src in (("bf16", img), ("bf16", img.to(BF)), ("f32", img)):
        out = Buf((N, H + 2, W + 2, K), DT[dt], dev)
        launch(dt, "siss_im2col3x3", src.to(dev), int(src.dtype == BF), out.t, N, Cin, H, W, K, flip)
        want = R.im2col3x3(src, K, flip, DT[dt])
        assert float(want[..., 9 * Cin:].abs().max() if K > 9 * Cin else 0) == 0 and float(want[:, 0].abs().max()) == 0
        out.check(want, f"im2col3x3 {dt} rows from a {src.dtype} image, flip = {flip}")
    out = Buf((N, H + 2, W + 2, K), F32, dev)
    refused("f32", "siss_im2col3x3", img.to(BF).to(dev), 1, out.t, N, Cin, H, W, K, flip)           # no bf16 image in the f32 mode


# ================================================================ sums through f32 atomics, exact by construction
@pytest.mark.parametrize("out2", [0, 1])
@pytest.mark.parametrize("rows", [1, 37, 5000])
@pytest.mark.parametrize("C", [8, 96, 320, 2048])
def test_colsum_exact(dev, C, rows, out2):
    nsets, stride = 2, C + 5
    y = ints((nsets * rows, C), -8, 8, BF, 21)
    pre = ints((nsets * stride,), -3, 3, F32, 22)
    o1 = Buf((nsets * stride,), F32, dev, body=pre)
    o2 = Buf((nsets * stride,), F32, dev, body=pre + 1) if out2 else None
    launch("bf16", "siss_colsum", y.to(dev), rows, C, nsets, stride, o1.t, o2.t if out2 else None)
    add = torch.zeros(nsets, stride, dtype=torch.int64)
    add[:, :C] = R.colsum(y.long(), nsets, rows)
    assert int(add.abs().max()) + 4 < 2 ** 24
    o1.check((pre.long() + add.reshape(-1)).float(), "colsum out")
    if out2:
        o2.check((pre.long() + 1 + add.reshape(-1)).float(), "colsum out2")


def test_colsum_refuses_more_than_256_chunks(dev):
    y = torch.zeros(4, 2056, dtype=BF, device=dev)
    refused("bf16", "siss_colsum", y, 4, 2056, 1, 2056, torch.zeros(2056, device=dev), None)


@pytest.mark.parametrize("nsets,set_images,C,hw", [(2, 3, 3, 49), (1, 1, 4, 1), (2, 2, 1, 70000)])
def test_nchw_channel_sums_exact(dev, nsets, set_images, C, hw):
    stride = C + 3
    img = ints((nsets * set_images, C, hw), -8, 8, F32, 23)
    pre = ints((nsets * stride,), -3, 3, F32, 24)
    for dt in DT:                                                          # lib.F32_SAME: one kernel serves both modes
        out = Buf((nsets * stride,), F32, dev, body=pre)
        launch(dt, "siss_nchw_channel_sums", img.to(dev), nsets, set_images, C, hw, stride, out.t)
        add = torch.zeros(nsets, stride, dtype=torch.int64)
        add[:, :C] = R.nchw_channel_sums(img.long(), nsets, set_images)
        assert int(add.abs().max()) + 4 < 2 ** 24
        out.check((pre.long() + add.reshape(-1)).float(), "nchw_channel_sums")


# ================================================================ csrc/timeemb.hip (f32 throughout; lib.F32_SAME)
def within(got, ref, bound, what):
    """|got - ref| <= bound element by element (f64); returns and prints the worst error / bound ratio."""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), what
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[small-kernels] {what}: worst |err| {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} > 1 (worst |err| {float(err.max()):.3e})"
    return ratio


LINEAR = [(3, 5, 70), (11, 3, 64), (16, 256, 200)]


@pytest.mark.parametrize("M,N,K", LINEAR)
def test_linear_small_exact_integers(dev, M, N, K):
    """Integers in [-4, 4], no activation: every sum is an integer far below 2^24, so any order gives the int64 reference's bits.
    N = 3 leaves wave ranges of linear_bwd_dx_kernel empty; rows M .. 2M - 1 of dy use saved row m % Mx."""
    x, W, b = ints((M, K), -4, 4, F32, 25), ints((N, K), -4, 4, F32, 26), ints((N,), -4, 4, F32, 27)
    y = Buf((M, N), F32, dev)
    launch("bf16", "siss_linear_small_fwd", x.to(dev), W.to(dev), b.to(dev), y.t, M, N, K, 0)
    y.check(R.linear_fwd(x.long(), W.long(), b.long(), 0).float(), "linear_small_fwd")
    M2, ssw, ssb = 2 * M, N * K + 7, N + 3
    dy = ints((M2, N), -4, 4, F32, 28)
    dx_r, dW_r, db_r = R.linear_bwd(dy.long(), None, x.long(), W.long(), M, M, 0)
    pw, pb, pdx = ints((2 * ssw,), -5, 5, F32, 29), ints((2 * ssb,), -5, 5, F32, 30), ints((M2, K), -5, 5, F32, 31)
    ew, eb = pw.long().reshape(2, ssw).clone(), pb.long().reshape(2, ssb).clone()
    ew[:, :N * K] += dW_r.reshape(2, -1)
    eb[:, :N] += db_r
    for mode in ("none", "overwrite", "accumulate"):
        dW, db, db2 = Buf((2 * ssw,), F32, dev, body=pw), Buf((2 * ssb,), F32, dev, body=pb), Buf((2 * ssb,), F32, dev, body=pb + 1)
        dx = Buf((M2, K), F32, dev, body=pdx)
        launch("f32", "siss_linear_small_bwd", dy.to(dev), None, x.to(dev), W.to(dev), None if mode == "none" else dx.t,
               int(mode == "accumulate"), dW.t, db.t, db2.t, M2, M, M, ssw, ssb, N, K, 0)
        dW.check(ew.reshape(-1).float(), f"linear_small_bwd dW (dx {mode})")
        db.check(eb.reshape(-1).float(), "linear_small_bwd db")
        db2.check((eb.reshape(-1) + 1).float(), "linear_small_bwd db2")
        dx.check({"none": pdx, "overwrite": dx_r.float(), "accumulate": (pdx.long() + dx_r).float()}[mode], f"linear_small_bwd dx ({mode})")


@pytest.mark.parametrize("M,N,K", LINEAR)
def test_linear_small_silu_within_the_dot_product_bound(dev, M, N, K):
    """N(0, 1) data, SiLU on the input and on the output (yact).  |err| <= (n + 2) 2^-24 sum |term| for a dot product of n f32 terms
    in any order, plus each term's activation error: (4 + 2 |z|) 2^-24 relative for silu_f, (8 + 4 |z|) 2^-24 for dsilu_f."""
    x, W, b = rnd((M, K), F64, 32), rnd((N, K), F64, 33), rnd((N,), F64, 34)
    x, W, b = x.float().double(), W.float().double(), b.float().double()
    y = Buf((M, N), F32, dev)
    launch("bf16", "siss_linear_small_fwd", x.float().to(dev), W.float().to(dev), b.float().to(dev), y.t, M, N, K, 1)
    sx, ax = R.silu(x), 4 + 2 * x.abs()
    tsum = sx.abs() @ W.abs().T + b.abs()
    within(y.t.cpu(), R.linear_fwd(x, W, b, 1), (K + 3) * U * tsum + U * ((sx.abs() * ax) @ W.abs().T), f"linear_small_fwd {M, N, K}")
    M2, ssw, ssb = 2 * M, N * K + 7, N + 3
    dy, yact = rnd((M2, N), F32, 35).double(), rnd((M, N), F32, 36).double()
    dx_r, dW_r, db_r = R.linear_bwd(dy, yact, x, W, M, M, 1)
    idx = torch.arange(M2) % M
    de, ade = dy * R.dsilu(yact[idx]), 8 + 4 * yact[idx].abs()
    xa, axa = sx[idx], ax[idx]
    pw, pb, pdx = rnd((2, ssw), F32, 37).double(), rnd((2, ssb), F32, 38).double(), rnd((M2, K), F32, 39).double()
    dW, db = Buf((2 * ssw,), F32, dev, body=pw.reshape(-1)), Buf((2 * ssb,), F32, dev, body=pb.reshape(-1))
    db2, dx = Buf((2 * ssb,), F32, dev, body=pb.reshape(-1)), Buf((M2, K), F32, dev, body=pdx)
    launch("bf16", "siss_linear_small_bwd", dy.float().to(dev), yact.float().to(dev), x.float().to(dev), W.float().to(dev), dx.t, 1,
           dW.t, db.t, db2.t, M2, M, M, ssw, ssb, N, K, 1)
    within(dx.t.cpu(), pdx + dx_r, (N + 3) * U * (de.abs() @ W.abs() + pdx.abs()) + U * ((de.abs() * ade) @ W.abs()),
           f"linear_small_bwd dx {M, N, K}")
    sets = [slice(s * M, (s + 1) * M) for s in range(2)]
    tW = torch.stack([de[s].abs().T @ xa[s].abs() for s in sets]) + pw[:, :N * K].reshape(2, N, K).abs()
    aW = torch.stack([(de[s].abs() * ade[s]).T @ xa[s].abs() + de[s].abs().T @ (xa[s].abs() * axa[s]) for s in sets])
    got = dW.t.cpu().reshape(2, ssw)
    within(got[:, :N * K].reshape(2, N, K), pw[:, :N * K].reshape(2, N, K) + dW_r, (M + 3) * U * tW + U * aW, f"linear_small_bwd dW {M, N, K}")
    same(got[:, N * K:], pw[:, N * K:].float(), "the floats between the sets of dW")
    tb = de.abs().reshape(2, M, N).sum(1) + pb[:, :N].abs()
    ab = (de.abs() * ade).reshape(2, M, N).sum(1)
    for o, nm in ((db, "db"), (db2, "db2")):
        g = o.t.cpu().reshape(2, ssb)
        within(g[:, :N], pb[:, :N] + db_r, (M + 3) * U * tb + U * ab, f"linear_small_bwd {nm} {M, N, K}")
        same(g[:, N:], pb[:, N:].float(), f"the floats between the sets of {nm}")


MULTI = [(3, 37, 200), (11, 549, 300), (8, 64, 256)]


@pytest.mark.parametrize("M,Ntot,K", MULTI)
def test_linear_multi_fwd(dev, M, Ntot, K):
    woff, boff, _, used = R.multi_tables(Ntot, K, 40)
    P, x = rnd((used,), F32, 41).double(), rnd((M, K), F32, 42).double()
    y = Buf((M, Ntot), F32, dev)
    launch("f32", "siss_linear_multi_fwd", x.float().to(dev), P.float().to(dev), woff.to(dev), boff.to(dev), y.t, M, Ntot, K)
    rows = P[woff[:, None] + torch.arange(K)[None, :]].abs()
    sx = R.silu(x).abs()
    within(y.t.cpu(), R.multi_fwd(x, P, woff, boff, K), (K + 3) * U * (sx @ rows.T + P[boff].abs()) + U * ((sx * (4 + 2 * x.abs())) @ rows.T),
           f"linear_multi_fwd {M, Ntot, K}")
    y.guards("linear_multi_fwd y")


@pytest.mark.parametrize("set_rows", [3, 33])
@pytest.mark.parametrize("M,Ntot,K", MULTI)
def test_linear_multi_bwd(dev, M, Ntot, K, set_rows):
    """Shuffled weight rows with gaps, biases and shared biases in regions of their own, set stride beyond what a set uses; 33 rows
    per set = one 32-row chunk and a one-row tail; Ntot = 549 = one 512-column split and a 37-column one (a tail for the 4-wide
    unroll and for the 32-column blocks).  Floats of the gradient buffer that no table points to stay bitwise."""
    woff, boff, boff2, used = R.multi_tables(Ntot, K, 43)
    stride, Mx, M2 = used + 13, set_rows, 2 * set_rows
    P, x = rnd((used,), F32, 44).double(), rnd((Mx, K), F32, 45).double()
    dy, G0 = rnd((M2, Ntot), F32, 46).double(), rnd((2 * stride,), F32, 47).double()
    G = Buf((2 * stride,), F32, dev, body=G0)
    dx = Buf((M2, K), F32, dev, fill=0.0)
    launch("bf16", "siss_linear_multi_bwd", dy.float().to(dev), x.float().to(dev), P.float().to(dev), G.t, woff.to(dev), boff.to(dev),
           boff2.to(dev), dx.t, M2, Mx, set_rows, stride, Ntot, K)
    G_r, dx_r = R.multi_bwd(dy, x, P, G0, woff, boff, boff2, Mx, set_rows, stride, K)
    sx = R.silu(x).abs()
    tG, _ = R.multi_bwd(dy.abs(), x, P, G0.abs(), woff, boff, boff2, Mx, set_rows, stride, K, sx=sx)
    aG, _ = R.multi_bwd(dy.abs(), x, P, torch.zeros_like(G0), woff, boff, boff2, Mx, set_rows, stride, K, sx=sx * (4 + 2 * x.abs()))
    touched = torch.zeros(2 * stride, dtype=torch.bool)
    for s in range(2):
        touched[s * stride + (woff[:, None] + torch.arange(K)[None, :]).reshape(-1)] = True
        touched[s * stride + boff] = True
        touched[s * stride + boff2] = True
    aG[~touched] = 0
    aG[(torch.arange(2)[:, None] * stride + torch.cat([boff, boff2])[None, :]).reshape(-1)] = 0      # bias sums carry no activation
    got = G.t.cpu()
    within(got[touched], G_r[touched], (set_rows + 3) * U * tG[touched] + U * aG[touched], f"linear_multi_bwd grads {M, Ntot, K, set_rows}")
    same(got[~touched], G0.float()[~touched], "gradient floats no table points to")
    rows = P[woff[:, None] + torch.arange(K)[None, :]].abs()
    within(dx.t.cpu(), dx_r, (Ntot + 3) * U * (dy.abs() @ rows), f"linear_multi_bwd dx {M, Ntot, K, set_rows}")
    G.guards("linear_multi_bwd grads"); dx.guards("linear_multi_bwd dx")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dim", [6, 128, 320])
def test_timestep_sincos(dev, dim, flip, shift):
    """Against f64; allowed: twice the worst error of torch's own f32 evaluation of the same (diffusers) expression on the CPU --
    both round the same f32 argument t * freq -- with a floor of 2^-22."""
    t = torch.tensor([0, 1, 500, 998, 999])
    ref = R.timestep_sincos(t, dim, flip, shift)
    e_ref = float((R.timestep_sincos(t, dim, flip, shift, F32).double() - ref).abs().max())
    out = Buf((5, dim), F32, dev)
    launch("f32", "siss_timestep_sincos", t.to(dev), out.t, 5, dim, flip, float(shift))
    got = out.t.cpu()
    err = float((got.double() - ref).abs().max())
    print(f"[small-kernels] timestep_sincos dim {dim} flip {flip} shift {shift}: e_ref {e_ref:.3e}, kernel {err:.3e}, allowed {max(2 * e_ref, 2.0 ** -22):.3e}")
    half = dim // 2
    sin_half = got[0, half:] if flip else got[0, :half]                    # t = 0: the sin half is exactly zero, the cos half one
    cos_half = got[0, :half] if flip else got[0, half:]
    assert float(sin_half.abs().max()) == 0 and float((cos_half - 1).abs().max()) == 0
    out.guards("timestep_sincos")
    assert err <= max(2 * e_ref, 2.0 ** -22), f"kernel {err:.3e} > 2 x torch f32 {e_ref:.3e}"


# ================================================================ csrc/attention.hip
def rel_rowmax(x, ref):
    """worst element error relative to its row's largest reference value"""
    return float(((x.double() - ref).abs() / ref.abs().amax(-1, keepdim=True).clamp_min(1e-300)).max())


SOFTMAX = [(1, 1.0), (63, 1.0), (64, 1.0), (65, 1.0), (256, 1.0), (256, 30.0), (1000, 1.0), (1024, 1.0)]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("S,spread", SOFTMAX)
def test_softmax_fwd_bwd(dev, dt, S, spread):
    """f32 form: at most 4x the error of torch's f32 softmax / f32 autograd against f64, per element relative to its row's largest
    reference value.  bf16 form: 2^-8 |ref| (one rounding) on top of that, the reference formed from the bf16-rounded inputs."""
    T, rows = DT[dt], 7
    s = (rnd((rows, S), F32, 48) * spread).to(T)
    if spread > 1:                       # scores over +-30 (the max subtraction), two of them near the top so that no row is one-hot
        s = (rnd((rows, S), F32, 48) * 10).clamp(-30, 30).to(T)
        s[:, 0], s[:, 1], s[:, -1] = 30, 29.5, -30
    ref = R.softmax_fwd(s.double())
    e_ref = rel_rowmax(torch.softmax(s.float(), -1), ref)
    p = Buf((rows, S), T, dev)
    launch(dt, "siss_softmax_fwd", s.to(dev), p.t, rows, S)
    got = p.t.cpu()
    d = 4 * e_ref * ref.amax(-1, keepdim=True)
    tol = d + (2.0 ** -8 * ref if dt == "bf16" else 0)
    err = (got.double() - ref).abs()
    print(f"[small-kernels] softmax_fwd {dt} S {S} spread {spread}: e_ref {e_ref:.3e}, kernel {rel_rowmax(got, ref):.3e}, worst err / allowed {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    p.guards("softmax_fwd")
    fwd_ok = bool((err <= tol).all())
    # backward: p_rows = rows and rows = 2 * p_rows (the second cotangent set re-reads the saved rows)
    pin = ref.to(T)
    results = []
    for nr in (rows, 2 * rows):
        dp = rnd((nr, S), T, 49)
        sg = s.float().requires_grad_(True)
        pf = torch.softmax(sg, -1)
        sd = s.double().requires_grad_(True)
        pd = torch.softmax(sd, -1)
        g64 = torch.cat([torch.autograd.grad(pd, sd, dp[z * rows:(z + 1) * rows].double(), retain_graph=True)[0] for z in range(nr // rows)])
        g32 = torch.cat([torch.autograd.grad(pf, sg, dp[z * rows:(z + 1) * rows].float(), retain_graph=True)[0] for z in range(nr // rows)])
        e_b = rel_rowmax(g32, g64)                                       # torch's f32 autograd against f64 autograd
        refb = R.softmax_bwd(pin.double(), dp.double(), rows, 0.25)      # the launcher's own inputs: the (rounded) saved p
        ds = Buf((nr, S), T, dev)
        launch(dt, "siss_softmax_bwd", pin.to(dev), dp.to(dev), ds.t, nr, rows, S, 0.25)
        gb = ds.t.cpu()
        tolb = 4 * e_b * refb.abs().amax(-1, keepdim=True) + (2.0 ** -8 * refb.abs() if dt == "bf16" else 0)
        errb = (gb.double() - refb).abs()
        print(f"[small-kernels] softmax_bwd {dt} S {S} spread {spread} rows {nr}: e_ref {e_b:.3e}, kernel {rel_rowmax(gb, refb):.3e}, "
              f"worst err / allowed {float((errb / tolb.clamp_min(1e-300)).max()):.3f}")
        ds.guards("softmax_bwd")
        results.append(bool((errb <= tolb).all()))
    assert fwd_ok, "softmax_fwd beyond 4 x torch's own f32 error (+ one bf16 rounding)"
    assert all(results), "softmax_bwd beyond 4 x torch's own f32 error (+ one bf16 rounding)"


def test_softmax_bf16_refuses_rows_longer_than_1024(dev):
    t = torch.zeros(4, 1025, dtype=BF, device=dev)
    refused("bf16", "siss_softmax_fwd", t, t.clone(), 4, 1025)
    refused("bf16", "siss_softmax_bwd", t, t, t.clone(), 4, 4, 1025, 1.0)


MHA = [(8, 3, 1, 1.0), (8, 1, 50, 1.0), (8, 3, 64, 1.0), (8, 3, 300, 1.0), (8, 1, 64, 6.0), (32, 3, 50, 1.0), (32, 1, 126, 1.0), (16, 3, 200, 1.0)]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("D,heads,S,qscale", MHA)
def test_mha_small_fwd_bwd(dev, dt, D, heads, S, qscale):
    """f64 softmax(scale q k^T) v per head, natural-log lse, and the backward of two cotangent sets against one saved forward (saved
    index n2 % nx).  Allowed: 4x the error of torch's own f32 evaluation (forward) / f32 autograd (backward) against f64, relative to
    each output tensor's largest value; 2^-8 |ref| more for the bf16 form's bf16 outputs; lse is f32 in both forms.  S = 300 runs the
    i += 256 row loops, 126 is the backward's largest S at D = 32."""
    T, N, n2, C, scale = DT[dt], 2, 4, D * heads, D ** -0.5
    q, k, v = (rnd((N, S, C), T, 50 + i) for i in range(3))
    q = (q.float() * qscale).to(T)
    do = rnd((n2, S, C), T, 53)
    o_ref, lse_ref = R.mha_fwd(q.double(), k.double(), v.double(), D, scale)
    o32, lse32 = R.mha_fwd(q.float(), k.float(), v.float(), D, scale)

    def rel(x, ref):
        return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    report, ok = [], True

    def hold(name, got, ref, e_ref, rounded, floor=0.0):
        nonlocal ok
        tol = 4 * e_ref * ref.abs().max() + floor + (2.0 ** -8 * ref.abs() if rounded else torch.zeros_like(ref))
        err = (got.double() - ref).abs()
        worst = float((err / tol.clamp_min(1e-300)).max())
        report.append(f"{name}: e_ref {e_ref:.3e} kernel {rel(got, ref):.3e} err/allowed {worst:.3f}")
        ok = ok and math.isfinite(worst) and worst <= 1.0

    o, lse = Buf((N, S, C), T, dev), Buf((N, heads, S), F32, dev)
    launch(dt, "siss_mha_small_fwd", q.to(dev), k.to(dev), v.to(dev), o.t, lse.t, N, S, C, D, scale)
    og, lg = o.t.cpu(), lse.t.cpu()
    o.guards("mha_small_fwd o"); lse.guards("mha_small_fwd lse")
    hold("o", og, o_ref, rel(o32, o_ref), dt == "bf16")
    hold("lse", lg, lse_ref, rel(lse32, lse_ref), False)
    # backward from the launcher's own inputs: the saved o (rounded to the activation type) and lse (f32) of the reference forward
    o_in, lse_in = o_ref.to(T), lse_ref.float()
    refs = R.mha_bwd(q.double(), k.double(), v.double(), o_in.double(), lse_in.double(), do.double(), D, scale)
    qg, kg, vg = (t.float().requires_grad_(True) for t in (q, k, v))
    of, _ = R.mha_fwd(qg, kg, vg, D, scale)
    g32 = [torch.autograd.grad(of, (qg, kg, vg), do[z * N:(z + 1) * N].float(), retain_graph=True) for z in range(2)]
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    od, _ = R.mha_fwd(qd, kd, vd, D, scale)
    g64 = [torch.autograd.grad(od, (qd, kd, vd), do[z * N:(z + 1) * N].double(), retain_graph=True) for z in range(2)]
    outs = [Buf((n2, S, C), T, dev) for _ in range(3)]
    launch(dt, "siss_mha_small_bwd", q.to(dev), k.to(dev), v.to(dev), o_in.to(dev), lse_in.to(dev), do.to(dev), outs[0].t, outs[1].t,
           outs[2].t, n2, N, S, C, D, scale)
    # S = 1 is degenerate: softmax is the constant 1, torch evaluates it without a rounding (e_ref = 0) and dq = dk = 0 exactly, so
    # "4 x e_ref of the largest value" is zero.  There the allowed error comes from the kernel's arithmetic instead: it rebuilds
    # p = exp(scale q.k - lse) from an f32 lse (|p - 1| <= (D + 2) 2^-24 (|lse| + scale sum |q||k|) + the exponential's 2 ulp) and
    # forms dp - delta as the difference of two f32 dot products of the same D terms (<= 2 (D + 2) 2^-24 sum |dO||v|).
    floors = [0.0, 0.0, 0.0]
    if S == 1:
        idx = torch.arange(n2) % N
        qa, ka, va, da = (R._heads(t.double().abs(), D) for t in (q[idx], k[idx], v[idx], do))
        cancel = 2 * (D + 2) * U * scale * (da * va).sum(-1, keepdim=True)
        perr = (D + 2) * U * (lse_ref[idx].abs()[..., None] + scale * (qa * ka).sum(-1, keepdim=True)) + 4 * U
        floors = [R._unheads(cancel * ka), R._unheads(cancel * qa), R._unheads(perr * da)]
    for i, nm in enumerate(("dq", "dk", "dv")):
        got = outs[i].t.cpu()
        outs[i].guards(f"mha_small_bwd {nm}")
        e_ref = rel(torch.cat([g32[z][i] for z in range(2)]), torch.cat([g64[z][i] for z in range(2)]))
        hold(nm, got, refs[i], e_ref, dt == "bf16", floors[i])
    print(f"[small-kernels] mha_small {dt} D {D} heads {heads} S {S} qscale {qscale}: " + "; ".join(report))
    assert ok, "; ".join(report)


MHA_S = [64, 126, 127, 196, 256, 481, 482, 1024]


@pytest.mark.parametrize("D", [8, 16, 32])
def test_mha_small_forward_and_backward_accept_the_same_training_shapes(dev, D):
    """What siss_mha_small_takes(S, D, training = 1) grants, both launchers run; what only training = 0 grants, the forward runs
    (inference keeps its limit) and the backward refuses -- and UNetEngine refuses it BEFORE a step, naming S and D.  The limits
    are the kernels' LDS images in 64 KiB: no shape that trained before stops training."""
    from siss_amd import lib
    from siss_amd.unet import UNetEngine
    for S in MHA_S:
        inf, trn = lib.query("siss_mha_small_takes", S, D, 0), lib.query("siss_mha_small_takes", S, D, 1)
        assert inf == int(8 * S * D <= 65536) and trn == int(16 * S * D + 8 * S <= 65536), (S, D, inf, trn)
        assert inf or not trn
        lse = torch.zeros(1, 1, S, device=dev)
        for dt in DT:
            t = [torch.zeros(1, S, D, dtype=DT[dt], device=dev) for _ in range(8)]
            fwd = ("siss_mha_small_fwd", *t[:4], lse, 1, S, D, D, D ** -0.5)
            bwd = ("siss_mha_small_bwd", *t[:4], lse, *t[4:], 1, 1, S, D, D, D ** -0.5)
            launch(dt, *fwd) if inf else refused(dt, *fwd)
            launch(dt, *bwd) if trn else refused(dt, *bwd)
        if trn:
            UNetEngine._mha_check(S, D, training=True)
        else:
            with pytest.raises(ValueError, match=rf"S = {S} tokens, D = {D}\b"):
                UNetEngine._mha_check(S, D, training=True)
        if inf:
            UNetEngine._mha_check(S, D, training=False)
    assert lib.query("siss_mha_small_takes", 64, 24, 0) == 0


def test_engine_refuses_an_untrainable_attention_shape_before_the_step(dev):
    """attention_head_dim = 16 at 16 x 16 (S = 256): the forward kernel takes it, the backward kernel cannot.  The stepper refuses when
    it is built; forward() alone still serves inference; backward() refuses before its first launch, not inside a site's closure."""
    from siss_amd.config import UNet2DConfig
    from siss_amd.step import SISSStepper
    from siss_amd.unet import UNetEngine
    from oracle import schedule as Sch
    cfg = UNet2DConfig(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
                       down_block_types=("AttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "AttnUpBlock2D"),
                       layers_per_block=1, attention_head_dim=16, norm_num_groups=32, norm_eps=1e-6, downsample_padding=0,
                       flip_sin_to_cos=False, freq_shift=1)
    eng = UNetEngine(cfg, dev)
    eng.init_random(seed=1)
    assert (256, 16) in eng.mha_small_sites() and (64, 16) in eng.mha_small_sites()
    eng.check_trainable(sample_size=8)                                   # S = 64 and 16: trains
    with pytest.raises(ValueError, match=r"S = 256 tokens, D = 16\b"):
        SISSStepper(eng, Sch.alphas_cumprod(), lr=1e-4, train_batch_size=1)
    x = torch.randn(1, 3, 16, 16, device=dev)
    pred = eng.forward(x, torch.tensor([5], device=dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all())
    ntape = len(eng.tape)
    with pytest.raises(ValueError, match=r"S = 256 tokens, D = 16\b"):
        eng.backward(torch.zeros(2, 3, 16, 16, device=dev), nsets=2)
    assert len(eng.tape) == ntape                                        # no closure of the tape ran


# ================================================================ csrc/conv_small.hip
def native_w(w):
    """[CO][C][3][3] -> the kernels' [9][CO][C]"""
    CO, C = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9, CO, C).contiguous()


@pytest.mark.parametrize("N2,H,W,C,CO", [(2, 5, 7, 24, 3), (1, 1, 1, 8, 1), (2, 8, 8, 320, 4), (2, 4, 4, 128, 2)])
def test_conv_out_dgrad(dev, N2, H, W, C, CO):
    """f64 autograd of F.conv2d (pinned in the host test); bf16 output: 2^-8 |ref| + (9 CO + 2) 2^-24 sum |c| |w|; halo untouched."""
    c, w = rnd((N2, CO, H, W), F32, 54), native_w(rnd((CO, C, 3, 3), F32, 55) / 8)
    dx = Buf((N2, H + 2, W + 2, C), BF, dev)
    launch("bf16", "siss_conv_out_dgrad", c.to(dev), w.to(dev), dx.t, N2, H, W, C, CO)
    got = dx.t.cpu()
    keep = dx.host.clone()
    R.inner(keep)[:] = R.inner(got)
    dx.check(keep, "conv_out_dgrad halo and guards")
    ref = R.conv_out_dgrad(c.double(), w.double())
    bound = 2.0 ** -8 * ref.abs() + (9 * CO + 2) * U * R.conv_out_dgrad(c.double(), w.double(), absolute=True)
    within(R.inner(got), ref, bound, f"conv_out_dgrad {N2, H, W, C, CO}")


@pytest.mark.parametrize("C", [8, 64, 128])
@pytest.mark.parametrize("exact", [1, 0])
def test_conv_out_wgrad(dev, C, exact):
    """Two sets of two cotangent images against two saved images (index n2 % nx), set strides beyond 9 CO C / CO, targets pre-filled
    (the launcher adds).  exact: integers in [-8, 8] -- every partial sum an integer below 2^24, the f32 atomics give the int64
    reference's bits in any order.  Otherwise N(0, 1) data within the dot-product bound at n = set_images * H * W."""
    nsets, si, nx, H, W, CO = 2, 2, 2, 5, 7, 3
    ssw, ssb = 9 * CO * C + 5, CO + 3
    if exact:
        c, x = ints((nsets * si, CO, H, W), -8, 8, F32, 56), ints((nx, H + 2, W + 2, C), -8, 8, BF, 57)
        pw, pb = ints((nsets, ssw), -3, 3, F32, 58), ints((nsets, ssb), -3, 3, F32, 59)
    else:
        c, x = rnd((nsets * si, CO, H, W), F32, 56), rnd((nx, H + 2, W + 2, C), BF, 57)
        pw, pb = rnd((nsets, ssw), F32, 58), rnd((nsets, ssb), F32, 59)
    x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0            # the saved activation's zero halo (3x3 zero padding)
    dW, db = Buf((nsets * ssw,), F32, dev, body=pw.reshape(-1)), Buf((nsets * ssb,), F32, dev, body=pb.reshape(-1))
    launch("bf16", "siss_conv_out_wgrad", c.to(dev), x.to(dev), dW.t, db.t, nsets, si, nx, ssw, ssb, H, W, C, CO)
    acc = torch.int64 if exact else F64
    rW, rb = R.conv_out_wgrad(c.to(acc), x.to(acc), nsets, si, nx)
    eW, eb = pw.to(acc).clone(), pb.to(acc).clone()
    eW[:, :9 * CO * C] += rW.reshape(nsets, -1)
    eb[:, :CO] += rb
    if exact:
        assert int(eW.abs().max()) < 2 ** 24
        dW.check(eW.reshape(-1).float(), "conv_out_wgrad dW")
        db.check(eb.reshape(-1).float(), "conv_out_wgrad dbias")
        return
    aW, ab = R.conv_out_wgrad(c.double(), x.double(), nsets, si, nx, absolute=True)
    n = si * H * W
    gW, gb = dW.t.cpu().reshape(nsets, ssw), db.t.cpu().reshape(nsets, ssb)
    within(gW[:, :9 * CO * C], eW[:, :9 * CO * C], (n + 3) * U * (aW.reshape(nsets, -1) + pw[:, :9 * CO * C].abs().double()), f"conv_out_wgrad dW C {C}")
    within(gb[:, :CO], eb[:, :CO], (n + 3) * U * (ab + pb[:, :CO].abs().double()), f"conv_out_wgrad dbias C {C}")
    same(gW[:, 9 * CO * C:], pw[:, 9 * CO * C:], "floats between the sets of dW")
    same(gb[:, CO:], pb[:, CO:], "floats between the sets of dbias")


@pytest.mark.parametrize("C", [24, 320])
def test_conv_out_wgrad_refuses_channel_counts_off_the_powers_of_two(dev, C):
    z = torch.zeros(1, 6, 6, C, dtype=BF, device=dev)
    refused("bf16", "siss_conv_out_wgrad", torch.zeros(1, 3, 4, 4, device=dev), z, torch.zeros(27 * C, device=dev),
            torch.zeros(3, device=dev), 1, 1, 1, 27 * C, 3, 4, 4, C, 3)


def test_conv_out_fprop_f32_form_at_20_channels(dev):
    """siss_conv_out_fprop_f32 takes any C: 9 C f32 fused multiply-adds in sequence, within the dot-product bound at n = 9 C + 1."""
    B, H, W, C, CO = 2, 5, 7, 20, 3
    x = padded(B, H, W, C, F32, 60)
    x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0
    w, b = native_w(rnd((CO, C, 3, 3), F32, 61) / 8), rnd((CO,), F32, 62)
    pred = Buf((B, CO, H, W), F32, dev)
    launch("f32", "siss_conv_out_fprop", x.to(dev), w.to(dev), b.to(dev), pred.t, B, H, W, C, CO)
    got = pred.t.cpu()
    pred.guards("conv_out_fprop_f32")
    ref = R.conv_out_fprop(x.double(), w.double(), b.double())
    tsum = R.conv_out_fprop(x.double().abs(), w.double().abs(), b.double().abs())
    within(got, ref, (9 * C + 3) * U * tsum, "conv_out_fprop_f32 C 20")

"""tests/small_kernels_ref.py against torch's own operators, in f64 on the CPU, at the shapes tests/test_hip_small_kernels.py uses:
a wrong reference must not bless a wrong kernel.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import small_kernels_ref as R

F64 = torch.float64
SHAPES = [(2, 4, 6), (3, 8, 8), (1, 2, 2)]
CS = [8, 24, 96, 320, 20]


def _pad(x):
    """NCHW -> padded NHWC with a zero halo"""
    N, C, H, W = x.shape
    p = torch.zeros(N, H + 2, W + 2, C, dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return p


def _nchw(p):
    return R.inner(p).permute(0, 3, 1, 2)


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("N,H,W", SHAPES)
@pytest.mark.parametrize("C", [8, 20])
def test_upsample_and_its_backward(N, H, W, C):
    x = _rand(N, C, H, W, seed=1).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    out = torch.full((N, 2 * H + 2, 2 * W + 2, C), 7.0, dtype=F64)
    e = R.upsample2x(_pad(x.detach()), out)
    assert torch.equal(_nchw(e), y.detach())
    assert float((e[:, 0] - 7).abs().max()) == 0 and float((e[:, :, -1] - 7).abs().max()) == 0          # the halo is the caller's
    dy = _rand(N, C, 2 * H, 2 * W, seed=2)
    (dx,) = torch.autograd.grad(y, x, dy)
    got = R.upsample2x_bwd(_pad(dy).float(), torch.zeros(N, H + 2, W + 2, C))                                # f32 in, f32 sums
    torch.testing.assert_close(_nchw(got).double(), dx, rtol=0, atol=1e-5)


@pytest.mark.parametrize("N,H,W", SHAPES)
@pytest.mark.parametrize("C", [8, 24])
def test_space_to_depth_channel_order(N, H, W, C):
    x = _rand(N, C, H, W, seed=3)
    z = R.space_to_depth(_pad(x), torch.zeros(N, H // 2 + 2, W // 2 + 2, 4 * C, dtype=F64))
    # pixel_unshuffle puts channel c of plane (py, px) at c * 4 + py * 2 + px; this project at (py * 2 + px) * C + c
    pu = F.pixel_unshuffle(x, 2).reshape(N, C, 4, H // 2, W // 2).permute(0, 2, 1, 3, 4).reshape(N, 4 * C, H // 2, W // 2)
    assert torch.equal(_nchw(z), pu)
    back = R.depth_to_space(z, torch.full((N, H + 2, W + 2, C), 5.0, dtype=F64), 0)
    ps = F.pixel_shuffle(pu.reshape(N, 4, C, H // 2, W // 2).permute(0, 2, 1, 3, 4).reshape(N, 4 * C, H // 2, W // 2), 2)
    assert torch.equal(_nchw(back), ps) and torch.equal(ps, x)
    acc = R.depth_to_space(z.float(), torch.ones(N, H + 2, W + 2, C), 1)
    torch.testing.assert_close(_nchw(acc), (x + 1).float())
    # a column view of a wider tensor reads the same pixels
    wide = torch.full((N, H + 2, W + 2, C + 16), 9.0, dtype=F64)
    wide[..., 8:8 + C] = _pad(x)
    assert torch.equal(R.space_to_depth(wide[..., 8:8 + C], torch.zeros_like(z)), z)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_concat_compact_transpose(N, H, W):
    a, b = _rand(N, 8, H, W, seed=4), _rand(N, 24, H, W, seed=5)
    out = torch.full((N, H + 2, W + 2, 32), 3.0, dtype=F64)
    e = R.concat(_pad(a), _pad(b), out)
    assert torch.equal(_nchw(e), torch.cat([a, b], 1)) and float((e[:, 0] - 3).abs().max()) == 0
    t = R.concat_tail(_pad(b), out, 8)
    assert torch.equal(_nchw(t)[:, 8:], b) and float((_nchw(t)[:, :8] - 3).abs().max()) == 0
    da, db = R.concat_bwd(e, torch.zeros(N, H + 2, W + 2, 8, dtype=F64), torch.ones(N, H + 2, W + 2, 24, dtype=F64), 0)
    assert torch.equal(_nchw(da), a) and torch.equal(_nchw(db), b)
    _, db1 = R.concat_bwd(e.float(), torch.zeros(N, H + 2, W + 2, 8), torch.ones(N, H + 2, W + 2, 24), 1)
    torch.testing.assert_close(_nchw(db1), (b + 1).float())
    comp = R.pad_to_compact(_pad(a))
    assert torch.equal(comp, a.permute(0, 2, 3, 1).reshape(N, H * W, 8))
    back = R.compact_add_to_pad(comp, None, torch.full((N, H + 2, W + 2, 8), 2.0, dtype=F64))
    assert torch.equal(_nchw(back), a) and float((back[:, :, 0] - 2).abs().max()) == 0
    res = R.compact_add_to_pad(comp.float(), _pad(a).float(), torch.zeros(N, H + 2, W + 2, 8))
    torch.testing.assert_close(_nchw(res), (2 * a).float())
    torch.testing.assert_close(_nchw(R.add_inplace(_pad(a).float(), _pad(a).float())), (2 * a).float())


@pytest.mark.parametrize("B,Rr,C", [(3, 1, 1), (2, 33, 31), (2, 64, 96), (1, 257, 40)])
def test_transpose(B, Rr, C):
    x = _rand(B, Rr, C, seed=6)
    assert torch.equal(R.transpose(x), x.transpose(1, 2))


IM2COL = [(2, 1, 5, 7, 64), (2, 3, 5, 7, 64), (1, 4, 16, 16, 64), (1, 3, 1, 1, 64),
          (2, 2, 5, 7, 32), (2, 4, 5, 7, 40), (1, 3, 4, 6, 32), (1, 8, 4, 6, 72), (2, 5, 3, 3, 48)]


@pytest.mark.parametrize("N,Cin,H,W,K", IM2COL)
def test_im2col_is_unfold(N, Cin, H, W, K):
    img = _rand(N, Cin, H, W, seed=7)
    e = R.im2col3x3(img, K, 0, F64)
    u = F.unfold(img, 3, padding=1).reshape(N, Cin, 9, H, W)                     # unfold's rows: ci * 9 + tap
    want = u.permute(0, 3, 4, 2, 1).reshape(N, H, W, 9 * Cin)                    # -> tap * Cin + ci
    assert torch.equal(R.inner(e)[..., :9 * Cin], want)
    assert float(e[..., 9 * Cin:].abs().max() if K > 9 * Cin else 0) == 0
    assert float(e[:, 0].abs().max() + e[:, -1].abs().max() + e[:, :, 0].abs().max() + e[:, :, -1].abs().max()) == 0


@pytest.mark.parametrize("N,CO,H,W,C", [(2, 3, 5, 7, 8), (1, 4, 4, 4, 24), (1, 1, 1, 1, 8)])
def test_flipped_im2col_times_weights_is_the_input_gradient(N, CO, H, W, C):
    """One-panel product of the flip = 1 im2col of the cotangent with conv_out's weights == d conv2d / d input."""
    x = _rand(N, C, H, W, seed=8).requires_grad_(True)
    w = _rand(CO, C, 3, 3, seed=9)
    c = _rand(N, CO, H, W, seed=10)
    (dx,) = torch.autograd.grad(F.conv2d(x, w, padding=1), x, c)
    K = 40
    cols = R.im2col3x3(c, K, 1, F64)                                             # [N][H+2][W+2][K], k = tap * CO + o
    wk = torch.zeros(C, K, dtype=F64)
    wk[:, :9 * CO] = w.permute(1, 2, 3, 0).reshape(C, 9 * CO)                    # [C][tap * CO + o]
    got = R.inner(cols) @ wk.T                                                   # [N][H][W][C]
    torch.testing.assert_close(got.permute(0, 3, 1, 2), dx)


def test_sums():
    g = torch.Generator().manual_seed(11)
    y = torch.randint(-8, 9, (2 * 37, 24), generator=g)
    assert torch.equal(R.colsum(y, 2, 37), y.double().reshape(2, 37, 24).sum(1).long())
    img = torch.randint(-8, 9, (6, 3, 49), generator=g)
    assert torch.equal(R.nchw_channel_sums(img, 2, 3), img.reshape(2, 3, 3, 49).sum((1, 3)))


def _diffusers_timestep_embedding(t, dim, flip_sin_to_cos, shift, dtype):
    """diffusers' get_timestep_embedding (scale = 1, max_period = 10000), restated."""
    half = dim // 2
    exponent = -math.log(10000) * torch.arange(0, half, dtype=dtype) / (half - shift)
    emb = t[:, None].to(dtype) * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
    return emb


@pytest.mark.parametrize("dim", [6, 128, 320])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_sincos_is_the_diffusers_expression(dim, flip, shift):
    t = torch.tensor([0, 1, 500, 998, 999])
    for dt in (F64, torch.float32):
        assert torch.equal(R.timestep_sincos(t, dim, flip, shift, dt), _diffusers_timestep_embedding(t, dim, flip, shift, dt))
    e = R.timestep_sincos(t, dim, flip, shift)
    assert float(e[0, dim // 2:].abs().max() if flip else e[0, :dim // 2].abs().max()) == 0      # sin(0) marks the sin half


@pytest.mark.parametrize("M,N,K", [(3, 5, 70), (11, 3, 64), (16, 256, 200)])
@pytest.mark.parametrize("act", [0, 1])
def test_linear_small_is_autograd(M, N, K, act):
    x = _rand(M, K, seed=12).requires_grad_(True)
    W = _rand(N, K, seed=13).requires_grad_(True)
    b = _rand(N, seed=14).requires_grad_(True)
    y = F.linear(F.silu(x) if act else x, W, b)
    torch.testing.assert_close(R.linear_fwd(x.detach(), W.detach(), b.detach(), act), y.detach())
    dy = _rand(2 * M, N, seed=15)
    z = F.silu(y) if act else y                                  # the next op applied SiLU to y: dy_eff = dy * dsilu(y)
    dxs, dWs, dbs = [], [], []
    for s in range(2):
        gx, gW, gb = torch.autograd.grad(z, (x, W, b), dy[s * M:(s + 1) * M], retain_graph=True)
        dxs.append(gx); dWs.append(gW); dbs.append(gb)
    # R.linear_bwd's dx is the cotangent of act(x): chain it through act for the comparison with autograd's d / dx
    dx, dW, db = R.linear_bwd(dy, y.detach() if act else None, x.detach(), W.detach(), M, M, act)
    if act:
        dx = dx * R.dsilu(x.detach()).repeat(2, 1)
    torch.testing.assert_close(dx, torch.cat(dxs))
    torch.testing.assert_close(dW, torch.stack(dWs))
    torch.testing.assert_close(db, torch.stack(dbs))
    xi, Wi, bi = (torch.randint(-4, 5, s, generator=torch.Generator().manual_seed(16 + i)) for i, s in enumerate([(M, K), (N, K), (N,)]))
    assert R.linear_fwd(xi, Wi, bi, 0).dtype == torch.int64
    assert torch.equal(R.linear_fwd(xi, Wi, bi, 0), F.linear(xi.double(), Wi.double(), bi.double()).long())


@pytest.mark.parametrize("M,Ntot,K", [(3, 37, 200), (11, 549, 300), (8, 64, 256)])
def test_linear_multi_is_autograd(M, Ntot, K):
    woff, boff, boff2, used = R.multi_tables(Ntot, K, 17)
    P = _rand(used, seed=18).requires_grad_(True)
    x = _rand(M, K, seed=19).requires_grad_(True)
    rows = P[woff[:, None] + torch.arange(K)[None, :]]
    y = F.linear(F.silu(x), rows, P[boff])
    torch.testing.assert_close(R.multi_fwd(x.detach(), P.detach(), woff, boff, K), y.detach())
    dy = _rand(2 * M, Ntot, seed=20)
    stride = used + 13
    G0 = _rand(2 * stride, seed=21)
    G, dx = R.multi_bwd(dy, x.detach(), P.detach(), G0, woff, boff, boff2, M, M, stride, K)
    sx = F.silu(x.detach())
    for s in range(2):
        gP, = torch.autograd.grad(y, P, dy[s * M:(s + 1) * M], retain_graph=True)
        want = G0[s * stride:s * stride + used] + gP
        want[boff2] += dy[s * M:(s + 1) * M].sum(0)                      # the conv1 bias that shares the gradient
        torch.testing.assert_close(G[s * stride:s * stride + used], want)
        assert torch.equal(G[s * stride + used:(s + 1) * stride], G0[s * stride + used:(s + 1) * stride])
        gs, = torch.autograd.grad(y, x, dy[s * M:(s + 1) * M], retain_graph=True)
        torch.testing.assert_close(dx[s * M:(s + 1) * M] * R.dsilu(x.detach()), gs)     # dx is the cotangent of silu(x)
    assert sx.shape == (M, K)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 256, 1000, 1024])
def test_softmax_is_autograd(S):
    s = (_rand(7, S, seed=22) * 3).requires_grad_(True)
    p = torch.softmax(s, -1)
    torch.testing.assert_close(R.softmax_fwd(s.detach()), p.detach())
    dp = _rand(14, S, seed=23)
    want = torch.cat([torch.autograd.grad(p, s, dp[z * 7:(z + 1) * 7], retain_graph=True)[0] for z in range(2)])
    torch.testing.assert_close(R.softmax_bwd(p.detach(), dp, 7, 0.25), 0.25 * want)


@pytest.mark.parametrize("D,heads,S", [(8, 3, 50), (8, 1, 1), (16, 3, 200), (32, 1, 126), (8, 3, 300)])
def test_mha_is_autograd(D, heads, S):
    C, scale = D * heads, D ** -0.5
    q, k, v = (_rand(2, S, C, seed=24 + i).requires_grad_(True) for i in range(3))
    qh, kh, vh = (t.reshape(2, S, heads, D).transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh, scale=scale).transpose(1, 2).reshape(2, S, C)
    o_ref, lse = R.mha_fwd(q.detach(), k.detach(), v.detach(), D, scale)
    torch.testing.assert_close(o_ref, o.detach())
    torch.testing.assert_close(lse, torch.logsumexp(scale * qh @ kh.transpose(-1, -2), -1).detach())
    do = _rand(4, S, C, seed=27)
    grads = [torch.autograd.grad(o, (q, k, v), do[z * 2:(z + 1) * 2], retain_graph=True) for z in range(2)]
    got = R.mha_bwd(q.detach(), k.detach(), v.detach(), o_ref, lse, do, D, scale)
    for i in range(3):
        torch.testing.assert_close(got[i], torch.cat([grads[z][i] for z in range(2)]))


@pytest.mark.parametrize("N2,H,W,C,CO", [(2, 5, 7, 24, 3), (1, 1, 1, 8, 1), (2, 8, 8, 320, 4), (2, 4, 4, 128, 2)])
def test_conv_out_is_conv2d_and_its_autograd(N2, H, W, C, CO):
    x = _rand(N2, C, H, W, seed=28).requires_grad_(True)
    w = _rand(CO, C, 3, 3, seed=29).requires_grad_(True)
    b = _rand(CO, seed=30)
    y = F.conv2d(x, w, b, padding=1)
    wn = w.detach().permute(2, 3, 0, 1).reshape(9, CO, C)
    torch.testing.assert_close(R.conv_out_fprop(_pad(x.detach()), wn, b), y.detach())
    c = _rand(N2, CO, H, W, seed=31)
    dx, dw = torch.autograd.grad(y, (x, w), c)
    torch.testing.assert_close(R.conv_out_dgrad(c, wn).permute(0, 3, 1, 2), dx)
    dW, dbias = R.conv_out_wgrad(c, _pad(x.detach()), 1, N2, N2)
    torch.testing.assert_close(dW[0], dw.permute(2, 3, 0, 1).reshape(9, CO, C))
    torch.testing.assert_close(dbias[0], c.sum((0, 2, 3)))
    if N2 == 2:                                   # two sets of one image against ONE saved image (index n2 % nx)
        dW2, db2 = R.conv_out_wgrad(c, _pad(x.detach())[:1], 2, 1, 1)
        for s in range(2):
            _, dws = torch.autograd.grad(F.conv2d(x[:1], w, b, padding=1), (x, w), c[s:s + 1])
            torch.testing.assert_close(dW2[s], dws.permute(2, 3, 0, 1).reshape(9, CO, C))
            torch.testing.assert_close(db2[s], c[s].sum((1, 2)))
    assert float((R.conv_out_dgrad(c, wn, absolute=True) - R.conv_out_dgrad(c, wn).abs()).min()) >= -1e-12


@pytest.mark.parametrize("D", [8, 16, 32])
def test_mha_small_acceptance_arithmetic(D):
    """The limits tests/test_hip_small_kernels.py expects of siss_mha_small_takes, from the kernels' LDS images (csrc/attention.hip):
    forward 8 S D bytes, backward 16 S D + 8 S bytes, 64 KiB each."""
    fwd = max(S for S in range(1, 2049) if 8 * S * D <= 65536)
    bwd = max(S for S in range(1, 2049) if 16 * S * D + 8 * S <= 65536)
    assert (fwd, bwd) == {8: (1024, 481), 16: (512, 248), 32: (256, 126)}[D]

"""Plain references of the small kernels (csrc/elementwise.hip, timeemb.hip, attention.hip, conv_small.hip and their `_f32`
forms in f32_path.hip): index arithmetic on the project's layouts, f64 for sums, int64 where a case is exact.

Layouts: padded NHWC [N][H + 2][W + 2][C] (interior pixel (y, x) at padded (y + 1, x + 1)), compact [N][H * W][C], NCHW images, and
the flat parameter buffer with woff / boff tables.  A function that stands for a launcher which writes INTO a padded tensor takes
that tensor as pre-filled by the caller and returns the whole expected tensor: what the launcher does not promise to write (the
halo, the columns it leaves alone) is the caller's fill, bit for bit.

tests/test_small_kernels_host.py checks each of these against torch's own operator on the CPU, so that a wrong reference cannot
bless a wrong kernel; tests/test_hip_small_kernels.py compares the kernels with them.
"""
import math

import torch

F64 = torch.float64


def inner(p):
    """Interior view [N][H][W][C] of a padded tensor."""
    return p[:, 1:-1, 1:-1]


def _add(dtype, *terms):
    """f32 sum of the terms IN ORDER, then one rounding to dtype (none for f32): the kernels' add8 / four-term block sum."""
    t = terms[0].float()
    for u in terms[1:]:
        t = t + u.float()
    return t.to(dtype)                       # f32 -> bf16: round to nearest even


# ---------------------------------------------------------------- data movement on padded NHWC
def upsample2x(inp, out):
    """out[n, y, x, :] = inp[n, y / 2, x / 2, :]; out is the pre-filled [N][2H + 2][2W + 2][C]."""
    H, W = inp.shape[1] - 2, inp.shape[2] - 2
    y, x = torch.arange(2 * H), torch.arange(2 * W)
    e = out.clone()
    inner(e)[:] = inp[:, (1 + y // 2)[:, None], (1 + x // 2)[None, :]]
    return e


def upsample2x_bwd(dout, din):
    """din[n, y, x, :] = the 2 x 2 block sum of dout in the order (0,0), (0,1), (1,0), (1,1), rounded once."""
    d = inner(dout)
    e = din.clone()
    inner(e)[:] = _add(din.dtype, d[:, 0::2, 0::2], d[:, 0::2, 1::2], d[:, 1::2, 0::2], d[:, 1::2, 1::2])
    return e


def concat(a, b, out):
    Ca = a.shape[-1]
    e = out.clone()
    inner(e)[..., :Ca] = inner(a)
    inner(e)[..., Ca:] = inner(b)
    return e


def concat_tail(b, out, Ca):
    e = out.clone()
    inner(e)[..., Ca:] = inner(b)
    return e


def concat_bwd(dcat, da, db, accumulate_b):
    Ca = da.shape[-1]
    ea, eb = da.clone(), db.clone()
    inner(ea)[:] = inner(dcat)[..., :Ca]
    tail = inner(dcat)[..., Ca:]
    inner(eb)[:] = _add(db.dtype, inner(db), tail) if accumulate_b else tail
    return ea, eb


def add_inplace(a, b):
    e = a.clone()
    inner(e)[:] = _add(a.dtype, inner(a), inner(b))
    return e


def space_to_depth(inp, z):
    """z[n, i, j, (py * 2 + px) * C + c] = inp[n, 2i + py, 2j + px, c]; inp may be a column view of a wider tensor."""
    C = inp.shape[-1]
    e = z.clone()
    for py in range(2):
        for px in range(2):
            pl = py * 2 + px
            inner(e)[..., pl * C:(pl + 1) * C] = inner(inp)[:, py::2, px::2]
    return e


def depth_to_space(dz, din, accumulate):
    C = din.shape[-1]
    e = din.clone()
    for py in range(2):
        for px in range(2):
            pl = py * 2 + px
            v = inner(dz)[..., pl * C:(pl + 1) * C]
            t = inner(e)[:, py::2, px::2]
            t[:] = _add(din.dtype, inner(din)[:, py::2, px::2], v) if accumulate else v
    return e


def pad_to_compact(inp):
    N, Hp, Wp, C = inp.shape
    return inner(inp).reshape(N, (Hp - 2) * (Wp - 2), C).clone()


def compact_add_to_pad(comp, res, out):
    N, Hp, Wp, C = out.shape
    c = comp.reshape(N, Hp - 2, Wp - 2, C)
    e = out.clone()
    inner(e)[:] = c if res is None else _add(out.dtype, c, inner(res))
    return e


def transpose(x):
    """[B][R][C] -> [B][C][R]"""
    B, R, C = x.shape
    e = torch.empty(B, C, R, dtype=x.dtype)
    for r in range(R):
        e[:, :, r] = x[:, r, :]
    return e


def im2col3x3(img, K, flip, dtype):
    """NCHW image -> rows [N][H + 2][W + 2][K] of dtype: k = tap * Cin + ci holds img[ci, y + dy, x + dx] (flip: y - dy, x - dx),
    tap = (dy + 1) * 3 + (dx + 1), zero outside the image, in the halo rows and at k >= 9 Cin."""
    N, Cin, H, W = img.shape
    zp = torch.zeros(N, Cin, H + 4, W + 4, dtype=img.dtype)
    zp[:, :, 2:-2, 2:-2] = img
    e = torch.zeros(N, H + 2, W + 2, K, dtype=dtype)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if flip:
            dy, dx = -dy, -dx
        for ci in range(Cin):
            inner(e)[..., tap * Cin + ci] = zp[:, ci, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W].to(dtype)
    return e


# ---------------------------------------------------------------- sums (int64 when the inputs are integers)
def colsum(y, nsets, rows_per_set):
    """y [nsets * rows_per_set][C] -> [nsets][C]"""
    acc = torch.int64 if not y.is_floating_point() else F64
    return y.to(acc).reshape(nsets, rows_per_set, -1).sum(1)


def nchw_channel_sums(img, nsets, set_images):
    """img [nsets * set_images][C][hw] -> [nsets][C]"""
    acc = torch.int64 if not img.is_floating_point() else F64
    C = img.shape[1]
    return img.to(acc).reshape(nsets, set_images, C, -1).sum((1, 3))


# ---------------------------------------------------------------- time embedding
def timestep_sincos(t, dim, flip_sin_to_cos, freq_shift, dtype=F64):
    """out[b, j] = sin(t_b f_j), out[b, half + j] = cos(t_b f_j), f_j = exp(-ln(10000) j / (half - freq_shift)); the halves swap
    under flip_sin_to_cos.  dtype = float32 evaluates the same expression in f32 (torch's own rounding: the tests' e_ref)."""
    half = dim // 2
    j = torch.arange(half, dtype=dtype)
    freq = torch.exp(-math.log(10000.0) * j / (half - freq_shift))
    arg = t.to(dtype)[:, None] * freq[None, :]
    s, c = torch.sin(arg), torch.cos(arg)
    return torch.cat([c, s], 1) if flip_sin_to_cos else torch.cat([s, c], 1)


def silu(z):
    return z * torch.sigmoid(z)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def linear_fwd(x, W, b, act_in):
    """y[m][n] = sum_k act(x[m][k]) W[n][k] + b[n]; integer tensors stay int64 (act_in = 0 only)."""
    xa = silu(x) if act_in else x
    return xa @ W.T + b


def linear_bwd(dy, yact, x, W, Mx, set_rows, act_in):
    """Row m of dy uses saved row m % Mx of x / yact.  Returns dx [M2][K], dW [nsets][N][K], db [nsets][N] (the sums the launcher
    ADDS to its targets) and the |term| sums the a-priori bounds need are left to the caller."""
    M2 = dy.shape[0]
    idx = torch.arange(M2) % Mx
    de = dy * dsilu(yact[idx]) if yact is not None else dy
    xa = silu(x[idx]) if act_in else x[idx]
    nsets = M2 // set_rows
    dx = de @ W
    dW = torch.stack([de[s * set_rows:(s + 1) * set_rows].T @ xa[s * set_rows:(s + 1) * set_rows] for s in range(nsets)])
    db = de.reshape(nsets, set_rows, -1).sum(1)
    return dx, dW, db


def multi_tables(Ntot, K, seed):
    """woff / boff / boff2 of a flat buffer: weight rows in shuffled order with gaps, biases in a second region, the shared
    conv1 biases in a third.  Returns (woff, boff, boff2, floats a set uses)."""
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(Ntot, generator=g)
    woff = 5 + order * (K + 3)
    b0 = 5 + Ntot * (K + 3) + 11
    boff = b0 + torch.randperm(Ntot, generator=g) * 2
    b1 = b0 + 2 * Ntot + 7
    boff2 = b1 + torch.randperm(Ntot, generator=g)
    return woff, boff, boff2, b1 + Ntot + 9


def multi_fwd(x, P, woff, boff, K):
    """y[m][n] = silu(x[m]) . P[woff[n] : woff[n] + K] + P[boff[n]]"""
    rows = P[woff[:, None] + torch.arange(K)[None, :]]          # [Ntot][K]
    return silu(x) @ rows.T + P[boff][None, :]


def multi_bwd(dy, x, P, G, woff, boff, boff2, Mx, set_rows, set_stride, K, sx=None):
    """The flat gradient buffer G (pre-filled; set s at s * set_stride) after the launcher's additions, and dx [M2][K] (its
    additions to a zeroed dx).  sx [Mx][K] stands in for silu(x) when given (the error bounds' |term| sums)."""
    M2, Ntot = dy.shape
    sx = (silu(x) if sx is None else sx)[torch.arange(M2) % Mx]
    rows = P[woff[:, None] + torch.arange(K)[None, :]]
    dx = dy @ rows
    e = G.clone()
    for s in range(M2 // set_rows):
        sl = slice(s * set_rows, (s + 1) * set_rows)
        g = e[s * set_stride:]
        dw = dy[sl].T @ sx[sl]                                    # [Ntot][K]
        bs = dy[sl].sum(0)
        for n in range(Ntot):                                     # one by one: two columns may share a bias slot
            w0 = int(woff[n])
            g[w0:w0 + K] += dw[n]
            g[int(boff[n])] += bs[n]
            g[int(boff2[n])] += bs[n]
    return e, dx


# ---------------------------------------------------------------- attention
def softmax_fwd(s):
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(p, dp, p_rows, scale):
    """ds[r] = scale * p[r % p_rows] * (dp[r] - <p, dp>)"""
    pr = p[torch.arange(dp.shape[0]) % p_rows]
    return scale * pr * (dp - (pr * dp).sum(-1, keepdim=True))


def _heads(x, D):
    """compact [N][S][C] -> [N][heads][S][D]"""
    N, S, C = x.shape
    return x.reshape(N, S, C // D, D).permute(0, 2, 1, 3)


def _unheads(x):
    N, Hh, S, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(N, S, Hh * D)


def mha_fwd(q, k, v, D, scale):
    """o [N][S][C] = softmax(scale q k^T) v per head; lse [N][heads][S] = natural-log logsumexp of the scaled scores."""
    qh, kh, vh = _heads(q, D), _heads(k, D), _heads(v, D)
    s = scale * (qh @ kh.transpose(-1, -2))
    return _unheads(softmax_fwd(s) @ vh), torch.logsumexp(s, -1)


def mha_bwd(q, k, v, o, lse, dout, D, scale):
    """The backward launcher's own operation: n2 cotangent samples against nx saved ones (saved index n2 % nx), probabilities
    rebuilt as exp(scale q k^T - lse), delta = <dout, o>.  Returns dq, dk, dv [n2][S][C]."""
    n2, nx = dout.shape[0], q.shape[0]
    idx = torch.arange(n2) % nx
    qh, kh, vh, oh, doh = (_heads(t, D) for t in (q[idx], k[idx], v[idx], o[idx], dout))
    p = torch.exp(scale * (qh @ kh.transpose(-1, -2)) - lse[idx][..., None])
    dp = doh @ vh.transpose(-1, -2)
    delta = (doh * oh).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    return _unheads(ds @ kh), _unheads(ds.transpose(-1, -2) @ qh), _unheads(p.transpose(-1, -2) @ doh)


# ---------------------------------------------------------------- conv_out (weights native [9][CO][C], tap = ky * 3 + kx)
def conv_out_fprop(x, w, bias):
    """x padded NHWC [B][H + 2][W + 2][C] (zero halo) -> pred NCHW [B][CO][H][W]"""
    B, Hp, Wp, C = x.shape
    H, W = Hp - 2, Wp - 2
    pred = bias.reshape(1, -1, 1, 1).repeat(B, 1, H, W)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        pred += torch.einsum("nyxc,oc->noyx", x[:, ky:ky + H, kx:kx + W], w[tap])
    return pred


def conv_out_dgrad(c, w, absolute=False):
    """c NCHW [N2][CO][H][W] -> the interior [N2][H][W][C] of dx: dx[y, x] = sum_{tap, o} c[o, y - (ky - 1), x - (kx - 1)] w[tap][o].
    absolute: the same sum over |c| |w| (the a-priori error bound's right-hand side)."""
    N2, CO, H, W = c.shape
    if absolute:
        c, w = c.abs(), w.abs()
    cp = torch.zeros(N2, CO, H + 2, W + 2, dtype=c.dtype)
    cp[:, :, 1:-1, 1:-1] = c
    dx = torch.zeros(N2, H, W, w.shape[-1], dtype=c.dtype)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        dx += torch.einsum("noyx,oc->nyxc", cp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w[tap])
    return dx


def conv_out_wgrad(c, x, nsets, set_images, nx, absolute=False):
    """c [nsets * set_images][CO][H][W], x padded NHWC saved input of nx images (index n2 % nx) -> dW [nsets][9][CO][C],
    dbias [nsets][CO]; int64 for integer inputs."""
    N2, CO, H, W = c.shape
    if absolute:
        c, x = c.abs(), x.abs()
    xs = x[torch.arange(N2) % nx]
    dW = []
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        xt = xs[:, ky:ky + H, kx:kx + W]                                        # [N2][H][W][C]
        t = c.reshape(nsets, set_images, CO, H * W).permute(0, 2, 1, 3).reshape(nsets, CO, -1)
        u = xt.reshape(nsets, set_images * H * W, -1)
        dW.append(t @ u)                                                        # [nsets][CO][C]
    return torch.stack(dW, 1), c.reshape(nsets, set_images, CO, -1).sum((1, 3))

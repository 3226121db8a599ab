"""The reference of csrc/feature_sets.hip and siss_amd/feature_sets.py: f64 squared distances, radii, the four PRDC figures, the three
kernel sums and the KID value; the a-priori bound of the f32 distance; the acceptance functions the GPU tests apply; exact integer
data; the realistic rows of the issue; and an emulation of the four launchers on host tensors (the arguments as lib.call gets them).

The bound.  The kernel's distance is d2 = max(0, fl(S - 2 t)) with t the f32 fmaf chain of the dot product, S = fl(sa + sb), and
sa, sb the squared norms summed in f64 and rounded once.  With u = 2^-24, gamma_d = d u / (1 - d u), P = sum_i |a_i b_i| and
A = |a|^2 + |b|^2:
    |t - a.b|          <= gamma_d P                    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the fused
                                                        multiply-adds round once per term, which the bound covers)
    |sa - |a|^2|       <= u |a|^2 (1 + d 2^-53)        (one rounding of an f64 sum whose own error is d 2^-53 relative)
    |S - A|            <= u A + u A (1 + u)            (the two roundings above, then the addition's)
    |fl(S - 2t) - (S - 2t)| <= u |S - 2t| <= u (A + 2 P) (1 + 2u + gamma_d)       (-2 t is exact; the fma rounds once)
so |d2_f32 - d2| <= 2 gamma_d P + 3 u A + 2 u P + O(u^2 (A + P)) <= 2 gamma_d P + 4 u (A + 2 P) =: b(a, b); the clamp at 0 moves the
value towards the true one, which is >= 0.  (The f64 reference's own error, ~1e-16 (A + P), disappears in the slack between 3 u A
+ 2 u P and 4 u (A + 2 P).)  It is derived, not measured.
"""
import numpy as np
import torch

from sscd_search_ref import BAND_SHARE, U, bits, chain_sims, exact_rows, exact_sims, gamma   # noqa: F401  (shared with the SSCD search)

MAX_K, MAX_PIECES, TARGET_WAVES, QT, GT, MAX_SUBSETS = 16, 256, 2048, 32, 64, 21845


# ---------------------------------------------------------------- f64
def f64(x):
    return np.asarray(x, np.float64)


def d2_64(q, g):
    """[nq, ng] f64 squared distances of f32 rows (the expansion in f64, clamped at 0)."""
    q, g = f64(q), f64(g)
    return np.maximum((q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2.0 * (q @ g.T), 0.0)


def bound(q, g):
    """[nq, ng]: b(a, b) of the module docstring."""
    q, g = f64(q), f64(g)
    d = q.shape[1]
    P = np.abs(q) @ np.abs(g).T
    A = (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :]
    return 2 * gamma(d) * P + 4 * U * (A + 2 * P)


def radii(d2self, k):
    """[n]: the k-th smallest entry of each row of the [n, n] matrix d2self, the diagonal left out; +inf when n - 1 < k."""
    n = d2self.shape[0]
    m = np.array(d2self, np.float64, copy=True)
    m[np.arange(n), np.arange(n)] = np.inf
    if n - 1 < k:
        return np.full(n, np.inf)
    return np.sort(m, axis=1)[:, k - 1]


def ball(d2qg, radius_g, self0=-1):
    """(inside, min_d2, argmin) of the [nq, ng] matrix: counts of d2 <= radius_g[j], the row minimum and the lowest index attaining it
    (-1: no candidate); NaN entries and the pairs (i, self0 + i) are no candidates."""
    m = np.array(d2qg, np.float64, copy=True)
    nq, ng = m.shape
    ok = ~np.isnan(m)
    if self0 >= 0:
        for i in range(nq):
            if 0 <= self0 + i < ng:
                ok[i, self0 + i] = False
    inside = None if radius_g is None else (ok & (np.where(ok, m, np.inf) <= np.asarray(radius_g, np.float64)[None, :])).sum(1).astype(np.int32)
    m = np.where(ok, m, np.inf)
    mn = m.min(axis=1)
    arg = np.where(ok.any(1), np.argmax(ok & (m == mn[:, None]), axis=1), -1).astype(np.int32)
    return inside, mn, arg


def prdc(real, fake, k, dist=d2_64):
    """{precision, recall, density, coverage} of f32 rows with squared distances and `<=` (Kynkaanniemi et al. 2019; Naeem et al. 2020)."""
    rr, ff, fr = dist(real, real), dist(fake, fake), dist(fake, real)
    r_r, r_f = radii(rr, k), radii(ff, k)
    in_f = (fr <= r_r[None, :]).sum(1)
    in_r = (fr.T <= r_f[None, :]).sum(1)
    return dict(precision=float((in_f > 0).mean()), recall=float((in_r > 0).mean()), density=float(in_f.sum() / (k * len(fake))),
                coverage=float((fr.T.min(1) <= r_r).mean()))


def kernel_sums(x, idx_x, y, idx_y, gam, coef, dots=None):
    """[S, 3] f64: per subset the sums (xx off the diagonal, yy off the diagonal, xy) of (gam * dot + coef)^3.  `dots`: a function
    (a, b) -> [na, nb] f64 dot products (default: the f64 product of the rows)."""
    dots = dots or (lambda a, b: f64(a) @ f64(b).T)
    x, y, idx_x, idx_y = np.asarray(x), np.asarray(y), np.asarray(idx_x), np.asarray(idx_y)
    out = np.zeros((idx_x.shape[0], 3))
    off = ~np.eye(idx_x.shape[1], dtype=bool)
    for b in range(idx_x.shape[0]):
        xs, ys = x[idx_x[b]], y[idx_y[b]]
        for j, (p, q, mask) in enumerate(((xs, xs, off), (ys, ys, off), (xs, ys, None))):
            kv = (gam * dots(p, q) + coef) ** 3
            out[b, j] = kv[mask].sum() if mask is not None else kv.sum()
    return out


def kid_values(sums, m):
    """[S]: (kxx + kyy) / (m (m - 1)) - 2 kxy / m^2."""
    sums = f64(sums)
    return (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


def kid(sums, m):
    """(mean, population std) of the per-subset values."""
    v = kid_values(sums, m)
    return float(v.mean()), float(v.std())


def kernel_sum_bounds(x, idx_x, y, idx_y, gam, coef):
    """[S, 3]: per sum the a-priori distance of the kernel's value from kernel_sums: with e = gam * b_dot the error of the cubic's
    argument (b_dot = gamma_d sum|a_i b_i|, the bound of sscd_search_ref) and v = gam |s| + coef, |(v')^3 - v^3| <= 3 (v + e)^2 e per
    pair, plus the summation term N 2^-53 sum|k| over the N summed terms (each cube's own f64 roundings, 4 of them, are counted with
    it: (N + 4) 2^-53)."""
    x, y, idx_x, idx_y = np.asarray(x), np.asarray(y), np.asarray(idx_x), np.asarray(idx_y)
    g = gamma(x.shape[1])
    out = np.zeros((idx_x.shape[0], 3))
    off = ~np.eye(idx_x.shape[1], dtype=bool)
    for b in range(idx_x.shape[0]):
        xs, ys = f64(x[idx_x[b]]), f64(y[idx_y[b]])
        for j, (p, q, mask) in enumerate(((xs, xs, off), (ys, ys, off), (xs, ys, None))):
            s = p @ q.T
            e = gam * g * (np.abs(p) @ np.abs(q).T)
            v = gam * np.abs(s) + coef
            per = 3 * (v + e) ** 2 * e
            kabs = np.abs((gam * s + coef) ** 3) + per
            if mask is not None:
                per, kabs = per[mask], kabs[mask]
            out[b, j] = per.sum() + (per.size + 4) * 2.0 ** -53 * kabs.sum()
    return out


# ---------------------------------------------------------------- acceptance
def accept_radius(rad, d2self, bself, k):
    """AssertionError unless each radius is within its row's largest pair bound of the f64 radius (an order statistic moves by at
    most the largest perturbation of its row).  Returns (r64, B)."""
    n = d2self.shape[0]
    r64 = radii(d2self, k)
    b = np.array(bself, copy=True)
    b[np.arange(n), np.arange(n)] = 0.0
    B = b.max(axis=1)
    err = np.abs(f64(rad) - r64)
    assert (err <= B).all(), f"radius off by {err.max():.3e} at row {err.argmax()}, bound {B[err.argmax()]:.3e}"
    return r64, B


def accept_ball(inside, min_d2, argmin, d2qg, bqg, r64_g, B_g):
    """AssertionError unless, with b_ij the pair bound and B_j the radius bound: inside[i] lies between the count of pairs with
    d64 <= r64_j - (b_ij + B_j) and the count of pairs with d64 <= r64_j + (b_ij + B_j); the undecided band holds at most BAND_SHARE of
    all pairs; min_d2 is within the row's largest bound of the f64 minimum; argmin's f64 distance is within twice that of it.
    Returns (sure [nq, ng], maybe [nq, ng], band share)."""
    slack = bqg + np.asarray(B_g)[None, :]
    sure = d2qg <= np.asarray(r64_g)[None, :] - slack
    maybe = d2qg <= np.asarray(r64_g)[None, :] + slack
    band = float((maybe & ~sure).sum()) / sure.size
    assert band <= BAND_SHARE, f"the undecided band holds {band:.4%} of the pairs"
    inside = np.asarray(inside)
    lo, hi = sure.sum(1), maybe.sum(1)
    assert ((lo <= inside) & (inside <= hi)).all(), f"inside outside its interval at rows {np.flatnonzero((inside < lo) | (inside > hi))[:5].tolist()}"
    Bmax = bqg.max(axis=1)
    m64 = d2qg.min(axis=1)
    err = np.abs(f64(min_d2) - m64)
    assert (err <= Bmax).all(), f"min_d2 off by {err.max():.3e}, bound {Bmax[err.argmax()]:.3e}"
    argmin = np.asarray(argmin)
    assert ((argmin >= 0) & (argmin < d2qg.shape[1])).all()
    assert (d2qg[np.arange(len(argmin)), argmin] <= m64 + 2 * Bmax).all(), "argmin names a row that is not a nearest one"
    return sure, maybe, band


def prdc_intervals(real, fake, k):
    """{figure: (lo, hi)}: what the a-priori bounds leave of each PRDC figure.  Every figure is monotone in its decisions
    `d2 <= radius`; a decision is SURE when it holds in f64 with the pair's and the radius' bounds against it and POSSIBLE when it
    holds with both in its favour, so the figure of any arithmetic within the bounds lies between the two evaluations."""
    rr, ff, fr = d2_64(real, real), d2_64(fake, fake), d2_64(fake, real)
    brr, bff, bfr = bound(real, real), bound(fake, fake), bound(fake, real)
    np.fill_diagonal(brr, 0.0), np.fill_diagonal(bff, 0.0)
    r_r, B_r, r_f, B_f = radii(rr, k), brr.max(1), radii(ff, k), bff.max(1)
    out = {}
    slack = bfr + B_r[None, :]
    sure, maybe = fr <= r_r[None, :] - slack, fr <= r_r[None, :] + slack
    out["precision"] = (sure.any(1).mean(), maybe.any(1).mean())
    out["density"] = (sure.sum() / (k * len(fake)), maybe.sum() / (k * len(fake)))
    slack = bfr.T + B_f[None, :]
    out["recall"] = ((fr.T <= r_f[None, :] - slack).any(1).mean(), (fr.T <= r_f[None, :] + slack).any(1).mean())
    m64, slack = fr.T.min(1), bfr.T.max(1) + B_r
    out["coverage"] = ((m64 <= r_r - slack).mean(), (m64 <= r_r + slack).mean())
    return out


def assert_in(figures, intervals, eps=1e-12):
    for name, (lo, hi) in intervals.items():
        assert lo - eps <= figures[name] <= hi + eps, f"{name} = {figures[name]!r} outside [{lo!r}, {hi!r}]"


# ---------------------------------------------------------------- data
def exact_d2(q, g):
    """The exact squared distances of exact_rows data (every norm, dot product and their combination is an integer times 2^-10 below
    2^24: exact in f32 in any order, and equal to this f64 value)."""
    q, g = f64(q) * 32, f64(g) * 32
    return ((q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2 * (q @ g.T)) * 2.0 ** -10


def realistic(n_real=1537, n_fake=515, d=2048, seed=0):
    """(real [1537, 2048], fake [515, 2048]) f32: ReLU features on an 8-dimensional latent, the fake latent shifted by 0.3:
    W = N(0, 1) [8, d]; rows max(0, z W / sqrt(8) + 0.05 N(0, 1)), z ~ N(0, I_8) for the real and N(0.3, I_8) for the fake rows; drawn
    from default_rng(seed) in the order W, z_real, noise_real, z_fake, noise_fake."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((8, d))
    zr = rng.standard_normal((n_real, 8))
    er = rng.standard_normal((n_real, d))
    zf = rng.standard_normal((n_fake, 8)) + 0.3
    ef = rng.standard_normal((n_fake, d))
    real = np.maximum(0.0, zr @ W / np.sqrt(8) + 0.05 * er)
    fake = np.maximum(0.0, zf @ W / np.sqrt(8) + 0.05 * ef)
    return real.astype(np.float32), fake.astype(np.float32)


# ---------------------------------------------------------------- the launchers, emulated
def pieces_for(nq, ng, per_row=1):
    """split_for of csrc/feature_sets.hip: the number of pieces the second set is cut into."""
    ntiles, nqt = -(-ng // GT), -(-nq // QT) * per_row
    want = max(1, min(-(-TARGET_WAVES // nqt), MAX_PIECES, ntiles))
    tpp = -(-ntiles // want)
    return -(-ntiles // tpp)


def _r16(n):
    return -(-n // 16) * 16


def ws_bytes(name, *a):
    if name == "siss_feat_knn_ws_bytes":
        n, k = a
        return -1 if n < 1 or not 1 <= k <= MAX_K else _r16(n * pieces_for(n, n) * k * 4)
    if name == "siss_feat_ball_ws_bytes":
        nq, ng = a
        return -1 if nq < 1 or ng < 1 else _r16(nq * pieces_for(nq, ng) * 12)
    if name == "siss_kid_ws_bytes":
        S, s = a
        return -1 if not 1 <= S <= MAX_SUBSETS or s < 1 else _r16(3 * S * -(-s // QT) * pieces_for(s, s, 3 * S) * 8)
    raise KeyError(name)


def sq32(x):
    """siss_feat_sqnorm: the f64 sum of squares over ascending k, rounded once."""
    x = f64(x)
    s = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        s = s + x[:, k] * x[:, k]
    return s.astype(np.float32)


def d2_32(dot, sa, sb):
    """The kernel's distance from f32 dots and squared norms (the fma's single rounding taken as the rounding of the f64 value of
    S - 2 t: differs on a double-rounding near-tie only), and the mask of the NaN pairs."""
    S = (np.asarray(sa, np.float32)[:, None] + np.asarray(sb, np.float32)[None, :]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (S.astype(np.float64) - 2.0 * np.asarray(dot, np.float64)).astype(np.float32)
    return np.where(t > 0, t, np.float32(0)).astype(np.float32), np.isnan(t)


def _ok(x, n, d):
    return (x is not None and torch.is_tensor(x) and x.dtype == torch.float32 and tuple(x.shape) == (n, d) and x.is_contiguous()
            and n >= 1 and 4 <= d <= 4096 and d % 4 == 0)


def call(name, *a):
    """Emulate `name` on host tensors and return 0 (1: the launcher's refusal); None for a launcher that is not csrc/feature_sets.hip's."""
    if name == "siss_feat_sqnorm":
        x, n, d, sq = a
        if not _ok(x, n, d) or sq is None:
            return 1
        sq.copy_(torch.from_numpy(sq32(x.numpy())))
    elif name == "siss_feat_knn_radius":
        x, n, d, sq, k, radius, ws, nbytes = a
        if not _ok(x, n, d) or sq is None or radius is None or ws is None or not 1 <= k <= MAX_K or nbytes < ws_bytes("siss_feat_knn_ws_bytes", n, k):
            return 1
        v, nan = d2_32(chain_sims(x.numpy(), x.numpy()), sq.numpy(), sq.numpy())
        m = np.where(nan, np.inf, v.astype(np.float64))
        radius.copy_(torch.from_numpy(radii(m, k).astype(np.float32)))
    elif name == "siss_feat_ball_stats":
        q, nq, sq_q, g, ng, sq_g, rad, d, self0, inside, min_d2, argmin, ws, nbytes = a
        if (not _ok(q, nq, d) or not _ok(g, ng, d) or sq_q is None or sq_g is None or min_d2 is None or argmin is None or ws is None
                or (rad is not None and inside is None) or nbytes < ws_bytes("siss_feat_ball_ws_bytes", nq, ng)):
            return 1
        v, nan = d2_32(chain_sims(q.numpy(), g.numpy()), sq_q.numpy(), sq_g.numpy())
        m = np.where(nan, np.nan, v.astype(np.float64))
        ins, mn, arg = ball(m, None if rad is None else rad.numpy(), self0)
        if rad is not None:
            assert inside.dtype == torch.int32
            inside.copy_(torch.from_numpy(ins))
        assert argmin.dtype == torch.int32 and min_d2.dtype == torch.float32
        min_d2.copy_(torch.from_numpy(mn.astype(np.float32))); argmin.copy_(torch.from_numpy(arg))
    elif name == "siss_kid_sums":
        x, nx, ix, y, ny, iy, d, S, s, gam, coef, out, ws, nbytes = a
        if (not _ok(x, nx, d) or not _ok(y, ny, d) or ix is None or iy is None or out is None or ws is None or not 1 <= S <= MAX_SUBSETS or s < 1
                or nbytes < ws_bytes("siss_kid_ws_bytes", S, s)):
            return 1
        assert ix.dtype == torch.int32 and iy.dtype == torch.int32 and tuple(ix.shape) == (S, s) and tuple(iy.shape) == (S, s)
        assert out.dtype == torch.float64 and tuple(out.shape) == (S, 3)
        out.copy_(torch.from_numpy(kernel_sums(x.numpy(), ix.numpy(), y.numpy(), iy.numpy(), gam, coef,
                                               dots=lambda p, q: chain_sims(p, q).astype(np.float64))))
    else:
        return None
    return 0

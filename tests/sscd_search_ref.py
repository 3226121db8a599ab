"""The reference of csrc/sscd_search.hip: f64 similarities, the a-priori bound of an f32 dot product, the two acceptance functions the
GPU tests apply to the launchers' results, exact integer data, and an emulation of the three launchers on host tensors (the arguments as
lib.call gets them) for the host tests of siss_amd/sscd_search.py.

The bound.  An f32 dot product of d terms summed in ANY order differs from the exact one by at most
    b(q, g) = gamma_d * sum_i |q_i g_i| <= gamma_d * ||q|| ||g||,   gamma_d = d u / (1 - d u),  u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the fused multiply-adds of the kernel round once per term, which the bound
covers).  For unit rows at d = 512 this is 3.05e-5.  It is derived, not measured.
"""
import numpy as np
import torch

U = 2.0 ** -24
NQ, NG, D = 33, 20011, 512                     # the Gaussian case of the issue
PLANTED = ((0, 7, 0.9), (16, 1026, 0.7), (32, 20010, 0.55))      # (query, gallery row, cosine)
BAND_SHARE = 1e-3                              # the undecided band of a threshold may hold at most this share of all pairs


def gamma(d):
    return d * U / (1 - d * U)


def sims64(q, g):
    """[nq, ng] f64 dot products of f32 rows."""
    return np.asarray(q, np.float64) @ np.asarray(g, np.float64).T


def bound(q, g):
    """[nq, ng]: gamma_d * sum_i |q_i g_i| in f64."""
    return gamma(np.shape(q)[1]) * (np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(g, np.float64)).T)


def candidates(s64, self0=-1):
    """[nq, ng] bool: the pairs a search may return -- not the excluded self pair, not a NaN similarity."""
    ok = ~np.isnan(s64)
    if self0 >= 0:
        for i in range(s64.shape[0]):
            if 0 <= self0 + i < s64.shape[1]:
                ok[i, self0 + i] = False
    return ok


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------- acceptance
def accept_topk(val, idx, s64, b, k, self0=-1):
    """AssertionError unless (val, idx) [nq, k] is an acceptable top-k of the f64 similarities s64 under the bound b [nq, ng]:
    nothing skipped (min(k, candidates) entries, then (-inf, -1)); every value within b of the f64 similarity of its index; every index
    with f64 similarity >= (k-th largest f64 value) - 2 b; values non-increasing; indices ascending among bitwise-equal values; no
    repeated index; no excluded or NaN pair."""
    val, idx = np.asarray(val, np.float32), np.asarray(idx)
    nq, ng = s64.shape
    assert val.shape == (nq, k) and idx.shape == (nq, k), (val.shape, idx.shape, (nq, k))
    ok = candidates(s64, self0)
    for i in range(nq):
        cand = np.flatnonzero(ok[i])
        m = min(k, len(cand))
        assert (idx[i, :m] >= 0).all() and (idx[i, :m] < ng).all(), f"query {i}: {m} entries are due, got indices {idx[i].tolist()}"
        assert (idx[i, m:] == -1).all() and np.isneginf(val[i, m:]).all(), f"query {i}: slots beyond {m} are not (-inf, -1)"
        if m == 0:
            continue
        ii, vv = idx[i, :m], val[i, :m]
        assert len(set(ii.tolist())) == m, f"query {i}: an index repeats in {ii.tolist()}"
        assert ok[i, ii].all(), f"query {i}: an excluded or NaN pair was returned: {ii[~ok[i, ii]].tolist()}"
        err = np.abs(vv.astype(np.float64) - s64[i, ii])
        assert (err <= b[i, ii]).all(), f"query {i}: value off by {err.max():.3e}, bound {b[i, ii][err.argmax()]:.3e}"
        kth = np.sort(s64[i, cand])[-m]
        slack = 2 * b[i, cand].max()
        assert (s64[i, ii] >= kth - slack).all(), (f"query {i}: index {ii[(s64[i, ii] < kth - slack)].tolist()} is not among the {m} "
                                                   f"largest (k-th f64 value {kth!r}, 2b = {slack:.3e})")
        assert (vv[:-1] >= vv[1:]).all(), f"query {i}: values are not non-increasing: {vv.tolist()}"
        tie = bits(vv[:-1]) == bits(vv[1:])
        assert (ii[:-1][tie] < ii[1:][tie]).all(), f"query {i}: equal values whose indices do not ascend: {ii.tolist()}"


def accept_above(counts, offsets, idx, val, s64, b, thr, self0=-1):
    """AssertionError unless the CSR (offsets, idx, val) with its counts is an acceptable answer to `similarity >= thr`: every
    candidate pair with s64 >= thr + b listed, none with s64 < thr - b, the band in between (either way) at most BAND_SHARE of all
    pairs; counts the list lengths; indices ascending; values within b.  Returns the band's share."""
    counts, offsets, idx, val = np.asarray(counts), np.asarray(offsets), np.asarray(idx), np.asarray(val, np.float32)
    nq, ng = s64.shape
    ok = candidates(s64, self0)
    assert offsets.shape == (nq + 1,) and offsets[0] == 0 and (np.diff(offsets) == counts).all(), "counts are not the list lengths"
    assert len(idx) >= offsets[-1] and len(val) >= offsets[-1]
    sure = ok & (np.nan_to_num(s64, nan=-np.inf) >= thr + b)
    never = ~ok | (np.nan_to_num(s64, nan=-np.inf) < thr - b)
    band = 1.0 - (sure.sum() + never.sum()) / float(nq * ng)
    assert band <= BAND_SHARE, f"the undecided band holds {band:.4%} of the pairs"
    for i in range(nq):
        ii, vv = idx[offsets[i]:offsets[i + 1]], val[offsets[i]:offsets[i + 1]]
        assert ((ii >= 0) & (ii < ng)).all() and (np.diff(ii) > 0).all(), f"query {i}: the list does not ascend in index"
        listed = np.zeros(ng, bool)
        listed[ii] = True
        assert not (sure[i] & ~listed).any(), f"query {i}: rows {np.flatnonzero(sure[i] & ~listed)[:5].tolist()} are above thr + b, not listed"
        assert not (never[i] & listed).any(), f"query {i}: rows {np.flatnonzero(never[i] & listed)[:5].tolist()} are listed, below thr - b"
        err = np.abs(vv.astype(np.float64) - s64[i, ii])
        assert (err <= b[i, ii]).all(), f"query {i}: a listed value is off by {err.max():.3e}"
    return band


# ---------------------------------------------------------------- data
def exact_rows(n, d, seed):
    """[n, d] f32 rows with entries in {-1, 0, 1} * 2^-5: every partial sum of a dot product is an integer times 2^-10 below 2^24,
    exact in f32 in any order."""
    r = np.random.default_rng(seed)
    return (r.integers(-1, 2, size=(n, d)) * 2.0 ** -5).astype(np.float32)


def exact_sims(q, g):
    """The exact similarities of exact_rows data: integer arithmetic carried in f64 (every product is +-1 or 0, every partial sum an
    integer below 2^53, so the f64 product of the rows scaled to integers is exact in any order)."""
    return ((np.asarray(q, np.float64) * 32) @ (np.asarray(g, np.float64) * 32).T) * 2.0 ** -10


def exact_topk(s, k, self0=-1):
    """(val f32, idx int32) [nq, k]: THE top-k of exact similarities s (value descending, index ascending), (-inf, -1) beyond."""
    nq, ng = s.shape
    ok = candidates(s, self0)
    val, idx = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int32)
    for i in range(nq):
        cand = np.flatnonzero(ok[i])
        order = cand[np.lexsort((cand, -s[i, cand]))][:k]
        val[i, :len(order)], idx[i, :len(order)] = s[i, order], order
    return val, idx


def exact_above(s, thr, self0=-1):
    """(counts int32, offsets int64, idx int32, val f32): THE lists of similarity >= thr for exact similarities."""
    ok = candidates(s, self0) & (np.nan_to_num(s, nan=-np.inf) >= np.float32(thr))
    counts = ok.sum(1).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    rows, cols = np.nonzero(ok)
    return counts, offsets, cols.astype(np.int32), s[rows, cols].astype(np.float32)


def gaussian_case():
    """(q [33, 512], g [20011, 512]) f32 unit rows of numpy.random.default_rng(0), with the neighbours of PLANTED: gallery row j is
    c * q_i + sqrt(1 - c^2) * (a unit vector orthogonal to q_i), in f64, rounded to f32."""
    r = np.random.default_rng(0)
    q = r.standard_normal((NQ, D))
    g = r.standard_normal((NG, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    for i, j, c in PLANTED:
        w = g[j] - (g[j] @ q[i]) * q[i]
        g[j] = c * q[i] + np.sqrt(1 - c * c) * w / np.linalg.norm(w)
    return q.astype(np.float32), g.astype(np.float32)


# ---------------------------------------------------------------- the launchers, emulated
MAX_K, MAX_PIECES, TARGET_WAVES, QT, GT = 32, 256, 2048, 32, 64


def pieces_for(nq, ng):
    """split_for of csrc/sscd_search.hip: the number of pieces the gallery is cut into."""
    ntiles, nqt = -(-ng // GT), -(-nq // QT)
    want = max(1, min(-(-TARGET_WAVES // nqt), MAX_PIECES, ntiles))
    tpp = -(-ntiles // want)
    return -(-ntiles // tpp)


def ws_bytes(nq, ng, k):
    if nq < 1 or ng < 1 or ng > 2 ** 31 - 1 or not 0 <= k <= MAX_K:
        return -1
    p = pieces_for(nq, ng)
    return -(-(nq * p * 12) // 16) * 16 if k == 0 else nq * p * k * 8


def chain_sims(q, g):
    """[nq, ng] f32: the fmaf chain over ascending k from +0 (each step: the exact product and the sum in f64, rounded to f32 -- a
    double rounding that differs from one fused rounding only on a 2^-29 near-tie, good enough for host tests); NaN stays NaN."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    s = np.zeros((q.shape[0], g.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(q.shape[1]):
            s = (s.astype(np.float64) + np.outer(q[:, k].astype(np.float64), g[:, k].astype(np.float64))).astype(np.float32)
    return s + np.float32(0)


def _rows_ok(q, nq, g, ng, d):
    return (q is not None and g is not None and nq >= 1 and 1 <= ng <= 2 ** 31 - 1 and 4 <= d <= 4096 and d % 4 == 0
            and tuple(q.shape) == (nq, d) and tuple(g.shape) == (ng, d) and q.dtype == torch.float32 and g.dtype == torch.float32
            and q.is_contiguous() and g.is_contiguous())


def call(name, *a):
    """Emulate `name` on host tensors and return 0 (1: the launcher's refusal); None for a launcher that is not csrc/sscd_search.hip's."""
    if name == "siss_sscd_topk":
        q, nq, g, ng, d, k, self0, val, idx, ws, nbytes = a
        if not (_rows_ok(q, nq, g, ng, d) and 1 <= k <= MAX_K and ws is not None and nbytes >= ws_bytes(nq, ng, k)):
            return 1
        assert tuple(val.shape) == (nq, k) and tuple(idx.shape) == (nq, k) and idx.dtype == torch.int32 and val.dtype == torch.float32
        s = chain_sims(q.numpy(), g.numpy()).astype(np.float64)
        v, i = exact_topk(s, k, self0)
        val.copy_(torch.from_numpy(v)); idx.copy_(torch.from_numpy(i))
    elif name in ("siss_sscd_count_above", "siss_sscd_fill_above"):
        q, nq, g, ng, d, thr, self0 = a[:7]
        ws, nbytes = a[-2:]
        if not (_rows_ok(q, nq, g, ng, d) and ws is not None and nbytes >= ws_bytes(nq, ng, 0)):
            return 1
        s = chain_sims(q.numpy(), g.numpy()).astype(np.float64)
        counts, offsets, cols, vals = exact_above(s, thr, self0)
        if name == "siss_sscd_count_above":
            assert tuple(a[7].shape) == (nq,) and a[7].dtype == torch.int32
            a[7].copy_(torch.from_numpy(counts))
        else:
            off, idx, val = a[7:10]
            assert tuple(off.shape) == (nq + 1,) and off.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float32
            assert off.numpy().tolist() == offsets.tolist(), "offsets are not the exclusive scan of the counts"
            idx[:len(cols)] = torch.from_numpy(cols); val[:len(cols)] = torch.from_numpy(vals)
    else:
        return None
    return 0

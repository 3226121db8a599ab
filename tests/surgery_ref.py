"""Plain restatements of gradient surgery (siss_amd/surgery.py, csrc/surgery.hip) for tests/test_surgery_host.py and
tests/test_hip_surgery.py.  numpy on the CPU, no GPU.

ONE definition, twice:

* The f64 DEFINITION (sums_f64, project_f64, scalars_f64, step_f64).  A group is a stretch [off[g], off[g + 1]) of the flat pair (x, a).
  Per group the exact sums xx, aa, xa; the group conflicts when xa > 0 (strictly; xx = 0 or aa = 0 never does); mode forget:
  a' = a - phi (xa / xx) x; mode keep: x' = x - phi (xa / aa) a; mode mutual: both, each from the ORIGINAL pair.  s = knob / |a'| over
  the whole buffer (0 where it would be inf under the inf guard), g = clip (x' - s a'), then optimizer_ref.adamw_f64's update.

* The RESTATEMENT of the kernels' own order (job_rows, group_sums, scalars_coef, update_f32), bit for bit:
    jobs    each group is cut into jobs of C floats from its start, the last one shorter (plan).
    a row   thread t of 256 owns granules t, t + 256, ... of the job: per granule the f32 sum ((t0 + t1) + t2) + t3 of four f32
            products, added to the thread's f64 sum in ascending granule order; then element 4 * granules + t of the scalar tail (f64
            product); the xor butterfly over the 64 lanes of a wave (32, 16, 8, 4, 2, 1); the four waves added in ascending order from 0.
    a group lane l of one wave adds rows first + l, first + l + 64, ... in ascending order from 0; the butterfly.
    global  thread t of one block adds the per-group terms of groups t, t + 256, ... in ascending order from 0; the butterfly; the four
            waves in ascending order from 0.
  The scalar block's f64 expressions are written here as the kernel writes them, operation for operation; every f64 value is rounded
  to f32 once.  Pass 2: g = ((cx x) - (ca a)) clip, each operation rounded to f32 on its own, then optimizer_ref.adamw_f32's update.
"""
import math

import numpy as np

import optimizer_ref as O

f32, f64 = np.float32, np.float64
U = O.U
THREADS = 256
MODES = ("forget", "keep", "mutual")
SLOT_CONFLICTS, SLOT_COS, SLOT_REMOVED_A, SLOT_REMOVED_X = 12, 13, 14, 15
WRITTEN = list(O.NAMES.values()) + [12, 13, 14, 15]                 # slots 7, 10, 11 are nobody's
_LANE = np.arange(64)


# ================================================================ the f64 definition
def sums_f64(x, a, off):
    """[T, 3] exact sums (math.fsum over f64 products of the f32 values) per group"""
    x, a = np.asarray(x, f64), np.asarray(a, f64)
    return np.array([[math.fsum(x[lo:hi] * x[lo:hi]), math.fsum(a[lo:hi] * a[lo:hi]), math.fsum(x[lo:hi] * a[lo:hi])]
                     for lo, hi in zip(off, off[1:])], f64).reshape(-1, 3)


def conflicts(S):
    return [bool(xa > 0 and xx > 0 and aa > 0) for xx, aa, xa in S]


def project_f64(x, a, off, mode):
    """(x', a', sums [T, 3], phi [T]) of the definition, in f64"""
    x, a = np.asarray(x, f64), np.asarray(a, f64)
    S = sums_f64(x, a, off)
    phi = conflicts(S)
    x2, a2 = x.copy(), a.copy()
    for g, (lo, hi) in enumerate(zip(off, off[1:])):
        xx, aa, xa = S[g]
        if not phi[g]:
            continue
        if mode in ("forget", "mutual"):
            a2[lo:hi] = a[lo:hi] - (xa / xx) * x[lo:hi]
        if mode in ("keep", "mutual"):
            x2[lo:hi] = x[lo:hi] - (xa / aa) * a[lo:hi]
    return x2, a2, S, phi


def scalars_f64(S, mode, nmode, knob, max_norm, beta1, beta2, step):
    """The scalar fields of the definition from the group sums S [T, 3] (any f64 sums): dict with norm_x, norm_a, dot, scale,
    pre_clip_norm, clip_coef, step, bc1, bc2_sqrt, conflicts, cos, removed_a, removed_x, and the f64 coefficients cx, ca [T]."""
    S = np.asarray(S, f64).reshape(-1, 3)
    phi = conflicts(S)
    pa, px = mode in ("forget", "mutual"), mode in ("keep", "mutual")
    XX, AA, XA = (math.fsum(S[:, i]) for i in range(3))
    na2 = max(math.fsum(aa - xa * xa / xx if (f and pa) else aa for (xx, aa, xa), f in zip(S, phi)), 0.0)
    nx2 = max(math.fsum(xx - xa * xa / aa if (f and px) else xx for (xx, aa, xa), f in zip(S, phi)), 0.0)
    s = float(f32(knob)) / math.sqrt(na2) if na2 > 0 else math.inf
    if nmode == 2 and math.isinf(s):
        s = 0.0
    ca = np.array([s + xa / aa if (f and px) else s for (xx, aa, xa), f in zip(S, phi)], f64)
    cx = np.array([1.0 + s * xa / xx if (f and pa) else 1.0 for (xx, aa, xa), f in zip(S, phi)], f64)
    g2 = max(math.fsum(cx * cx * S[:, 0] - 2 * cx * ca * S[:, 2] + ca * ca * S[:, 1]), 0.0)
    gn = math.sqrt(g2)
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    nx, na = math.sqrt(XX), math.sqrt(AA)
    return dict(norm_x=nx, norm_a=na, dot=XA, scale=s, pre_clip_norm=gn, clip_coef=min(float(f32(max_norm)) / (gn + 1e-6), 1.0),
                step=float(step), bc1=1.0 - b1 ** step, bc2_sqrt=math.sqrt(1.0 - b2 ** step), conflicts=sum(phi),
                cos=XA / (nx * na) if nx > 0 and na > 0 else 0.0, removed_a=1.0 - na2 / AA if AA > 0 else 0.0,
                removed_x=1.0 - nx2 / XX if XX > 0 else 0.0, cx=cx, ca=ca, norm_a_projected=math.sqrt(na2))


def per_element(c, off):
    return np.repeat(np.asarray(c), np.diff(np.asarray(off)))


def step_f64(gx, ga, p, m, v, step, hp, off, mode, nmode, knob, max_norm):
    """One whole update of the definition in f64: ((p, m, v, g), scalars).  mode None: the plain step (optimizer_ref.step_f64)."""
    if mode is None:
        return O.step_f64(gx, ga, p, m, v, step, hp, nmode, knob, max_norm)
    x2, a2, S, _ = project_f64(gx, ga, off, mode)
    sc = scalars_f64(S, mode, nmode, knob, max_norm, hp[1], hp[2], step)
    plain = dict(sc, scale=1.0)                                # (adamw_f64 forms (x' - 1 * (s a')) * clip)
    return O.adamw_f64(x2, sc["scale"] * a2, p, m, v, plain, hp), sc


# ================================================================ the plan
def plan(off, C):
    """(starts, groups, first) as siss_amd.surgery.job_plan builds them -- restated, not imported"""
    starts, groups, first = [], [], [0]
    for g in range(len(off) - 1):
        st = off[g]
        while st < off[g + 1]:
            starts.append(st); groups.append(g)
            st += C
        first.append(len(starts))
    return starts, groups, first


def job_extents(off, C):
    """[(start, length, group)] of every job"""
    starts, groups, _ = plan(off, C)
    return [(st, min(C, off[g + 1] - st), g) for st, g in zip(starts, groups)]


# ================================================================ the kernels' order
def butterfly(v):
    """wave_sum_d over the last axis (64 lanes): v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1; every lane ends with the same value"""
    v = np.asarray(v, f64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v


def block_fold(t):
    """256 thread sums -> one value: the butterfly per wave, then the four waves in ascending order from 0"""
    w = butterfly(np.asarray(t, f64).reshape(4, 64))[:, 0]
    out = f64(0)
    for i in range(4):
        out = out + w[i]
    return out


def strided_sums(terms, lanes):
    """lane l adds terms l, l + lanes, ... in ascending order from 0 (a missing term adds +0: exact)"""
    terms = np.asarray(terms, f64)
    k = -(-len(terms) // lanes) if len(terms) else 0
    pad = np.zeros(k * lanes, f64)
    pad[:len(terms)] = terms
    acc = np.zeros(lanes, f64)
    for row in pad.reshape(k, lanes):
        acc = acc + row
    return acc


def job_row(x, a):
    """The three sums of one job's stretch (f32 arrays) in the gram kernel's order"""
    x, a = np.asarray(x, f32), np.asarray(a, f32)
    nv = x.size // 4 * 4
    out = []
    for l, r in ((x, x), (a, a), (x, a)):
        t = (l[:nv] * r[:nv]).reshape(-1, 4)
        grp = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
        assert grp.dtype == f32
        acc = strided_sums(grp.astype(f64), THREADS)
        tail = l[nv:].astype(f64) * r[nv:].astype(f64)
        acc[:len(tail)] = acc[:len(tail)] + tail
        out.append(block_fold(acc))
    return out


def job_rows(gx, ga, off, C):
    gx, ga = np.asarray(gx, f32), np.asarray(ga, f32)
    with np.errstate(all="ignore"):
        return np.array([job_row(gx[st:st + ln], ga[st:st + ln]) for st, ln, _ in job_extents(off, C)], f64).reshape(-1, 3)


def group_sums(rows, first):
    """[T, 3]: one wave per group"""
    out = np.zeros((len(first) - 1, 3), f64)
    with np.errstate(all="ignore"):
        for g in range(len(first) - 1):
            for c in range(3):
                out[g, c] = butterfly(strided_sums(rows[first[g]:first[g + 1], c], 64))[0]
    return out


def block_sum(terms):
    return block_fold(strided_sums(terms, THREADS))


def scalars_coef(S, mode, nmode, knob, max_norm, beta1, beta2, step_before):
    """(block [16] f32 with the written slots filled and zeros elsewhere, coef [T, 2] f32) from the group sums S [T, 3], as
    scalars_coef_kernel forms them: numpy f64 scalars and arrays, the kernel's expressions operation for operation."""
    S = np.asarray(S, f64).reshape(-1, 3)
    gxx, gaa, gxa = S[:, 0], S[:, 1], S[:, 2]
    pa, px = mode != "keep", mode != "forget"
    with np.errstate(all="ignore"):
        phi = (gxa > 0) & (gxx > 0) & (gaa > 0)
        xx, aa, xa = block_sum(gxx), block_sum(gaa), block_sum(gxa)
        na2 = block_sum(np.where(phi & pa, gaa - gxa * gxa / gxx, gaa))
        nx2 = block_sum(np.where(phi & px, gxx - gxa * gxa / gaa, gxx))
        cnt = block_sum(phi.astype(f64))
        na2, nx2 = (f64(0) if na2 < 0 else na2), (f64(0) if nx2 < 0 else nx2)
        s = f64(f32(knob)) / np.sqrt(na2)
        if nmode == 2 and np.isinf(s):
            s = f64(0)
        ca = np.where(phi & px, s + gxa / gaa, s)
        cx = np.where(phi & pa, 1.0 + s * gxa / gxx, 1.0)
        g2 = block_sum(cx * cx * gxx - 2 * cx * ca * gxa + ca * ca * gaa)
        if g2 < 0:
            g2 = f64(0)
        gn, nx, na = np.sqrt(g2), np.sqrt(xx), np.sqrt(aa)
        clip = f64(f32(max_norm)) / (gn + 1e-6)
        if clip > 1:
            clip = f64(1)
        step = f32(step_before) + f32(1)
        b1, b2 = float(f32(beta1)), float(f32(beta2))
        blk = np.zeros(16, f32)
        blk[:7] = [f32(nx), f32(na), f32(xa), f32(s), f32(gn), f32(clip), step]
        blk[8], blk[9] = f32(1.0 - b1 ** float(step)), f32(math.sqrt(1.0 - b2 ** float(step)))
        blk[12] = f32(cnt)
        blk[13] = f32(xa / (nx * na)) if (nx > 0 and na > 0) else f32(0)
        blk[14] = f32(1.0 - na2 / aa) if aa > 0 else f32(0)
        blk[15] = f32(1.0 - nx2 / xx) if xx > 0 else f32(0)
        coef = np.stack([cx.astype(f32), ca.astype(f32)], axis=1)
    return blk, coef


def update_f32(gx, ga, p, m, v, blk, coef, off, hp, decay=None):
    """recombine_surgery_kernel on f32 arrays: (p, m, v, g), every operation rounded on its own.  blk: the 16-float block (clip, bc1,
    bc2_sqrt are read; NOT slot 3: the coefficient table carries s)."""
    gx, ga, p, m, v = (np.asarray(t, f32) for t in (gx, ga, p, m, v))
    lr, b1, b2, eps, wd = hp
    clip, bc1, bc2s = (f32(blk[i]) for i in (5, 8, 9))
    cx, ca = per_element(np.asarray(coef, f32)[:, 0], off), per_element(np.asarray(coef, f32)[:, 1], off)
    step_size = lr / bc1
    decay = O.decay_two_roundings(hp) if decay is None else f32(decay)
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    with np.errstate(all="ignore"):
        g = ((cx * gx) - (ca * ga)) * clip
        p = p * decay
        m = m + (g - m) * omb1
        v = v * b2 + (g * g) * omb2
        den = np.sqrt(v) / bc2s + eps
        p = p - step_size * (m / den)
    assert all(t.dtype == f32 for t in (g, p, m, v, den, cx, ca)) and step_size.dtype == f32
    return p, m, v, g


# ================================================================ seeded cases
def offsets_of(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


def case(lengths, seed, conflict="mixed", integers=False):
    """(gx, ga, off): a pair over groups of the given lengths.  conflict: 'mixed' (every third group conflicts strongly, every third
    is opposed, the rest are independent draws), 'none' (every group has xa < 0), or a set of group indices that conflict (the others
    have xa < 0).  Specials of 'mixed' (where the group exists): group 1 has x = 0, group 2 has a = 0, group 4 has xa EXACTLY 0.
    integers: values in [-8, 8] (every product and sum exact)."""
    rng = np.random.default_rng(seed)
    off = offsets_of(lengths)
    n = off[-1]
    if integers:
        gx, ga = rng.integers(-8, 9, n).astype(f32), rng.integers(-8, 9, n).astype(f32)
    else:
        gx, ga = (0.01 * rng.standard_normal(n)).astype(f32), (0.02 * rng.standard_normal(n)).astype(f32)
    for g, (lo, hi) in enumerate(zip(off, off[1:])):
        if conflict == "mixed":
            kind = ("yes", "no", "free")[g % 3]
        else:
            kind = "yes" if (conflict != "none" and g in conflict) else "no"
        x, a = gx[lo:hi], ga[lo:hi]
        if kind != "free":
            # a = (+-)|x| pattern mixed with its own draw: xa clearly of the wanted sign
            sign = f32(1 if kind == "yes" else -1)
            a[:] = sign * (f32(2) * x) + (a if integers else f32(0.25) * a)
            if float(np.dot(x.astype(f64), a.astype(f64))) * float(sign) <= 0:      # (tiny integer groups)
                a[:] = sign * f32(2) * x
                if not x.any():
                    x[0] = 1; a[0] = sign * 2
    if conflict == "mixed":
        T = len(lengths)
        if T > 1:
            gx[off[1]:off[2]] = 0
        if T > 2:
            ga[off[2]:off[3]] = 0
        if T > 4 and off[5] - off[4] >= 4:                     # x = (1, 1, 0..), a = (1, -1, ..) on the first granule, zero elsewhere
            lo, hi = off[4], off[5]
            gx[lo:hi], ga[lo:hi] = 0, 0
            gx[lo:lo + 2] = [3, 3]
            ga[lo:lo + 2] = [5, -5]
    return gx, ga, off

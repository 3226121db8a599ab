"""Plain restatements of csrc/optimizer.hip for tests/test_hip_optimizer.py; tests/test_optimizer_host.py pins them to torch's own
operators on the CPU.  numpy + torch on the CPU, no GPU.

Two restatements of the flat-buffer update:

* The f64 REFERENCE (norm_sums_f64, scalars_f64, adamw_f64).  It takes the f32 gradients, states and parameters as given and the
  hyper-parameters as the C ABI carries them -- lr, beta1, beta2, eps, wd rounded to f32 -- widened to double; `1 - beta`,
  `1 - beta^step`, `lr / bc1` and `1 - lr * wd` are formed in double.  THIS is the optimizer the library implements: its effective
  beta2 is f32(0.999) = 0.99900001287, used self-consistently by the second-moment update and by its bias correction (an f64
  optimizer handed the decimal 0.999 is a different, equally valid one; the two differ by 1.3e-8 in beta2).

* The f32 RESTATEMENT of the kernels' own operation order (norm_sums_f32, scalars_f32, adamw_f32), every operation rounded on its own
  (the file is built without fused multiply-add contraction), in numpy.  numpy's f32 `sqrt` and divide are correctly rounded; torch's
  CPU `sqrt` is not on every host ("A host detail" in docs/kernels.md), so torch does not appear in it.

And the data-movement kernels: bf16 rounding to nearest even on the bit patterns, the tap-reversed transpose of the dgrad weight
copy, the 16 phase-tap weights of the sub-pixel upsample, the fold of their gradients onto the nine taps, the zero-range mask.
"""
import math

import numpy as np
import torch

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
THREADS, MAX_BLOCKS = 256, 2048


def hyper(lr, beta1, beta2, eps, wd):
    """The five hyper-parameters as the C ABI carries them: f32."""
    return tuple(f32(h) for h in (lr, beta1, beta2, eps, wd))


def wide(hp):
    """... widened to (Python) double"""
    return tuple(float(h) for h in hp)


def grid_for(n):
    """siss_grad_norm_partials' block count: clamp(ceil(n / 4 / 256), 1, 2048)"""
    return min(max(-(-(n // 4) // THREADS), 1), MAX_BLOCKS)


# ------------------------------------------------------------------ pass 1: the three sums
def norm_sums_f64(gx, ga):
    """(|gx|^2, |ga|^2, <gx, ga>, sum |gx ga|) in f64 (exactly summed products: math.fsum)"""
    x, a = np.asarray(gx, f64), np.asarray(ga, f64)
    return math.fsum(x * x), math.fsum(a * a), math.fsum(x * a), math.fsum(np.abs(x * a))


def norm_sums_f32(gx, ga):
    """The kernel's construction: per 16-byte group the f32 sum ((t0 + t1) + t2) + t3 of four f32 products, the groups added in f64;
    the n % 4 tail as f64 products.  (The ORDER of the f64 additions is the device's own; its effect is 2^-53 n relative.)"""
    x, a = np.asarray(gx, f32), np.asarray(ga, f32)
    nv = x.size // 4 * 4
    out = []
    for l, r in ((x, x), (a, a), (x, a)):
        t = (l[:nv] * r[:nv]).reshape(-1, 4)                            # f32 products, each rounded
        grp = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]                 # f32 (0.f + t0 is exact)
        assert grp.dtype == f32
        out.append(math.fsum(grp.astype(f64)) + math.fsum(l[nv:].astype(f64) * r[nv:].astype(f64)))
    return tuple(out)


# ------------------------------------------------------------------ the scalar block
def _scale(xx, aa, xa, mode, knob):
    na = math.sqrt(aa)
    if mode == 1:
        s = float(f32(knob)) - (xa / aa if aa else math.nan)
        return -(s if s > 0 else 0.0)
    s = float(f32(knob)) / na if na else math.inf
    return 0.0 if (mode == 2 and math.isinf(s)) else s


def scalars_f64(xx, aa, xa, mode, knob, max_norm, beta1, beta2, step):
    """The f64 reference of the block: dict of norm_x, norm_a, dot, scale, pre_clip_norm, clip_coef, step, bc1, bc2_sqrt from exact
    sums.  knob, max_norm, beta1, beta2 are f32 values widened; step is the count AFTER this update."""
    s = _scale(xx, aa, xa, mode, knob)
    g2 = max(xx - 2 * s * xa + s * s * aa, 0.0)
    gn = math.sqrt(g2)
    coef = min(float(f32(max_norm)) / (gn + 1e-6), 1.0)                 # torch.nn.utils.clip_grad_norm_
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    return dict(norm_x=math.sqrt(xx), norm_a=math.sqrt(aa), dot=xa, scale=s, pre_clip_norm=gn, clip_coef=coef, step=float(step),
                bc1=1.0 - b1 ** step, bc2_sqrt=math.sqrt(1.0 - b2 ** step))


NAMES = {"norm_x": 0, "norm_a": 1, "dot": 2, "scale": 3, "pre_clip_norm": 4, "clip_coef": 5, "step": 6, "bc1": 8, "bc2_sqrt": 9}


def scalars_f32(xx, aa, xa, mode, knob, max_norm, beta1, beta2, step_before, pow64=True):
    """The 16-float block as scalars_kernel forms it from its (f64) sums: everything in double and rounded once, the step counter
    incremented in f32.  pow64: the bias corrections in double, rounded once (the kernel since this test exists); pow64 = False: the
    earlier `1.f - powf(beta, step)`, with numpy's correctly rounded f32 pow standing in for the device's powf."""
    step = f32(step_before) + f32(1)
    r = scalars_f64(xx, aa, xa, mode, knob, max_norm, beta1, beta2, float(step))
    blk = np.zeros(16, f32)
    for k, i in NAMES.items():
        blk[i] = f32(r[k])
    if not pow64:
        blk[8] = f32(1) - np.power(f32(beta1), step)
        blk[9] = np.sqrt(f32(1) - np.power(f32(beta2), step))
        assert blk[8].dtype == f32
    return blk


# ------------------------------------------------------------------ pass 2
def decay_two_roundings(hp):
    """1.f - lr * wd with the product and the difference each rounded to f32 (no contraction)"""
    return f32(1) - hp[0] * hp[4]


def decay_fused(hp):
    """... as ONE fused multiply-add: f32(1 - lr wd) of the exact product (48 bits: exact in double; the difference is then rounded
    to double and to f32, which equals one rounding unless the double lands exactly on an f32 tie: asserted)"""
    d = 1.0 - float(hp[0]) * float(hp[4])
    up, dn = f32(np.nextafter(f32(d), f32(2))), f32(np.nextafter(f32(d), f32(0)))
    assert d not in ((float(f32(d)) + float(up)) / 2, (float(f32(d)) + float(dn)) / 2)
    return f32(d)


def adamw_f32(gx, ga, p, m, v, blk, hp, decay=None):
    """recombine_adamw_kernel on f32 arrays, fed the 16-float scalar block: (p, m, v, g), every operation rounded on its own."""
    gx, ga, p, m, v = (np.asarray(t, f32) for t in (gx, ga, p, m, v))
    lr, b1, b2, eps, wd = hp
    s, clip, bc1, bc2s = (f32(blk[i]) for i in (3, 5, 8, 9))
    step_size = lr / bc1
    decay = decay_two_roundings(hp) if decay is None else f32(decay)
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    with np.errstate(all="ignore"):
        g = (gx - s * ga) * clip
        p = p * decay
        m = m + (g - m) * omb1                                          # lerp
        v = v * b2 + (g * g) * omb2
        den = np.sqrt(v) / bc2s + eps
        p = p - step_size * (m / den)
    assert all(t.dtype == f32 for t in (g, p, m, v, den)) and step_size.dtype == f32 and omb2.dtype == f32
    return p, m, v, g


def adamw_f64(gx, ga, p, m, v, sc, hp):
    """The f64 reference of pass 2 from the f64 scalars `sc` (scalars_f64): (p, m, v, g)."""
    gx, ga, p, m, v = (np.asarray(t, f64) for t in (gx, ga, p, m, v))
    lr, b1, b2, eps, wd = wide(hp)
    g = (gx - sc["scale"] * ga) * sc["clip_coef"]
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (g * g) * (1.0 - b2)
    den = np.sqrt(v) / sc["bc2_sqrt"] + eps
    p = p - (lr / sc["bc1"]) * (m / den)
    return p, m, v, g


def step_f64(gx, ga, p, m, v, step, hp, mode, knob, max_norm):
    """One whole update in f64 (sums, scalars, pass 2); `step` is the count after it."""
    xx, aa, xa, _ = norm_sums_f64(gx, ga)
    sc = scalars_f64(xx, aa, xa, mode, knob, max_norm, hp[1], hp[2], step)
    return adamw_f64(gx, ga, p, m, v, sc, hp), sc


def warm_state(n, k, hp, seed):
    """(m, v) after k - 1 plain f64 AdamW moment updates on N(0, 1) gradients (so that m / sqrt(v) is O(1) at step k), as f32"""
    rng = np.random.default_rng(seed)
    _, b1, b2, _, _ = wide(hp)
    m, v = np.zeros(n), np.zeros(n)
    for _ in range(k - 1):
        g = rng.standard_normal(n)
        m += (g - m) * (1 - b1)
        v = v * b2 + g * g * (1 - b2)
    return m.astype(f32), v.astype(f32)


# ------------------------------------------------------------------ bf16
def bf16_bits(x):
    """f32 -> bf16 bit patterns (uint16), round to nearest even on the bits; a NaN stays a (quiet) NaN"""
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)
    nan = np.isnan(np.asarray(x, f32))
    r = np.where(nan, (b >> 16).astype(np.uint32) | 0x40, r)
    return r.astype(np.uint16)


def bf16(x):
    """... as a torch.bfloat16 tensor of x's shape"""
    return torch.from_numpy(bf16_bits(x).view(np.int16).copy()).view(torch.bfloat16).reshape(np.shape(x))


# ------------------------------------------------------------------ weight copies
def dgrad_weight(w):
    """[taps][co][ci] -> [taps][ci][co] with the tap order reversed"""
    w = np.asarray(w)
    out = np.empty((w.shape[0], w.shape[2], w.shape[1]), w.dtype)
    for t in range(w.shape[0]):
        for c in range(w.shape[2]):
            out[w.shape[0] - 1 - t, c, :] = w[t, :, c]
    return out


def job_table(shapes, align=64):
    """The device job table of siss_conv_weight_dgrad_multi* for weights laid out one after another, each start rounded up to
    `align` elements: (records, total elements, total 64 x 64 tiles)"""
    rec = np.zeros(len(shapes), dtype=np.dtype([("src", "<i8"), ("dst", "<i8"), ("taps", "<i4"), ("co", "<i4"), ("ci", "<i4"), ("tile0", "<i4")]))
    off = tiles = 0
    for i, (t, co, ci) in enumerate(shapes):
        rec[i] = (off, off, t, co, ci, tiles)
        off += -(-t * co * ci // align) * align
        tiles += t * (-(-co // 64)) * (-(-ci // 64))
    return rec, off, tiles


# ------------------------------------------------------------------ sub-pixel upsample
def phase_tap(k, p):
    """which of the two taps of phase p the 3x3 filter index k lands on"""
    return int(k >= 1) if p == 0 else int(k >= 2)


def phase_weights(w):
    """w [9][Co][Ci] f32 -> wf [16 = plane * 4 + tap][Co][Ci] f32: the sum of the 3x3 taps that land on the phase tap, added in f32
    in (ky, kx) order starting from 0.f.  (The bf16 form rounds this once; the dgrad operand is the per-panel transpose.)"""
    w = np.asarray(w, f32)
    out = np.zeros((16,) + w.shape[1:], f32)
    for pt in range(16):
        plane, tap = pt >> 2, pt & 3
        py, px, a, b = plane >> 1, plane & 1, tap >> 1, tap & 1
        for ky in range(3):
            for kx in range(3):
                if phase_tap(ky, py) == a and phase_tap(kx, px) == b:
                    out[pt] = out[pt] + w[ky * 3 + kx]
    return out


def phase_fold(d4, dW):
    """d4 [16][...] f32 (one set), dW [9][...] f32 -> dW + the fold: acc = ((d0 + d1) + d2) + d3 over the four planes, then ONE add"""
    d4, dW = np.asarray(d4, f32), np.asarray(dW, f32)
    out = np.empty_like(dW)
    for k in range(9):
        ky, kx = divmod(k, 3)
        acc = np.zeros(dW.shape[1:], f32)
        for plane in range(4):
            tap = phase_tap(ky, plane >> 1) * 2 + phase_tap(kx, plane & 1)
            acc = acc + d4[plane * 4 + tap]
        out[k] = dW[k] + acc
    assert out.dtype == f32
    return out


# ------------------------------------------------------------------ zero ranges
def zero_table(starts, lens):
    """siss_zero_ranges' table: n starts, then the n + 1 prefix sums of the lengths (int64, 16-byte granules); and the total"""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    pre = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate([starts, pre]), int(pre[-1])


def zero_mask(nfloats, starts, lens):
    """bool [nfloats]: the floats of the listed granules"""
    d = np.zeros(nfloats // 4 + 1, np.int64)
    np.add.at(d, np.asarray(starts, np.int64), 1)
    np.add.at(d, np.asarray(starts, np.int64) + np.asarray(lens, np.int64), -1)
    cover = np.cumsum(d)[:nfloats // 4]
    assert int(cover.max(initial=0)) <= 1, "stretches overlap"
    return np.repeat(cover > 0, 4)


# ------------------------------------------------------------------ the seeded inputs and the bounds that the GPU test AND the host test use
SIZES = [1, 2, 3, 5, 1027, 100_003, 2_097_152 + 1027]      # the tail alone; tail + vectors; the grid-stride loop (> 2048 x 256 x 4 floats)
HYPER = {                                                  # lr, beta1, beta2, eps, wd
    "celeb": (5e-6, 0.95, 0.999, 1e-8, 1e-6),              # config/delete_celeb.yaml
    "sd": (1e-5, 0.9, 0.999, 1e-8, 1e-2),                  # config/delete_sd.yaml
    "mnist": (1e-4, 0.95, 0.999, 1e-8, 1e-6),              # config/train_tshirt_mnist.yaml
    "lr5e-3": (5e-3, 0.95, 0.999, 1e-8, 1e-2),
}
BETAS = [(0.95, 0.999), (0.9, 0.999)]
STEPS = [1, 2, 3, 6, 31, 100, 1000]
PRECISION_N = 4099                                          # 1024 vectors = 4 blocks, and a 3-float tail


def gauss_pair(n, seed):
    rng = np.random.default_rng(seed)
    return (0.01 * rng.standard_normal(n)).astype(f32), (0.02 * rng.standard_normal(n)).astype(f32)


def int_pair(n, seed):
    """integers in [-8, 8]: every product, group sum and f64 sum is exact.  ga[0] != 0 (mode 0 divides by |ga|)."""
    rng = np.random.default_rng(seed)
    gx, ga = rng.integers(-8, 9, n).astype(f32), rng.integers(-8, 9, n).astype(f32)
    gx[0], ga[0] = -3, 5
    return gx, ga


def int_sums(gx, ga):
    x, a = np.asarray(gx).astype(np.int64), np.asarray(ga).astype(np.int64)
    return int((x * x).sum()), int((a * a).sum()), int((x * a).sum())


def near_cancelling_pair(n, seed, knob):
    """gx = s ga + 1e-3 noise with s = knob / |ga|: g = gx - s ga is a thousandth of either term"""
    rng = np.random.default_rng(seed)
    ga = rng.standard_normal(n).astype(f32)
    s = float(f32(knob)) / math.sqrt(math.fsum(ga.astype(f64) ** 2))
    return (s * ga.astype(f64) + 1e-3 * rng.standard_normal(n)).astype(f32), ga


def cancelling_int_pair(n):
    """(gx, ga, knob) with gx = s ga EXACTLY: |ga| = 5 (or 4 at n = 1), s = 2; the last element sits in the tail"""
    gx, ga = np.zeros(n, f32), np.zeros(n, f32)
    if n == 1:
        ga[0], knob = 4, 8.0
    else:
        ga[0], ga[n - 1], knob = 3, 4, 10.0
    gx[:] = 2 * ga
    return gx, ga, knob


def ratio_pair(n, ratio10):
    """Integer pair with <gx, ga> / |ga|^2 = ratio10 / 10 exactly: ga = 10 k, gx = ratio10 k + (a vector orthogonal to k)"""
    rng = np.random.default_rng(n + 7)
    k = rng.integers(1, 4, n).astype(np.int64)
    orth = np.zeros(n, np.int64)
    m = n // 2 * 2
    orth[0:m:2], orth[1:m:2] = k[1:m:2], -k[0:m:2]
    return (ratio10 * k + orth).astype(f32), (10 * k).astype(f32)


def scalar_bounds(gx, ga, mode, knob, max_norm):
    """{field: (f64 reference, allowed |error|)} of the scalar block on arbitrary f32 data, with u = 2^-24, to first order in u.

    The kernel's sums: every term is an f32 product (one rounding) that passes through at most three f32 additions inside its
    16-byte group (0.f + t0 is exact), then f64 additions (2^-53 each: nothing beside u): each term carries (1 + theta), |theta| <= 4u,
    the tail terms (f64 products) none.  So |d xx| <= 4u xx, |d aa| <= 4u aa, |d xa| <= 4u sum |x a|.
      norm_x, norm_a   sqrt halves the relative error (2u), the rounding to f32 adds u: 3u <= 4u relative.
      dot              4u sum |x a| + u |dot| (its rounding).
      scale, mode 0/2  knob / |ga|: 2u from |ga| + u: 3u <= 4u relative.
      scale, mode 1    -(max(eta - xa / aa, 0)): max is 1-Lipschitz; |d (xa / aa)| <= (4u sum |x a| + 4u |xa|) / aa; + u |s|.
      pre_clip_norm    g2 = xx - 2 s xa + s^2 aa from the three sums: |d g2| <= E = 4u (xx + 2 |s| sum |x a| + s^2 aa)  (in modes 0 / 2
                       s^2 aa = knob^2 whatever aa's error, and that share of E takes s's own 2u instead; in mode 1 s's error above
                       enters through d g2 / d s = 2 (s aa - xa) and is ADDED to E);  |d sqrt(g2)| = |d g2| / (gn + gn') <= E / (2 gn)
                       to first order and <= sqrt(E) always; + u gn (its rounding).
      clip_coef        min(max_norm / (gn + 1e-6), 1) is monotone in gn: it lies between its values at gn + b and at gn - b
                       (b = pre_clip_norm's allowance before rounding), widened by its own rounding u.
    """
    xx, aa, xa, axa = norm_sums_f64(gx, ga)
    ref = scalars_f64(xx, aa, xa, mode, knob, max_norm, 0.5, 0.5, 1)
    s, gn = ref["scale"], ref["pre_clip_norm"]
    out = {"norm_x": (ref["norm_x"], 4 * U * ref["norm_x"]), "norm_a": (ref["norm_a"], 4 * U * ref["norm_a"]),
           "dot": (xa, U * abs(xa) + 4 * U * axa)}
    E = 4 * U * (xx + 2 * abs(s) * axa + s * s * aa)
    if mode == 1:
        ds = 4 * U * (axa + abs(xa)) / aa
        out["scale"] = (s, ds + U * abs(s))
        E += 2 * abs(s * aa - xa) * ds
    else:
        out["scale"] = (s, 4 * U * abs(s))
    b = min(E / (2 * gn), math.sqrt(E)) if gn > 0 else math.sqrt(E)
    out["pre_clip_norm"] = (gn, U * gn + b)
    M = float(f32(max_norm))
    lo, hi = min(M / (gn + b + 1e-6), 1.0) * (1 - U), min(M / (max(gn - b, 0.0) + 1e-6), 1.0) * (1 + U)
    out["clip_coef"] = ((lo + hi) / 2, (hi - lo) / 2)
    return out


def scalar_errors(blk, bounds):
    """{field: error / allowed} of a 16-float block against scalar_bounds' table (inf for a NaN)"""
    out = {}
    for k, (ref, tol) in bounds.items():
        err = abs(float(blk[NAMES[k]]) - ref)
        out[k] = (err / tol if tol > 0 else (0.0 if err == 0 else math.inf)) if math.isfinite(err) else math.inf
    return out


def bias_correction_errors(blk, beta1, beta2, k):
    """(|bc1 - ref| / (u ref), |bc2_sqrt - ref| / (u ref)) against the f64 values of the f32 betas at step k"""
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    r1, r2 = 1.0 - b1 ** k, math.sqrt(1.0 - b2 ** k)
    return abs(float(blk[8]) - r1) / (U * r1), abs(float(blk[9]) - r2) / (U * r2)


def precision_case(k, hp, zero_init, seed=0):
    """The inputs of the step-precision test at step k: gradient, p0, and (m, v) after k - 1 f64 steps"""
    rng = np.random.default_rng(1000 * seed + k)
    n = PRECISION_N
    g = rng.standard_normal(n).astype(f32)
    p0 = np.zeros(n, f32) if zero_init else rng.standard_normal(n).astype(f32)
    m, v = warm_state(n, k, hp, seed=k + 1)
    return g, p0, m, v


def torch_adamw(g, p0, m, v, k, hp, dtype):
    """torch.optim.AdamW(foreach=False) at step k on one tensor of `dtype`, hyper-parameters = the f32 values widened: (p, m, v)"""
    lr, b1, b2, eps, wd = wide(hp)
    p = torch.from_numpy(np.asarray(p0)).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": torch.from_numpy(np.asarray(m)).to(dtype).clone(),
                    "exp_avg_sq": torch.from_numpy(np.asarray(v)).to(dtype).clone()}
    p.grad = torch.from_numpy(np.asarray(g)).to(dtype).clone()
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == k
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def update_errors(got, ref, p0):
    """(p, m, v) errors: max |p - p_ref| / max |p_ref - p0|, and m, v relative to their largest reference value"""
    (p, m, v), (pr, mr, vr) = ([np.asarray(t, f64) for t in got], [np.asarray(t, f64) for t in ref])
    return (float(np.abs(p - pr).max() / np.abs(pr - np.asarray(p0, f64)).max()), float(np.abs(m - mr).max() / np.abs(mr).max()),
            float(np.abs(v - vr).max() / np.abs(vr).max()))

"""Plain restatements of csrc/train_state.hip and of the epoch sampler for tests/test_hip_train_state.py; tests/test_train_state_host.py
pins them to torch's own operators on the CPU.  numpy + torch on the CPU, no GPU.  The helpers, sizes, hyper-parameters and u are
tests/optimizer_ref.py's: the single-set update is the two-set one with a zero second set (s = 0), plus the EMA line.

The EMA decay (diffusers 0.27.2 training_utils.EMAModel.get_decay / .step; diffusers is not a dependency, so this is the contract):
k = optimization_step after the increment, s = max(0, k - update_after_step - 1); s == 0 -> decay = 0 (returned before any clamp);
else decay = 1 - (1 + s / inv_gamma)^-power with warmup, (1 + s) / (10 + s) without; then max(min(decay, max_decay), min_decay).
The device keeps one_minus_decay = 1 - decay, formed in double and rounded once.
"""
import math

import numpy as np

import optimizer_ref as R

f32, f64 = np.float32, np.float64
U, SIZES, HYPER = R.U, R.SIZES, R.HYPER
# slots of the 16-float block (siss_train_scalars_words)
NAMES = {"grad_norm": 0, "clip_coef": 1, "step": 2, "bc1": 3, "bc2_sqrt": 4, "ema_step": 5, "one_minus_decay": 6, "ema_decay": 7}
TSHIRT_EMA = dict(max_decay=0.9999, min_decay=0.0, inv_gamma=1.0, power=0.75, use_warmup=True, update_after=0)   # config/train_tshirt_mnist.yaml
STEPS = [1, 2, 3, 31, 1000, 100_000]


def ema_args(e):
    """the schedule as the launchers take it: four doubles, two ints"""
    return (float(e["max_decay"]), float(e["min_decay"]), float(e["inv_gamma"]), float(e["power"]), int(e["use_warmup"]), int(e["update_after"]))


def decay_f64(k, max_decay=0.9999, min_decay=0.0, inv_gamma=1.0, power=2 / 3, use_warmup=False, update_after=0):
    s = max(0, k - update_after - 1)
    if s <= 0:
        return 0.0
    d = 1.0 - (1.0 + s / inv_gamma) ** -power if use_warmup else (1.0 + s) / (10.0 + s)
    return max(min(d, max_decay), min_decay)


def first_capped_step(e):
    """the first optimization_step whose uncapped decay exceeds max_decay"""
    free = dict(e, max_decay=1.0)
    k = 2
    while decay_f64(k, **free) <= e["max_decay"]:
        k = k * 2
    lo, hi = k // 2, k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if decay_f64(mid, **free) > e["max_decay"] else (mid, hi)
    return hi


# ------------------------------------------------------------------ pass 1 and the block
def norm_sum_f32(g):
    """the kernel's |g|^2: R.norm_sums_f32's construction (f32 group sums of four f32 products, added in f64; f64 tail)"""
    return R.norm_sums_f32(g, np.zeros_like(np.asarray(g, f32)))[0]


def scalars_f64(xx, max_norm, beta1, beta2, step, ema, ema_step):
    """the f64 reference of the block from an exact |g|^2; step / ema_step are the counts AFTER this update"""
    r = R.scalars_f64(xx, 0.0, 0.0, 2, 1.0, max_norm, beta1, beta2, step)
    d = decay_f64(ema_step, **ema)
    return dict(grad_norm=r["pre_clip_norm"], clip_coef=r["clip_coef"], step=float(step), bc1=r["bc1"], bc2_sqrt=r["bc2_sqrt"],
                ema_step=float(ema_step), one_minus_decay=1.0 - d, ema_decay=d)


def scalars_f32(xx, max_norm, beta1, beta2, step_before, ema, ema_step_before, pad=0.0):
    """the 16-float block as train_scalars_kernel forms it: everything in double, rounded once; both counters incremented in f32"""
    step, k = f32(step_before) + f32(1), f32(ema_step_before) + f32(1)
    r = scalars_f64(xx, max_norm, beta1, beta2, float(step), ema, int(k))
    blk = np.full(16, pad, f32)
    for name, i in NAMES.items():
        blk[i] = f32(r[name])
    return blk


def as_two_set_block(blk):
    """the block in optimizer_ref.adamw_f32's layout with s = 0"""
    old = np.zeros(16, f32)
    old[R.NAMES["clip_coef"]], old[R.NAMES["bc1"]], old[R.NAMES["bc2_sqrt"]] = blk[NAMES["clip_coef"]], blk[NAMES["bc1"]], blk[NAMES["bc2_sqrt"]]
    return old


# ------------------------------------------------------------------ pass 2 and the EMA line
def ema_f32(ema, p, blk):
    """s_param.sub_(one_minus_decay * (s_param - param)), every operation rounded to f32"""
    ema, p, omd = np.asarray(ema, f32), np.asarray(p, f32), f32(blk[NAMES["one_minus_decay"]])
    out = ema - omd * (ema - p)
    assert out.dtype == f32
    return out


def update_f32(g, p, m, v, ema, blk, hp, decay=None):
    """clip_adamw_ema_kernel on f32 arrays fed the block: (p, m, v, ema, g'), the AdamW part by optimizer_ref.adamw_f32 (g' = (g - 0 * 0)
    * clip is g * clip bit for bit), the EMA line on the NEW p; ema may be None"""
    g = np.asarray(g, f32)
    p, m, v, gc = R.adamw_f32(g, np.zeros_like(g), p, m, v, as_two_set_block(blk), hp, decay=decay)
    return p, m, v, (None if ema is None else ema_f32(ema, p, blk)), gc


def update_f64(g, p, m, v, ema, step, hp, max_norm, ema_sched, ema_step):
    """one whole update in f64: (p, m, v, ema), scalars"""
    g = np.asarray(g, f32)
    (p, m, v, _), _ = R.step_f64(g, np.zeros_like(g), p, m, v, step, hp, 2, 1.0, max_norm)
    sc = scalars_f64(R.norm_sums_f64(g, np.zeros_like(g))[0], max_norm, hp[1], hp[2], step, ema_sched, ema_step)
    ema = np.asarray(ema, f64)
    return (p, m, v, ema - sc["one_minus_decay"] * (ema - p)), sc


def block_errors(blk, g, max_norm):
    """{field: error / allowed} of grad_norm and clip_coef against optimizer_ref.scalar_bounds with a zero second set (there: |d xx| <=
    4u xx, so pre_clip_norm within u gn + 2u gn, clip_coef between its values at gn -+ that)"""
    b = R.scalar_bounds(g, np.zeros_like(np.asarray(g, f32)), 2, 1.0, max_norm)
    out = {}
    for name, key in (("grad_norm", "pre_clip_norm"), ("clip_coef", "clip_coef")):
        ref, tol = b[key]
        err = abs(float(blk[NAMES[name]]) - ref)
        out[name] = err / tol if math.isfinite(err) and tol > 0 else (0.0 if err == 0 else math.inf)
    return out


def one_rounding_errors(blk, beta1, beta2, step, ema, ema_step):
    """(bc1, bc2_sqrt, one_minus_decay) errors in units of u * reference, against f64 (the betas as f32 values widened)"""
    e1, e2 = R.bias_correction_errors(as_two_set_block(blk), beta1, beta2, step)
    ref = 1.0 - decay_f64(ema_step, **ema)
    return e1, e2, abs(float(blk[NAMES["one_minus_decay"]]) - ref) / (U * ref)


def gauss(n, seed):
    return R.gauss_pair(n, seed)[0]


def ints(n, seed):
    return R.int_pair(n, seed)[0]


def state(n, seed):
    """(p, m, v, ema) of a run in progress"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(f32)
    return p, (0.01 * rng.standard_normal(n)).astype(f32), (1e-4 * rng.random(n)).astype(f32), (p + 0.01 * rng.standard_normal(n)).astype(f32)


# ------------------------------------------------------------------ the epoch sampler
def epoch_batches(n, batch_size, seed, epoch):
    """the index lists of one epoch: the permutation of a generator seeded by (seed, epoch), cut into batches, the partial one kept"""
    perm = np.random.default_rng([int(seed), int(epoch)]).permutation(n).tolist()
    return [perm[i:i + batch_size] for i in range(0, n, batch_size)]


def remaining(n, batch_size, seed, num_epochs, epoch, position):
    """every (epoch, position, indices) from (epoch, position) to the end of the run"""
    out = []
    for e in range(epoch, num_epochs):
        for pos, idx in enumerate(epoch_batches(n, batch_size, seed, e)):
            if (e, pos) >= (epoch, position):
                out.append((e, pos, idx))
    return out

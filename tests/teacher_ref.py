"""Plain restatements of csrc/teacher.hip and of the teacher-target objective (siss_amd/teacher.py) for tests/test_teacher_host.py
and tests/test_hip_teacher.py.  numpy + torch on the CPU, no GPU.

* the targets and the cotangent in the kernel's own f32 operation order, every operation rounded on its own (numpy f32 arithmetic):
      esd     y = u - eta * (k - u)          anchor / keep-teacher   y = k          keep-noise   y = f32(noise)
      d = pred - y        cot = (2 * scale) * d
* the per-row sums of d^2: the f32 d widened, squares and sum in f64 (the order of the f64 additions moves the sum by parts in 2^53;
  the test allows 1 ulp of the f32 result);
* the weighted pass 1: tests/optimizer_ref.py's scalar block with the scaling factor GIVEN, s = -weight, from the three sums taken in
  the DEVICE'S order of f64 additions (norm_sums_device: thread, wave butterfly, block, the scalar kernel's fold), so that the block is
  compared bit for bit;
* the objective written with torch.autograd on a student network and a detached teacher network:
      L = sum_keep (eps_theta(x_t) - y_keep)^2 / B + weight * sum_forget (eps_theta(a_t) - y_forget)^2 / B
  (the loop's normalisation: the elementwise squared error summed and divided by the batch size, as every objective of the loop).
"""
import math

import numpy as np
import torch

import optimizer_ref as O

f32, f64 = np.float32, np.float64
KEEPS = ("noise", "teacher", "none")
FORGETS = ("esd", "anchor")
THREADS = 256
CHUNK, MAX_BLOCKS_X = 4096, 64                     # floats one block sums at a time; blocks per row (csrc/teacher.hip)


def rows(keep, forget, B):
    """(R, Rt, k offset, u offset or None): the student's and the teacher's row counts and where the forget rows' k and u start in the
    teacher's output -- written out from the issue's layout, independently of siss_amd.teacher.row_layout."""
    R = B if keep == "none" else 2 * B
    k = B if keep == "teacher" else 0
    u = k + B if forget == "esd" else None
    return R, k + B + (B if forget == "esd" else 0), k, u


def partials_words(R, chw):
    return R * (-(-chw // CHUNK))


def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even), as f32"""
    return (O.bf16_bits(np.asarray(x, f32)).astype(np.uint32) << 16).view(f32).reshape(np.shape(x))


def targets(noise, teach, B, keep, forget, eta):
    """y [R, chw] f32 in the kernel's operation order.  noise [B, chw] (f32 values: a bf16 noise is passed as its f32 image), teach
    [Rt, chw] f32."""
    noise, teach = np.asarray(noise, f32), np.asarray(teach, f32)
    R, Rt, k0, u0 = rows(keep, forget, B)
    assert teach.shape[0] >= Rt
    k, eta = teach[k0:k0 + B], f32(eta)
    if forget == "esd":
        u = teach[u0:u0 + B]
        yf = u - eta * (k - u)                      # three f32 roundings
        assert yf.dtype == f32
    else:
        yf = k
    if keep == "none":
        return yf.copy()
    return np.concatenate([noise if keep == "noise" else teach[:B], yf], 0)


def seed(pred, noise, teach, B, keep, forget, eta, scale):
    """(cot [R, chw] f32, sums [R] f64, y [R, chw] f32) of siss_teacher_seed."""
    pred = np.asarray(pred, f32)
    y = targets(noise, teach, B, keep, forget, eta)
    two_scale = f32(2) * f32(scale)
    d = pred - y
    cot = two_scale * d
    assert d.dtype == f32 and cot.dtype == f32
    sums = (d.astype(f64) ** 2).sum(1)               # (f64 squares are exact; numpy's pairwise f64 sum)
    return cot, sums, y


def ulp32(x):
    x = f32(abs(x))
    return float(np.spacing(x))


# ------------------------------------------------------------------ the weighted pass 1
def weighted_scalars_f64(xx, aa, xa, weight, max_norm, beta1, beta2, step):
    """optimizer_ref.scalars_f64 with s = -weight (weight an f32 value widened); `step` is the count after the update."""
    s = -float(f32(weight))
    g2 = max(xx - 2 * s * xa + s * s * aa, 0.0)
    gn = math.sqrt(g2)
    coef = min(float(f32(max_norm)) / (gn + 1e-6), 1.0)
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    return dict(norm_x=math.sqrt(xx), norm_a=math.sqrt(aa), dot=xa, scale=s, pre_clip_norm=gn, clip_coef=coef, step=float(step),
                bc1=1.0 - b1 ** step, bc2_sqrt=math.sqrt(1.0 - b2 ** step))


def weighted_scalars_f32(xx, aa, xa, weight, max_norm, beta1, beta2, step_before):
    """The 16-float block as weighted_scalars_kernel forms it from its f64 sums: everything in double, rounded once."""
    step = f32(step_before) + f32(1)
    r = weighted_scalars_f64(xx, aa, xa, weight, max_norm, beta1, beta2, float(step))
    blk = np.zeros(16, f32)
    for k, i in O.NAMES.items():
        blk[i] = f32(r[k])
    return blk


def _butterfly(v):
    """wave_sum_d over the last axis (64 lanes): v += v[lane ^ o] for o = 32 .. 1; lane 0's value"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _fold256(th):
    """[..., 256] per-thread f64 sums -> [...]: four wave butterflies, then ((0 + w0) + w1) + w2) + w3"""
    w = _butterfly(th.reshape(*th.shape[:-1], 4, 64))
    a = np.zeros(th.shape[:-1], f64)
    for i in range(4):
        a = a + w[..., i]
    return a


def _strided_sum(v, width):
    """thread j of `width` adds v[j], v[j + width], ... in that order, from 0"""
    pad = -len(v) % width
    rows = np.concatenate([v, np.zeros(pad, f64)]).reshape(-1, width)
    th = np.zeros(width, f64)
    for r in rows:
        th = th + r
    return th


def norm_sums_device(gx, ga):
    """(|gx|^2, |ga|^2, <gx, ga>) as pass 1 forms them, f64 addition for f64 addition: per 16-byte granule the f32 sum of four f32
    products (optimizer_ref.norm_sums_f32), a thread's granules in grid-stride order, the n % 4 tail as f64 products on block 0's
    first threads, lanes -> waves -> block row, then the scalar kernel's one-block fold of the rows."""
    x, a = np.asarray(gx, f32), np.asarray(ga, f32)
    n = x.size
    nv, nblk = n // 4 * 4, O.grid_for(n)
    out = []
    for l, r in ((x, x), (a, a), (x, a)):
        t = (l[:nv] * r[:nv]).reshape(-1, 4)
        grp = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
        assert grp.dtype == f32
        th = _strided_sum(grp.astype(f64), nblk * THREADS)
        for j, i in enumerate(range(nv, n)):                              # (at most three elements: threads 0 .. 2 of block 0)
            th[j] = th[j] + float(l[i]) * float(r[i])
        rows_ = _fold256(th.reshape(nblk, THREADS))
        out.append(float(_fold256(_strided_sum(rows_, THREADS))))
    return tuple(out)


def weighted_block(gx, ga, weight, max_norm, beta1, beta2, step_before):
    """... from the gradient pair, through the device's own order of the three sums"""
    return weighted_scalars_f32(*norm_sums_device(gx, ga), weight, max_norm, beta1, beta2, step_before)


def weighted_step_f64(gx, ga, p, m, v, step, hp, weight, max_norm):
    """One whole update in f64 with g = clip (g_x + weight g_a); `step` is the count after it.  ((p, m, v, g), scalars)"""
    xx, aa, xa, _ = O.norm_sums_f64(gx, ga)
    sc = weighted_scalars_f64(xx, aa, xa, weight, max_norm, hp[1], hp[2], step)
    return O.adamw_f64(gx, ga, p, m, v, sc, hp), sc


# ------------------------------------------------------------------ the objective under autograd
def teacher_targets(teacher, x_t, a_t, t, cond, keep, forget, eta, noise, empty=None, anchor=None):
    """(y_keep or None, y_forget): the targets from a DETACHED teacher network -- a callable (x, t, ctx) -> eps.  cond [B, L, X];
    empty / anchor [1, L, X]."""
    B = a_t.shape[0]
    with torch.no_grad():
        if forget == "esd":
            k, u = teacher(a_t, t, cond), teacher(a_t, t, empty.expand(B, *empty.shape[1:]))
            yf = u - eta * (k - u)
        else:
            yf = teacher(a_t, t, anchor.expand(B, *anchor.shape[1:]))
        yk = None if keep == "none" else (noise if keep == "noise" else teacher(x_t, t, cond))
    return yk, yf


def objective(student, teacher, x_t, a_t, t, cond, noise, keep, forget, eta, weight, batch, empty=None, anchor=None, forget_target=None):
    """(L, L_keep, L_forget) with L = L_keep + weight * L_forget, each the elementwise squared error summed and divided by `batch`.
    forget_target: replaces y_forget (the negative control regresses the forget rows onto the drawn noise)."""
    yk, yf = teacher_targets(teacher, x_t, a_t, t, cond, keep, forget, eta, noise, empty, anchor)
    if forget_target is not None:
        yf = forget_target
    la = ((student(a_t, t, cond) - yf.detach()) ** 2).sum() / batch
    lx = la.new_zeros(()) if keep == "none" else ((student(x_t, t, cond) - yk.detach()) ** 2).sum() / batch
    return lx + weight * la, lx, la


def gradient_pair(student, params, teacher, *args, **kw):
    """(g_x, g_a, L_keep, L_forget): the gradients of the two terms on their own (lists over `params`), by two backward passes."""
    _, lx, la = objective(student, teacher, *args, **kw)
    ga = torch.autograd.grad(la, params, retain_graph=True, allow_unused=True)
    gx = torch.autograd.grad(lx, params, allow_unused=True) if lx.requires_grad else [None] * len(params)
    z = lambda g, p: torch.zeros_like(p) if g is None else g
    return [z(g, p) for g, p in zip(gx, params)], [z(g, p) for g, p in zip(ga, params)], float(lx), float(la)


class ToyNet(torch.nn.Module):
    """A two-layer network eps(x, t, ctx) on flattened rows: the restatement is checked against itself on it (tests/test_teacher_host.py)."""

    def __init__(self, chw, ctx, hidden=11, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter(torch.randn(hidden, chw + ctx + 1, generator=g, dtype=torch.float64) * 0.3)
        self.w2 = torch.nn.Parameter(torch.randn(chw, hidden, generator=g, dtype=torch.float64) * 0.3)

    def forward(self, x, t, ctx):
        z = torch.cat([x.flatten(1), ctx.mean(1), t.double()[:, None] / 1000], 1)
        return (torch.tanh(z @ self.w1.t()) @ self.w2.t()).view(x.shape)

"""The launchers of csrc/optimizer.hip (and the two f32 forms of csrc/f32_path.hip that stand in for them) called DIRECTLY, against
tests/optimizer_ref.py (which tests/test_optimizer_host.py pins to torch's own operators on the CPU, and runs ALONE against every
bound applied here on the same seeded inputs).

    siss_grad_norms_scale, siss_grad_norm_partials, siss_grad_scalars, siss_recombine_clip_adamw, siss_cast_f32_bf16 / siss_copy_f32,
    siss_conv_weight_dgrad_layout, siss_conv_weight_dgrad_multi, siss_conv_weight_dgrad_multi_f32, siss_upsample_phase_weights[_f32],
    siss_upsample_phase_wgrad_fold, siss_zero_ranges

Every output lies between guard stretches filled with a sentinel and the WHOLE buffer is compared; the inputs must come back
bit-identical.  Sizes n = 1, 2, 3, 5 (the n % 4 tail alone), 1027, 100,003 (vectors + tail) and 2,097,152 + 1027 (the grid-stride loops
behind 2048 blocks x 256 threads x 4 floats).

What is held to what:
* the three sums on integers in [-8, 8] (all exact): norm_x, norm_a bitwise f32(sqrt(f64(int))), dot bitwise f32(int); a single non-zero
  at the seams of the index space gives the exact square (a lost or double-counted element shows);
* the scalar block on Gaussian data against f64 with the a-priori bounds of optimizer_ref.scalar_bounds (u = 2^-24; derived there from
  the kernel's construction -- four f32 operations per term, f64 sums): norm_x, norm_a, scale 4u relative; dot u |dot| + 4u sum |x a|;
  pre_clip_norm u gn + min(E / (2 gn), sqrt(E)), E = 4u (xx + 2 |s| sum |x a| + s^2 aa); clip_coef between its values at gn -+ that;
* bc1, bc2_sqrt within 2u relative of the f64 values at steps 1 .. 100,000 (one rounding of a double: u; 2u leaves the double
  pow / sqrt their own last place);
* the element-wise pass BITWISE: the f32 restatement fed the block read back from the device reproduces p, m, v, g_out, and the
  shadow is bitwise the bf16 rounding of the new p;
* the step's precision against the f64 update: 4 x the same figure of torch's own f32 CPU AdamW (the project's margin for "a multiple
  of torch's own f32 error", set before any measurement);
* casts, weight copies, phase weights, the fold and the zero fill: bitwise.
Measured values: docs/kernels.md, "The flat-buffer update: measured precision".
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import optimizer_ref as R
from test_hip_small_kernels import Buf, bits, same

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
f32 = np.float32
U = R.U
SENT = 77.0                                                 # exact in bf16
GUARD = 64                                                  # elements: 128 B of bf16, 256 B of f32
BIG = R.SIZES[-1]
SMALL = [n for n in R.SIZES if n <= 1027]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def launch(name, *args, f32_mode=False):
    from siss_amd import lib
    with lib.f32_mode(f32_mode):
        lib.call(name, *args)
    torch.cuda.synchronize()


def refused(name, *args, f32_mode=False):
    with pytest.raises(RuntimeError, match="bad argument"):
        launch(name, *args, f32_mode=f32_mode)


class Flat(Buf):
    """Buf for one flat stretch of n elements with a FIXED guard (Buf sizes its guard by the last dimension: 8 M elements here)."""

    def __init__(self, n, dtype, dev, body=None, fill=SENT, guard=GUARD):
        self.shape, self.n, self.g = (n,), n, guard
        self.flat = torch.full((n + 2 * guard,), fill, dtype=dtype)
        if body is not None:
            self.host[:] = torch.as_tensor(body).to(dtype)
        self.d = self.flat.to(dev)

    def np(self):
        return self.t.cpu().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Scal:
    """The 16-float scalar block (pads pre-filled with a sentinel that must survive, the step counter preset) and the partial sums"""

    def __init__(self, dev, step_before=0):
        init = np.full(16, 33.0, f32)
        init[list(R.NAMES.values())] = 0
        init[6] = step_before
        self.init = init
        self.blk = Flat(16, F32, dev, body=init)
        self.partials = Flat(3 * R.MAX_BLOCKS, F64, dev, fill=-5.0)

    def read(self, n=None):
        """the block from the device; pads and guards checked, and the partial sums past 3 * grid_for(n)"""
        b = self.blk.np().copy()
        keep = self.init.copy()
        idx = list(R.NAMES.values())
        keep[idx] = b[idx]
        self.blk.check(T(keep), "scalar block: pads and guards")
        if n is not None:
            got = self.partials.d.cpu()
            same(got[GUARD + 3 * R.grid_for(n):], self.partials.flat[GUARD + 3 * R.grid_for(n):], "partial sums beyond the grid")
            same(got[:GUARD], self.partials.flat[:GUARD], "partial sums: guard before")
        return b


def norms(dev, gx, ga, mode, knob, max_norm=1.0, betas=(0.95, 0.999), step_before=0, sc=None):
    """siss_grad_norms_scale on host arrays: the block read back; the inputs must come back bit-identical"""
    n = len(gx)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    sc = sc or Scal(dev, step_before)
    launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob, max_norm, betas[0], betas[1], sc.partials.t, sc.blk.t)
    bx.check(T(gx), "gx after the norms"); ba.check(T(ga), "ga after the norms")
    return sc.read(n)


def f32_of(x):
    return float(f32(x))


# ================================================================ pass 1 and the scalar block
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", R.SIZES)
def test_norms_on_integers_are_exact(dev, n, mode):
    knob = 1e-2 if mode == 1 else 5.0
    gx, ga = R.int_pair(n, n)
    xx, aa, xa = R.int_sums(gx, ga)
    blk = norms(dev, gx, ga, mode, knob)
    assert blk[0] == f32(math.sqrt(xx)) and blk[1] == f32(math.sqrt(aa)) and blk[2] == f32(xa), (blk[:3], xx, aa, xa)
    ref = R.scalars_f64(float(xx), float(aa), float(xa), mode, knob, 1.0, 0.95, 0.999, 1)
    for k in ("scale", "pre_clip_norm", "clip_coef"):       # doubles from exact sums, rounded once: u (and 2^-20 of it for the doubles)
        assert abs(float(blk[R.NAMES[k]]) - ref[k]) <= U * (1 + 2.0 ** -20) * abs(ref[k]), (k, blk[R.NAMES[k]], ref[k])
    assert blk[6] == 1


@pytest.mark.parametrize("n", [1027, BIG])
def test_one_hot_probe_counts_every_element_once(dev, n):
    """gx = 3, ga = 5 at ONE index, zero elsewhere: norm_x = 3, norm_a = 5, dot = 15 exactly, at index 0, 3, the last vector element,
    the first tail element, n - 1, and the block seams (element 1023 | 1024; at the large size also 2048 blocks x 1024 elements, where
    the grid-stride loop begins its second pass)."""
    nv = n // 4 * 4
    pos = sorted({0, 3, nv - 1, nv, n - 1, 1023, 1024} | ({2048 * 1024 - 1, 2048 * 1024} if n == BIG else set()))
    gx, ga = torch.zeros(n + 2 * GUARD, device=dev), torch.zeros(n + 2 * GUARD, device=dev)
    sc = Scal(dev)
    for i in pos:
        gx[GUARD + i], ga[GUARD + i] = 3.0, 5.0
        launch("siss_grad_norms_scale", gx[GUARD:GUARD + n], ga[GUARD:GUARD + n], n, 2, 5.0, 1.0, 0.95, 0.999, sc.partials.t, sc.blk.t)
        blk = sc.read(n)
        assert (blk[0], blk[1], blk[2]) == (3.0, 5.0, 15.0), (i, blk[:3])
        gx[GUARD + i], ga[GUARD + i] = 0.0, 0.0
    assert blk[6] == len(pos)


def hold(blk, gx, ga, mode, knob, what, max_norm=1.0):
    worst = R.scalar_errors(blk, R.scalar_bounds(gx, ga, mode, knob, max_norm))
    print(f"[optimizer] {what}: error / allowed " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", R.SIZES)
def test_scalars_on_gaussian_data_within_the_a_priori_bounds(dev, n, mode):
    knob = 1e-2 if mode == 1 else 5.0
    gx, ga = R.gauss_pair(n, n + mode)
    hold(norms(dev, gx, ga, mode, knob), gx, ga, mode, knob, f"norms_scale n {n} mode {mode}")


@pytest.mark.parametrize("n", R.SIZES)
def test_near_cancelling_pair(dev, n):
    gx, ga = R.near_cancelling_pair(n, n + 3, 5.0)
    hold(norms(dev, gx, ga, 0, 5.0), gx, ga, 0, 5.0, f"norms_scale near-cancelling n {n}")


@pytest.mark.parametrize("n", R.SIZES)
def test_exactly_cancelling_pair_clamps_at_zero(dev, n):
    gx, ga, knob = R.cancelling_int_pair(n)
    blk = norms(dev, gx, ga, 0, knob)
    assert blk[3] == 2 and blk[4] == 0 and blk[5] == 1 and not np.isnan(blk).any(), blk


@pytest.mark.parametrize("n", R.SIZES)
def test_mode_1_scale_on_exact_ratios(dev, n):
    """eta = 1e-2.  <gx, ga> / |ga|^2 = 0.5: eta - 0.5 < 0, s compares equal to 0 (its sign is not asserted).  Ratio -0.3: s = -(eta + 0.3),
    a double from exact sums, rounded once: bitwise."""
    blk = norms(dev, *R.ratio_pair(n, 5), 1, 1e-2)
    assert blk[3] == 0, blk[3]
    blk = norms(dev, *R.ratio_pair(n, -3), 1, 1e-2)
    assert blk[3] == f32(-(f32_of(1e-2) + 0.3)), blk[3]


# ---------------------------------------------------------------- the step counter and the bias corrections
@pytest.mark.parametrize("b1,b2", R.BETAS)
@pytest.mark.parametrize("k", [1, 2, 3, 6, 31, 100, 1000, 100_000])
def test_step_counter_and_bias_corrections(dev, k, b1, b2):
    gx, ga = R.int_pair(5, 5)
    blk = norms(dev, gx, ga, 2, 5.0, betas=(b1, b2), step_before=k - 1)
    e1, e2 = R.bias_correction_errors(blk, b1, b2, k)
    print(f"[optimizer] betas {b1, b2} step {k}: |bc1 - f64| / (u bc1) {e1:.2f}, |bc2_sqrt - f64| / (u bc2_sqrt) {e2:.2f} (allowed 2)")
    assert blk[6] == k
    assert e1 <= 2.0 and e2 <= 2.0, (k, e1, e2)


# ================================================================ pass 2, bitwise
class State:
    """p, m, v (+ optional shadow, g_out) in sentinel buffers, and the host images they are compared with"""

    def __init__(self, dev, p, m, v, shadow=True, gout=True):
        n = len(p)
        self.n, self.dev = n, dev
        self.p, self.m, self.v = (Flat(n, F32, dev, body=t) for t in (p, m, v))
        self.shadow = Flat(n, BF, dev) if shadow else None
        self.gout = Flat(n, F32, dev) if gout else None

    def slices(self, lo, hi):
        return (self.p.t[lo:hi], self.m.t[lo:hi], self.v.t[lo:hi], None if self.shadow is None else self.shadow.t[lo:hi],
                None if self.gout is None else self.gout.t[lo:hi])

    def adamw(self, bx, ba, blk_dev, hp, lo=0, hi=None):
        hi = self.n if hi is None else hi
        p, m, v, sh, go = self.slices(lo, hi)
        launch("siss_recombine_clip_adamw", bx.t[lo:hi], ba.t[lo:hi], p, m, v, sh, go, hi - lo, *(float(h) for h in hp), blk_dev)


DECAY_FORM = {}


def restate(gx, ga, p, m, v, blk, hp, got_p):
    """the f32 restatement; `decay = 1.f - lr * wd` is taken with two roundings, and as the fused value ONLY where the two differ and
    the device's p is bitwise the fused one (recorded in DECAY_FORM and printed)"""
    out = R.adamw_f32(gx, ga, p, m, v, blk, hp)
    form = "two roundings"
    two, fused = R.decay_two_roundings(hp), R.decay_fused(hp)
    if two != fused and not np.array_equal(out[0].view(np.int32), got_p.view(np.int32)):
        alt = R.adamw_f32(gx, ga, p, m, v, blk, hp, decay=fused)
        if np.array_equal(alt[0].view(np.int32), got_p.view(np.int32)):
            out, form = alt, "fused"
    DECAY_FORM[tuple(float(h) for h in hp)] = form if two != fused else "two roundings == fused"
    return out


def three_steps(dev, n, hp, shadow, gout):
    """mode 0, mode 1, then mode 2 with ga = 0, the state carried"""
    rng = np.random.default_rng(n)
    p, m, v = rng.standard_normal(n).astype(f32), np.zeros(n, f32), np.zeros(n, f32)
    st = State(dev, p, m, v, shadow, gout)
    sc = Scal(dev)
    for step, (mode, knob) in enumerate([(0, 5.0), (1, 1e-2), (2, 5.0)], 1):
        gx, ga = R.gauss_pair(n, 100 * step + n)
        if mode == 2:
            ga[:] = 0
        bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
        launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob, 1.0, float(hp[1]), float(hp[2]), sc.partials.t, sc.blk.t)
        blk = sc.read(n)
        assert blk[6] == step
        if mode == 2:
            assert blk[3] == 0 and blk[4] == blk[0], blk            # s = 0 (not inf), pre_clip_norm == norm_x
        st.adamw(bx, ba, sc.blk.t, hp)
        got_p = st.p.np()
        p, m, v, g = restate(gx, ga, p, m, v, blk, hp, got_p)
        what = f"n {n} step {step} mode {mode}"
        assert np.isfinite(got_p).all(), what
        st.p.check(T(p), f"p, {what}"); st.m.check(T(m), f"m, {what}"); st.v.check(T(v), f"v, {what}")
        if gout:
            st.gout.check(T(g), f"g_out, {what}")
        if shadow:
            st.shadow.check(R.bf16(p), f"shadow, {what}")
            same(st.shadow.t.cpu(), T(got_p).to(BF), f"shadow against p.to(bfloat16), {what}")
        bx.check(T(gx), f"gx, {what}"); ba.check(T(ga), f"ga, {what}")
        same(T(sc.read(n)), T(blk), "the scalar block after pass 2")


@pytest.mark.parametrize("name", list(R.HYPER))
@pytest.mark.parametrize("n", R.SIZES)
def test_adamw_pass_is_bitwise_the_f32_restatement(dev, n, name):
    hp = R.hyper(*R.HYPER[name])
    three_steps(dev, n, hp, True, True)
    print(f"[optimizer] {name} n {n}: decay = 1.f - lr * wd came out as: {DECAY_FORM[tuple(float(h) for h in hp)]}")


@pytest.mark.parametrize("shadow,gout", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("n", SMALL)
def test_adamw_pass_with_shadow_and_g_out_absent(dev, n, shadow, gout):
    three_steps(dev, n, R.hyper(*R.HYPER["lr5e-3"]), shadow, gout)


# ================================================================ pass 2, precision of the step
@pytest.mark.parametrize("zero_init", [True, False], ids=["p0=0", "p0~N(0,1)"])
@pytest.mark.parametrize("name", ["lr5e-3", "sd"])
@pytest.mark.parametrize("k", R.STEPS)
def test_step_precision_within_4x_torch_f32(dev, k, name, zero_init):
    """At step k (counter preset, m and v from k - 1 f64 steps on Gaussian gradients): max |p - p_f64| / max |p_f64 - p0|, and m, v
    relative to their largest value, against 4 x the same figures of torch's f32 CPU AdamW(foreach=False) fed the same f32 gradient
    and the f32-rounded hyper-parameters.  Mode 2 with ga = 0 and no clipping: g is gx itself."""
    hp = R.hyper(*R.HYPER[name])
    g, p0, m, v = R.precision_case(k, hp, zero_init)
    z = np.zeros_like(g)
    (pr, mr, vr, _), _ = R.step_f64(g, z, p0, m, v, k, hp, 2, 5.0, 1e30)
    e_ref = R.update_errors(R.torch_adamw(g, p0, m, v, k, hp, torch.float32), (pr, mr, vr), p0)
    n = len(g)
    st, sc = State(dev, p0, m, v, False, True), Scal(dev, k - 1)
    bx, ba = Flat(n, F32, dev, body=g), Flat(n, F32, dev, body=z)
    launch("siss_grad_norms_scale", bx.t, ba.t, n, 2, 5.0, 1e30, float(hp[1]), float(hp[2]), sc.partials.t, sc.blk.t)
    blk = sc.read(n)
    assert blk[6] == k and blk[3] == 0 and blk[5] == 1
    st.adamw(bx, ba, sc.blk.t, hp)
    st.gout.check(T(g), "g_out is gx")
    e = R.update_errors((st.p.np(), st.m.np(), st.v.np()), (pr, mr, vr), p0)
    print(f"[optimizer] {name} {'p0=0' if zero_init else 'p0~N'} step {k}: error (torch f32 e_ref): p {e[0]:.2e} ({e_ref[0]:.2e}) = {e[0] / e_ref[0]:.2f} x, "
          f"m {e[1]:.2e} ({e_ref[1]:.2e}) = {e[1] / e_ref[1]:.2f} x, v {e[2]:.2e} ({e_ref[2]:.2e}) = {e[2] / e_ref[2]:.2f} x; allowed 4 x")
    st.p.guards("p"); st.m.guards("m"); st.v.guards("v")
    assert all(e[i] <= 4 * e_ref[i] for i in range(3)), (k, e, e_ref)


# ================================================================ the sharded halves
def shard_bounds(n, k):
    """k shards of [0, n): lengths multiples of 4, the last one takes the tail"""
    per = max(n // 4 // k, 1) * 4
    cuts = [min(i * per, n // 4 * 4) for i in range(k)] + [n]
    assert all(c % 4 == 0 for c in cuts[:-1]) and all(b > a for a, b in zip(cuts, cuts[1:])), cuts
    return cuts


SHARDS = [(5, 1), (1027, 1), (1027, 2), (1027, 8), (100_003, 300), (BIG, 2)]


@pytest.mark.parametrize("data", ["integers", "gaussian"])
@pytest.mark.parametrize("n,k", SHARDS)
def test_sharded_halves(dev, n, k, data):
    """siss_grad_norm_partials per shard -> [k, 3] rows -> siss_grad_scalars; then siss_recombine_clip_adamw shard by shard with a COPY
    of the block: bitwise the whole-buffer update, and nothing outside [lo, hi) changes at any point."""
    hp = R.hyper(*R.HYPER["lr5e-3"])
    gx, ga = R.int_pair(n, n) if data == "integers" else R.gauss_pair(n, n + 9)
    rng = np.random.default_rng(n + k)
    p, m, v = rng.standard_normal(n).astype(f32), (0.01 * rng.standard_normal(n)).astype(f32), (1e-4 * rng.random(n)).astype(f32)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    whole, sc = State(dev, p, m, v), Scal(dev, 4)
    launch("siss_grad_norms_scale", bx.t, ba.t, n, 0, 5.0, 1.0, float(hp[1]), float(hp[2]), sc.partials.t, sc.blk.t)
    blk = sc.read(n)
    whole.adamw(bx, ba, sc.blk.t, hp)
    # the halves
    cuts = shard_bounds(n, k)
    rows = Flat(3 * k, F64, dev, fill=-5.0)
    part = Flat(3 * R.MAX_BLOCKS, F64, dev, fill=-5.0)
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        nblk = ctypes.c_int(-1)
        launch("siss_grad_norm_partials", bx.t[lo:hi], ba.t[lo:hi], hi - lo, part.t, ctypes.byref(nblk))
        assert nblk.value == R.grid_for(hi - lo) == min(max(math.ceil((hi - lo) // 4 / 256), 1), 2048), (lo, hi, nblk.value)
        rows.t.view(k, 3)[i] = part.t.view(-1, 3)[:nblk.value].sum(0)
    part.guards("partials")
    sc2 = Scal(dev, 4)
    launch("siss_grad_scalars", rows.t, k, 0, 5.0, 1.0, float(hp[1]), float(hp[2]), sc2.blk.t)
    blk2 = sc2.read()
    rows.guards("the [k, 3] rows")
    if data == "integers":
        same(T(blk2), T(blk), f"scalar block of {k} shards against the whole buffer")
    else:
        hold(blk2, gx, ga, 0, 5.0, f"grad_scalars n {n} shards {k}")
    bx.check(T(gx), "gx"); ba.check(T(ga), "ga")
    # pass 2 on the shards, with a copy of the WHOLE-buffer block (so that the element-wise pass has the same scalars)
    copy = Flat(16, F32, dev, body=blk)
    sh = State(dev, p, m, v)
    bufs = lambda s: [b for b in (s.p, s.m, s.v, s.shadow, s.gout)]
    expect = [b.d.clone() for b in bufs(sh)]
    for lo, hi in zip(cuts, cuts[1:]):
        sh.adamw(bx, ba, copy.t, hp, lo, hi)
        for e, b, w in zip(expect, bufs(sh), bufs(whole)):
            e[GUARD + lo:GUARD + hi] = w.t[lo:hi]
            assert torch.equal(bits(b.d), bits(e)), f"shard [{lo}, {hi}) of n {n}: something outside it changed, or it differs from the whole-buffer update"
    for b, w in zip(bufs(sh), bufs(whole)):
        same(b.d.cpu(), w.d.cpu(), "the concatenated shards against the whole-buffer update")
    copy.check(T(blk), "the copied block")


# ================================================================ casts
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,
                     0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345], np.uint32)


@pytest.mark.parametrize("n", R.SIZES)
def test_cast_and_copy(dev, n):
    x = (np.random.default_rng(n).standard_normal(n) * 3).astype(f32)
    src = Flat(n, F32, dev, body=x)
    dst = Flat(n, BF, dev)
    launch("siss_cast_f32_bf16", src.t, dst.t, n)
    dst.check(R.bf16(x), f"cast_f32_bf16 n {n}")
    same(dst.t.cpu(), T(x).to(BF), "cast_f32_bf16 against torch's .to(bfloat16)")
    cp = Flat(n, F32, dev)
    launch("siss_cast_f32_bf16", src.t, cp.t, n, f32_mode=True)          # -> siss_copy_f32
    cp.check(T(x), f"copy_f32 n {n}")
    src.check(T(x), "the source")


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4])
def test_cast_and_copy_special_values(dev, shift):
    """+-0, denormals, exact ties both ways (also among the denormals), just above / below a tie, the largest finite f32 (which becomes
    inf), +-inf; NaNs (one whose payload lies in the low 16 bits only) stay NaNs.  `shift` moves the vector through the 16-byte group
    and into the tail."""
    sp = np.concatenate([np.zeros(shift, np.uint32), SPECIALS]).view(f32)
    n, nn = len(sp), 3
    src, dst, cp = Flat(n, F32, dev, body=T(sp)), Flat(n, BF, dev), Flat(n, F32, dev)
    same(src.t.cpu(), T(sp), "the specials reach the device bit for bit")
    launch("siss_cast_f32_bf16", src.t, dst.t, n)
    got = dst.t.cpu()
    same(got[:-nn], R.bf16(sp)[:-nn], "cast_f32_bf16 of the special values")
    assert R.bf16_bits(sp)[shift + 12] == 0x7F80 and bool(got[-nn:].float().isnan().all()), got[-nn:]
    dst.guards("cast_f32_bf16")
    launch("siss_cast_f32_bf16", src.t, cp.t, n, f32_mode=True)
    cp.check(T(sp), "copy_f32 of the special values")


# ================================================================ weight copies
WSHAPES = [(9, 72, 136), (1, 320, 768), (9, 12, 20), (1, 5, 64), (9, 64, 3), (1, 128, 128), (1, 1, 1), (9, 33, 31), (1, 64, 3)]


def test_dgrad_weight_copies(dev):
    rec, total, tiles = R.job_table(WSHAPES)
    master = np.random.default_rng(5).standard_normal(total).astype(f32)
    want = np.full(total, SENT, f32)                                    # the alignment gaps between weights keep the sentinel
    for (t, co, ci), r in zip(WSHAPES, rec):
        o = int(r["src"])
        want[o:o + t * co * ci] = R.dgrad_weight(master[o:o + t * co * ci].reshape(t, co, ci)).reshape(-1)
        one = Buf((t, ci, co), BF, dev)
        launch("siss_conv_weight_dgrad_layout", T(master[o:o + t * co * ci]).to(dev), one.t, t, co, ci)
        one.check(R.bf16(want[o:o + t * co * ci]), f"conv_weight_dgrad_layout {t, co, ci}")
    jobs = torch.from_numpy(rec.view(np.uint8)).to(dev)
    src = Flat(total, F32, dev, body=master)
    out = Flat(total, BF, dev)
    launch("siss_conv_weight_dgrad_multi", src.t, out.t, jobs, len(WSHAPES), tiles)
    out.check(R.bf16(want), "conv_weight_dgrad_multi (f32 master)")
    out32 = Flat(total, F32, dev)
    launch("siss_conv_weight_dgrad_multi_bf16", src.t, out32.t, jobs, len(WSHAPES), tiles, f32_mode=True)      # -> siss_conv_weight_dgrad_multi_f32
    out32.check(T(want), "conv_weight_dgrad_multi_f32")
    src.check(T(master), "the master")


# ================================================================ sub-pixel upsample: phase weights and the fold
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("Co,Ci", [(1, 1), (3, 5), (32, 96), (272, 272)])
def test_upsample_phase_weights(dev, Co, Ci, dt):
    """16 x 272^2 > 4096 blocks x 256 threads: the grid-stride loop.  wf bitwise the f32 sums (rounded once in the bf16 form), wd its
    per-panel transpose."""
    w = np.random.default_rng(Co + Ci).standard_normal((9, Co, Ci)).astype(f32)
    ref = R.phase_weights(w)
    dtype = BF if dt == "bf16" else F32
    wf, wd = Flat(16 * Co * Ci, dtype, dev), Flat(16 * Co * Ci, dtype, dev)
    src = Flat(9 * Co * Ci, F32, dev, body=w.reshape(-1))
    launch("siss_upsample_phase_weights", src.t, wf.t, wd.t, Co, Ci, f32_mode=(dt == "f32"))
    conv = R.bf16 if dt == "bf16" else T
    wf.check(conv(ref.reshape(-1)), f"phase weights wf {Co, Ci} {dt}")
    wd.check(conv(np.ascontiguousarray(ref.transpose(0, 2, 1)).reshape(-1)), f"phase weights wd {Co, Ci} {dt}")
    src.check(T(w.reshape(-1)), "the master")


@pytest.mark.parametrize("data", ["gaussian", "integers"])
@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("Co,Ci", [(1, 1), (3, 5), (32, 96), (272, 272), (352, 352)])
def test_upsample_phase_wgrad_fold(dev, Co, Ci, nsets, data):
    """9 x 352^2 > 4096 x 256: the grid-stride loop.  set_stride = 9 Co Ci + 20 with sentinel between the sets; dW pre-filled (the
    launcher ADDS); bitwise acc = ((d0 + d1) + d2) + d3, dW += acc on Gaussian data, exact on integers."""
    per, stride = Co * Ci, 9 * Co * Ci + 20
    rng = np.random.default_rng(Co + Ci + nsets)
    if data == "integers":
        d4, pre = rng.integers(-8, 9, (nsets, 16, per)).astype(f32), rng.integers(-8, 9, (nsets, 9, per)).astype(f32)
    else:
        d4, pre = rng.standard_normal((nsets, 16, per)).astype(f32), rng.standard_normal((nsets, 9, per)).astype(f32)
    body = np.full((nsets, stride), SENT, f32)
    body[:, :9 * per] = pre.reshape(nsets, -1)
    want = body.copy()
    for s in range(nsets):
        want[s, :9 * per] = R.phase_fold(d4[s], pre[s]).reshape(-1)
        if data == "integers":                                            # ... where the restatement is the int64 sum
            i4 = d4[s].astype(np.int64)
            for k9 in range(9):
                acc = sum(i4[pl * 4 + R.phase_tap(k9 // 3, pl >> 1) * 2 + R.phase_tap(k9 % 3, pl & 1)] for pl in range(4))
                assert np.array_equal(want[s, k9 * per:(k9 + 1) * per].astype(np.int64), pre[s, k9].astype(np.int64) + acc)
    src = Flat(nsets * 16 * per, F32, dev, body=d4.reshape(-1))
    dW = Flat(nsets * stride, F32, dev, body=body.reshape(-1))
    launch("siss_upsample_phase_wgrad_fold", src.t, dW.t, stride, nsets, Co, Ci)
    dW.check(T(want.reshape(-1)), f"phase_wgrad_fold {Co, Ci} x {nsets} sets, {data}")
    src.check(T(d4.reshape(-1)), "the phase-tap gradients")


# ================================================================ siss_zero_ranges
def zero_tables():
    rng = np.random.default_rng(6)
    t = {"n = 1": ([3], [5], 16), "single granules": ([1, 4, 9, 30], [1, 1, 1, 1], 40),
         "adjacent": ([2, 5, 6, 10, 20], [3, 1, 4, 10, 12], 32), "first and last granule": ([0, 63], [1, 1], 64)}
    lens = rng.integers(1, 6, 1000)
    gaps = rng.integers(0, 4, 1000)                                       # 0: adjacent stretches among them
    starts = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    order = rng.permutation(1000)                                         # the table need not be sorted by address
    t["1000 stretches"] = (starts[order].tolist(), lens[order].tolist(), int(starts[-1] + lens[-1]) + 3)
    big = 8192 * 256 + 4099                                               # more granules than 8192 blocks x 256 threads: 33.6 MB zeroed, 40 MB buffer
    t["beyond the grid"] = ([5, big // 2 + 1000, big + 200_000], [big // 2, big - big // 2 - 7, 7], 2_500_000)
    return t


@pytest.mark.parametrize("name", list(zero_tables()))
def test_zero_ranges(dev, name):
    """Buffer pre-filled with a non-zero bit pattern; exactly the listed 16-byte granules become +0.0 and every other byte stays."""
    starts, lens, granules = zero_tables()[name]
    nf = 4 * granules
    pattern = 0x7F4D_2C0B                                                 # a NaN pattern: a "zero" written as x * 0 would show
    init = torch.full((nf + 2 * GUARD,), pattern, dtype=torch.int32)
    buf = init.to(dev)
    tab, total = R.zero_table(starts, lens)
    if name == "beyond the grid":
        assert total > 8192 * 256
    launch("siss_zero_ranges", buf[GUARD:GUARD + nf].view(F32), torch.from_numpy(tab).to(dev), len(starts), total)
    want = init.clone()
    want[GUARD:GUARD + nf][torch.from_numpy(R.zero_mask(nf, starts, lens))] = 0
    got = buf.cpu()
    ne = got != want
    assert not bool(ne.any()), f"zero_ranges '{name}': {int(ne.sum())} ints differ, the first at float {int(ne.nonzero()[0]) - GUARD}"


# ================================================================ refusals
def test_refusals_write_nothing(dev):
    n = 1027
    gx, ga = R.gauss_pair(n, 1)
    hp = [float(h) for h in R.hyper(*R.HYPER["lr5e-3"])]
    bx, ba = Flat(n + 4, F32, dev, body=np.append(gx, [0] * 4)), Flat(n + 4, F32, dev, body=np.append(ga, [0] * 4))
    sc = Scal(dev, 3)
    st = State(dev, gx, ga, np.abs(gx))
    nblk = ctypes.c_int(-1)
    norms_args = lambda x, a, nn, mode: ("siss_grad_norms_scale", x, a, nn, mode, 5.0, 1.0, 0.95, 0.999, sc.partials.t, sc.blk.t)
    adamw_args = lambda x, p, nn: ("siss_recombine_clip_adamw", x, ba.t[:n], p, st.m.t, st.v.t, st.shadow.t, st.gout.t, nn, *hp, sc.blk.t)
    for args in (norms_args(bx.t[1:n + 1], ba.t[:n], n, 0), norms_args(bx.t[:n], ba.t[1:n + 1], n, 0),      # 4 bytes off alignment
                 norms_args(bx.t[:n], ba.t[:n], 0, 0), norms_args(bx.t[:n], ba.t[:n], n, 3), norms_args(bx.t[:n], ba.t[:n], n, -1),
                 ("siss_grad_norm_partials", bx.t[1:n + 1], ba.t[:n], n, sc.partials.t, ctypes.byref(nblk)),
                 ("siss_grad_norm_partials", bx.t[:n], ba.t[:n], 0, sc.partials.t, ctypes.byref(nblk)),
                 ("siss_grad_scalars", sc.partials.t, 0, 0, 5.0, 1.0, 0.95, 0.999, sc.blk.t),
                 ("siss_grad_scalars", sc.partials.t, 1, 3, 5.0, 1.0, 0.95, 0.999, sc.blk.t),
                 adamw_args(bx.t[1:n + 1], st.p.t, n), adamw_args(bx.t[:n], st.p.t, 0), adamw_args(bx.t[:n - 1], st.p.t[1:], n - 1),
                 ("siss_cast_f32_bf16", bx.t[1:n + 1], st.shadow.t, n), ("siss_cast_f32_bf16", bx.t[:n], st.shadow.t, 0),
                 ("siss_cast_f32_bf16", bx.t[:n], st.shadow.t[1:], n - 1),                                   # a bf16 target 2 bytes off 8
                 ("siss_zero_ranges", st.gout.t[1:], sc.partials.t, 1, 1), ("siss_zero_ranges", st.gout.t, sc.partials.t, 0, 1),
                 ("siss_upsample_phase_weights", bx.t, st.shadow.t, st.shadow.t, 0, 1),
                 ("siss_upsample_phase_wgrad_fold", bx.t, st.gout.t, 9, 0, 1, 1),
                 ("siss_conv_weight_dgrad_layout", bx.t, st.shadow.t, 0, 1, 1)):
        refused(*args)
    assert nblk.value == -1
    same(sc.blk.d.cpu(), sc.blk.flat, "the scalar block after the refusals")
    same(sc.partials.d.cpu(), sc.partials.flat, "the partial sums after the refusals")
    for b in (st.p, st.m, st.v, st.shadow, st.gout, bx, ba):
        same(b.d.cpu(), b.flat, "a buffer after the refusals")

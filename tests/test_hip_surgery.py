"""csrc/surgery.hip and what stands on it (siss_amd/surgery.py, FlatAdamW.launch(surgery=...), SISSStepper(surgery=...),
deletion.surgery), on the GPU.

* The two entry points called DIRECTLY against tests/surgery_ref.py, every buffer between sentinel guards (tests/test_hip_optimizer.py's
  Flat / Scal).  Group lengths from {4, 64, C - 4, C, C + 4, 2C + 8, 3C} (C = siss_surgery_chunk()), one buffer with n % 4 = 3, and one
  of 4.2 M floats in 700 groups at C = 1024 (4,600 jobs: the persistent loop wraps behind 2048 blocks).  Conflicting, opposed and
  independent groups mixed, one group with x = 0, one with a = 0, one with xa exactly 0; an integer-valued case whose sums are exact.
  BITWISE: the job rows, the group sums, the coefficient table, p / m / v / shadow / g_out.  The scalar slots: the f64 expressions are
  restated operation for operation from the device's own (bitwise checked) group sums, so slots 0-5 and 12-15 are held to one f32
  rounding of a double (u (1 + 2^-20), the bound tests/test_hip_optimizer.py holds the block to on exact sums), bc1 / bc2_sqrt to 2u
  as there; slots 7, 10, 11, the guards and the slab rows beyond the job count keep their fill.
* Identity by construction: with no conflicting group the plain siss_recombine_clip_adamw on the surgery's scalar block equals the
  surgery update (torch.equal on p, m, v, shadow).  Negative control: one conflicting group moves exactly that group's stretch.
* The results do not depend on the grid (siss_surgery_test_config caps it at 3 blocks).  The refusals leave every buffer unchanged.
* Two optimizer steps of the tiny f32 engine, SISS and double_forward_with_neg_del, mutual / tensor, against the fp32 oracle's
  gradients pushed through the f64 definition, at the bounds of tests/test_hip_f32_mode.py (scalars 2e-4, masked update cosine
  0.9999); surgery_conflicts >= 1 at both steps is asserted; the definition WITHOUT surgery misses the bounds at step 2.
* bf16 engine: a captured surgery step replays to the eager step's bits; a step without the key calls no new entry point; the whole
  step equals FlatAdamW's surgery pair on the gradients that very step produced.
* One rank with forced collectives (tests/rccl_surgery_worker.py); delete_celeb and delete_sd through main.main.

The backward pass of the f32 engine is not bitwise repeatable (tests/test_hip_ewc.py's docstring), so nothing here compares two f32 runs
bit for bit.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as O
import surgery_ref as R
from test_hip_optimizer import BF, F32, F64, Flat, Scal, State, T, launch, refused
from test_hip_small_kernels import same
from test_hip_surface import KW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
U = R.U
HP = O.hyper(*O.HYPER["sd"])
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)
EXTRA_ROWS = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def default_config():
    """every test starts and ends on the library's default chunk length and grid cap"""
    from siss_amd import lib
    assert lib.query("siss_surgery_test_config", 0, 0) == 0
    yield
    assert lib.query("siss_surgery_test_config", 0, 0) == 0


def chunk():
    from siss_amd import lib
    return int(lib.query("siss_surgery_chunk"))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def np_bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


class Pair:
    """One gradient pair on the device with its plan, and every slab the two entry points write -- all between guards"""

    def __init__(self, dev, gx, ga, off, step_before=0):
        self.dev, self.gx, self.ga, self.off, self.n, self.C = dev, gx, ga, list(off), len(gx), chunk()
        starts, groups, self.first = R.plan(self.off, self.C)
        self.J, self.G = len(starts), len(off) - 1
        self.bx, self.ba = Flat(self.n, F32, dev, body=gx), Flat(self.n, F32, dev, body=ga)
        self.groups_host = torch.tensor(self.off, dtype=torch.int64)
        self.plan_host = torch.tensor(starts + groups + self.first + self.off, dtype=torch.int64)
        self.plan = self.plan_host.to(dev)
        self.rows = Flat(3 * (self.J + EXTRA_ROWS), F64, dev, fill=-5.0)
        self.gs = Flat(3 * self.G, F64, dev, fill=-5.0)
        self.coef = Flat(2 * self.G, F32, dev)
        self.sc = Scal(dev, step_before)
        self.step_before = step_before

    def pass1_args(self, mode, nmode=0, knob=5.0, max_norm=1.0):
        return (self.bx.t, self.ba.t, self.n, self.groups_host, self.G, self.plan, self.J, R.MODES.index(mode), nmode, knob, max_norm,
                float(HP[1]), float(HP[2]), self.rows.t, self.gs.t, self.coef.t, self.sc.blk.t)

    def pass1(self, mode, **kw):
        launch("siss_grad_norms_scale_surgery", *self.pass1_args(mode, **kw))
        self.bx.check(T(self.gx), "gx after pass 1"); self.ba.check(T(self.ga), "ga after pass 1")
        assert torch.equal(self.plan.cpu(), self.plan_host), "the plan was written to"

    def pass2_args(self, st, hp=HP):
        p, m, v, sh, go = st.slices(0, self.n)
        return (self.bx.t, self.ba.t, p, m, v, sh, go, self.n, self.groups_host, self.G, self.plan, self.J, self.coef.t,
                *(float(h) for h in hp), self.sc.blk.t)

    def pass2(self, st, hp=HP):
        launch("siss_recombine_clip_adamw_surgery", *self.pass2_args(st, hp))
        self.bx.check(T(self.gx), "gx after pass 2"); self.ba.check(T(self.ga), "ga after pass 2")

    def block(self):
        """the 16 floats; slots 7, 10, 11 and the guards keep their fill"""
        blk = self.sc.blk.np().copy()
        keep = self.sc.init.copy()
        keep[R.WRITTEN] = blk[R.WRITTEN]
        self.sc.blk.check(T(keep), "scalar block: slots 7, 10, 11 and the guards")
        return blk

    def check_pass1(self, mode, nmode=0, knob=5.0, max_norm=1.0, what=""):
        """rows, group sums, coefficients bitwise; the scalar slots; returns (block, coef) as read from the device"""
        rows = R.job_rows(self.gx, self.ga, self.off, self.C)
        body = np.full(3 * (self.J + EXTRA_ROWS), -5.0, f64)
        body[:3 * self.J] = rows.reshape(-1)
        self.rows.check(T(body), f"{what}: the job rows (and the slab beyond the job count)")
        S = R.group_sums(rows, self.first)
        self.gs.check(T(S.reshape(-1)), f"{what}: the group sums")
        blk_ref, coef_ref = R.scalars_coef(S, mode, nmode, knob, max_norm, HP[1], HP[2], self.step_before)
        self.coef.check(T(coef_ref.reshape(-1)), f"{what}: the coefficient table")
        blk = self.block()
        exact = 0
        for i in (0, 1, 2, 3, 4, 5, 12, 13, 14, 15):
            r, g = float(blk_ref[i]), float(blk[i])
            assert (np.isnan(r) and np.isnan(g)) or abs(g - r) <= U * (1 + 2.0 ** -20) * abs(r), (what, "slot", i, g, r)
            exact += int(blk[i] == blk_ref[i] or (np.isnan(r) and np.isnan(g)))
        assert blk[6] == self.step_before + 1
        for i in (8, 9):
            assert abs(float(blk[i]) - float(blk_ref[i])) <= 2 * U * abs(float(blk_ref[i])), (what, "slot", i)
        print(f"[surgery] {what}: {self.J} jobs, {self.G} groups, {int(blk[12])} conflict; {exact} of 10 restated slots bitwise")
        return blk, self.coef.np().reshape(-1, 2).copy(), S


def restate_update(gx, ga, p, m, v, blk, coef, off, hp, got_p):
    """tests/test_hip_optimizer.py's `restate`: decay = 1.f - lr * wd with two roundings, the fused value only where the two differ and
    the device's p is bitwise the fused one"""
    out = R.update_f32(gx, ga, p, m, v, blk, coef, off, hp)
    two, fused = O.decay_two_roundings(hp), O.decay_fused(hp)
    if two != fused and not np_bits_equal(out[0], got_p):
        alt = R.update_f32(gx, ga, p, m, v, blk, coef, off, hp, decay=fused)
        if np_bits_equal(alt[0], got_p):
            return alt
    return out


def state_for(dev, n, seed, shadow=True, gout=True):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(f32)
    m, v = O.warm_state(n, 3, HP, seed=seed + 1)
    return (p, m, v), State(dev, p, m, v, shadow, gout)


def check_update(pair, st, host, blk, coef, what):
    p, m, v = host
    got_p = st.p.np().copy()
    rp, rm, rv, rg = restate_update(pair.gx, pair.ga, p, m, v, blk, coef, pair.off, HP, got_p)
    st.p.check(T(rp), what + ": p"); st.m.check(T(rm), what + ": m"); st.v.check(T(rv), what + ": v")
    if st.gout is not None:
        st.gout.check(T(rg), what + ": g_out")
    if st.shadow is not None:
        st.shadow.check(O.bf16(rp), what + ": shadow")
    return rp, rm, rv, rg


def lengths_of(name, C):
    return {"seams": [4, 64, C - 4, C, C + 4, 2 * C + 8, 3 * C, 64, 4, 260],
            "tail3": [64, C + 4, 4, 8, 128, 2 * C + 8 + 3]}[name]


# ================================================================ 1. the two passes against the restatement
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", ["seams", "tail3"])
def test_both_passes_are_bitwise_the_restatement(dev, shape, mode):
    gx, ga, off = R.case(lengths_of(shape, chunk()), 17 + len(shape))
    assert (off[-1] % 4 == 3) == (shape == "tail3")
    pair = Pair(dev, gx, ga, off, step_before=2)
    pair.pass1(mode)
    blk, coef, S = pair.check_pass1(mode, what=f"{shape} / {mode}")
    phi = R.conflicts(S)
    assert 2 <= sum(phi) < len(phi) and blk[12] == sum(phi), "the case mixes conflicting and quiet groups"
    assert S[1, 0] == 0 and S[2, 1] == 0 and S[4, 2] == 0 and S[4, 0] > 0 and not (phi[1] or phi[2] or phi[4]), "x = 0, a = 0, xa = 0"
    assert (blk[14] > 0) == (mode != "keep") and (blk[15] > 0) == (mode != "forget") and 0 < abs(blk[13]) < 1
    quiet = [g for g, f in enumerate(phi) if not f]
    assert (coef[quiet, 0] == 1).all() and (coef[quiet, 1] == blk[3]).all(), "a quiet group has exactly cx = 1.0f, ca = (float)s"
    host, st = state_for(dev, off[-1], 3)
    pair.pass2(st)
    check_update(pair, st, host, blk, coef, f"{shape} / {mode}")
    pair.block()                                               # (pass 2 writes no slot)


@pytest.mark.parametrize("mode", R.MODES)
def test_integer_valued_pair_has_exact_sums(dev, mode):
    C = chunk()
    gx, ga, off = R.case([4, 64, C - 4, C + 4, 260, 2 * C + 8 + 3], 5, integers=True)
    pair = Pair(dev, gx, ga, off)
    pair.pass1(mode, nmode=2)
    blk, coef, S = pair.check_pass1(mode, nmode=2, what=f"integers / {mode}")
    x, a = gx.astype(np.int64), ga.astype(np.int64)
    exact = np.array([[(x[lo:hi] ** 2).sum(), (a[lo:hi] ** 2).sum(), (x[lo:hi] * a[lo:hi]).sum()] for lo, hi in zip(off, off[1:])])
    assert np.array_equal(S, exact.astype(f64)), "integer sums are exact"
    assert blk[0] == f32(np.sqrt(f64(exact[:, 0].sum()))) and blk[1] == f32(np.sqrt(f64(exact[:, 1].sum()))) and blk[2] == f32(exact[:, 2].sum())
    assert blk[12] == sum(int(xa > 0) for xa in exact[:, 2])
    host, st = state_for(dev, off[-1], 8, shadow=False)
    pair.pass2(st)
    check_update(pair, st, host, blk, coef, f"integers / {mode}")


def test_an_all_zero_forget_set_under_the_inf_guard(dev):
    """mode 2: s = 0 where it would be inf; nothing conflicts, nothing is NaN, the update is the keep gradient's"""
    gx, _, off = R.case([64, 260, 1024 + 8], 2)
    ga = np.zeros_like(gx)
    pair = Pair(dev, gx, ga, off)
    pair.pass1("mutual", nmode=2)
    blk, coef, _ = pair.check_pass1("mutual", nmode=2, what="ga = 0, inf guard")
    assert blk[3] == 0 and blk[12] == 0 and blk[13] == 0 and blk[14] == 0 and blk[15] == 0 and not np.isnan(blk).any()
    assert (coef == np.array([1, 0], f32)).all()
    host, st = state_for(dev, off[-1], 4)
    pair.pass2(st)
    check_update(pair, st, host, blk, coef, "ga = 0, inf guard")


def test_a_large_buffer_whose_jobs_outnumber_the_grid(dev):
    """4.2 M floats in 700 groups at C = 1024: 4,600 jobs behind at most 2048 blocks, a tail of 3"""
    from siss_amd import lib
    assert lib.query("siss_surgery_test_config", 1024, 0) == 0 and chunk() == 1024
    lengths = [4, 64, 1020, 1024, 1028, 2056, 36868] * 100
    lengths[-1] += 3
    gx, ga, off = R.case(lengths, 23)
    pair = Pair(dev, gx, ga, off, step_before=9)
    assert pair.G == 700 and pair.J == 4600 > O.MAX_BLOCKS and off[-1] % 4 == 3 and off[-1] > 4_200_000
    pair.pass1("mutual")
    blk, coef, S = pair.check_pass1("mutual", what="4.2 M floats")
    assert 200 <= blk[12] < 700
    host, st = state_for(dev, off[-1], 6)
    pair.pass2(st)
    check_update(pair, st, host, blk, coef, "4.2 M floats")


# ================================================================ 2. identity, negative control, grid independence
@pytest.mark.parametrize("mode", R.MODES)
def test_without_a_conflict_the_update_is_the_plain_pass_2(dev, mode):
    """The surgery gram pass, then the PLAIN siss_recombine_clip_adamw on that scalar block and the surgery update on copies"""
    C = chunk()
    gx, ga, off = R.case([4, 64, C - 4, C + 4, 260, 2 * C + 8 + 3], 31, conflict="none")
    gx[::7] = -0.0                                             # (cx = 1: 1 * -0 = -0, the sign of a zero survives too)
    n = off[-1]
    pair = Pair(dev, gx, ga, off, step_before=1)
    pair.pass1(mode)
    blk, coef, _ = pair.check_pass1(mode, what=f"no conflict / {mode}")
    assert blk[12] == 0 and blk[14] == 0 and blk[15] == 0 and blk[13] < 0
    assert (coef[:, 0] == 1).all() and (coef[:, 1] == blk[3]).all()
    host, a = state_for(dev, n, 12)
    _, b = state_for(dev, n, 12)
    pair.pass2(a)
    p, m, v, sh, go = b.slices(0, n)
    launch("siss_recombine_clip_adamw", pair.bx.t, pair.ba.t, p, m, v, sh, go, n, *(float(h) for h in HP), pair.sc.blk.t)
    for key in ("p", "m", "v", "shadow", "gout"):
        assert torch.equal(bits(getattr(a, key).d), bits(getattr(b, key).d)), f"{mode}: {key} differs from the plain pass 2"
    assert not torch.equal(a.p.d.cpu(), a.p.flat), "the update moved nothing"
    # ... and the scalar block is the plain pass 1's where the two compute the same thing (the sums' orders differ: 4u, not bits)
    sc = Scal(dev, 1)
    launch("siss_grad_norms_scale", pair.bx.t, pair.ba.t, n, 0, 5.0, 1.0, float(HP[1]), float(HP[2]), sc.partials.t, sc.blk.t)
    plain = sc.read(n)
    for i in (0, 1, 2, 3, 4, 5):
        assert abs(float(plain[i]) - float(blk[i])) <= 2 * U * abs(float(plain[i])), (i, plain[i], blk[i])
    assert (plain[[6, 8, 9]] == blk[[6, 8, 9]]).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_one_conflicting_group_moves_exactly_its_stretch(dev, mode):
    """Group 3 of 6 conflicts.  Against the PLAIN pass 2 fed the surgery's own block (its s and clip): every byte outside the group's
    stretch is equal; inside it g_out and the first moment differ on more than nine elements in ten (a changed coefficient changes
    every g whose gradient is not zero, and m takes a tenth of g), the second moment and the parameters on some (the warm moments are
    those of N(0, 1) gradients, a hundred times these: v takes g^2 / 1000, near its last place, and the parameters move by lr m / den,
    a few of their last places) -- nothing is asked of the bf16 shadow inside the stretch"""
    C = chunk()
    gx, ga, off = R.case([64, C + 4, 260, 2 * C + 8, 128, 64 + 3], 41, conflict={3})
    n = off[-1]
    pair = Pair(dev, gx, ga, off)
    pair.pass1(mode)
    blk, coef, S = pair.check_pass1(mode, what=f"one conflict / {mode}")
    assert R.conflicts(S) == [g == 3 for g in range(6)] and blk[12] == 1
    assert (coef[3] != np.array([1, blk[3]], f32)).any() and all((coef[g] == np.array([1, blk[3]], f32)).all() for g in (0, 1, 2, 4, 5))
    host, a = state_for(dev, n, 14)
    _, b = state_for(dev, n, 14)
    pair.pass2(a)
    check_update(pair, a, host, blk, coef, f"one conflict / {mode}")
    p, m, v, sh, go = b.slices(0, n)
    launch("siss_recombine_clip_adamw", pair.bx.t, pair.ba.t, p, m, v, sh, go, n, *(float(h) for h in HP), pair.sc.blk.t)
    lo, hi = off[3], off[4]
    for key in ("p", "m", "v", "shadow", "gout"):
        x, y = bits(getattr(a, key).t), bits(getattr(b, key).t)
        assert torch.equal(x[:lo], y[:lo]) and torch.equal(x[hi:], y[hi:]), f"{mode}: {key} changed outside the conflicting group"
        diff = float((x[lo:hi] != y[lo:hi]).float().mean())
        floor = {"gout": 0.9, "m": 0.9, "p": 0.0, "v": 0.0}.get(key)
        assert floor is None or diff > floor, f"{mode}: {key} moved on {diff:.3f} of the conflicting group"


def test_the_grid_size_changes_no_bit(dev):
    from siss_amd import lib
    gx, ga, off = R.case(lengths_of("seams", chunk()) + lengths_of("tail3", chunk()), 51)       # (the odd length last: inner offsets % 4 = 0)
    n = off[-1]
    outs = []
    for cap in (0, 3, 1):
        assert lib.query("siss_surgery_test_config", 0, cap) == 0
        pair = Pair(dev, gx, ga, off, step_before=4)
        pair.pass1("mutual")
        _, st = state_for(dev, n, 16)
        pair.pass2(st)
        outs.append([t.d.cpu() for t in (pair.rows, pair.gs, pair.coef, pair.sc.blk, st.p, st.m, st.v, st.shadow, st.gout)])
    assert pair.J > 3
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "a result depends on the grid size"


# ================================================================ 3. refusals
def test_refusals_leave_every_buffer_unchanged(dev):
    from siss_amd import lib
    C = chunk()
    gx, ga, off = R.case([64, C + 4, 260], 61)
    n = off[-1]
    pair = Pair(dev, gx, ga, off)
    host, st = state_for(dev, n, 18)
    a1, a2 = list(pair.pass1_args("mutual")), list(pair.pass2_args(st))
    P1, P2 = lib.PARAMS["siss_grad_norms_scale_surgery"], lib.PARAMS["siss_recombine_clip_adamw_surgery"]

    def with_(args, params, **kw):
        out = list(args)
        for k, v in kw.items():
            out[params.index(k)] = v
        return out
    unsorted = torch.tensor([0, off[2], off[1], n], dtype=torch.int64)
    misaligned = torch.tensor([0, off[1] + 2, off[2], n], dtype=torch.int64)
    short = torch.tensor([0, off[1], off[2], n - 4], dtype=torch.int64)
    empty = torch.tensor([0, off[1], off[1], n], dtype=torch.int64)
    bad1 = [dict(gx=None), dict(ga=None), dict(groups=None), dict(plan=None), dict(partials=None), dict(group_sums=None),
            dict(coef=None), dict(scalars=None), dict(gx=pair.bx.d[pair.bx.g + 1:pair.bx.g + 1 + n]),
            dict(ga=pair.ba.d[pair.ba.g + 3:pair.ba.g + 3 + n]), dict(groups=unsorted), dict(groups=misaligned), dict(groups=short),
            dict(groups=empty), dict(T=0), dict(T=-1), dict(T=2), dict(mode=1), dict(mode=3), dict(smode=3), dict(smode=-1),
            dict(jobs=pair.J + 1), dict(jobs=0), dict(n=0), dict(n=n + 4)]
    for kw in bad1:
        refused("siss_grad_norms_scale_surgery", *with_(a1, P1, **kw))
    bad2 = [dict(gx=None), dict(p=None), dict(m=None), dict(v=None), dict(groups=None), dict(plan=None), dict(coef=None),
            dict(scalars=None), dict(p=st.p.d[st.p.g + 1:st.p.g + 1 + n]), dict(g_out=st.gout.d[st.gout.g + 2:st.gout.g + 2 + n]),
            dict(shadow=st.shadow.d[st.shadow.g + 1:st.shadow.g + 1 + n]), dict(groups=unsorted), dict(groups=misaligned), dict(T=0),
            dict(jobs=pair.J - 1), dict(n=0)]
    for kw in bad2:
        refused("siss_recombine_clip_adamw_surgery", *with_(a2, P2, **kw))
    # a chunk length that is no multiple of 1024 is no configuration
    assert lib.query("siss_surgery_test_config", 1000, 0) == 1 and lib.query("siss_surgery_test_config", 0, 4096) == 1 and chunk() == C
    pair.bx.check(T(gx), "gx"); pair.ba.check(T(ga), "ga")
    pair.rows.check(T(np.full(3 * (pair.J + EXTRA_ROWS), -5.0)), "job rows"); pair.gs.check(T(np.full(3 * pair.G, -5.0)), "group sums")
    pair.coef.check(T(np.full(2 * pair.G, 77.0, f32)), "coefficients"); pair.sc.blk.check(T(pair.sc.init), "scalar block")
    p, m, v = host
    st.p.check(T(p), "p"); st.m.check(T(m), "m"); st.v.check(T(v), "v")
    st.shadow.check(torch.full((n,), 77.0, dtype=BF), "shadow"); st.gout.check(T(np.full(n, 77.0, f32)), "g_out")
    # ... and the accepted call still runs
    pair.pass1("mutual")
    pair.check_pass1("mutual", what="after the refusals")


# ================================================================ engines and steppers
def make_engine(dtype=torch.bfloat16):
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    return UNetEngine(UNet2DConfig(**KW), "cuda:0", dtype=dtype)


_W = {}


def weights():
    if "sd" not in _W:
        _W["sd"] = make_engine().init_random(seed=4)
    return _W["sd"]


def batch(step, dev, B=2):
    g = torch.Generator().manual_seed(100 + step)
    x0 = (torch.rand(B, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    a0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).repeat(B, 1, 1, 1).to(dev)
    noise = torch.randn(B, 3, 16, 16, generator=g).to(dev)
    return x0, a0, noise, torch.tensor([999, 300, 999, 50][:B], device=dev), torch.tensor([0.9, 0.2, 0.7, 0.4][:B], device=dev)


def stepper(surgery=None, dtype=torch.bfloat16, **kw):
    """surgery: None or (mode, granularity)"""
    from siss_amd.step import SISSStepper
    from siss_amd.surgery import Surgery
    from oracle import schedule as S
    eng = make_engine(dtype)
    eng.load_state_dict(weights())
    sg = Surgery(eng, *surgery) if surgery else None
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2,
                     mixed_precision="bf16" if dtype == torch.bfloat16 else None, surgery=sg, **HPK, **kw)
    return eng, st


def state_of(eng, st):
    return dict(p=eng.ps.flat.clone(), shadow=eng.ps.shadow.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), scalars=st.opt.scalars.clone())


# ================================================================ 4. the step against the f64 definition
def by_name(d, names, dtype=f64):
    return np.concatenate([d[n].detach().double().flatten().numpy() for n in names]).astype(dtype)


def split(vec, like, names):
    out, off = {}, 0
    for n in names:
        k = like[n].numel()
        out[n] = torch.from_numpy(np.ascontiguousarray(vec[off:off + k])).view(like[n].shape)
        off += k
    return out


@pytest.mark.parametrize("loss_fn", ["importance_sampling_with_mixture", "double_forward_with_neg_del"])
def test_f32_step_with_surgery_matches_the_f64_definition(dev, loss_fn):
    """Two steps, mutual / tensor.  Gradients g_x, g_a: the fp32 oracle's at the engine's weights before the step (max_grad_norm 1e30:
    unclipped).  Update: tests/surgery_ref.py's f64 definition, one group per parameter tensor (the sums of a tensor do not depend on
    the layout of its elements).  Bounds: the step bounds of tests/test_hip_f32_mode.py (scalars 2e-4 relative, masked update cosine >=
    0.9999 over more than half of the elements).  The seeds are those of that test; on the CPU oracle they give 142 to 144
    conflicting tensors of 144 at both steps and both losses (the two attention blocks' key biases have gradients that are rounding
    noise: their decisions are compared with nobody's), and a scaling factor 1.7 (SISS) to 2.9 (no importance sampling) times the plain
    step's at step 2, so that the definition WITHOUT surgery misses the scalar bound and the update bound there."""
    from siss_amd.step import SISSStepper
    from siss_amd.surgery import Surgery
    from oracle import schedule as S
    from oracle.loss import OracleDeletionLoss
    from oracle.step import unlearning_step
    from parity_util import check_scalars, masked_update_cosine
    from test_hip_f32_mode import _pair
    TOL = 2e-4
    eng, net, sd = _pair(KW, seed=5)
    net = net.float()
    names = list(sd)
    off = R.offsets_of([sd[n].numel() for n in names])
    ac = S.alphas_cumprod()
    okw = dict(lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    hp = O.hyper(okw["lr"], *okw["betas"], okw["eps"], okw["weight_decay"])
    opt = torch.optim.AdamW(net.parameters(), **okw)
    sg = Surgery(eng, "mutual", "tensor")
    assert sg.groups == len(names) and set(sg.names) == set(names)
    st = SISSStepper(eng, ac, scaling_norm=5.0, lambd=0.5, train_batch_size=4, mixed_precision=None, loss_fn=loss_fn, surgery=sg, **okw)
    m = v = np.zeros(off[-1])
    keys = ("norm_loss_x", "norm_loss_a", "scaling_factor", "pre_clip_norm")
    gen = torch.Generator().manual_seed(7)
    for step in (1, 2):
        before = {n: t.clone() for n, t in eng.state_dict().items()}
        net.load_state_dict(before)
        mb = dict(x0=torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1, a0=(torch.rand(1, 3, 16, 16, generator=gen) * 2 - 1).repeat(4, 1, 1, 1),
                  noise=torch.randn(4, 3, 16, 16, generator=gen), t=torch.tensor([999, 400, 999, 50]), u=torch.tensor([0.9, 0.2, 0.7, 0.4]))
        _, gx, ga, _ = unlearning_step(net, opt, OracleDeletionLoss(*S.gamma_sigma(ac)), loss_fn, ac, [mb], train_batch_size=4,
                                       scaling_norm=5.0, max_grad_norm=1e30,
                                       loss_params={"lambd": 0.5} if loss_fn.startswith("importance") else None)
        gxv, gav, pv = by_name(gx, names), by_name(ga, names), by_name(before, names)
        (p1, m1, v1, gf), sc = R.step_f64(gxv, gav, pv, m, v, step, hp, off, "mutual", 0, 5.0, 1.0)
        (p0, _, _, gf0), sc0 = R.step_f64(gxv, gav, pv, m, v, step, hp, off, None, 0, 5.0, 1.0)
        st.step(mb["x0"], mb["a0"], mb["noise"], mb["t"].cuda(), mb["u"])
        got = st.stats()
        ref = dict(norm_loss_x=sc["norm_x"], norm_loss_a=sc["norm_a"], scaling_factor=sc["scale"], pre_clip_norm=sc["pre_clip_norm"])
        plain = dict(norm_loss_x=sc0["norm_x"], norm_loss_a=sc0["norm_a"], scaling_factor=sc0["scale"], pre_clip_norm=sc0["pre_clip_norm"])
        after = eng.state_dict()
        cos, frac = masked_update_cosine(before, split(p1, before, names), after, split(gf, before, names))
        print(f"\n[surgery] {loss_fn} step {step}: " + ", ".join(f"{k} {got[k]:.7g} / {ref[k]:.7g} (plain {plain[k]:.7g})" for k in keys)
              + f"; conflicts {got['surgery_conflicts']} / {sc['conflicts']} of {len(names)}, cos {got['surgery_cos']:.6f} / {sc['cos']:.6f}, "
              f"removed_a {got['surgery_removed_a']:.6f} / {sc['removed_a']:.6f}, removed_x {got['surgery_removed_x']:.6f} / "
              f"{sc['removed_x']:.6f}; masked update cosine {cos:.6f}")
        assert got["surgery_conflicts"] >= 1 and sc["conflicts"] >= 1, "the precondition: at least one tensor conflicts"
        check_scalars(ref, got, keys=keys, tol=TOL)
        assert cos >= 0.9999 and frac > 0.5, (cos, frac)
        assert got["step"] == step and got["surgery_mode"] == "mutual" and got["surgery_groups"] == len(names)
        for k in ("cos", "removed_a", "removed_x"):
            assert abs(got["surgery_" + k] - sc[k]) <= 10 * TOL * abs(sc[k]), (k, got["surgery_" + k], sc[k])
        grams = sg.grams()
        assert set(grams) == set(names) and sum(c for *_, c in grams.values()) == got["surgery_conflicts"]
        # tensor by tensor: the same decision wherever the oracle's own is not numerical noise (the key projection's bias of an attention
        # block has a gradient that is zero in exact arithmetic -- softmax ignores a shift of every key -- and rounding noise in any
        # run: the sign of its xa is nobody's) and not within 1 % of its threshold
        S64 = R.sums_f64(gxv, gav, off)
        whole = np.sqrt(S64[:, 0].sum() * S64[:, 1].sum())
        firm = [g for g, (xx, aa, xa) in enumerate(S64) if np.sqrt(xx * aa) >= 1e-8 * whole and abs(xa) >= 1e-2 * np.sqrt(xx * aa)]
        assert len(firm) >= len(names) - 8, (len(firm), len(names))
        for g in firm:
            assert grams[names[g]][3] == bool(S64[g, 2] > 0), (names[g], grams[names[g]], S64[g])
        assert abs(got["surgery_conflicts"] - sc["conflicts"]) <= len(names) - len(firm)
        if step == 2:
            # the precondition of the negative control, from the definition alone; then the control
            assert abs(ref["scaling_factor"] - plain["scaling_factor"]) >= 100 * TOL * abs(ref["scaling_factor"]), (ref, plain)
            with pytest.raises(AssertionError):
                check_scalars(plain, got, keys=("scaling_factor",), tol=TOL)
            cos0, _ = masked_update_cosine(before, split(p0, before, names), after, split(gf0, before, names))
            print(f"[surgery] {loss_fn} step 2: masked update cosine against the definition WITHOUT surgery {cos0:.6f}")
            assert cos0 < 0.9999, "the plain definition passes the update bound too: the surgery is not in the update"
        m, v = m1, v1


# ================================================================ 5. the bf16 step: the pair it runs, capture, the call log
def test_the_step_is_the_surgery_pair_on_its_own_gradients(dev):
    """the stepper's update = FlatAdamW.launch(surgery=...) on the gradients that very step produced; global and tensor differ"""
    from siss_amd import lib
    from siss_amd.optim import FlatAdamW
    from siss_amd.surgery import Surgery
    results = {}
    for gran in ("tensor", "global"):
        eng, st = stepper(("mutual", gran))
        snap, orig = {}, lib.call

        def spy(name, *a, **k):
            if name == "siss_grad_norms_scale_surgery":
                snap.update(g=eng.ps.grads.clone(), p=eng.ps.flat.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), sc=st.opt.scalars.clone())
            return orig(name, *a, **k)
        lib.call = spy
        try:
            st.step(*batch(0, dev))
        finally:
            lib.call = orig
        torch.cuda.synchronize()
        assert snap, "the surgery pass 1 did not run"
        ref = FlatAdamW(snap["p"], max_grad_norm=1.0, **{"lr": HPK["lr"], "betas": HPK["betas"], "eps": HPK["eps"], "weight_decay": HPK["weight_decay"]})
        ref.m.copy_(snap["m"]); ref.v.copy_(snap["v"]); ref.scalars.copy_(snap["sc"])
        ref.launch(snap["g"], scaling_norm=5.0, surgery=Surgery(eng, "mutual", gran))
        torch.cuda.synchronize()
        assert torch.equal(eng.ps.flat, ref.p) and torch.equal(st.opt.m, ref.m) and torch.equal(st.opt.v, ref.v)
        assert torch.equal(bits(st.opt.scalars), bits(ref.scalars))
        got = st.stats()
        assert got["surgery_conflicts"] >= 1 and got["surgery_granularity"] == gran and got["surgery_groups"] == (1 if gran == "global" else len(eng.ps.specs))
        assert set(st.surgery.grams()) == ({"*"} if gran == "global" else set(eng.ps.specs))
        results[gran] = eng.ps.flat.clone()
    assert not torch.equal(results["tensor"], results["global"])


def test_captured_surgery_step_replays_to_the_eager_bits(dev):
    eng, st = stepper(("mutual", "tensor"))
    loaded = eng.ps.flat.clone()
    args = batch(0, dev)
    st.step(*args)
    torch.cuda.synchronize()
    eager = state_of(eng, st)
    eager_slabs = (st.surgery.group_sums.clone(), st.surgery.coef.clone())
    assert float(eager["scalars"][R.SLOT_CONFLICTS]) >= 1
    eng2, st2 = stepper(("mutual", "tensor"))

    def reset():
        eng2.ps.flat.copy_(loaded)
        eng2.refresh_weights(cast_shadow=True)
        st2.opt.m.zero_(); st2.opt.v.zero_(); st2.opt.scalars.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st2.step(*args)                                  # settle allocations (and the sparse-fill plan) on the capture stream
        st2.step(*args)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st2.step(*args)
    torch.cuda.current_stream().wait_stream(side)
    reset()
    eng2.ps.grads.fill_(3.0)
    st2.surgery.group_sums.fill_(-1.0); st2.surgery.coef.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    got = state_of(eng2, st2)
    for key in ("p", "shadow", "m", "v", "scalars"):
        assert torch.equal(bits(got[key]), bits(eager[key])), f"replayed {key} differs from the eager step's"
    assert torch.equal(st2.surgery.group_sums, eager_slabs[0]) and torch.equal(bits(st2.surgery.coef), bits(eager_slabs[1]))


def test_a_step_without_the_key_calls_no_new_entry_point(dev):
    from siss_amd import lib
    logs = []
    for surgery in (None, ("mutual", "tensor")):
        eng, st = stepper(surgery)
        calls, orig = [], lib.call
        lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
        try:
            st.step(*batch(0, dev))
            torch.cuda.synchronize()
        finally:
            lib.call = orig
        logs.append(calls)
        if surgery is None:
            assert st.surgery is None and not [k for k in st.stats() if k.startswith("surgery")]
    plain, keyed = logs
    assert not [c for c in plain if "surgery" in c], "a step without the key reached csrc/surgery.hip"
    assert plain.count("siss_grad_norms_scale") == 1 and plain.count("siss_recombine_clip_adamw") == 1
    swap = {"siss_grad_norms_scale": "siss_grad_norms_scale_surgery", "siss_recombine_clip_adamw": "siss_recombine_clip_adamw_surgery"}
    assert keyed == [swap.get(c, c) for c in plain]


def test_surgery_is_refused_for_the_losses_without_a_pair_and_with_the_other_variants(dev):
    from siss_amd.ewc import FisherAnchor
    from siss_amd.step import SISSStepper
    from siss_amd.surgery import Surgery
    from oracle import schedule as S
    eng = make_engine()
    eng.load_state_dict(weights())
    sg = Surgery(eng, "mutual", "tensor")
    for loss_fn, extra in (("erasediff", dict(eta=1e-2)), ("simple_neg_del", {}), ("naive_del", {})):
        with pytest.raises(ValueError, match="surgery") as e:
            SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, loss_fn=loss_fn, surgery=sg, **HPK, **extra)
        assert loss_fn in str(e.value)
    names = [n for n in eng.ps.specs if "attentions" in n]
    with pytest.raises(ValueError, match=r"surgery.*trainable"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, trainable=names, surgery=sg, **HPK)
    with pytest.raises(ValueError, match=r"surgery.*ewc"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, ewc=FisherAnchor.uniform(eng, 1.0), surgery=sg, **HPK)
    _, st = stepper(("keep", "global"))
    with pytest.raises(ValueError, match="set_ewc"):
        st.set_ewc(FisherAnchor.uniform(st.e, 1.0))


# ================================================================ 6. one rank, forced collectives
def test_forced_collectives_on_one_rank_equal_the_step_without_a_group(dev):
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_surgery_worker.py"), ROOT], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL_SURGERY ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line[-1][len("RCCL_SURGERY "):])
    assert out["dp_on"] and out["equal_params"] and out["equal_moments"] and out["equal_block"] and out["equal_sums"], out
    assert out["exchange"] == "allreduce" and out["all_reduces"] >= 1 and out["conflicts"] >= 1, out
    assert r.stdout.count("gradient surgery: there is no sharded surgery update") == 1, r.stdout[-2000:]


# ================================================================ 7. the tasks
CELEB = ["--config-name=delete_celeb", "checkpoint_path=/nonexistent", "unet.sample_size=16", "unet.block_out_channels=[64,128]",
         "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]", "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1",
         "unet.attention_head_dim=null"]
SD = ["--config-name=delete_sd", "pretrained_model_name_or_path=/nonexistent",
      "+unet={sample_size:16,in_channels:4,out_channels:4,block_out_channels:[64,128],down_block_types:[CrossAttnDownBlock2D,DownBlock2D],"
      "up_block_types:[UpBlock2D,CrossAttnUpBlock2D],attention_head_dim:2,cross_attention_dim:64}"]
FIELDS = ("surgery_mode", "surgery_granularity", "surgery_groups", "surgery_conflicts", "surgery_cos", "surgery_removed_a", "surgery_removed_x")


def run_task(tmp_path, task, name, *extra):
    sys.path.insert(0, ROOT)
    import main as entry
    from siss_amd import tasks
    out = tmp_path / name
    ov = ["training_steps=3", "train_batch_size=2", "gradient_accumulation_steps=1", "allow_random_init=true", "allow_synthetic=true",
          f"data_dir={tmp_path}/nodata", "mixed_precision=bf16"]
    if task == "delete_sd":
        emb = tmp_path / "prompt.pt"
        if not emb.exists():
            torch.save(torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(1)), emb)
        ov.append(f"validation_prompts=[{emb}]")
    steppers, orig = [], tasks._DeleteBase.run

    def run(self):
        steppers.append(orig(self))
        return steppers[-1]
    tasks._DeleteBase.run = run
    try:
        entry.main([*(SD if task == "delete_sd" else CELEB), f"output_dir={out}", *ov, *extra])
    finally:
        tasks._DeleteBase.run = orig
    rundir = os.path.join(out, os.listdir(out)[0])
    return steppers[-1], [json.loads(l) for l in open(os.path.join(rundir, "train_log_rank0.jsonl"))]


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_with_the_key(dev, tmp_path, task):
    st, lines = run_task(tmp_path, task, "keyed", "+deletion.surgery={mode:mutual}")
    assert len(lines) == 3
    for l in lines:
        assert all(k in l for k in FIELDS), sorted(l)
        assert (l["surgery_mode"], l["surgery_granularity"]) == ("mutual", "tensor") and l["surgery_groups"] == len(st.e.ps.specs)
        assert 0 <= l["surgery_conflicts"] <= l["surgery_groups"] and -1 <= l["surgery_cos"] <= 1
        assert 0 <= l["surgery_removed_a"] <= 1 and 0 <= l["surgery_removed_x"] <= 1
    print(f"[surgery] {task}: " + "; ".join(f"step {l['global_step']} conflicts {l['surgery_conflicts']} / {l['surgery_groups']} cos "
                                           f"{l['surgery_cos']:.4f} removed_a {l['surgery_removed_a']:.4f}" for l in lines))
    grams = st.surgery.grams()
    assert set(grams) == set(st.e.ps.specs), "grams() names every tensor"
    assert sum(c for *_, c in grams.values()) == lines[-1]["surgery_conflicts"]
    # without the key: no fields
    _, plain = run_task(tmp_path, task, "plain")
    assert len(plain) == 3 and not [k for l in plain for k in l if k.startswith("surgery")]


def test_task_refuses_the_key_with_another_variant_or_a_loss_without_a_pair(dev, tmp_path):
    for i, (other, name) in enumerate((("+deletion.trainable=[attentions]", "deletion.trainable"),
                                       ("+deletion.ewc={strength:10,batches:2}", "deletion.ewc"),
                                       ("deletion.loss_fn=simple_neg_del", "simple_neg_del"))):
        with pytest.raises(ValueError, match=name):
            run_task(tmp_path, "delete_celeb", f"refused{i}", "+deletion.surgery={mode:mutual}", other)
        out = tmp_path / f"refused{i}"
        logs = [f for _, _, fs in os.walk(out) for f in fs if f.startswith("train_log")] if out.exists() else []
        assert not logs, "a refused run reached the loop"

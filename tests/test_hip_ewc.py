"""csrc/ewc.hip and what stands on it (siss_amd/ewc.py, FlatAdamW.launch(ewc=...), SISSStepper(ewc=...), deletion.ewc), on the GPU.

* siss_fisher_accumulate and the fold of siss_grad_norms_scale_ewc, bitwise against tests/ewc_ref.py, buffers between sentinel guards
  (tests/test_hip_optimizer.py's Flat / Scal), n = 1027 (two blocks, tail 3) and n = 4,197,379 (the grid-stride loop wraps twice,
  tail 3); slots 0..11 of the block are what siss_grad_norms_scale writes on the folded g_x; the two logged values within one f32
  rounding (2^-23 relative) of the f64 sums over the same f32 d and t; integers give exact sums; a misaligned F is refused.
* Identities BY VALUE (torch.equal): with strength * F * d = 0 the keyed pair leaves p, m, v, the shadow and slots 0..11 equal to
  the plain pair's.  By value and not by bit pattern, because the one bit the fold can change there is the sign of a zero:
  g_x = -0 becomes -0 + (+0) = +0.  Negative control: F = 1, pstar = p + 1 moves the parameters elsewhere.
* from_batches on the tiny f32 engine: F is bitwise the restatement's accumulation of the gradients the shared per-batch helper of
  siss_amd/saliency.py left in gradient set 0; the training state is untouched; normalize gives mean 1 within 2^-22.
* Two optimizer steps of the f32 engine against the f64 oracle, SISS and simple_neg_del, at the bounds of tests/test_hip_f32_mode.py
  (scalars 2e-4, masked update cosine), with the negative control that the restatement WITHOUT the penalty misses them at step 2.
* A captured keyed step replays to the eager step's bits; an unkeyed step calls no new entry point.
* One rank with forced collectives (tests/rccl_ewc_worker.py); delete_celeb and delete_sd through main.main.

The backward pass of the f32 engine is not bitwise repeatable (csrc/f32_path.hip sums GroupNorm's column sums atomically), so nothing
here compares two f32 runs bit for bit: the f32 checks feed ONE run's gradients to both sides.  Whole steps are compared between runs
on the bf16 engine only, where tests/test_hip_saliency.py documents that every kernel of this UNet's step is repeatable.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import ewc_ref as E
import optimizer_ref as O
from test_hip_optimizer import BF, F32, F64, Flat, Scal, T, launch, refused
from test_hip_small_kernels import same
from test_hip_surface import KW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
HP = O.hyper(*O.HYPER["sd"])
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)
LAM = 7.5
WRITTEN = list(O.NAMES.values()) + [E.PENALTY_SLOT, E.GRAD_NORM_SLOT]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def knob_of(mode):
    return 1e-2 if mode == 1 else 5.0


# ================================================================ 1. siss_fisher_accumulate
@pytest.mark.parametrize("n", E.SIZES)
def test_fisher_accumulate_is_bitwise_the_restatement(dev, n):
    rng = np.random.default_rng(n)
    want = (rng.standard_normal(n) ** 2).astype(f32)
    Fb = Flat(n, F32, dev, body=want)
    for i, w in enumerate((1.0, 0.125, 1.0 / 3.0)):
        g = (10.0 ** -i * rng.standard_normal(n)).astype(f32)
        gb = Flat(n, F32, dev, body=g)
        launch("siss_fisher_accumulate", gb.t, Fb.t, n, w)
        want = E.fisher_accumulate_f32(g, want, w)
        Fb.check(T(want), f"n {n}: F after accumulation {i} (w = {w})")
        gb.check(T(g), "g after the accumulation")


def test_fisher_accumulate_refuses_misaligned_buffers(dev):
    n = 1027
    rng = np.random.default_rng(0)
    g, F = rng.standard_normal(n + 1).astype(f32), rng.standard_normal(n + 1).astype(f32)
    gb, Fb = Flat(n + 1, F32, dev, body=g), Flat(n + 1, F32, dev, body=F)
    refused("siss_fisher_accumulate", gb.t[:n], Fb.t[1:], n, 1.0)            # F four bytes off a 16-byte line
    refused("siss_fisher_accumulate", gb.t[1:], Fb.t[:n], n, 1.0)
    refused("siss_fisher_accumulate", gb.t[:n], Fb.t[:n], 0, 1.0)
    Fb.check(T(F), "F after three refusals")
    gb.check(T(g), "g after three refusals")


# ================================================================ 2. the fold
class Fold:
    """One launch of siss_grad_norms_scale_ewc on host arrays, every buffer between guards."""

    def __init__(self, dev, gx, ga, p, pstar, F, lam, mode, step_before):
        n = len(gx)
        self.n, self.host = n, dict(gx=gx, ga=ga, p=p, pstar=pstar, F=F)
        self.b = {k: Flat(n, F32, dev, body=v) for k, v in self.host.items()}
        self.sc = Scal(dev, step_before)
        self.ep = Flat(2 * O.MAX_BLOCKS, F64, dev, fill=-5.0)
        b = self.b
        launch("siss_grad_norms_scale_ewc", b["gx"].t, b["ga"].t, b["p"].t, b["pstar"].t, b["F"].t, n, lam, mode, knob_of(mode), 1.0,
               float(HP[1]), float(HP[2]), self.sc.partials.t, self.ep.t, self.sc.blk.t)

    def block(self):
        """the 16 floats; the slots nobody writes, the guards and both slabs beyond the grid keep their fill"""
        blk = self.sc.blk.np().copy()
        keep = self.sc.init.copy()
        keep[WRITTEN] = blk[WRITTEN]
        self.sc.blk.check(T(keep), "scalar block: unwritten slots and guards")
        g = O.grid_for(self.n)
        for slab, width, what in ((self.sc.partials, 3, "norm partial sums"), (self.ep, 2, "penalty partial sums")):
            got = slab.d.cpu()
            same(got[slab.g + width * g:], slab.flat[slab.g + width * g:], what + " beyond the grid")
            same(got[:slab.g], slab.flat[:slab.g], what + ": guard before")
        return blk

    def untouched(self):
        for k in ("ga", "p", "pstar", "F"):
            self.b[k].check(T(self.host[k]), f"{k} after the fold")


def plain_block(dev, gx2, ga, mode, step_before):
    n = len(gx2)
    bx, ba, sc = Flat(n, F32, dev, body=gx2), Flat(n, F32, dev, body=ga), Scal(dev, step_before)
    launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob_of(mode), 1.0, float(HP[1]), float(HP[2]), sc.partials.t, sc.blk.t)
    return sc.read(n), sc


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", E.SIZES)
def test_fold_is_bitwise_the_restatement_and_pass_1_on_the_folded_gradient(dev, n, mode):
    gx, ga, p, pstar, F = E.case(n, n % 1000 + mode)
    step_before = mode
    run = Fold(dev, gx, ga, p, pstar, F, LAM, mode, step_before)
    gx2, d, t = E.fold_f32(gx, p, pstar, F, LAM)
    assert float(np.abs(t).max()) > 1e-3 * float(np.abs(gx).max()), "the case does not exercise the fold"
    run.b["gx"].check(T(gx2), f"n {n} mode {mode}: gx after the fold (= the restatement's gx')")
    run.untouched()
    blk = run.block()
    ref, sc_ref = plain_block(dev, gx2, ga, mode, step_before)
    same(T(blk[:12].copy()), T(ref[:12].copy()), f"n {n} mode {mode}: slots 0..11 against siss_grad_norms_scale on gx'")
    g3 = 3 * O.grid_for(n)
    same(run.sc.partials.t[:g3].cpu(), sc_ref.partials.t[:g3].cpu(), "the three partial sums per block")
    assert blk[6] == step_before + 1
    pen, tn = E.penalty_f64(F, d, t, LAM)
    print(f"[ewc] n {n} mode {mode}: ewc_penalty {blk[12]!r} / {pen!r}, ewc_grad_norm {blk[13]!r} / {tn!r}")
    assert pen > 0 and abs(float(blk[E.PENALTY_SLOT]) - pen) <= 2.0 ** -23 * pen, (float(blk[12]), pen)
    assert tn > 0 and abs(float(blk[E.GRAD_NORM_SLOT]) - tn) <= 2.0 ** -23 * tn, (float(blk[13]), tn)


@pytest.mark.parametrize("n", E.SIZES)
def test_fold_on_integers_is_exact(dev, n):
    gx, ga, p, pstar, F = E.int_case(n, n)
    run = Fold(dev, gx, ga, p, pstar, F, 1.0, 0, 0)
    d = (p - pstar).astype(np.int64)
    t = F.astype(np.int64) * d
    run.b["gx"].check(T((gx.astype(np.int64) + t).astype(f32)), "gx' on integers")
    run.untouched()
    blk = run.block()
    sfd, stt = int((F.astype(np.int64) * d * d).sum()), int((t * t).sum())
    assert stt > 0 and blk[E.PENALTY_SLOT] == f32(0.5 * sfd) and blk[E.GRAD_NORM_SLOT] == f32(math.sqrt(stt)), (blk[12], sfd, blk[13], stt)
    xx, aa, xa = O.int_sums((gx.astype(np.int64) + t).astype(f32), ga)
    want = O.scalars_f32(float(xx), float(aa), float(xa), 0, knob_of(0), 1.0, HP[1], HP[2], 0)
    idx = list(O.NAMES.values())                             # (slots 7, 10, 11 are pads nobody writes: Fold.block() held them)
    same(T(blk[idx].copy()), T(want[idx].copy()), "the written slots of 0..11 from exact integer sums")


# ================================================================ 3. identities, by value
class State:
    def __init__(self, dev, p, m, v):
        n = len(p)
        rng = np.random.default_rng(11)
        self.p, self.m, self.v = (Flat(n, F32, dev, body=b) for b in (p, m, v))
        self.shadow = Flat(n, BF, dev, body=rng.standard_normal(n).astype(f32))

    def args(self):
        return self.p.t, self.m.t, self.v.t, self.shadow.t, None


def run_pair(dev, gx, ga, p, m, v, mode, step_before, anchor=None):
    """pass 1 + pass 2 on fresh copies; anchor = (pstar, F, strength) takes the keyed pass 1.  {name: host tensor}, guards included."""
    n = len(gx)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    sc, st = Scal(dev, step_before), State(dev, p, m, v)
    hp = [float(h) for h in HP]
    if anchor is None:
        launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob_of(mode), 1.0, hp[1], hp[2], sc.partials.t, sc.blk.t)
    else:
        pstar, F, lam = anchor
        bs, bF = Flat(n, F32, dev, body=pstar), Flat(n, F32, dev, body=F)
        ep = Flat(2 * O.MAX_BLOCKS, F64, dev, fill=-5.0)
        launch("siss_grad_norms_scale_ewc", bx.t, ba.t, st.p.t, bs.t, bF.t, n, lam, mode, knob_of(mode), 1.0, hp[1], hp[2],
               sc.partials.t, ep.t, sc.blk.t)
    launch("siss_recombine_clip_adamw", bx.t, ba.t, *st.args(), n, *hp, sc.blk.t)
    ba.check(T(ga), "ga after the pair")
    return dict(p=st.p.d.cpu(), m=st.m.d.cpu(), v=st.v.d.cpu(), shadow=st.shadow.d.cpu(), block=sc.blk.t.cpu()[:12].clone(),
                whole_block=sc.blk.t.cpu().clone())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", E.SIZES)
def test_a_vanishing_penalty_gradient_gives_the_plain_pair_by_value(dev, n, mode):
    """torch.equal compares VALUES: -0.0 == +0.0.  That is the comparison meant here -- where strength * F * d is (+-)0 the fold's
    gx + t can turn a -0 gradient into +0 (-0 + +0 = +0) and nothing else, and a zero's sign changes no norm and no update."""
    gx, ga, p, pstar, F = E.case(n, n % 1000 + 7 * mode)
    gx[::5] = -0.0                                           # the one case in which bits may differ
    gx[1::5] = 0.0
    m, v = O.warm_state(n, 3, HP, seed=5)
    plain = run_pair(dev, gx, ga, p, m, v, mode, 2)
    cases = {"F = 0": (pstar, np.zeros(n, f32), LAM), "pstar = p": (p.copy(), F, LAM), "uniform F at theta = theta*": (p.copy(), np.ones(n, f32), LAM)}
    for name, anchor in cases.items():
        keyed = run_pair(dev, gx, ga, p, m, v, mode, 2, anchor)
        for key in ("p", "m", "v", "shadow", "block"):
            assert torch.equal(keyed[key], plain[key]), f"n {n} mode {mode}, {name}: {key} differs from the plain pair's"
        assert float(keyed["whole_block"][E.PENALTY_SLOT]) == 0.0 and float(keyed["whole_block"][E.GRAD_NORM_SLOT]) == 0.0, name
    moved = run_pair(dev, gx, ga, p, m, v, mode, 2, (p + f32(1), np.ones(n, f32), LAM))        # negative control
    assert not torch.equal(moved["p"], plain["p"]) and not torch.equal(moved["block"], plain["block"])
    assert float(moved["whole_block"][E.PENALTY_SLOT]) > 0


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


def stepper(ewc=None, dtype=torch.bfloat16, **kw):
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    eng = make_engine(dtype)
    eng.load_state_dict(weights())
    anchor = ewc(eng) if callable(ewc) else ewc
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2,
                     mixed_precision="bf16" if dtype == torch.bfloat16 else None, ewc=anchor, **HPK, **kw)
    return eng, st


def shifted_uniform(strength, shift=1e-3):
    """L2-SP around a point `shift` away from the loaded weights (on the real parameters): the penalty acts from the first step"""
    def make(eng):
        from siss_amd.ewc import FisherAnchor
        a = FisherAnchor.uniform(eng, strength)
        a.pstar.add_(shift * a.fisher)
        return a
    return make


def keep_batches(seed=9, B=2):
    g = torch.Generator().manual_seed(seed)
    while True:
        yield torch.rand(B, 3, 16, 16, generator=g) * 2 - 1


def state_of(eng, st):
    return dict(p=eng.ps.flat.clone(), shadow=eng.ps.shadow.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), scalars=st.opt.scalars.clone())


# ================================================================ 4. from_batches
def test_from_batches_accumulates_the_helpers_gradients_and_leaves_the_state_alone(dev):
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor, real_mask
    from siss_amd.saliency import forget_gradient
    eng, st = stepper(dtype=torch.float32)
    st.step(*batch(0, dev))                                  # a warm state: non-zero moments, step count 1, a recorded fill plan
    before = state_of(eng, st)
    plans = dict(eng._fill_plans)
    hook, seen_hooks, inner = (lambda: None), [], eng.backward
    eng.on_early_grads_final = hook

    def spy_backward(*a, **k):
        seen_hooks.append(eng.on_early_grads_final)
        return inner(*a, **k)
    eng.backward = spy_backward
    fed, orig = [], lib.call

    def spy_call(name, *a, **k):
        if name == "siss_fisher_accumulate":
            assert a[0].data_ptr() == eng.ps.grads[0].data_ptr() and a[2] == eng.ps.total
            fed.append((a[0].clone(), a[3]))
        return orig(name, *a, **k)
    lib.call = spy_call
    try:
        anchor = FisherAnchor.from_batches(st, keep_batches(), 3, strength=2.0, generator=torch.Generator(device=dev).manual_seed(0),
                                           normalize=False)
    finally:
        lib.call = orig
        del eng.backward
    torch.cuda.synchronize()
    assert seen_hooks == [None] * 3 and eng.on_early_grads_final is hook and st._pending == []
    eng.on_early_grads_final = None
    assert len(fed) == 3 and all(w == 1.0 / 3 for _, w in fed)
    want = np.zeros(eng.ps.total, f32)
    for g, w in fed:
        assert float(g.abs().max()) > 0
        want = E.fisher_accumulate_f32(g.cpu().numpy(), want, w)
    same(anchor.fisher.cpu(), T(want), "F against the restatement's accumulation of the three micro-batch gradients")
    assert not torch.equal(fed[0][0], fed[1][0]), "every micro-batch must be a gradient of its own"
    # ... and those gradients are forget_gradient's: its one-batch form from the same generator state yields the first of them (to
    # the f32 engine's run-to-run noise: this is a second backward pass)
    g1 = forget_gradient(st, keep_batches(), 1, generator=torch.Generator(device=dev).manual_seed(0))
    assert float((g1 - fed[0][0]).norm() / g1.norm()) < 1e-4
    for key, t in state_of(eng, st).items():
        assert torch.equal(bits(t), bits(before[key])), f"from_batches changed {key}"
    assert torch.equal(anchor.pstar, eng.ps.flat) and anchor.pstar.data_ptr() != eng.ps.flat.data_ptr()
    assert int(eng.ps.grads.count_nonzero()) == 0, "the gradient buffers are not zero on return"
    assert st._micro == 0 and eng.wgrad_overwrite is False and dict(eng._fill_plans) == plans
    real = real_mask(eng.ps.specs, eng.ps.total, dev)
    assert int(anchor.fisher[~real].count_nonzero()) == 0 and bool((anchor.fisher >= 0).all())
    assert anchor.source == "computed" and anchor.mean == float(anchor.fisher[real].double().mean()) > 0
    normed = FisherAnchor.from_batches(st, keep_batches(), 3, strength=2.0, generator=torch.Generator(device=dev).manual_seed(0),
                                       normalize=True)
    mean = float(normed.fisher[real].double().mean())
    print(f"[ewc] normalised F: mean over the real parameters {mean!r} (before: {normed.mean!r}, max {normed.max!r}, zeros {normed.zeros})")
    assert abs(mean - 1.0) <= 2.0 ** -22 and int(normed.fisher[~real].count_nonzero()) == 0
    with pytest.raises(RuntimeError, match="middle of an accumulation"):
        st._micro = 1
        try:
            FisherAnchor.from_batches(st, keep_batches(), 1, strength=1.0)
        finally:
            st._micro = 0


# ================================================================ 5. the step against the f64 oracle
def by_name(d, names, dtype=f64):
    return np.concatenate([d[n].detach().double().flatten().numpy() for n in names]).astype(dtype)


def split(vec, like, names):
    out, off = {}, 0
    for n in names:
        k = like[n].numel()
        out[n] = torch.from_numpy(np.ascontiguousarray(vec[off:off + k])).view(like[n].shape)
        off += k
    return out


@pytest.mark.parametrize("loss_fn", ["importance_sampling_with_mixture", "simple_neg_del"])
def test_f32_step_with_the_anchor_matches_the_f64_restatement(dev, loss_fn):
    """Two steps.  Gradients g_x, g_a: the fp32 oracle's at the engine's weights before the step.  Update: tests/ewc_ref.py's f64 step
    with the penalty.  Bounds: the step bounds of tests/test_hip_f32_mode.py (scalars 2e-4 relative, masked update cosine >= 0.9999 over
    more than half of the elements).  F is non-uniform (0.5 .. 1.5, a fixed pattern per tensor); the strength is set after step 1, from
    the restatement, to |g_x| / |F d| of step 2, so that the penalty gradient is as long as g_x itself; the precondition (it moves
    norm_loss_x by >= 100 x the scalar bound) is asserted, and the restatement WITHOUT the penalty then misses the bound."""
    from siss_amd.ewc import FisherAnchor
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from oracle.loss import OracleDeletionLoss
    from oracle.step import unlearning_step
    from parity_util import check_scalars, masked_update_cosine
    from test_hip_f32_mode import _pair
    TOL = 2e-4
    eng, net, sd = _pair(KW, seed=5)
    net = net.float()
    names = list(sd)
    ps = eng.ps
    g = torch.Generator().manual_seed(3)
    F_ref = {n: 0.5 + torch.rand(sd[n].shape, generator=g) for n in names}
    F_flat = torch.zeros_like(ps.flat)
    for n, sp in ps.specs.items():
        F_flat[sp.off:sp.off + sp.numel] = ps.to_native(sp, F_ref[n].to(dev)).reshape(-1)
    anchor = FisherAnchor(eng, F_flat, ps.flat.detach().clone(), 1.0)
    single = loss_fn == "simple_neg_del"
    ac = S.alphas_cumprod()
    okw = dict(lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    hp = O.hyper(okw["lr"], *okw["betas"], okw["eps"], okw["weight_decay"])
    opt = torch.optim.AdamW(net.parameters(), **okw)
    st = SISSStepper(eng, ac, scaling_norm=5.0, lambd=0.5, train_batch_size=4, mixed_precision=None, loss_fn=loss_fn, inf_guard=single,
                     ewc=anchor, **okw)
    mode, knob = (2, 1.0) if single else (0, 5.0)
    pstar = by_name(sd, names)
    F = by_name(F_ref, names)
    m = v = np.zeros_like(pstar)
    keys = ("norm_loss_x", "pre_clip_norm") if single else ("norm_loss_x", "norm_loss_a", "scaling_factor", "pre_clip_norm")
    gen = torch.Generator().manual_seed(7)
    for step in (1, 2):
        before = {n: t.clone() for n, t in eng.state_dict().items()}
        net.load_state_dict(before)
        mb = dict(x0=torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1, a0=(torch.rand(1, 3, 16, 16, generator=gen) * 2 - 1).repeat(4, 1, 1, 1),
                  noise=torch.randn(4, 3, 16, 16, generator=gen), t=torch.tensor([999, 400, 999, 50]), u=torch.tensor([0.9, 0.2, 0.7, 0.4]))
        _, gx, ga, gfin = unlearning_step(net, opt, OracleDeletionLoss(*S.gamma_sigma(ac)), loss_fn, ac, [mb], train_batch_size=4,
                                          scaling_norm=5.0, max_grad_norm=1e30, inf_guard=single,
                                          loss_params={"superfactor": 1.0} if single else {"lambd": 0.5})
        if single:                                           # one backward, no split: the (unclipped) gradient is g_x, g_a = 0
            gx, ga = gfin, {n: torch.zeros_like(t) for n, t in gfin.items()}
        gxv, gav, pv = by_name(gx, names), by_name(ga, names), by_name(before, names)
        if step == 2:                                        # the strength: |lambda F d| = |g_x|
            anchor.strength = float(f32(np.linalg.norm(gxv) / np.linalg.norm(F * (pv - pstar))))
        lam = anchor.strength
        (p1, m1, v1, gf), sc, pen, tn, _ = E.step_f64(gxv, gav, pv, pstar, F, lam, m, v, step, hp, mode, knob, 1.0)
        (p0, _, _, gf0), sc0, _, _, _ = E.step_f64(gxv, gav, pv, pstar, F, None, m, v, step, hp, mode, knob, 1.0)
        st.step(mb["x0"], mb["a0"], mb["noise"], mb["t"].cuda(), mb["u"])
        got = st.stats()
        ref = dict(norm_loss_x=sc["norm_x"], norm_loss_a=sc["norm_a"], scaling_factor=sc["scale"], pre_clip_norm=sc["pre_clip_norm"])
        plain = dict(norm_loss_x=sc0["norm_x"], norm_loss_a=sc0["norm_a"], scaling_factor=sc0["scale"], pre_clip_norm=sc0["pre_clip_norm"])
        after = eng.state_dict()
        cos, frac = masked_update_cosine(before, split(p1, before, names), after, split(gf, before, names))
        print(f"\n[ewc] {loss_fn} step {step}: strength {lam:.6g}; " + ", ".join(f"{k} {got[k]:.7g} / {ref[k]:.7g} (unkeyed {plain[k]:.7g})" for k in keys)
              + f"; ewc_penalty {got['ewc_penalty']:.7g} / {pen:.7g}, ewc_grad_norm {got['ewc_grad_norm']:.7g} / {tn:.7g}; masked update cosine {cos:.6f}")
        check_scalars(ref, got, keys=keys, tol=TOL)
        assert cos >= 0.9999 and frac > 0.5, (cos, frac)
        assert got["ewc_strength"] == lam and got["step"] == step
        if step == 1:                                        # theta = theta*: no penalty, the unkeyed step
            assert got["ewc_penalty"] == 0.0 and got["ewc_grad_norm"] == 0.0 and pen == 0.0
            check_scalars(plain, got, keys=keys, tol=TOL)
        else:
            assert abs(got["ewc_penalty"] - pen) <= 10 * TOL * pen and abs(got["ewc_grad_norm"] - tn) <= 10 * TOL * tn
            # the precondition, from the restatement alone; then the negative control
            assert abs(ref["norm_loss_x"] - plain["norm_loss_x"]) >= 100 * TOL * abs(ref["norm_loss_x"]), (ref, plain)
            with pytest.raises(AssertionError):
                check_scalars(plain, got, keys=("norm_loss_x",), tol=TOL)
            cos0, _ = masked_update_cosine(before, split(p0, before, names), after, split(gf0, before, names))
            print(f"[ewc] {loss_fn} step 2: masked update cosine against the UNKEYED restatement {cos0:.6f}")
            assert cos0 < 0.9999, "the unkeyed restatement passes the update bound too: the anchor is not in the update"
        m, v = m1, v1


def test_keyed_step_1_is_the_plain_pair_on_the_same_gradients(dev):
    """theta = theta* at the first step: the keyed update equals, by value, the plain pair on the gradients that very step produced
    (f32 engine; the gradients are taken from the run itself, see the module docstring) -- and on the bf16 engine, whose steps
    repeat bit for bit, the whole keyed step equals the unkeyed stepper's."""
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    eng, st = stepper(lambda e: FisherAnchor.uniform(e, 50.0), dtype=torch.float32)
    snap, orig = {}, lib.call

    def spy(name, *a, **k):
        if name == "siss_grad_norms_scale_ewc":
            snap.update(g=eng.ps.grads.clone(), p=eng.ps.flat.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), sc=st.opt.scalars.clone())
        return orig(name, *a, **k)
    lib.call = spy
    try:
        st.step(*batch(0, dev))
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    assert snap, "the keyed pass 1 did not run"
    from siss_amd.optim import FlatAdamW
    p0 = snap["p"].clone()                                   # (the reference optimizer updates snap["p"] in place)
    ref = FlatAdamW(snap["p"], max_grad_norm=1.0, **{"lr": HPK["lr"], "betas": HPK["betas"], "eps": HPK["eps"], "weight_decay": HPK["weight_decay"]})
    ref.m.copy_(snap["m"]); ref.v.copy_(snap["v"]); ref.scalars.copy_(snap["sc"])
    ref.launch(snap["g"], scaling_norm=5.0)
    torch.cuda.synchronize()
    assert torch.equal(eng.ps.flat, ref.p) and torch.equal(st.opt.m, ref.m) and torch.equal(st.opt.v, ref.v)
    assert torch.equal(st.opt.scalars[:12], ref.scalars[:12]) and float(st.opt.scalars[12]) == 0.0 and float(st.opt.scalars[13]) == 0.0
    assert not torch.equal(eng.ps.flat, p0), "the step moved nothing"
    # bf16: run against run
    e1, s1 = stepper()
    e2, s2 = stepper(lambda e: FisherAnchor.uniform(e, 50.0))
    s1.step(*batch(0, dev)); s2.step(*batch(0, dev))
    torch.cuda.synchronize()
    a, b = state_of(e1, s1), state_of(e2, s2)
    for key in ("p", "shadow", "m", "v"):
        assert torch.equal(a[key], b[key]), f"bf16 step 1 under a uniform anchor: {key} differs from the unkeyed stepper's"
    assert torch.equal(a["scalars"][:12], b["scalars"][:12])
    l1, l2 = s1.stats(), s2.stats()
    assert json.dumps({k: l2[k] for k in l1}, sort_keys=True) == json.dumps(l1, sort_keys=True), "logged scalars of step 1 differ"
    assert (l2["ewc_penalty"], l2["ewc_grad_norm"], l2["ewc_strength"]) == (0.0, 0.0, 50.0)
    assert "ewc_penalty" not in l1
    # ... and at step 2 the anchor pulls: the two runs part
    s1.step(*batch(1, dev)); s2.step(*batch(1, dev))
    torch.cuda.synchronize()
    assert s2.stats()["ewc_penalty"] > 0 and not torch.equal(e1.ps.flat, e2.ps.flat)


# ================================================================ 6. capture, and the unkeyed call log
def test_captured_keyed_step_replays_to_the_eager_bits(dev):
    eng, st = stepper(shifted_uniform(20.0))
    loaded = eng.ps.flat.clone()
    args = batch(0, dev)
    st.step(*args)
    torch.cuda.synchronize()
    eager = state_of(eng, st)
    assert float(eager["scalars"][E.PENALTY_SLOT]) > 0
    eng2, st2 = stepper(shifted_uniform(20.0))

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
    graph.replay()
    torch.cuda.synchronize()
    got = state_of(eng2, st2)
    for key in ("p", "shadow", "m", "v", "scalars"):
        assert torch.equal(bits(got[key]), bits(eager[key])), f"replayed {key} differs from the eager step's"


def test_unkeyed_step_calls_no_new_entry_point(dev):
    from siss_amd import lib
    logs = []
    for ewc in (None, shifted_uniform(20.0)):
        eng, st = stepper(ewc)
        calls, orig = [], lib.call
        lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
        try:
            st.step(*batch(0, dev))
            torch.cuda.synchronize()
        finally:
            lib.call = orig
        logs.append(calls)
    plain, keyed = logs
    assert not [c for c in plain if "ewc" in c or "fisher" in c], "an unkeyed step reached csrc/ewc.hip"
    assert plain.count("siss_grad_norms_scale") == 1 and plain.count("siss_recombine_clip_adamw") == 1
    i = plain.index("siss_grad_norms_scale")
    assert plain[i + 1] == "siss_recombine_clip_adamw"
    # the keyed step: the same launches, pass 1 replaced
    assert keyed == [("siss_grad_norms_scale_ewc" if c == "siss_grad_norms_scale" else c) for c in plain]


def test_ewc_is_exclusive_with_the_other_selections(dev):
    from siss_amd.ewc import FisherAnchor
    from siss_amd.saliency import SaliencyMask
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    eng = make_engine()
    eng.load_state_dict(weights())
    anchor = FisherAnchor.uniform(eng, 1.0)
    names = [n for n in eng.ps.specs if "attentions" in n]
    with pytest.raises(ValueError, match=r"ewc.*trainable"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, trainable=names, ewc=anchor, **HPK)
    with pytest.raises(ValueError, match=r"ewc.*saliency"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, saliency=SaliencyMask.ones(eng), ewc=anchor, **HPK)
    _, st = stepper()
    st.set_saliency(SaliencyMask.ones(st.e))
    with pytest.raises(ValueError, match="set_ewc"):
        st.set_ewc(FisherAnchor.uniform(st.e, 1.0))
    _, st = stepper(lambda e: FisherAnchor.uniform(e, 1.0))
    with pytest.raises(ValueError, match="set_saliency"):
        st.set_saliency(SaliencyMask.ones(st.e))
    other = make_engine()
    other.ps.total += 64
    with pytest.raises(ValueError):
        FisherAnchor(other, anchor.fisher, anchor.pstar, 1.0)


# ================================================================ 7. one rank, forced collectives
def test_forced_collectives_on_one_rank_equal_the_step_without_a_group(dev):
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_ewc_worker.py"), ROOT], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL_EWC ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line[-1][len("RCCL_EWC "):])
    assert out["dp_on"] and out["equal_params"] and out["equal_moments"] and out["equal_block"], out
    assert out["exchange"] == "allreduce" and out["all_reduces"] >= 1 and out["penalty"] > 0, out
    assert r.stdout.count("Fisher anchor: there is no sharded fold") == 1, r.stdout[-2000:]


# ================================================================ 8. the tasks
CELEB = ["--config-name=delete_celeb", "checkpoint_path=/nonexistent", "unet.sample_size=16", "unet.block_out_channels=[64,128]",
         "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]", "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1",
         "unet.attention_head_dim=null"]
SD = ["--config-name=delete_sd", "pretrained_model_name_or_path=/nonexistent",
      "+unet={sample_size:16,in_channels:4,out_channels:4,block_out_channels:[64,128],down_block_types:[CrossAttnDownBlock2D,DownBlock2D],"
      "up_block_types:[UpBlock2D,CrossAttnUpBlock2D],attention_head_dim:2,cross_attention_dim:64}"]
EWC_FIELDS = ("ewc_penalty", "ewc_grad_norm", "ewc_strength")


def run_task(tmp_path, task, name, *extra):
    sys.path.insert(0, ROOT)
    import main as entry
    out = tmp_path / name
    ov = ["training_steps=3", "train_batch_size=2", "gradient_accumulation_steps=1", "allow_random_init=true", "allow_synthetic=true",
          f"data_dir={tmp_path}/nodata", "mixed_precision=bf16"]
    if task == "delete_sd":
        emb = tmp_path / "prompt.pt"
        if not emb.exists():
            torch.save(torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(1)), emb)
        ov.append(f"validation_prompts=[{emb}]")
    entry.main([*(SD if task == "delete_sd" else CELEB), f"output_dir={out}", *ov, *extra])
    rundir = os.path.join(out, os.listdir(out)[0])
    return rundir, [json.loads(l) for l in open(os.path.join(rundir, "train_log_rank0.jsonl"))]


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_with_the_key(dev, tmp_path, task):
    from siss_amd.ewc import CONFIG_FILE, FISHER_FILE
    from safetensors.torch import load_file
    rundir, lines = run_task(tmp_path, task, "keyed", "+deletion.ewc={strength:10,batches:2}")
    assert os.path.isfile(os.path.join(rundir, FISHER_FILE)) and os.path.isfile(os.path.join(rundir, CONFIG_FILE))
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    assert (c["strength"], c["batches"], c["batch_size"], c["seed"], c["normalize"], c["source"]) == (10.0, 2, 2, 0, True, "computed")
    assert c["mean"] > 0 and c["max"] >= c["mean"] and c["zeros"] >= 0 and c["total"] >= c["real_params"] > 0 and c["tensors"] > 0
    F = load_file(os.path.join(rundir, FISHER_FILE))["fisher"]
    assert F.shape == (c["total"],) and F.dtype == torch.float32 and bool((F >= 0).all())
    assert abs(float(F.double().sum()) / c["real_params"] - 1.0) <= 2.0 ** -22, "normalised: mean 1 over the real parameters (padding 0)"
    assert len(lines) == 3
    for st in lines:
        assert all(k in st for k in EWC_FIELDS) and st["ewc_strength"] == 10.0, st
    print(f"[ewc] {task}: " + "; ".join(f"step {l['global_step']} penalty {l['ewc_penalty']:.6g} |t| {l['ewc_grad_norm']:.6g}" for l in lines))
    assert lines[0]["ewc_penalty"] == 0.0 and lines[0]["ewc_grad_norm"] == 0.0 and lines[2]["ewc_penalty"] > 0 and lines[2]["ewc_grad_norm"] > 0
    # a second run that loads the first run's F logs the same three steps, and says that it loaded
    rundir2, lines2 = run_task(tmp_path, task, "reloaded", "+deletion.ewc={strength:10,batches:2,path:'%s'}" % rundir)
    assert json.load(open(os.path.join(rundir2, CONFIG_FILE)))["source"] == "loaded"
    assert torch.equal(load_file(os.path.join(rundir2, FISHER_FILE))["fisher"], F)
    for k in EWC_FIELDS + ("norm_loss_x", "norm_loss_a", "scaling_factor", "pre_clip_norm"):
        assert [l[k] for l in lines2] == [l[k] for l in lines], (k, [l[k] for l in lines2], [l[k] for l in lines])
    # without the key: no files, no fields -- and the same first step (theta = theta*)
    rundir3, plain = run_task(tmp_path, task, "plain")
    assert not os.path.exists(os.path.join(rundir3, FISHER_FILE)) and not os.path.exists(os.path.join(rundir3, CONFIG_FILE))
    assert len(plain) == 3 and not [k for l in plain for k in l if k.startswith("ewc")]
    assert plain[0]["norm_loss_x"] == lines[0]["norm_loss_x"] and plain[0]["pre_clip_norm"] == lines[0]["pre_clip_norm"]


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_refuses_the_exclusive_keys_before_the_first_step(dev, tmp_path, task):
    pat = "attentions" if task == "delete_celeb" else "attn2"
    for i, (other, name) in enumerate((("+deletion.trainable=[%s]" % pat, "deletion.trainable"),
                                       ("+deletion.lora={rank:2,targets:['%s.*to_q.weight']}" % pat, "deletion.lora"),
                                       ("+deletion.saliency={fraction:0.5,batches:1}", "deletion.saliency"))):
        with pytest.raises(ValueError, match=name):
            run_task(tmp_path, task, f"refused{i}", "+deletion.ewc={strength:10,batches:2}", other)
        out = tmp_path / f"refused{i}"
        logs = [f for _, _, fs in os.walk(out) for f in fs if f.startswith("train_log")] if out.exists() else []
        assert logs == [], "a refused run reached the loop"

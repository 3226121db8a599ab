"""The launchers of csrc/train_state.hip called DIRECTLY against tests/train_state_ref.py (which tests/test_train_state_host.py pins to
torch on the CPU and runs alone against every bound applied here), with the harness of tests/test_hip_optimizer.py: every output
between guard stretches filled with a sentinel, the WHOLE buffer compared, the inputs returned bit-identical; sizes
optimizer_ref.SIZES.  Then TrainStepper against the fp32 oracle, the resumable state, and the task loop through main.main.

    siss_grad_norm_single, siss_clip_adamw_ema, siss_ema_advance, siss_ema_step, siss_swap_f32

What is held to what:
* |g| on integers in [-8, 8]: bitwise f32(sqrt(int));
* grad_norm, clip_coef on Gaussian data within optimizer_ref.scalar_bounds (zero second set);
* bc1, bc2_sqrt, one_minus_decay within 2u relative of f64 (one rounding of a double) at steps 1 .. 100,000 and one past the cap;
* pass 2 BITWISE the f32 restatement fed the block read back (p, m, v, ema, g_out; shadow = bf16 of the new p);
* with ema = null: bitwise the p, m, v, shadow of siss_grad_norms_scale(mode 2) + siss_recombine_clip_adamw on (g, 0);
* the fused EMA bitwise the unfused pair (siss_clip_adamw_ema without ema, then siss_ema_step);
* siss_swap_f32: swapped bitwise, shadow the bf16 rounding of the new a, twice = identity.
"""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optimizer_ref as R
import train_state_ref as T
from test_hip_optimizer import BF, F32, F64, GUARD, Flat, Scal, State, launch, refused
from test_hip_small_kernels import bits, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
BIG = R.SIZES[-1]
EMA = T.TSHIRT_EMA
RTOL = 1e-4                                                  # tests/test_hip_f32_mode.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    assert lib.query("siss_train_scalars_words") == 16 and lib.query("siss_train_partials_words") == R.MAX_BLOCKS
    return torch.device("cuda:0")


def Tn(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class TScal:
    """The 16-float block (pads pre-filled with a sentinel that must survive, both counters preset) and the partial sums"""

    def __init__(self, dev, step_before=0, ema_step_before=0):
        init = np.full(16, 33.0, f32)
        init[list(T.NAMES.values())] = 0
        init[T.NAMES["step"]], init[T.NAMES["ema_step"]] = step_before, ema_step_before
        self.init = init
        self.blk = Flat(16, F32, dev, body=init)
        self.partials = Flat(R.MAX_BLOCKS, F64, dev, fill=-5.0)

    def read(self, n=None):
        b = self.blk.np().copy()
        keep = self.init.copy()
        idx = list(T.NAMES.values())
        keep[idx] = b[idx]
        self.blk.check(Tn(keep), "scalar block: pads and guards")
        if n is not None:
            got = self.partials.d.cpu()
            same(got[GUARD + R.grid_for(n):], self.partials.flat[GUARD + R.grid_for(n):], "partial sums beyond the grid")
            same(got[:GUARD], self.partials.flat[:GUARD], "partial sums: guard before")
        return b


def norm_single(dev, g, sc, max_norm=1.0, betas=(0.95, 0.999), ema=EMA):
    n = len(g)
    bg = Flat(n, F32, dev, body=g)
    launch("siss_grad_norm_single", bg.t, n, max_norm, betas[0], betas[1], *T.ema_args(ema), sc.partials.t, sc.blk.t)
    bg.check(Tn(g), "g after the norm")
    return sc.read(n), bg


# ================================================================ pass 1 and the block
@pytest.mark.parametrize("n", R.SIZES)
def test_norm_on_integers_is_exact(dev, n):
    g = T.ints(n, n)
    xx = int((g.astype(np.int64) ** 2).sum())
    blk, _ = norm_single(dev, g, TScal(dev))
    assert blk[0] == f32(np.sqrt(np.float64(xx))), (blk[0], xx)
    ref = T.scalars_f64(float(xx), 1.0, 0.95, 0.999, 1, EMA, 1)
    assert abs(float(blk[1]) - ref["clip_coef"]) <= R.U * (1 + 2.0 ** -20) * ref["clip_coef"]     # a double from an exact sum, rounded once
    assert (blk[2], blk[5], blk[6], blk[7]) == (1, 1, 1, 0)                                       # first EMA step: decay 0


@pytest.mark.parametrize("n", [1027, BIG])
def test_one_hot_probe_counts_every_element_once(dev, n):
    nv = n // 4 * 4
    pos = sorted({0, 3, nv - 1, nv, n - 1, 1023, 1024} | ({2048 * 1024 - 1, 2048 * 1024} if n == BIG else set()))
    g = torch.zeros(n + 2 * GUARD, device=dev)
    sc = TScal(dev)
    for i in pos:
        g[GUARD + i] = 3.0
        launch("siss_grad_norm_single", g[GUARD:GUARD + n], n, 1.0, 0.95, 0.999, *T.ema_args(EMA), sc.partials.t, sc.blk.t)
        blk = sc.read(n)
        assert blk[0] == 3.0, (i, blk[0])
        g[GUARD + i] = 0.0
    assert blk[T.NAMES["step"]] == len(pos) == blk[T.NAMES["ema_step"]]


@pytest.mark.parametrize("n", R.SIZES)
def test_block_on_gaussian_data_within_the_a_priori_bounds(dev, n):
    g = T.gauss(n, n)
    blk, _ = norm_single(dev, g, TScal(dev))
    worst = T.block_errors(blk, g, 1.0)
    print(f"[train-state] n {n}: error / allowed {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("b1,b2", R.BETAS)
@pytest.mark.parametrize("k", T.STEPS + [T.first_capped_step(EMA)])
def test_counters_bias_corrections_and_one_minus_decay(dev, k, b1, b2):
    blk, _ = norm_single(dev, T.ints(5, 5), TScal(dev, k - 1, k - 1), betas=(b1, b2))
    e = T.one_rounding_errors(blk, b1, b2, k, EMA, k)
    print(f"[train-state] betas {b1, b2} step {k}: |err| / (u ref): bc1 {e[0]:.2f}, bc2_sqrt {e[1]:.2f}, 1 - decay {e[2]:.2f} (allowed 2); decay {blk[7]!r}")
    assert blk[T.NAMES["step"]] == k and blk[T.NAMES["ema_step"]] == k
    assert max(e) <= 2.0, (k, e)
    assert blk[T.NAMES["ema_decay"]] == f32(T.decay_f64(k, **EMA))


@pytest.mark.parametrize("sch", [dict(EMA, use_warmup=False), dict(EMA, update_after=3, min_decay=0.5), dict(EMA, inv_gamma=2.0, power=2 / 3, max_decay=0.99)])
def test_other_schedules_and_the_advance_launcher(dev, sch):
    """siss_ema_advance forms the same 1 - decay as the fold and touches the EMA fields only"""
    for k in (1, 2, 4, 5, 31, 1000):
        blk, _ = norm_single(dev, T.ints(5, 5), TScal(dev, 9, k - 1), ema=sch)
        ref = 1.0 - T.decay_f64(k, **sch)
        assert abs(float(blk[6]) - ref) <= 2 * R.U * ref, (k, blk[6], ref)
        sc = TScal(dev, 9, k - 1)
        launch("siss_ema_advance", *T.ema_args(sch), sc.blk.t)
        alone = sc.read()
        assert alone[5] == k and alone[6] == blk[6] and alone[7] == blk[7] and alone[2] == 9 and alone[0] == 0


# ================================================================ pass 2, bitwise
class EState(State):
    def __init__(self, dev, p, m, v, ema, shadow=True, gout=True):
        super().__init__(dev, p, m, v, shadow, gout)
        self.ema = None if ema is None else Flat(len(p), F32, dev, body=ema)

    def update(self, bg, blk_dev, hp, ema=True):
        launch("siss_clip_adamw_ema", bg.t, self.p.t, self.m.t, self.v.t, self.ema.t if (ema and self.ema is not None) else None,
               None if self.shadow is None else self.shadow.t, None if self.gout is None else self.gout.t, self.n,
               *(float(h) for h in hp), blk_dev)


def restate(g, p, m, v, ema, blk, hp, got_p):
    """the restatement; `1.f - lr * wd` with two roundings, or fused where the device's p says so (tests/test_hip_optimizer.py)"""
    out = T.update_f32(g, p, m, v, ema, blk, hp)
    two, fused = R.decay_two_roundings(hp), R.decay_fused(hp)
    if two != fused and not np.array_equal(out[0].view(np.int32), got_p.view(np.int32)):
        alt = T.update_f32(g, p, m, v, ema, blk, hp, decay=fused)
        if np.array_equal(alt[0].view(np.int32), got_p.view(np.int32)):
            out = alt
    return out


def carried_steps(dev, n, hp, shadow, gout, with_ema, first_step=1):
    p, m, v, ema = T.state(n, n)
    st = EState(dev, p, m, v, ema if with_ema else None, shadow, gout)
    sc = TScal(dev, first_step - 1, first_step - 1)
    for step in range(first_step, first_step + 3):
        g = T.gauss(n, 100 * step + n) * f32(30 if step == first_step + 1 else 1)          # one step that the clip really scales
        blk, bg = norm_single(dev, g, sc, betas=(float(hp[1]), float(hp[2])))
        assert blk[T.NAMES["step"]] == step
        st.update(bg, sc.blk.t, hp)
        got_p = st.p.np()
        p, m, v, ema_new, gc = restate(g, p, m, v, ema if with_ema else None, blk, hp, got_p)
        what = f"n {n} step {step}"
        assert np.isfinite(got_p).all(), what
        st.p.check(Tn(p), f"p, {what}"); st.m.check(Tn(m), f"m, {what}"); st.v.check(Tn(v), f"v, {what}")
        if with_ema:
            st.ema.check(Tn(ema_new), f"ema, {what}")
            ema = ema_new
        if gout:
            st.gout.check(Tn(gc), f"g_out, {what}")
        if shadow:
            st.shadow.check(R.bf16(p), f"shadow, {what}")
            same(st.shadow.t.cpu(), Tn(got_p).to(BF), f"shadow against p.to(bfloat16), {what}")
        bg.check(Tn(g), f"g, {what}")
        same(Tn(sc.read(n)), Tn(blk), "the scalar block after pass 2")


@pytest.mark.parametrize("name", ["mnist", "lr5e-3"])
@pytest.mark.parametrize("n", R.SIZES)
def test_update_is_bitwise_the_f32_restatement(dev, n, name):
    carried_steps(dev, n, R.hyper(*R.HYPER[name]), True, True, True)


@pytest.mark.parametrize("shadow,gout,with_ema", [(False, False, False), (True, False, True), (False, True, False), (False, False, True)])
@pytest.mark.parametrize("n", [5, 1027])
def test_update_with_optional_outputs_absent(dev, n, shadow, gout, with_ema):
    carried_steps(dev, n, R.hyper(*R.HYPER["sd"]), shadow, gout, with_ema, first_step=1000)


@pytest.mark.parametrize("name", ["celeb", "lr5e-3"])
@pytest.mark.parametrize("n", R.SIZES)
def test_single_set_pair_is_bitwise_the_two_set_pair_on_a_zero_second_set(dev, n, name):
    hp = R.hyper(*R.HYPER[name])
    p, m, v, _ = T.state(n, n + 1)
    g = T.gauss(n, n + 2) * f32(200)                            # |g| > 1: the clip coefficient is not 1
    z = np.zeros(n, f32)
    old, osc = State(dev, p, m, v, True, False), Scal(dev, 4)
    bx, ba = Flat(n, F32, dev, body=g), Flat(n, F32, dev, body=z)
    launch("siss_grad_norms_scale", bx.t, ba.t, n, 2, 5.0, 1.0, float(hp[1]), float(hp[2]), osc.partials.t, osc.blk.t)
    oblk = osc.read(n)
    old.adamw(bx, ba, osc.blk.t, hp)
    new, sc = EState(dev, p, m, v, None, True, False), TScal(dev, 4, 0)
    blk, bg = norm_single(dev, g, sc, betas=(float(hp[1]), float(hp[2])))
    new.update(bg, sc.blk.t, hp)
    assert (oblk[5] < 1 or n < 1027) and [blk[i] for i in (0, 1, 2, 3, 4)] == [oblk[i] for i in (4, 5, 6, 8, 9)], (blk, oblk)
    for a, b, what in ((new.p, old.p, "p"), (new.m, old.m, "m"), (new.v, old.v, "v"), (new.shadow, old.shadow, "shadow")):
        same(a.d.cpu(), b.d.cpu(), f"{what}: single-set against two-set, n {n}")


@pytest.mark.parametrize("n", R.SIZES)
def test_fused_ema_is_bitwise_the_unfused_pair(dev, n):
    hp = R.hyper(*R.HYPER["mnist"])
    p, m, v, ema = T.state(n, n + 5)
    g = T.gauss(n, n + 6)
    k = 31
    fused, sc = EState(dev, p, m, v, ema, True, False), TScal(dev, k - 1, k - 1)
    blk, bg = norm_single(dev, g, sc, betas=(float(hp[1]), float(hp[2])))
    assert 0 < blk[6] < 1
    fused.update(bg, sc.blk.t, hp)
    pair = EState(dev, p, m, v, ema, True, False)
    pair.update(bg, sc.blk.t, hp, ema=False)
    pair.ema.check(Tn(ema), "ema untouched without the pointer")
    launch("siss_ema_step", pair.p.t, pair.ema.t, n, sc.blk.t)
    for a, b, what in ((fused.p, pair.p, "p"), (fused.ema, pair.ema, "ema"), (fused.shadow, pair.shadow, "shadow")):
        same(a.d.cpu(), b.d.cpu(), f"{what}: fused against unfused, n {n}")
    pair.ema.check(Tn(T.ema_f32(ema, pair.p.np(), blk)), "siss_ema_step against the restatement")


# ================================================================ the swap
@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("n", R.SIZES)
def test_swap(dev, n, shadow):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    fa, fb = Flat(n, F32, dev, body=a), Flat(n, F32, dev, body=b)
    sh = Flat(n, BF, dev) if shadow else None
    launch("siss_swap_f32", fa.t, fb.t, None if sh is None else sh.t, n)
    fa.check(Tn(b), "a after the swap"); fb.check(Tn(a), "b after the swap")
    if shadow:
        sh.check(R.bf16(b), "shadow = bf16 of the new a")
    launch("siss_swap_f32", fa.t, fb.t, None if sh is None else sh.t, n)
    fa.check(Tn(a), "a after two swaps"); fb.check(Tn(b), "b after two swaps")
    if shadow:
        sh.check(R.bf16(a), "shadow after two swaps")


# ================================================================ refusals
def test_refusals_write_nothing(dev):
    n = 1027
    g = T.gauss(n, 1)
    hp = [float(h) for h in R.hyper(*R.HYPER["mnist"])]
    bg = Flat(n + 4, F32, dev, body=np.append(g, [0] * 4))
    sc = TScal(dev, 3, 3)
    st = EState(dev, g, g, np.abs(g), g)
    ea = T.ema_args(EMA)
    norm = lambda x, nn, e=ea, part=sc.partials.t, blk=sc.blk.t: ("siss_grad_norm_single", x, nn, 1.0, 0.95, 0.999, *e, part, blk)
    upd = lambda x, p, nn, ema=st.ema.t, sh=st.shadow.t, blk=sc.blk.t: ("siss_clip_adamw_ema", x, p, st.m.t, st.v.t, ema, sh, st.gout.t, nn, *hp, blk)
    for args in (norm(bg.t[1:n + 1], n), norm(bg.t[:n], 0), norm(None, n), norm(bg.t[:n], n, part=None), norm(bg.t[:n], n, blk=None),
                 norm(bg.t[:n], n, e=(0.9999, 0.0, 0.0, 0.75, 1, 0)), norm(bg.t[:n], n, e=(1.5, 0.0, 1.0, 0.75, 1, 0)),
                 upd(bg.t[1:n + 1], st.p.t, n), upd(bg.t[:n], st.p.t, 0), upd(bg.t[:n - 1], st.p.t[1:], n - 1), upd(None, st.p.t, n),
                 upd(bg.t[:n - 1], st.p.t[:n - 1], n - 1, ema=st.ema.t[1:]), upd(bg.t[:n - 1], st.p.t[:n - 1], n - 1, sh=st.shadow.t[1:]),
                 upd(bg.t[:n], st.p.t, n, blk=None),
                 ("siss_ema_advance", *ea, None), ("siss_ema_advance", 0.9999, 0.0, 1.0, -1.0, 1, 0, sc.blk.t),
                 ("siss_ema_step", st.p.t[1:], st.ema.t[:n - 1], n - 1, sc.blk.t), ("siss_ema_step", st.p.t, st.ema.t, 0, sc.blk.t),
                 ("siss_ema_step", st.p.t, None, n, sc.blk.t), ("siss_ema_step", st.p.t, st.ema.t, n, None),
                 ("siss_swap_f32", st.p.t, st.ema.t[1:], st.shadow.t, n - 1), ("siss_swap_f32", st.p.t, st.ema.t, st.shadow.t[1:], n - 1),
                 ("siss_swap_f32", st.p.t, st.ema.t, None, 0), ("siss_swap_f32", st.p.t, None, None, n), ("siss_swap_f32", st.p.t, st.p.t, None, n)):
        refused(*args)
    same(sc.blk.d.cpu(), sc.blk.flat, "the scalar block after the refusals")
    same(sc.partials.d.cpu(), sc.partials.flat, "the partial sums after the refusals")
    for b in (st.p, st.m, st.v, st.ema, st.shadow, st.gout, bg):
        same(b.d.cpu(), b.flat, "a buffer after the refusals")


# ================================================================ TrainStepper against the fp32 oracle
def _toy(dtype=torch.float32, seed=3):
    from test_hip_f32_mode import MNIST_TOY
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    unet = UNet2DModel(UNet2DConfig(**MNIST_TOY), device="cuda:0", compute_dtype=dtype)
    sd = unet.engine.init_random(seed=seed)
    return unet, sd, MNIST_TOY


OKW = dict(lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)


def _stepper(unet, ga=1, mp=None):
    from oracle import schedule as S
    from siss_amd.ema import EMAModel
    from siss_amd.train import TrainStepper
    ema = EMAModel(unet, decay=0.9999, use_ema_warmup=True, inv_gamma=1.0, power=0.75, model_cls=type(unet), model_config=unet.config)
    return TrainStepper(unet.engine, S.alphas_cumprod(), grad_accum=ga, ema=ema, mixed_precision=mp, **OKW), ema


def _batch(g, B=4, hw=16):
    return torch.rand(B, 1, hw, hw, generator=g) * 2 - 1, torch.randn(B, 1, hw, hw, generator=g), torch.randint(0, 1000, (B,), generator=g)


def _oracle_steps(unet, st, ema, ga, steps, tol, min_cos, check_ema):
    from oracle import schedule as S
    from oracle.unet import OracleUNet2D, UNetConfig
    from parity_util import masked_update_cosine
    from test_hip_f32_mode import MNIST_TOY
    eng = unet.engine
    net = OracleUNet2D(UNetConfig(**MNIST_TOY)).float()
    opt = torch.optim.AdamW(net.parameters(), **OKW)
    ac = S.alphas_cumprod().float()
    g = torch.Generator().manual_seed(7)
    wgo = eng.wgrad_overwrite
    for step in range(1, steps + 1):
        before = {n: v.clone() for n, v in eng.state_dict().items()}
        net.load_state_dict(before)
        ema_before = ema.flat.cpu().numpy().copy()
        opt.zero_grad()
        for _ in range(ga):
            x0, noise, t = _batch(g)
            xt = ac[t].sqrt().view(-1, 1, 1, 1) * x0 + (1 - ac[t]).sqrt().view(-1, 1, 1, 1) * noise
            loss = F.mse_loss(net(xt, t)[0].float(), noise.float())
            (loss / ga).backward()
            st.micro_step(x0, noise, t.cuda())
        pre = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0))
        gfin = {n: p.grad.clone() for n, p in net.named_parameters()}
        opt.step()
        got = st.stats()
        cos, frac = masked_update_cosine(before, dict(net.named_parameters()), eng.state_dict(), gfin)
        print(f"\n[train-step] GA {ga} step {step}: loss {got['loss']:.7g} / {float(loss):.7g}, |g| {got['pre_clip_norm']:.7g} / {pre:.7g}, "
              f"masked update cosine {cos:.6f}, ema_decay {got['ema_decay']:.6f}, lr {got['lr']}")
        assert abs(got["loss"] - float(loss)) <= tol * abs(float(loss)) and abs(got["pre_clip_norm"] - pre) <= tol * pre
        assert cos >= min_cos and frac > 0.5, (cos, frac)
        assert got["step"] == step and ema.optimization_step == step and got["lr"] == OKW["lr"]
        assert got["ema_decay"] == float(f32(T.decay_f64(step, **EMA))) == float(f32(ema.cur_decay_value))
        assert eng.wgrad_overwrite == wgo                     # left as found
        if check_ema:                                         # the EMA is the host restatement on the engine's OWN iterates
            blk = st.opt.train_scalars.cpu().numpy()
            same(ema.flat.cpu(), Tn(T.ema_f32(ema_before, eng.ps.flat.cpu().numpy(), blk)), f"ema after step {step}")


@pytest.mark.parametrize("ga", [1, 2])
def test_train_stepper_f32_against_the_fp32_oracle(dev, ga):
    unet, _, _ = _toy()
    st, ema = _stepper(unet, ga)
    _oracle_steps(unet, st, ema, ga, 3, 2 * RTOL, 0.9999, True)


def test_train_stepper_bf16_step(dev):
    from parity_util import SCALAR_RTOL, UPDATE_COS
    unet, _, _ = _toy(torch.bfloat16)
    st, ema = _stepper(unet, 1, "bf16")
    _oracle_steps(unet, st, ema, 1, 1, SCALAR_RTOL, UPDATE_COS, True)
    same(unet.engine.ps.shadow.cpu(), unet.engine.ps.flat.cpu().to(BF), "the operand shadow after the fused update")


# ================================================================ resume
def test_resume_restores_the_state_bitwise_and_continues_deterministically(dev, tmp_path):
    from siss_amd.checkpoint import load_state, save_state
    from siss_amd.data import EpochSampler
    unet, _, _ = _toy(seed=4)
    st, ema = _stepper(unet)
    gen = torch.Generator(device=dev).manual_seed(9)
    sampler = EpochSampler(10, 4, 42, 2)
    it = iter(sampler)
    for _ in range(2):
        _, _, idx = next(it)
        x0 = torch.stack([(torch.rand(1, 16, 16, generator=torch.Generator().manual_seed(i)) * 2 - 1) for i in idx]).to(dev)
        st.micro_step(x0, torch.randn(x0.shape, device=dev, generator=gen), torch.randint(0, 1000, (4,), device=dev, generator=gen))
    torch.cuda.synchronize()
    path = save_state(str(tmp_path / "checkpoint-2"), unet, ema, st,
                      dict(global_step=2, epoch=sampler.epoch, position=sampler.position, lr_position=2, generator=gen))
    unet2, _, _ = _toy(seed=5)
    st2, ema2 = _stepper(unet2)
    gen2 = torch.Generator(device=dev)
    state = load_state(path, unet2, ema2, st2, generator=gen2)
    ps, ps2 = unet.engine.ps, unet2.engine.ps

    def held(what):
        for name, a, b in (("p", ps.flat, ps2.flat), ("m", st.opt.m, st2.opt.m), ("v", st.opt.v, st2.opt.v), ("ema", ema.flat, ema2.flat)):
            for k, t in ps.flat_to_ref(a).items():
                same(ps2.flat_to_ref(b)[k], t, f"{name}.{k} {what}")
    held("after load_state")
    b1, b2 = st.opt.train_scalars.cpu(), st2.opt.train_scalars.cpu()
    same(b2, b1, "the scalar block")
    assert b2[2] == 2 and b2[5] == 2 and ema2.optimization_step == 2 == ema.optimization_step and st2.opt.train_ema_step == 2
    assert torch.equal(gen2.get_state(), gen.get_state())
    # the forward pass on a fixed input, under the plain and under the EMA weights
    x, t = torch.randn(2, 1, 16, 16, device=dev, generator=torch.Generator(device=dev).manual_seed(1)), torch.tensor([999, 17], device=dev)
    same(unet2.engine.forward(x, t).cpu(), unet.engine.forward(x, t).cpu(), "forward, plain weights")
    with ema.applied(unet), ema2.applied(unet2):
        e1, e2 = unet.engine.forward(x, t).cpu(), unet2.engine.forward(x, t).cpu()
    same(e2, e1, "forward, EMA weights")
    assert not torch.equal(e1, unet.engine.forward(x, t).cpu())
    held("after the swap and back")
    # one update on the SAME synthetic gradient from both states
    gsyn = torch.randn(ps.total, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 0.01
    st.opt.launch_single(gsyn, ema=ema)
    st2.opt.launch_single(gsyn.clone(), ema=ema2)
    held("after one more update")
    same(st2.opt.train_scalars.cpu(), st.opt.train_scalars.cpu(), "the scalar block after one more update")
    assert st.opt.train_scalars.cpu()[5] == 3 and ema2.optimization_step == 3
    # what the loop draws next
    resumed = EpochSampler(10, 4, 42, 2, epoch=state["epoch"], position=state["position"])
    assert list(resumed) == list(it) == T.remaining(10, 4, 42, 2, 0, 2)
    assert torch.equal(torch.randn(4, 1, 16, 16, device=dev, generator=gen2), torch.randn(4, 1, 16, 16, device=dev, generator=gen))
    assert torch.equal(torch.randint(0, 1000, (4,), device=dev, generator=gen2), torch.randint(0, 1000, (4,), device=dev, generator=gen))


def test_ema_step_after_an_update_something_else_made(dev):
    """EMAModel.step(parameters) on its own, from the model and from unet.parameters(): the block follows the host's count"""
    unet, _, _ = _toy(seed=6)
    _, ema = _stepper(unet)
    flat = unet.engine.ps.flat
    for k, params in ((1, unet), (2, unet.parameters()), (3, unet)):
        flat.add_(0.01 * torch.randn(flat.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(k)))
        before = ema.flat.cpu().numpy().copy()
        ema.step(params)
        blk = ema.scalars.cpu().numpy()
        assert blk[5] == k == ema.optimization_step and abs(float(blk[6]) - (1 - T.decay_f64(k, **EMA))) <= 2 * R.U
        same(ema.flat.cpu(), Tn(T.ema_f32(before, flat.cpu().numpy(), blk)), f"ema.step {k}")


# ================================================================ the loop through main.main
TOY = ["unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]", "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]",
       "+unet.layers_per_block=1", "resolution=16", "train_batch_size=4", "allow_synthetic=true", "pipeline.num_inference_steps=2"]


def test_train_loop_checkpoints_resumes_and_feeds_the_delete_task(dev, tmp_path):
    """10 synthetic images, B = 4 (batches of 4, 4, 2), two epochs = six steps, a checkpoint every 2, a grid every 3.  The resumed run
    stands for a run that was cut off after step 5: checkpoint-6 of the first run is taken away before it starts (main.py puts a
    resumed run back into its directory through resume_from_checkpoint, as the reference's does)."""
    import main
    out = tmp_path / "base"
    train = ["--config-name=train_tshirt_mnist", *TOY, f"output_dir={out}", "dataset.name=/nonexistent", "+synthetic_images=10", "num_epochs=2",
             "checkpointing_steps=2", "sampling_steps=3", "eval_batch_size=4", "lr_warmup_steps=2"]
    main.main(train)
    (run,) = glob.glob(str(out / "*"))
    for step in (2, 4, 6):
        assert sorted(os.listdir(os.path.join(run, f"checkpoint-{step}"))) == ["optimizer.safetensors", "state.json", "unet", "unet_ema"]
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(run, "samples_step*.png"))) == ["samples_step3.png", "samples_step6.png"]
    assert os.path.isfile(os.path.join(run, "unet", "config.json")) and os.path.isfile(os.path.join(run, "unet_ema", "diffusion_pytorch_model.safetensors"))
    lines = [json.loads(l) for l in open(os.path.join(run, "train_log_rank0.jsonl"))]
    assert [r["step"] for r in lines] == [1, 2, 3, 4, 5, 6] and [r["epoch"] for r in lines] == [0, 0, 0, 1, 1, 1]
    assert all(np.isfinite(r["loss"]) and r["pre_clip_norm"] > 0 for r in lines)
    assert [r["ema_decay"] for r in lines] == [float(f32(T.decay_f64(k, **EMA))) for k in range(1, 7)]
    from siss_amd.scheduler import lr_multiplier
    assert [r["lr"] for r in lines] == [1e-4 * lr_multiplier("cosine", k, 2, 6) for k in range(6)]
    st4 = json.load(open(os.path.join(run, "checkpoint-4", "state.json")))
    assert (st4["global_step"], st4["epoch"], st4["position"], st4["lr_position"]) == (4, 1, 1, 4)
    # resume
    import shutil
    shutil.rmtree(os.path.join(run, "checkpoint-6"))
    stamp = os.path.basename(run)
    main.main(train + [f"checkpoint_path={run}/checkpoint-4", f"resume_from_checkpoint={stamp}/checkpoint-4", "checkpoints_total_limit=2"])
    again = [json.loads(l) for l in open(os.path.join(run, "train_log_rank0.jsonl"))][6:]
    assert [r["step"] for r in again] == [5, 6] and [r["lr"] for r in again] == [r["lr"] for r in lines[4:]]
    assert [r["ema_decay"] for r in again] == [r["ema_decay"] for r in lines[4:]]
    assert sorted(d for d in os.listdir(run) if d.startswith("checkpoint-")) == ["checkpoint-4", "checkpoint-6"]
    # the delete task loads unet_ema of the checkpoint (its config.json carries the seven EMA keys) and runs one step
    dele = tmp_path / "deletion"
    main.main(["--config-name=delete_tshirt", *TOY, f"output_dir={dele}", f"checkpoint_path={run}/checkpoint-4", "training_steps=1", "save_final=false"])
    (drun,) = glob.glob(str(dele / "*"))
    (rec,) = [json.loads(l) for l in open(os.path.join(drun, "train_log_rank0.jsonl"))]
    assert rec["global_step"] == 1 and np.isfinite(rec["norm_loss_x"]) and rec["norm_loss_x"] > 0

"""csrc/teacher.hip and the teacher-target step (siss_amd/teacher.py, SISSStepper(loss_fn="teacher_target", teacher=...)) on the GPU,
against tests/teacher_ref.py (which tests/test_teacher_host.py checks against itself on the CPU).

1. siss_teacher_seed called directly: cot bitwise the f32 restatement, sums within 1 ulp of f32(the f64 sum), for every keep x forget
   combination, f32 and bf16 noise, eta in {0, 1, 2.5}, at (B, chw) = (1, 1), (1, 7), (2, 8), (2, 1024), (3, 1028), one row of three
   chunks and one whose 66 chunks outnumber the 64 blocks a row gets; eta = 0 gives u bit for bit; integer-valued inputs give exact
   sums; the guard words around every output and the inputs are intact; the refusals write nothing.
2. siss_grad_norms_weighted called directly: the scalar block bitwise the restatement at the sizes of tests/test_hip_optimizer.py; exact
   sums on integers; a following siss_recombine_clip_adamw moves p, m, v bitwise as the restated AdamW with g = clip (g_x + w g_a);
   w = 1 on g_a = 0 reproduces the plain pair's parameters.
3. Two steps of the f32 UNetCondEngine beside OracleUNet2DCondition in f64 with a second oracle network as the teacher, at the step
   bounds of tests/test_hip_f32_mode.py (scalars 2e-4 relative, masked update cosine >= 0.9999 over more than half of the elements);
   the same definition with the forget target replaced by the drawn noise misses them at step 2.
4. The bf16 step is FlatAdamW.launch(fixed_weight=...) on its own gradients; the teacher keeps every bit; esd and anchor differ.
5. A captured step replays to the eager step's bits.  6. The call logs.  7. deletion.lora combines, the other four are refused.
8. The delete_sd task with the key.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as O
import teacher_ref as R
from test_hip_optimizer import BF, F32, F64, GUARD, Flat, Scal, State, T, launch, refused, restate
from test_hip_small_kernels import bits, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
HP = O.hyper(*O.HYPER["sd"])
COMBOS = [(k, f) for k in R.KEEPS for f in R.FORGETS]
ETAS = (0.0, 1.0, 2.5)
# (B, chw): one element; a scalar-path row (chw % 4 != 0); two granules; a quarter chunk; 257 granules over three rows; three chunks, the
# last one partial (chw % 4 = 2: the scalar path over several chunks); 66 chunks, more than the 64 blocks a row gets (chw % 4 = 1)
SHAPES = [(1, 1), (1, 7), (2, 8), (2, 1024), (3, 1028), (1, 2 * R.CHUNK + 1030), (2, 3 * R.CHUNK + 1028), (1, 65 * R.CHUNK + 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ================================================================ 1. siss_teacher_seed
class Seed:
    """The buffers of one call: inputs and outputs between sentinel guards."""

    def __init__(self, dev, pred, noise, teach, noise_bf16):
        self.R, self.chw = pred.shape
        self.pred_h, self.teach_h = pred, teach
        self.noise_h = T(noise).to(BF) if noise_bf16 else T(noise)
        self.noise_f32 = self.noise_h.float().numpy()                 # what the kernel reads, as f32
        self.pred = Flat(pred.size, F32, dev, body=T(pred).flatten())
        self.teach = Flat(teach.size, F32, dev, body=T(teach).flatten())
        self.noise = Flat(noise.size, BF if noise_bf16 else F32, dev, body=self.noise_h.flatten())
        self.bf16 = noise_bf16
        self.cot = Flat(pred.size, F32, dev)
        self.sums = Flat(self.R, F32, dev)
        self.partials = Flat(R.partials_words(self.R, self.chw), F64, dev, fill=-5.0)

    def args(self, B, keep, forget, eta, scale, teach_rows=None):
        return (self.pred.t, self.noise.t, int(self.bf16), self.teach.t, self.teach_h.shape[0] if teach_rows is None else teach_rows, B,
                self.chw, R.KEEPS.index(keep), R.FORGETS.index(forget), eta, scale, self.cot.t, self.sums.t, self.partials.t)

    def inputs_intact(self, what):
        self.pred.check(T(self.pred_h).flatten(), f"pred, {what}")
        self.teach.check(T(self.teach_h).flatten(), f"teach, {what}")
        self.noise.check(self.noise_h.flatten(), f"noise, {what}")

    def outputs_untouched(self, what):
        for b, name in ((self.cot, "cot"), (self.sums, "sums"), (self.partials, "partials")):
            same(b.d.cpu(), b.flat, f"{name} written by a refused call, {what}")


def seed_inputs(B, chw, keep, seed, integers=False):
    rng = np.random.default_rng(seed)
    Rn = B if keep == "none" else 2 * B
    draw = (lambda *s: rng.integers(-8, 9, s).astype(f32)) if integers else (lambda *s: rng.standard_normal(s).astype(f32))
    return draw(Rn, chw), draw(B, chw), draw(3 * B, chw)             # (the teacher buffer always holds 3 B rows: the most a call reads)


@pytest.mark.parametrize("B,chw", SHAPES)
def test_seed_is_bitwise_the_restatement(dev, B, chw):
    from siss_amd import lib
    assert lib.query("siss_teacher_partials_words", 2 * B, chw) == R.partials_words(2 * B, chw)
    assert lib.query("siss_teacher_partials_words", 0, chw) == 0
    worst = 0.0
    for keep in R.KEEPS:
        pred, noise, teach = seed_inputs(B, chw, keep, 7 * B + chw)
        for noise_bf16 in (False, True):
            s = Seed(dev, pred, noise, teach, noise_bf16)
            for forget in R.FORGETS:
                for eta in ETAS:
                    what = f"B {B} chw {chw} keep {keep} forget {forget} bf16 {noise_bf16} eta {eta}"
                    scale = 1.0 / (2 * B)
                    launch("siss_teacher_seed", *s.args(B, keep, forget, eta, scale))
                    cot, sums, y = R.seed(pred, s.noise_f32, teach, B, keep, forget, eta, scale)
                    s.cot.check(T(cot).flatten(), f"cot, {what}")
                    got = s.sums.np()
                    s.sums.guards(f"sums, {what}")
                    s.partials.guards(f"partials, {what}")
                    for r in range(s.R):
                        err = abs(float(got[r]) - float(f32(sums[r]))) / R.ulp32(sums[r]) if sums[r] else abs(float(got[r]))
                        worst = max(worst, err)
                        assert err <= 1.0, (what, r, got[r], sums[r])
                    if forget == "esd" and eta == 0.0:
                        _, Rt, k0, u0 = R.rows(keep, forget, B)
                        u = teach[u0:u0 + B]
                        want = (f32(2) * f32(scale)) * (pred[-B:] - u)
                        same(s.cot.t.cpu().view(s.R, chw)[-B:], T(want), f"eta = 0: the esd target is not u, {what}")
                    s.inputs_intact(what)
    print(f"\n[teacher] seed B {B} chw {chw}: worst |sums - f32(f64 sum)| {worst:.2f} ulp (allowed 1)")


@pytest.mark.parametrize("B,chw", [(2, 8), (3, 1028), (1, 2 * R.CHUNK + 1030)])
def test_seed_on_integers_has_exact_sums(dev, B, chw):
    for keep, forget in COMBOS:
        pred, noise, teach = seed_inputs(B, chw, keep, 11, integers=True)
        s = Seed(dev, pred, noise, teach, True)                       # (integers in [-8, 8] are exact in bf16)
        launch("siss_teacher_seed", *s.args(B, keep, forget, 1.0, 0.25))
        cot, sums, y = R.seed(pred, noise, teach, B, keep, forget, 1.0, 0.25)
        assert sums.max() < 2 ** 24 and np.array_equal(sums, np.round(sums))
        s.cot.check(T(cot).flatten(), f"cot on integers, {keep} {forget}")
        s.sums.check(T(sums.astype(f32)), f"sums on integers, {keep} {forget}")


def test_seed_refusals_write_nothing(dev):
    B, chw = 2, 1028
    pred, noise, teach = seed_inputs(B, chw, "teacher", 3)
    s = Seed(dev, pred, noise, teach, False)
    ok = s.args(B, "teacher", "esd", 1.0, 0.25)
    names = ("pred", "noise", "noise_bf16", "teach", "teach_rows", "B", "chw", "keep_mode", "forget_mode", "eta", "scale", "cot", "sums", "partials")
    def but(**kw):
        return tuple(kw.get(n, a) for n, a in zip(names, ok))
    for name in ("pred", "teach", "cot", "sums", "partials"):
        refused("siss_teacher_seed", *but(**{name: None}))
    refused("siss_teacher_seed", *but(noise=None, keep_mode=0))       # keep: noise reads it
    refused("siss_teacher_seed", *but(B=0))
    refused("siss_teacher_seed", *but(B=-1))
    refused("siss_teacher_seed", *but(chw=0))
    refused("siss_teacher_seed", *but(teach_rows=3 * B - 1))          # keep: teacher + esd reads 3 B rows
    refused("siss_teacher_seed", *but(teach_rows=2 * B - 1, keep_mode=0))
    refused("siss_teacher_seed", *but(teach_rows=2 * B - 1, forget_mode=1))
    refused("siss_teacher_seed", *but(teach_rows=B - 1, keep_mode=2, forget_mode=1))
    for k, v in (("keep_mode", 3), ("keep_mode", -1), ("forget_mode", 2), ("forget_mode", -1)):
        refused("siss_teacher_seed", *but(**{k: v}))
    refused("siss_teacher_seed", *but(pred=s.pred.t.flatten()[1:]))   # not 16-byte aligned
    s.outputs_untouched("after the refusals")
    s.inputs_intact("after the refusals")
    launch("siss_teacher_seed", *but(noise=None))                     # keep: teacher never reads the noise
    launch("siss_teacher_seed", *but(teach_rows=2 * B, keep_mode=2))  # exactly enough rows
    cot, _, _ = R.seed(pred[:B], noise, teach, B, "none", "esd", 1.0, 0.25)
    same(s.cot.t.cpu()[:B * chw], T(cot).flatten(), "cot after the refusals")


# ================================================================ 2. siss_grad_norms_weighted
def weighted(dev, gx, ga, weight, sc=None, max_norm=1.0, step_before=0):
    n = len(gx)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    sc = sc or Scal(dev, step_before)
    launch("siss_grad_norms_weighted", bx.t, ba.t, n, weight, max_norm, float(HP[1]), float(HP[2]), sc.partials.t, sc.blk.t)
    bx.check(T(gx), "gx after the weighted norms"); ba.check(T(ga), "ga after the weighted norms")
    return sc.read(n), bx, ba, sc


WSIZES = [1, 3, 1027, 100_003, 2_097_152 + 1027]
assert set(WSIZES) <= set(O.SIZES)


@pytest.mark.parametrize("n", WSIZES)
def test_weighted_block_is_bitwise_the_restatement(dev, n):
    for weight, step_before in ((1.0, 0), (0.75, 6)):
        gx, ga = O.gauss_pair(n, n + 17)
        blk, *_ = weighted(dev, gx, ga, weight, step_before=step_before)
        ref = R.weighted_block(gx, ga, weight, 1.0, HP[1], HP[2], step_before)
        idx = list(O.NAMES.values())
        assert np.array_equal(blk[idx].view(np.uint32), ref[idx].view(np.uint32)), (n, weight, blk[idx], ref[idx])
        assert blk[3] == f32(-weight) and blk[6] == step_before + 1


@pytest.mark.parametrize("n", WSIZES)
def test_weighted_sums_on_integers_are_exact(dev, n):
    gx, ga = O.int_pair(n, n)
    xx, aa, xa = O.int_sums(gx, ga)
    blk, *_ = weighted(dev, gx, ga, 2.0)
    import math
    assert blk[0] == f32(math.sqrt(xx)) and blk[1] == f32(math.sqrt(aa)) and blk[2] == f32(xa), (blk[:3], xx, aa, xa)
    assert blk[3] == -2.0 and blk[4] == f32(math.sqrt(xx + 4 * xa + 4 * aa)), blk                # exact integers under the root


def test_weighted_refusals_write_nothing(dev):
    gx, ga = O.gauss_pair(1027, 1)
    bx, ba = Flat(1027, F32, dev, body=gx), Flat(1027, F32, dev, body=ga)
    sc = Scal(dev)
    ok = (bx.t, ba.t, 1027, 1.0, 1.0, 0.95, 0.999, sc.partials.t, sc.blk.t)
    for i, bad in ((0, None), (1, None), (7, None), (8, None), (2, 0), (3, 0.0), (3, -1.0), (3, float("inf")), (3, float("nan")),
                   (0, bx.t[1:])):
        refused("siss_grad_norms_weighted", *(bad if j == i else a for j, a in enumerate(ok)))
    same(sc.blk.d.cpu(), sc.blk.flat, "the scalar block after the refusals")
    same(sc.partials.d.cpu(), sc.partials.flat, "the partial sums after the refusals")


@pytest.mark.parametrize("n", [3, 1027, 100_003])
def test_the_plain_pass_2_after_the_weighted_pass_1(dev, n):
    """two steps, the state carried: p, m, v, g_out bitwise the restated AdamW with g = clip (g_x + w g_a), the shadow its bf16 rounding"""
    rng = np.random.default_rng(n)
    p, m, v = rng.standard_normal(n).astype(f32), np.zeros(n, f32), np.zeros(n, f32)
    st, sc = State(dev, p, m, v, True, True), Scal(dev)
    for step, weight in enumerate((0.75, 2.0), 1):
        gx, ga = O.gauss_pair(n, 100 * step + n)
        blk, bx, ba, _ = weighted(dev, gx, ga, weight, sc=sc)
        assert blk[6] == step and blk[3] == f32(-weight)
        st.adamw(bx, ba, sc.blk.t, HP)
        got_p = st.p.np()
        p, m, v, g = restate(gx, ga, p, m, v, blk, HP, got_p)
        # the restatement's g = (gx - s ga) * clip with s = -w IS clip (gx + w ga), operation for operation
        assert np.array_equal(g, (gx + f32(weight) * ga) * blk[5])
        what = f"n {n} step {step}"
        st.p.check(T(p), f"p, {what}"); st.m.check(T(m), f"m, {what}"); st.v.check(T(v), f"v, {what}")
        st.gout.check(T(g), f"g_out, {what}")
        st.shadow.check(O.bf16(p), f"shadow, {what}")


def test_weight_one_on_a_zero_forget_set_is_the_plain_pair(dev):
    n = 1027
    gx, _ = O.gauss_pair(n, 5)
    ga = np.zeros(n, f32)
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(n).astype(f32)
    out = []
    for path in ("weighted", "plain"):
        st, sc = State(dev, p0, np.zeros(n, f32), np.zeros(n, f32), True, False), Scal(dev)
        bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
        if path == "weighted":
            launch("siss_grad_norms_weighted", bx.t, ba.t, n, 1.0, 1.0, float(HP[1]), float(HP[2]), sc.partials.t, sc.blk.t)
        else:                                                        # the inf-guarded norm fix: s = 0 on |g_a| = 0
            launch("siss_grad_norms_scale", bx.t, ba.t, n, 2, 5.0, 1.0, float(HP[1]), float(HP[2]), sc.partials.t, sc.blk.t)
        st.adamw(bx, ba, sc.blk.t, HP)
        out.append((st.p.np().copy(), st.m.np().copy(), st.v.np().copy(), sc.read(n)))
    (pw, mw, vw, bw), (pp, mp, vp, bp) = out
    assert bw[3] == -1.0 and bp[3] == 0.0
    for i in (0, 1, 2, 4, 5, 6, 8, 9):
        assert bw[i] == bp[i], (i, bw, bp)
    assert np.array_equal(pw.view(np.uint32), pp.view(np.uint32)) and np.array_equal(mw, mp) and np.array_equal(vw, vp)


# ================================================================ engines, teachers and steppers
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)
LCTX, XDIM = 77, 64


def cond_config():
    from siss_amd.config import UNet2DConditionConfig
    from oracle.unet_cond import UNetCondConfig
    oc = UNetCondConfig.tiny(ch=(64, 128), heads=2, cross_dim=XDIM, sample_size=16, in_channels=4)
    oc.layers_per_block = 1
    kw = {k: getattr(oc, k) for k in ("sample_size", "in_channels", "out_channels", "block_out_channels", "down_block_types",
                                      "up_block_types", "layers_per_block", "attention_head_dim", "cross_attention_dim",
                                      "norm_num_groups", "norm_eps", "downsample_padding", "flip_sin_to_cos", "freq_shift")}
    return UNet2DConditionConfig(**kw)


_W = {}


def make_engine():
    from siss_amd.unet_cond import UNetCondEngine
    eng = UNetCondEngine(cond_config(), "cuda:0")
    if "sd" not in _W:
        _W["sd"] = eng.init_random(seed=4)
    else:
        eng.load_state_dict(_W["sd"])
    return eng


def embeddings(dev):
    g = torch.Generator().manual_seed(9)
    e = lambda: torch.randn(1, LCTX, XDIM, generator=g)
    return dict(prompt=e().to(dev), empty=e().to(dev), anchor=e().to(dev))


def batch(step, dev, B=2):
    g = torch.Generator().manual_seed(100 + step)
    x0 = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    a0 = torch.randn(1, 4, 16, 16, generator=g).repeat(B, 1, 1, 1).to(dev)
    noise = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    cond = {"encoder_hidden_states": embeddings(dev)["prompt"].repeat(B, 1, 1)}
    return x0, a0, noise, torch.tensor([999, 300, 999, 50][:B], device=dev), torch.tensor([0.9, 0.2, 0.7, 0.4][:B], device=dev), cond


def teacher_cfg(forget="esd", keep="teacher", guidance=1.0, weight=1.0):
    from siss_amd.teacher import parse_teacher
    return parse_teacher(dict(forget=forget, keep=keep, guidance=guidance, weight=weight,
                              anchor_prompt="an anchor" if forget == "anchor" else None))


def stepper(dev, cfg=None, loss_fn=None, **kw):
    """(engine, stepper) on the bf16 tiny conditional UNet; cfg: a TeacherConfig (then loss_fn = teacher_target with a Teacher) or None"""
    from siss_amd.step import SISSStepper
    from siss_amd.teacher import Teacher
    from oracle import schedule as S
    eng = make_engine()
    extra = {}
    if cfg is not None:
        e = embeddings(dev)
        extra = dict(teacher=Teacher(eng).set_embeddings(empty=e["empty"], anchor=e["anchor"]), teacher_cfg=cfg)
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16",
                     loss_fn=loss_fn or ("teacher_target" if cfg is not None else "double_forward_with_neg_del"), **HPK, **extra, **kw)
    return eng, st


def state_of(eng, st):
    return dict(p=eng.ps.flat.clone(), shadow=eng.ps.shadow.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), scalars=st.opt.scalars.clone())


# ================================================================ 3. the f32 step against the definition
def by_name(d, names):
    return np.concatenate([d[n].detach().double().flatten().numpy() for n in names])


def split(vec, like, names):
    out, off = {}, 0
    for n in names:
        k = like[n].numel()
        out[n] = torch.from_numpy(np.ascontiguousarray(vec[off:off + k])).view(like[n].shape)
        off += k
    return out


@pytest.mark.parametrize("forget,keep,weight", [("esd", "teacher", 1.0), ("anchor", "noise", 0.5)])
def test_f32_step_matches_the_definition(dev, forget, keep, weight):
    """Two steps.  The definition: tests/teacher_ref.py's objective under autograd on the f64 oracle network with a second oracle network
    holding the initial weights as the teacher, g = g_x + weight g_a, clip at 1, AdamW in f64.  The negative control regresses the forget
    rows onto the drawn noise instead: on the CPU oracle alone (the same architecture, generator and two steps), its |g_a| at step 2 was
    6.7 times the definition's for esd / teacher (3196 against 477) and 11.5 times for anchor / noise (3010 against 261) -- a random-init
    network's prediction is far from the noise, while the student starts AT the teacher -- and the cosine between the two updates 0.49
    and 0.96: it misses the scalar bound by four orders of magnitude, and the update bound.  That precondition is asserted from the
    definition alone before the control."""
    from siss_amd.step import SISSStepper
    from siss_amd.teacher import Teacher
    from oracle import schedule as S
    from oracle.unet_cond import OracleUNet2DCondition
    from parity_util import check_scalars, masked_update_cosine
    from test_hip_lora_conv import f32_pair
    TOL, B, L = 2e-4, 2, 13
    eng, net, sd, ch, xdim = f32_pair("cond", seed=5)
    tnet = OracleUNet2DCondition(net.cfg).double()
    tnet.load_state_dict({k: v.double() for k, v in sd.items()})
    for p in tnet.parameters():
        p.requires_grad_(False)
    names = [n for n, _ in net.named_parameters()]
    assert set(names) == set(sd)
    ac = S.alphas_cumprod()
    okw = dict(lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    hp = O.hyper(okw["lr"], *okw["betas"], okw["eps"], okw["weight_decay"])
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    prompt, empty, anchor = rnd(1, L, xdim), rnd(1, L, xdim), rnd(1, L, xdim)
    cfg = teacher_cfg(forget, keep, 1.0, weight)
    teacher = Teacher(eng).set_embeddings(empty=empty, anchor=anchor)
    st = SISSStepper(eng, ac, scaling_norm=5.0, train_batch_size=B, mixed_precision=None, loss_fn="teacher_target", teacher=teacher,
                     teacher_cfg=cfg, **okw)
    t_flat0 = teacher.engine.ps.flat.clone()
    student = lambda x, t, c: net(x, t, c)[0]
    teach = lambda x, t, c: tnet(x, t, c)[0]
    params = [p for _, p in net.named_parameters()]
    m = v = np.zeros(sum(sd[n].numel() for n in names))
    keys = ("norm_loss_x", "norm_loss_a", "scaling_factor", "pre_clip_norm")
    for step in (1, 2):
        before = {n: t.clone() for n, t in eng.state_dict().items()}
        net.load_state_dict({k: v_.double() for k, v_ in before.items()})
        x0, a0, noise = rnd(B, ch, 16, 16), rnd(1, ch, 16, 16).repeat(B, 1, 1, 1), rnd(B, ch, 16, 16)
        t = torch.tensor([999, 400])
        x_t, a_t = S.add_noise(ac.double(), x0.double(), noise.double(), t), S.add_noise(ac.double(), a0.double(), noise.double(), t)
        cond = prompt.double().repeat(B, 1, 1)
        args = (x_t, a_t, t, cond, noise.double())
        kw = dict(keep=keep, forget=forget, eta=1.0, weight=weight, batch=B, empty=empty.double(), anchor=anchor.double())
        gx, ga, lx, la = R.gradient_pair(student, params, teach, *args, **kw)
        ga0 = ga
        if step == 2:                                    # the control: the same definition, the forget rows regressed onto the noise
            ga0 = R.gradient_pair(student, params, teach, *args, **kw, forget_target=noise.double())[1]
        gxv, gav, ga0v = (by_name(dict(zip(names, g)), names) for g in (gx, ga, ga0))
        pv = by_name(before, names)
        (p1, m1, v1, gf), sc = R.weighted_step_f64(gxv, gav, pv, m, v, step, hp, weight, 1.0)
        (p0, _, _, gf0), sc0 = R.weighted_step_f64(gxv, ga0v, pv, m, v, step, hp, weight, 1.0)
        st.step(x0, a0, noise, t.cuda(), torch.zeros(B), {"encoder_hidden_states": prompt.repeat(B, 1, 1).cuda()})
        got = st.stats()
        ref = dict(norm_loss_x=sc["norm_x"], norm_loss_a=sc["norm_a"], scaling_factor=sc["scale"], pre_clip_norm=sc["pre_clip_norm"])
        ctl = dict(norm_loss_x=sc0["norm_x"], norm_loss_a=sc0["norm_a"], scaling_factor=sc0["scale"], pre_clip_norm=sc0["pre_clip_norm"])
        after = eng.state_dict()
        cos, frac = masked_update_cosine(before, split(p1, before, names), after, split(gf, before, names))
        print(f"\n[teacher] {forget} / {keep} step {step}: " + ", ".join(f"{k} {got[k]:.7g} / {ref[k]:.7g} (control {ctl[k]:.7g})" for k in keys)
              + f"; loss_x {got.get('loss_x/mean', float('nan')):.6g} / {lx / (ch * 256):.6g}, loss_a {got['loss_a/mean']:.6g} / "
              f"{la / (ch * 256):.6g}; masked update cosine {cos:.6f} over {frac:.2f}")
        if keep == "teacher" and step == 1:
            # the student IS the teacher at step 1: the keep rows' error, their loss and g_x are exactly zero
            assert got["loss_x/mean"] == 0.0 and got["loss_x/max"] == 0.0 and got["norm_loss_x"] == 0.0, got
            assert ref["norm_loss_x"] == 0.0 and lx == 0.0
        check_scalars(ref, got, keys=keys, tol=TOL)
        assert got["scaling_factor"] == -weight and got["step"] == step
        assert cos >= 0.9999 and frac > 0.5, (cos, frac)
        assert abs(got["loss_a/mean"] - la / (ch * 256)) <= TOL * la / (ch * 256)
        if step == 2:
            # the precondition of the negative control, from the definition alone; then the control
            assert abs(ref["norm_loss_a"] - ctl["norm_loss_a"]) >= 100 * TOL * abs(ref["norm_loss_a"]), (ref, ctl)
            with pytest.raises(AssertionError):
                check_scalars(ctl, got, keys=("norm_loss_a",), tol=TOL)
            cos0, _ = masked_update_cosine(before, split(p0, before, names), after, split(gf0, before, names))
            print(f"[teacher] {forget} / {keep} step 2: masked update cosine against the definition with the NOISE as the forget target {cos0:.6f}")
            assert cos0 < 0.9999, "the control passes the update bound too: the teacher's target is not in the update"
        m, v = m1, v1
    assert torch.equal(bits(teacher.engine.ps.flat), bits(t_flat0)), "the teacher's weights moved"


# ================================================================ 4. the bf16 step
def test_the_step_is_the_weighted_pair_on_its_own_gradients(dev):
    """the stepper's update = FlatAdamW.launch(fixed_weight=...) on the gradients that very step produced; the teacher keeps every bit
    over three steps; esd and anchor end in different parameters"""
    from siss_amd import lib
    from siss_amd.optim import FlatAdamW
    results = {}
    for forget in ("esd", "anchor"):
        eng, st = stepper(dev, teacher_cfg(forget, "teacher", 1.0, 0.75))
        th = st.teacher
        assert th.engine.ps.grads.numel() == 0 and th.engine is not eng and th.nbytes == eng.ps.total * 6
        assert torch.equal(bits(th.engine.ps.flat), bits(eng.ps.flat)) and torch.equal(bits(th.engine.ps.shadow), bits(eng.ps.shadow))
        frozen = (th.engine.ps.flat.clone(), th.engine.ps.shadow.clone())
        for step in range(3):
            snap, orig = {}, lib.call

            def spy(name, *a, **k):
                if name == "siss_grad_norms_weighted":
                    snap.update(g=eng.ps.grads.clone(), p=eng.ps.flat.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), sc=st.opt.scalars.clone())
                return orig(name, *a, **k)
            lib.call = spy
            try:
                st.step(*batch(step, dev))
            finally:
                lib.call = orig
            torch.cuda.synchronize()
            assert snap, "the weighted pass 1 did not run"
            ref = FlatAdamW(snap["p"], max_grad_norm=1.0, lr=HPK["lr"], betas=HPK["betas"], eps=HPK["eps"], weight_decay=HPK["weight_decay"])
            ref.m.copy_(snap["m"]); ref.v.copy_(snap["v"]); ref.scalars.copy_(snap["sc"])
            ref.launch(snap["g"], fixed_weight=0.75)
            torch.cuda.synchronize()
            assert torch.equal(eng.ps.flat, ref.p) and torch.equal(st.opt.m, ref.m) and torch.equal(st.opt.v, ref.v)
            assert torch.equal(bits(st.opt.scalars), bits(ref.scalars))
            got = st.stats()
            assert got["scaling_factor"] == -0.75 and got["step"] == step + 1 and "loss_x/mean" in got and "loss_a/mean" in got
            print(f"\n[teacher] bf16 {forget} step {step + 1}: |g_x| {got['norm_loss_x']:.6g} |g_a| {got['norm_loss_a']:.6g} loss_x "
                  f"{got['loss_x/mean']:.6g} loss_a {got['loss_a/mean']:.6g}")
            assert torch.equal(bits(th.engine.ps.flat), bits(frozen[0])) and torch.equal(bits(th.engine.ps.shadow), bits(frozen[1]))
        assert not torch.equal(eng.ps.flat, frozen[0]), "the student did not move"
        fields = st.log_fields()
        assert (fields["teacher_forget"], fields["teacher_keep"], fields["teacher_guidance"], fields["teacher_weight"]) == (forget, "teacher", 1.0, 0.75)
        assert fields["teacher_rows"] == (6 if forget == "esd" else 4)
        results[forget] = eng.ps.flat.clone()
    assert not torch.equal(results["esd"], results["anchor"])


def test_keep_none_runs_one_set_with_the_weight_in_the_scale(dev):
    eng, st = stepper(dev, teacher_cfg("esd", "none", 2.5, 0.5))
    st.step(*batch(0, dev))
    torch.cuda.synchronize()
    got = st.stats()
    assert not eng.ps.grads[1].any() and eng.ps.grads[0].any()
    assert got["scaling_factor"] == 0.0 and got["norm_loss_a"] == 0.0 and got["norm_loss_x"] > 0 and "loss_x/mean" not in got
    assert st.log_fields()["teacher_rows"] == 4
    # the same rows at weight 1: the gradient set is twice this one's (the weight is a factor of the cotangent)
    eng2, st2 = stepper(dev, teacher_cfg("esd", "none", 2.5, 1.0))
    st2.step(*batch(0, dev))
    torch.cuda.synchronize()
    ratio = float(st2.stats()["norm_loss_x"]) / float(got["norm_loss_x"])
    assert abs(ratio - 2.0) <= 2e-2, ratio


# ================================================================ 5. capture
def test_captured_teacher_step_replays_to_the_eager_bits(dev):
    cfg = teacher_cfg("esd", "teacher", 2.5, 0.75)
    eng, st = stepper(dev, cfg)
    loaded = eng.ps.flat.clone()
    args = batch(0, dev)
    # (one warm step first, so that the eager step compared below is not the trivial first one -- and starts where the graph starts)
    eng.ps.flat.add_(torch.randn(eng.ps.total, generator=torch.Generator().manual_seed(1)).to(dev) * 1e-3)
    eng.refresh_weights(cast_shadow=True)
    moved = eng.ps.flat.clone()
    st.step(*args)
    torch.cuda.synchronize()
    eager = state_of(eng, st)
    assert float(eager["scalars"][0]) > 0, "the keep gradient is zero: the student still equals the teacher"
    eng2, st2 = stepper(dev, cfg)
    assert torch.equal(st2.teacher.engine.ps.flat, loaded)

    def reset():
        eng2.ps.flat.copy_(moved)
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
    assert torch.equal(st2.teacher.engine.ps.flat, loaded), "the teacher moved"


# ================================================================ 6. the call logs
def logged_step(dev, cfg, steps=1, **kw):
    from siss_amd import lib
    eng, st = stepper(dev, cfg, **kw)
    calls, orig = [], lib.call
    lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
    try:
        for s in range(steps):
            del calls[:]
            st.step(*batch(s, dev))
            torch.cuda.synchronize()
    finally:
        lib.call = orig
    return eng, st, calls


TEACHER_ENTRY = ("siss_teacher_seed", "siss_grad_norms_weighted")


def test_a_step_without_the_key_calls_no_new_entry_point(dev):
    _, st, plain = logged_step(dev, None, steps=2)
    assert st.teacher is None and not [k for k in st.log_fields() if k.startswith("teacher")]
    assert not [c for c in plain if c in TEACHER_ENTRY], "a step without the key reached csrc/teacher.hip"
    assert plain.count("siss_grad_norms_scale") == 1 and plain.count("siss_recombine_clip_adamw") == 1
    assert plain.count("siss_mse_bwd_seed") == 1 and plain.count("siss_mixture_fwd") == 2
    _, _, keyed = logged_step(dev, teacher_cfg("esd", "teacher"), steps=2)
    # section 4's sequence: the two mixtures, the student's forward, the teacher's forward, the seed, the backward pass, the weighted
    # pass 1, the plain pass 2.  A forward starts with the timestep embedding; the plain step's log has one, this one's two
    fwd = "siss_timestep_sincos"
    assert plain.count(fwd) == 1 and keyed.count(fwd) == 2
    assert keyed.count("siss_mixture_fwd") == 2
    i1, i2 = [i for i, c in enumerate(keyed) if c == fwd]
    assert max(i for i, c in enumerate(keyed) if c == "siss_mixture_fwd") < i1
    iseed, inorm, iadam = keyed.index("siss_teacher_seed"), keyed.index("siss_grad_norms_weighted"), keyed.index("siss_recombine_clip_adamw")
    assert i1 < i2 < iseed < inorm < iadam and iadam == inorm + 1
    assert keyed.count("siss_teacher_seed") == 1 and keyed.count("siss_grad_norms_weighted") == 1
    assert "siss_mse_bwd_seed" not in keyed and "siss_grad_norms_scale" not in keyed
    # the student's part is the plain step's: its forward (from its first launch to the seed) and everything behind the seed but pass 1
    p_fwd = plain[plain.index(fwd):plain.index("siss_mse_bwd_seed")]
    assert keyed[i1:i2] == p_fwd, "the student's forward differs from the plain step's"
    p_bwd = plain[plain.index("siss_mse_bwd_seed") + 1:]
    k_bwd = keyed[iseed + 1:]
    assert k_bwd == [("siss_grad_norms_weighted" if c == "siss_grad_norms_scale" else c) for c in p_bwd]
    # the teacher's forward is a forward of 3 B rows: no backward launcher, no weight-gradient product
    assert len(keyed[i2:iseed]) >= len(p_fwd) // 2
    assert not [c for c in keyed[i2:iseed] if "bwd" in c or "gemm_tn" in c or "dgrad" in c or "wgrad" in c], keyed[i2:iseed]


# ================================================================ 7. combinations
def test_the_teacher_with_lora_updates_the_adapters_alone(dev):
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from siss_amd.teacher import Teacher
    from oracle import schedule as S
    eng = make_engine()
    e = embeddings(dev)
    teacher = Teacher(eng).set_embeddings(empty=e["empty"], anchor=e["anchor"])
    targets = [n for n in eng.ps.specs if n.endswith("attn1.to_q.weight") or n.endswith("attn2.to_v.weight")]
    state = LoRAState(eng, targets, 4, 8.0, seed=2)
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, mixed_precision="bf16", loss_fn="teacher_target",
                     teacher=teacher, teacher_cfg=teacher_cfg("esd", "noise", 1.0, 0.75), lora=state, **HPK)
    base, frozen, p0 = eng.ps.flat.clone(), teacher.engine.ps.flat.clone(), state.p.clone()
    for s in range(2):
        st.step(*batch(s, dev))
    torch.cuda.synchronize()
    got = st.stats()
    assert got["scaling_factor"] == -0.75 and got["step"] == 2
    assert not torch.equal(state.p, p0), "the adapters did not move"
    tm = torch.zeros(eng.ps.total, dtype=torch.bool, device=dev)
    for n in targets:
        sp = eng.ps.specs[n]
        tm[sp.off:sp.off + sp.numel] = True
    assert torch.equal(bits(eng.ps.flat[~tm]), bits(base[~tm])), "a base weight outside the targets moved"
    assert not torch.equal(eng.ps.flat[tm], base[tm]), "the merged targets did not move"
    assert torch.equal(bits(teacher.engine.ps.flat), bits(frozen)), "the teacher moved"
    f = st.log_fields()
    assert f["teacher_forget"] == "esd" and f["trainable_params"] == state.params


def test_the_teacher_is_refused_with_the_other_four_variants_before_any_launch(dev):
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    from siss_amd.saliency import SaliencyMask
    from siss_amd.step import SISSStepper
    from siss_amd.surgery import Surgery
    from siss_amd.teacher import Teacher
    from oracle import schedule as S
    eng = make_engine()
    e = embeddings(dev)
    teacher = Teacher(eng).set_embeddings(empty=e["empty"], anchor=e["anchor"])
    bare = Teacher(eng)
    _, st = stepper(dev, teacher_cfg())
    others = dict(trainable=[n for n in eng.ps.specs if "attentions" in n], saliency=SaliencyMask.ones(eng), ewc=FisherAnchor.uniform(eng, 1.0),
                  surgery=Surgery(eng, "mutual", "tensor"))
    calls, orig = [], lib.call
    lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
    try:
        for name, obj in others.items():
            with pytest.raises(ValueError, match=f"teacher=.*{name}=") as err:
                SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, loss_fn="teacher_target", teacher=teacher,
                            teacher_cfg=teacher_cfg(), **{name: obj}, **HPK)
            assert "no weighted form" in str(err.value)
        for setter, obj in (("set_saliency", others["saliency"]), ("set_ewc", others["ewc"]), ("set_surgery", others["surgery"])):
            with pytest.raises(ValueError, match="teacher"):
                getattr(st, setter)(obj)
        with pytest.raises(ValueError, match="empty prompt"):
            SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, loss_fn="teacher_target", teacher=bare,
                        teacher_cfg=teacher_cfg(), **HPK)
        assert not calls, f"a refusal launched {calls}"
    finally:
        lib.call = orig


# ================================================================ 8. the task
SD = ["--config-name=delete_sd", "pretrained_model_name_or_path=/nonexistent",
      "+unet={sample_size:16,in_channels:4,out_channels:4,block_out_channels:[64,128],down_block_types:[CrossAttnDownBlock2D,DownBlock2D],"
      "up_block_types:[UpBlock2D,CrossAttnUpBlock2D],attention_head_dim:2,cross_attention_dim:64}"]
FIELDS = ("teacher_forget", "teacher_keep", "teacher_guidance", "teacher_weight", "teacher_rows")


def run_task(tmp_path, name, *extra):
    sys.path.insert(0, ROOT)
    import main as entry
    from siss_amd import tasks
    out = tmp_path / name
    ov = ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "allow_random_init=true", "allow_synthetic=true",
          f"data_dir={tmp_path}/nodata", "mixed_precision=bf16"]
    steppers, orig = [], tasks._DeleteBase.run

    def run(self):
        steppers.append(orig(self))
        return steppers[-1]
    tasks._DeleteBase.run = run
    try:
        entry.main([*SD, f"output_dir={out}", *ov, *extra])
    finally:
        tasks._DeleteBase.run = orig
    rundir = os.path.join(out, os.listdir(out)[0])
    return steppers[-1], [json.loads(l) for l in open(os.path.join(rundir, "train_log_rank0.jsonl"))], rundir


@pytest.mark.parametrize("key,want", [("{forget:esd,keep:teacher}", ("esd", "teacher", 6)),
                                      ("{forget:anchor,keep:noise,weight:0.5,anchor_prompt:a photo}", ("anchor", "noise", 2))])
def test_task_with_the_key(dev, tmp_path, capsys, key, want):
    st, lines, rundir = run_task(tmp_path, "keyed", "deletion.loss_fn=teacher_target", "+deletion.teacher=" + key)
    assert len(lines) == 2
    for l in lines:
        assert all(k in l for k in FIELDS), sorted(l)
        assert (l["teacher_forget"], l["teacher_keep"], l["teacher_rows"]) == want and l["scaling_factor"] == -l["teacher_weight"]
    assert lines[1]["norm_loss_a"] > 0.0
    tj = json.load(open(os.path.join(rundir, "teacher.json")))
    assert tj["forget"] == want[0] and tj["keep"] == want[1] and tj["weights"] == "student" and tj["bytes"] == st.teacher.nbytes
    assert tj["total"] == st.e.ps.total and tj["tensors"] == len(st.e.ps.specs) and tj["real_params"] > 0
    out = capsys.readouterr().out
    assert out.count("[siss_amd] deletion.teacher:") == 1 and f"{st.teacher.nbytes} bytes" in out
    if want[0] == "anchor":
        assert not torch.equal(st.teacher.anchor, st.teacher.anchor * 0) and st.teacher.empty is None


def test_task_without_the_key_has_no_teacher_fields(dev, tmp_path):
    st, plain, rundir = run_task(tmp_path, "plain")
    assert st.teacher is None and len(plain) == 2 and not [k for l in plain for k in l if k.startswith("teacher")]
    assert not os.path.exists(os.path.join(rundir, "teacher.json"))

"""Prompt-embedding gradients and the augmented prompt on the GPU: the launchers of csrc/prompt_grad.hip called directly,
UNetCondEngine.context_vjp against the f64 oracle, and SDSampler.aug_prompt / get_text_cond_grad against tests/prompt_aug_ref.py.

What is held to what:
* siss_ctx_dgrad / siss_ctx_reduce on integer-valued bf16 operands in [-8, 8] (every partial sum exact in f32 in any order; the
  largest case stays below 2^24: |sum| <= 64 * 2560 * 3): BITWISE the int64 product; NaN in every unused row / column of the
  operand buffers, a sentinel behind the result;
* siss_noise_norm_cot against f64: scalar 4 * 2^-24 relative, cotangent 4 * 2^-24 of max |cot| (one rounding each for the difference,
  the norm and the quotient, plus one spare); p == u gives zeros; two runs give equal bits;
* siss_prompt_embed_update against the f64 update: 4 x the same figures of torch's own f32 CPU AdamW (the bound of
  tests/test_hip_optimizer.py's step-precision test, taken from there);
* context_vjp against the f64 oracle: f32 engine 1e-4 of max |ref| (the project's f32 bound), bf16 engine cosine >= 0.99 and 3e-2 of
  max |ref| (the bound input_vjp is held to);
* aug_prompt (f32 engine): noise norms 1e-4 relative; the embedding on the coordinates whose reference gradient exceeds 1e-3 of the
  largest in every iteration, to (the f32 deviation measured for context_vjp) * iterations + 1e-4.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import optimizer_ref as OR
import prompt_aug_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
SENT = 77.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


# ================================================================ 1. context dgrad, exact
def _site(dev, rows, C, X, seed, pad_cols=16, pad_rows=3):
    """One site's operands: dkv [rows + pad_rows, 2C + pad_cols] and wk / wv [X + pad_rows, C] bf16, integer-valued in the used
    part, NaN everywhere else; and the int64 product [rows, X]."""
    g = torch.Generator().manual_seed(seed)
    dkv = torch.full((rows + pad_rows, 2 * C + pad_cols), float("nan"))
    dkv[:rows, :2 * C] = torch.randint(-8, 9, (rows, 2 * C), generator=g).float()
    w = torch.full((2, X + pad_rows, C), float("nan"))
    w[:, :X] = torch.randint(-8, 9, (2, X, C), generator=g).float()
    ref = dkv[:rows, :C].long() @ w[0, :X].long().t() + dkv[:rows, C:2 * C].long() @ w[1, :X].long().t()
    return dkv.to(dev, BF), w.to(dev, BF), ref


@pytest.mark.parametrize("X", [64, 768])
@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("Sk", [13, 77])
def test_ctx_dgrad_is_bitwise_the_int64_product(dev, Sk, n, C, X):
    from siss_amd import lib
    rows = n * Sk
    dkv, w, ref = _site(dev, rows, C, X, seed=Sk * 1000 + n * 100 + C + X)
    assert int(ref.abs().max()) < 2 ** 24
    out = torch.full((rows * X + 64,), SENT, device=dev)
    lib.call("siss_ctx_dgrad", dkv[:, :C], dkv[:, C:], dkv.stride(0), w[0], w[1], out, rows, C, X, 0)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[rows * X:], torch.full((64,), SENT)), "the bytes behind the result"
    assert torch.equal(_bits(got[:rows * X].view(rows, X)), _bits(ref.float()))


@pytest.mark.parametrize("reduce", [False, True], ids=["per-sample", "reduced"])
@pytest.mark.parametrize("Sk", [13, 77])
def test_two_sites_of_different_width_sum_into_one_result(dev, Sk, reduce):
    from siss_amd import lib
    n, X = 3, 64
    rows = n * Sk
    slabs = torch.full((2, rows, X), float("nan"), device=dev)
    refs = []
    for s, C in enumerate((64, 320)):
        dkv, w, ref = _site(dev, rows, C, X, seed=Sk + C)
        lib.call("siss_ctx_dgrad", dkv[:, :C], dkv[:, C:], dkv.stride(0), w[0], w[1], slabs[s], rows, C, X, 0)
        refs.append(ref)
    total = (refs[0] + refs[1]).view(n, Sk, X)
    want = total.sum(0) if reduce else total
    assert int(want.abs().max()) < 2 ** 24
    out = torch.full((want.numel() + 64,), SENT, device=dev)
    lib.call("siss_ctx_reduce", slabs, out, 2, n, Sk * X, int(reduce))
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[want.numel():], torch.full((64,), SENT)), "the bytes behind the result"
    assert torch.equal(_bits(got[:want.numel()]), _bits(want.float().reshape(-1)))


def test_ctx_dgrad_f32_operands_and_refusals(dev):
    """the f32 form on the same integers (the f32 engine's operands), and the shapes / alignments the launcher does not take"""
    from siss_amd import lib
    rows, C, X = 13, 64, 64
    dkv, w, ref = _site(dev, rows, C, X, seed=9)
    dkv32, w32 = dkv.float(), w.float()
    out = torch.full((rows * X + 64,), SENT, device=dev)
    lib.call("siss_ctx_dgrad", dkv32[:, :C], dkv32[:, C:], dkv32.stride(0), w32[0], w32[1], out, rows, C, X, 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:rows * X].cpu().view(rows, X), ref.float()) and float(out[rows * X]) == SENT
    before = out.clone()
    for args in ((dkv[:, :C], dkv[:, C:], dkv.stride(0), w[0], w[1], out, rows, 60, X, 0),           # C % 8
                 (dkv[:, :C], dkv[:, C:], dkv.stride(0) + 4, w[0], w[1], out, rows, C, X, 0),       # row stride % 8
                 (dkv[:, 4:], dkv[:, C:], dkv.stride(0), w[0], w[1], out, rows, C, X, 0),           # 8 bytes off alignment
                 (dkv[:, :C], dkv[:, C:], dkv.stride(0), w[0], w[1], out, 0, C, X, 0),
                 (dkv[:, :C], dkv[:, C:], dkv.stride(0), w[0], w[1], out, rows, C, X, 2)):
        assert lib.call("siss_ctx_dgrad", *args, refusable=True) == 1, args[6:]
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(before))


# ================================================================ 2. noise norm and its cotangent
@pytest.mark.parametrize("n,chw", [(1, 1024), (3, 324), (2, 16384)])
def test_noise_norm_cot_against_f64(dev, n, chw):
    from siss_amd.prompt_aug import noise_norm_cot
    g = torch.Generator().manual_seed(n * chw)
    p, u = torch.randn(n, chw, generator=g), torch.randn(n, chw, generator=g)
    d = p.double() - u.double()
    nrm = float(d.square().sum().sqrt())
    ref = d / nrm
    runs = []
    for _ in range(2):
        cot = torch.full((n * chw + 64,), SENT, device=dev)
        loss = torch.full((3,), SENT, device=dev)
        noise_norm_cot(p.to(dev), u.to(dev), cot[:n * chw].view(n, chw), loss[1:2])
        torch.cuda.synchronize()
        runs.append((cot.cpu(), loss.cpu()))
    (cot, loss), (cot2, loss2) = runs
    assert torch.equal(_bits(cot), _bits(cot2)) and torch.equal(_bits(loss), _bits(loss2)), "two runs differ"
    assert float(loss[0]) == SENT and float(loss[2]) == SENT and torch.equal(cot[n * chw:], torch.full((64,), SENT))
    e_s = abs(float(loss[1]) - nrm) / nrm
    e_c = float((cot[:n * chw].view(n, chw).double() - ref).abs().max() / ref.abs().max())
    print(f"\n[noise_norm_cot] n {n} chw {chw}: scalar error {e_s / U:.2f} u, cotangent error {e_c / U:.2f} u of max |cot| (allowed 4 u)")
    assert e_s <= 4 * U and e_c <= 4 * U, (e_s, e_c)


def test_noise_norm_cot_of_equal_inputs_is_zero(dev):
    from siss_amd.prompt_aug import noise_norm_cot
    p = torch.randn(3, 324, generator=torch.Generator().manual_seed(1)).to(dev)
    cot, loss = torch.full((3, 324), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    noise_norm_cot(p, p.clone(), cot, loss)
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and torch.equal(cot, torch.zeros_like(cot))


# ================================================================ 3. the embedding update
def _update_f64(e, e0, g, m, v, step, lr, alpha, optim_epsilon):
    """(e, m, v, effective gradient, penalised) of one step in f64 from f64 copies of the f32 state"""
    from siss_amd.prompt_aug import ADAMW_BETAS, ADAMW_EPS, ADAMW_WEIGHT_DECAY
    L = e.shape[0]
    dist = (e - e0).square().sum(-1).sqrt()
    pen = optim_epsilon is not None and float(dist[1:].mean()) > optim_epsilon
    geff = g.clone()
    if pen:
        unit = torch.where(dist[:, None] > 0, (e - e0) / dist[:, None].clamp_min(1e-300), torch.zeros_like(e))
        geff = alpha * g + (1 - alpha) / (L - 1) * unit
    geff[0] = 0
    lr, b1, b2, eps, wd = OR.wide(OR.hyper(lr, ADAMW_BETAS[0], ADAMW_BETAS[1], ADAMW_EPS, ADAMW_WEIGHT_DECAY))   # the f32 values the C ABI carries
    p = e * (1 - lr * wd)
    m2 = m + (geff - m) * (1 - b1)
    v2 = v * b2 + geff * geff * (1 - b2)
    den = v2.sqrt() / math.sqrt(1 - b2 ** step) + eps
    p = p - lr / (1 - b1 ** step) * m2 / den
    return p, m2, v2, geff, pen


@pytest.mark.parametrize("optim_epsilon", [None, 0.0], ids=["plain", "penalty"])
@pytest.mark.parametrize("X", [64, 768])
def test_embed_update_against_f64(dev, X, optim_epsilon):
    from siss_amd.prompt_aug import ADAMW_BETAS, ADAMW_EPS, ADAMW_WEIGHT_DECAY, embed_update
    L, lr, alpha = 77, 0.1, 0.5
    hp = OR.hyper(lr, ADAMW_BETAS[0], ADAMW_BETAS[1], ADAMW_EPS, ADAMW_WEIGHT_DECAY)
    gen = torch.Generator().manual_seed(X)
    e0 = torch.randn(L, X, generator=gen)
    buf = torch.full((4, L * X + 64), SENT, device=dev)                      # e, m, v with sentinels behind them
    e, m, v = (buf[i, :L * X].view(L, X) for i in range(3))
    e.copy_(e0); m.zero_(); v.zero_()
    e0d = e0.to(dev)
    dist = torch.zeros(L, dtype=F64, device=dev)
    pens = []
    for step in (1, 2, 3):
        g = torch.randn(L, X, generator=gen)
        if step == 2:
            e[5].copy_(e0d[5])                                               # a row whose difference is zero: no penalty gradient there
        pre = [t.cpu().clone() for t in (e, m, v)]
        embed_update(e, e0d, g.to(dev), m, v, dist, step, lr, alpha, optim_epsilon)
        torch.cuda.synchronize()
        got = [t.cpu() for t in (e, m, v)]
        pr, mr, vr, geff, pen = _update_f64(pre[0].double(), e0.double(), g.double(), pre[1].double(), pre[2].double(), step, lr,
                                            alpha, optim_epsilon)
        pens.append(pen)
        tp = OR.torch_adamw(geff.float().numpy().reshape(-1), pre[0].numpy().reshape(-1), pre[1].numpy().reshape(-1),
                            pre[2].numpy().reshape(-1), step, hp, torch.float32)
        ref = tuple(t.numpy().reshape(-1) for t in (pr, mr, vr))
        e_ref = OR.update_errors(tp, ref, pre[0].numpy().reshape(-1))
        err = OR.update_errors(tuple(t.numpy().reshape(-1) for t in got), ref, pre[0].numpy().reshape(-1))
        print(f"\n[embed_update] X {X} step {step} penalised {pen}: error (torch f32): p {err[0]:.2e} ({e_ref[0]:.2e}), m {err[1]:.2e} "
              f"({e_ref[1]:.2e}), v {err[2]:.2e} ({e_ref[2]:.2e}); allowed 4 x")
        assert all(err[i] <= 4 * e_ref[i] for i in range(3)), (step, err, e_ref)
        # row 0: decay only, zero moments
        assert torch.equal(got[1][0], pre[1][0]) and torch.equal(got[2][0], pre[2][0]) and float(got[1][0].abs().max()) == 0
        assert float((got[0][0].double() - pre[0][0].double() * (1 - lr * ADAMW_WEIGHT_DECAY)).abs().max()) <= 2 * U * float(pre[0][0].abs().max())
        if pen and step == 2:                                                # row 5: alpha * g alone reached the moments
            want = (pre[1][5].double() + (alpha * g[5].double() - pre[1][5].double()) * (1 - ADAMW_BETAS[0]))
            assert float((got[1][5].double() - want).abs().max()) <= 4 * U * float(want.abs().max())
    assert pens == ([False, True, True] if optim_epsilon is not None else [False] * 3)
    assert torch.equal(buf[:3, L * X:].cpu(), torch.full((3, 64), SENT)), "the bytes behind e, m, v"


# ================================================================ 4 - 8. context_vjp
_ENGINES, _REFS, _DEV = {}, {}, {}


def _engine(case, dtype):
    """(engine, f64 oracle) of a case, weights from init_random(seed=1), shared by the tests of this module"""
    from siss_amd.unet_cond import UNetCondEngine
    from oracle.unet_cond import OracleUNet2DCondition
    key = (case, dtype)
    if key not in _ENGINES:
        hc, oc = R.configs(case)
        eng = UNetCondEngine(hc, "cuda:0", dtype=dtype)
        sd = eng.init_random(seed=1)
        net = _ENGINES.get((case, "net"))
        if net is None:
            net = OracleUNet2DCondition(oc).double()
            net.load_state_dict({k: v.double() for k, v in sd.items()})
            _ENGINES[(case, "net")] = net
        _ENGINES[key] = eng
    return _ENGINES[key], _ENGINES[(case, "net")]


def _vjp_inputs(case, L, B=2):
    c = R.CASES[case]
    g = torch.Generator().manual_seed(11 + L)
    hw, X = c["sample_size"], c["cross_dim"]
    return (torch.randn(B, 4, hw, hw, generator=g), torch.tensor([999, 300]), torch.randn(B, L, X, generator=g),
            torch.randn(B, 4, hw, hw, generator=g))


def _vjp_ref(case, L):
    """the f64 oracle's d <cot, net(x, t, ctx)> / d ctx, computed once per (case, L)"""
    if (case, L) not in _REFS:
        net = _engine(case, F32)[1]
        x, t, ctx, cot = _vjp_inputs(case, L)
        cr = ctx.double().requires_grad_(True)
        _REFS[(case, L)] = torch.autograd.grad(net(x.double(), t, cr)[0], cr, cot.double())[0]
    return _REFS[(case, L)]


def _vjp_deviation(dev, case, L, dtype):
    eng, _ = _engine(case, dtype)
    ref = _vjp_ref(case, L)
    x, t, ctx, cot = (a.to(dev) for a in _vjp_inputs(case, L))
    eng.forward(x, t, encoder_hidden_states=ctx)
    got = eng.context_vjp(cot.contiguous()).double().cpu()
    red = eng.context_vjp(cot.contiguous(), reduce=True).double().cpu()
    scale = float(ref.abs().max())
    out = {}
    for what, a, b in (("per-sample", got, ref), ("reduced", red, ref.sum(0))):
        out[what] = (float((a - b).abs().max()) / float(b.abs().max()), float((a * b).sum() / (a.norm() * b.norm())))
    assert tuple(got.shape) == tuple(ref.shape) and tuple(red.shape) == tuple(ref.shape[1:]) and scale > 0
    return out


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [77, 13])
@pytest.mark.parametrize("case", list(R.CASES))
def test_context_vjp_matches_the_f64_oracle(dev, case, L, dtype):
    res = _vjp_deviation(dev, case, L, dtype)
    if dtype == F32:
        _DEV[(case, L)] = max(e for e, _ in res.values())
    for what, (err, cos) in res.items():
        print(f"\n{case} L {L} {dtype} {what}: context VJP vs f64 oracle: max err {err:.2e} of max |ref|, cosine {cos:.6f}")
        if dtype == F32:
            assert err <= 1e-4, (what, err)
        else:
            assert cos >= 0.99 and err <= 3e-2, (what, cos, err)


def test_bf16_context_vjp_launches_no_weight_gradient_product(dev):
    from siss_amd import lib
    eng, _ = _engine("tiny", BF)
    assert eng.flash
    x, t, ctx, cot = (a.to(dev) for a in _vjp_inputs("tiny", 77))
    eng.forward(x, t, encoder_hidden_states=ctx)
    torch.cuda.synchronize()
    lib.dispatch_counts(reset=True)
    eng.context_vjp(cot.contiguous())
    torch.cuda.synchronize()
    got = lib.dispatch_counts(reset=True)
    assert got["gemm_tn_kernel<1>"] == got["gemm_tn_kernel<3>"] == got["gemm_tn_pair"] == 0, got
    grads = eng.ps.grads.clone()
    eng.zero_grad()
    eng.backward(cot.contiguous(), nsets=1)                   # positive control: the weight-gradient backward of the same forward
    torch.cuda.synchronize()
    got = lib.dispatch_counts(reset=True)
    assert got["gemm_tn_kernel<1>"] + got["gemm_tn_kernel<3>"] + got["gemm_tn_pair"] > 0, got
    eng.ps.grads.copy_(grads)


@pytest.mark.parametrize("path", ["flash fused-kv", "flash unfused", "materialised"])
def test_bf16_context_vjp_paths_agree_and_are_reproducible(dev, path):
    """the three bf16 code paths of the cross-attention backward against the f64 oracle at the bf16 bound, each bitwise equal to its
    own second call"""
    eng, _ = _engine("tiny", BF)
    ref = _vjp_ref("tiny", 77)
    x, t, ctx, cot = (a.to(dev) for a in _vjp_inputs("tiny", 77))
    try:
        eng.fuse_kv, eng.flash = path == "flash fused-kv", path != "materialised"
        eng.forward(x, t, encoder_hidden_states=ctx)
        a = eng.context_vjp(cot.contiguous()).clone()
        b = eng.context_vjp(cot.contiguous()).clone()
        torch.cuda.synchronize()
    finally:
        eng.fuse_kv, eng.flash = True, True
    assert torch.equal(_bits(a), _bits(b)), "two context_vjp calls on one forward differ"
    got = a.double().cpu()
    err, cos = float((got - ref).abs().max() / ref.abs().max()), float((got * ref).sum() / (got.norm() * ref.norm()))
    print(f"\ntiny bf16 {path}: max err {err:.2e}, cosine {cos:.6f}")
    assert cos >= 0.99 and err <= 3e-2, (cos, err)


def test_f32_context_vjp_is_reproducible(dev):
    eng, _ = _engine("tiny", F32)
    x, t, ctx, cot = (a.to(dev) for a in _vjp_inputs("tiny", 13))
    eng.forward(x, t, encoder_hidden_states=ctx)
    a = eng.context_vjp(cot.contiguous(), reduce=True).clone()
    b = eng.context_vjp(cot.contiguous(), reduce=True).clone()
    assert torch.equal(_bits(a), _bits(b))


def _launches(fn):
    """[(launcher, shape key, kernel symbol)] of the launches fn() makes, in order (lib.PROF's bookkeeping)"""
    from siss_amd import lib
    lib.PROF = []
    try:
        fn()
        torch.cuda.synchronize()
        return [(r[0], r[4], r[5]) for r in lib.PROF]
    finally:
        lib.PROF = None


def test_context_vjp_leaves_the_training_state_bitwise(dev):
    """After two SISS steps: a forward + context_vjp leaves weights, gradient buffers, shadow, moments, fill plans and the overwrite
    log as they were, and resets its own mode.  The full forward + backward(nsets=2) afterwards is compared with the same pass before
    the VJP in two ways that do not depend on the arrival order of float atomics: it makes the SAME launches in the same order, and
    its gradients are bitwise equal wherever a weight gradient is written by a one-split product -- the stretches the sparse-fill plan
    of this batch shape records as overwritten.  (Elsewhere -- multi-split products, bias / gamma / beta / time-embedding sums -- the
    backward pass adds with float atomics and two plain reruns already differ in the last bits; the cotangents themselves are formed
    without atomics.)"""
    from siss_amd import lib
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.step import SISSStepper
    from siss_amd.unet_cond import UNetCondEngine
    eng = UNetCondEngine(R.configs("tiny")[0], "cuda:0")
    eng.init_random(seed=2)
    B, hw, X = 2, 16, 64
    ac = DDPMScheduler(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012).alphas_cumprod
    st = SISSStepper(eng, ac, lr=1e-5, scaling_norm=7.5, lambd=0.5, train_batch_size=B, mixed_precision="bf16", inf_guard=True)
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = torch.randn(1, 77, X, device=dev, generator=g).repeat(B, 1, 1)
    for _ in range(2):                                   # two steps: AdamW moments, both gradient sets and a sparse-fill plan exist
        x0, a0, noise = (torch.randn((B, 4, hw, hw), device=dev, generator=g) for _ in range(3))
        st.step(x0, a0, noise, torch.randint(0, 1000, (B,), device=dev, generator=g), torch.rand(B, device=dev, generator=g),
                conditioning={"encoder_hidden_states": ctx})
    torch.cuda.synchronize()
    lib.overwrite_log()
    ps = eng.ps
    assert eng._fill_plans, "the steps recorded no sparse-fill plan"
    plan = max(eng._fill_plans.values(), key=lambda pl: len(pl["stretches"]))
    stretches = [(a, n) for a, n in plan["stretches"] if n > 0]
    covered = sum(n for _, n in stretches)
    assert stretches and covered > 0, plan             # (the bitwise comparison below is over these: not a vacuous region)
    x, t, _, _ = (a.to(dev) for a in _vjp_inputs("tiny", 77))
    cot2 = torch.randn(2 * B, 4, hw, hw, device=dev, generator=g)

    def full_pass():
        eng.forward(x, t, encoder_hidden_states=ctx)
        eng.zero_grad()
        eng.backward(cot2, nsets=2)

    def one_split(grads):
        flat = grads.reshape(-1)
        return torch.cat([_bits(flat[a:a + n]) for a, n in stretches])
    launched = _launches(full_pass)
    first = one_split(ps.grads)
    assert (eng.nb, eng.nsets, eng.gbase) == (2 * B, 2, 0)
    lib.overwrite_log()
    snap = [ps.flat.clone(), ps.grads.clone(), ps.shadow.clone(), st.opt.m.clone(), st.opt.v.clone()]
    fill = (eng._fill_key, eng._fill_plan, dict(eng._fill_plans), eng.wgrad_overwrite)
    grads_ptr = ps.grads.data_ptr()
    eng.forward(x, t, encoder_hidden_states=ctx)
    eng.context_vjp(cot2[:B].contiguous())
    eng.context_vjp(cot2[:B].contiguous(), reduce=True)
    torch.cuda.synchronize()
    for a, b in zip(snap, [ps.flat, ps.grads, ps.shadow, st.opt.m, st.opt.v]):
        assert torch.equal(_bits(a), _bits(b))
    assert (eng._fill_key, eng._fill_plan, eng.wgrad_overwrite) == (fill[0], fill[1], fill[3])
    assert eng._fill_plans.keys() == fill[2].keys() and all(eng._fill_plans[k] is v for k, v in fill[2].items())
    assert lib.overwrite_log() == []
    # context_vjp's own state: the mode flag, the accumulator, the swapped gradient buffer
    assert eng._vjp is False and eng._ctx_slabs is None and eng._ctx_site == 0 and eng._dx is None and eng.wgrads.idle
    assert ps.grads.data_ptr() == grads_ptr and ps.grads is not eng._vjp_sums
    assert (eng.nb, eng.nsets, eng.gbase) == (B, 1, 0)    # (what the one-set replay left; the next backward() sets its own)
    # the same full pass afterwards
    assert _launches(full_pass) == launched, "the pass after context_vjp launches something else"
    assert (eng.nb, eng.nsets, eng.gbase) == (2 * B, 2, 0)
    assert torch.equal(one_split(ps.grads), first), "one-split weight gradients differ after context_vjp"
    print(f"\n{len(launched)} launches per pass; {covered} of {2 * ps.total} gradient floats (two sets) compared bitwise ({len(stretches)} stretches)")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_autograd_grad_with_respect_to_the_text_is_context_vjp(dev, dtype):
    from siss_amd.model import UNet2DConditionModel
    m = UNet2DConditionModel(R.configs("tiny")[0], device=dev, compute_dtype=dtype)
    m.engine.init_random(seed=3)
    x, t, ctx, cot = (a.to(dev) for a in _vjp_inputs("tiny", 77))
    grads_before = m.engine.ps.grads.clone()
    e = ctx.clone().requires_grad_(True)
    (de,) = torch.autograd.grad(m(x, t, encoder_hidden_states=e)[0], e, cot)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(_bits(m.engine.ps.grads), _bits(grads_before))
    m.engine.forward(x, t, encoder_hidden_states=ctx)
    vjp = m.engine.context_vjp(cot.contiguous())
    assert de.shape == ctx.shape and torch.equal(_bits(de), _bits(vjp))
    assert m._supports_input_vjp is False


# ================================================================ 9 - 11. aug_prompt and get_text_cond_grad
_AUG = {}


def _aug_ref():
    """the f64 restatement's run of the end-to-end case, once"""
    if "ref" not in _AUG:
        net, sd = R.seeded_oracle("tiny", R.AUG_SEED)
        z, e, e_neg = R.aug_inputs("tiny")
        t = torch.full((R.AUG_N,), R.AUG_T)
        out, tr = R.aug_prompt(net, z.double(), t, e.double(), e_neg.double(), lr=R.AUG_LR, optim_iters=R.AUG_ITERS)
        _AUG["ref"] = (net, sd, z, e, e_neg, t, out, tr)
    return _AUG["ref"]


def _sampler(dev, dtype):
    from siss_amd.model import UNet2DConditionModel
    from siss_amd.sd_sampler import SDSampler
    if dtype not in _AUG:
        m = UNet2DConditionModel(R.configs("tiny")[0], device=dev, compute_dtype=dtype)
        m.load_state_dict(_aug_ref()[1])
        _AUG[dtype] = SDSampler(m, use_graph=False)
    s = _AUG[dtype]
    assert s.scheduler.set_timesteps(50)[0] == R.AUG_T
    return s


def _run_aug(dev, dtype, **kw):
    _, _, z, e, e_neg, _, _, _ = _aug_ref()
    return _sampler(dev, dtype).aug_prompt(prompt_embeds=e, negative_prompt_embeds=e_neg, latents=z, num_images_per_prompt=R.AUG_N,
                                           lr=R.AUG_LR, optim_iters=R.AUG_ITERS, return_trace=True, **kw)


def test_aug_prompt_matches_the_f64_restatement(dev):
    _, _, z, e, e_neg, t, ref_e, ref_tr = _aug_ref()
    out, tr = _run_aug(dev, F32)
    assert tuple(out.shape) == tuple(e.shape) and out.dtype == F32 and tr["iterations"] == R.AUG_ITERS and not tr["stopped_early"]
    for j, (a, b) in enumerate(zip(tr["noise_norm"], ref_tr["noise_norm"])):
        print(f"\niteration {j}: noise norm {a:.8f}, f64 restatement {b:.8f}, relative {abs(a - b) / b:.2e} (allowed 1e-4)")
    assert len(tr["noise_norm"]) == R.AUG_ITERS and all(abs(a - b) <= 1e-4 * b for a, b in zip(tr["noise_norm"], ref_tr["noise_norm"]))
    keep = R.kept_coordinates(ref_tr)
    share = float(keep[1:].double().mean())
    assert share >= 0.9, share
    dev4 = _DEV.get(("tiny", 77))
    if dev4 is None:
        dev4 = max(v[0] for v in _vjp_deviation(dev, "tiny", 77, F32).values())
    bound = dev4 * R.AUG_ITERS + 1e-4
    diff = (out[0].double().cpu() - ref_e[0]).abs()
    print(f"\nembedding: max deviation on the kept coordinates ({share:.4f} of rows 1..) {float(diff[keep].max()):.3e}, on all of rows 1.. "
          f"{float(diff[1:].max()):.3e}; allowed {bound:.3e} = {dev4:.2e} (f32 context_vjp deviation) * {R.AUG_ITERS} + 1e-4")
    assert float(diff[keep].max()) <= bound, (float(diff[keep].max()), bound)
    want0 = e[0, 0].double() * (1 - R.AUG_LR * 1e-2) ** R.AUG_ITERS
    assert float((out[0, 0].double().cpu() - want0).abs().max()) <= 4 * U * float(want0.abs().max())


def test_aug_prompt_on_the_bf16_engine(dev):
    _, _, _, e, _, _, _, ref_tr = _aug_ref()
    out, tr = _run_aug(dev, BF)
    assert bool(torch.isfinite(out).all()) and all(math.isfinite(v) for v in tr["noise_norm"])
    r0 = ref_tr["noise_norm"][0]
    print(f"\nbf16 engine: noise norms {tr['noise_norm']}, f64 restatement {ref_tr['noise_norm']}")
    assert abs(tr["noise_norm"][0] - r0) <= 3e-2 * r0
    # between the first two reference norms, clear of both by the tolerance above (prompt_aug_ref.early_stop_target): one update, then stop
    target = R.early_stop_target(ref_tr["noise_norm"][0], ref_tr["noise_norm"][1])
    assert target is not None
    out2, tr2 = _run_aug(dev, BF, target_loss=target)
    assert tr2["stopped_early"] and tr2["iterations"] == 1 and len(tr2["noise_norm"]) == 2, tr2


def test_aug_prompt_early_stop_leaves_the_embedding(dev):
    _, _, _, e, _, _, _, ref_tr = _aug_ref()
    out, tr = _run_aug(dev, F32, target_loss=2 * ref_tr["noise_norm"][0])
    assert tr["stopped_early"] and tr["iterations"] == 0 and torch.equal(out.cpu(), e)


def test_aug_prompt_cost_structure(dev):
    """1 + optim_iters forwards of n samples, optim_iters data-only backwards of n samples, no weight-gradient backward"""
    s = _sampler(dev, F32)
    eng = s.unet.engine
    calls = {"forward": [], "context_vjp": [], "backward": []}
    orig = {k: getattr(eng, k) for k in calls}

    def counted(k):
        def f(x, *a, **kw):
            calls[k].append(int(x.shape[0]))
            return orig[k](x, *a, **kw)
        return f
    try:
        for k in calls:
            setattr(eng, k, counted(k))
        _run_aug(dev, F32)
    finally:
        for k in calls:
            delattr(eng, k)
    assert calls == {"forward": [R.AUG_N] * (1 + R.AUG_ITERS), "context_vjp": [R.AUG_N] * R.AUG_ITERS, "backward": []}, calls


def test_refusals(dev):
    s = _sampler(dev, F32)
    _, _, z, e, e_neg, _, _, _ = _aug_ref()
    kw = dict(prompt_embeds=e, negative_prompt_embeds=e_neg, latents=z, num_images_per_prompt=R.AUG_N)
    for f in (s.aug_prompt, s.get_text_cond_grad):
        with pytest.raises(NotImplementedError, match="eta"):
            f(eta=0.5, **kw)
        with pytest.raises(NotImplementedError, match="prompt_embeds"):
            f(prompt="a photo", **kw)
        with pytest.raises(ValueError, match="guidance"):
            f(guidance_scale=1.0, **kw)
        with pytest.raises(ValueError, match="target_steps"):
            f(target_steps=[50], **kw)


def test_get_text_cond_grad(dev):
    from siss_amd.sd_sampler import cfg_ddim_step, ddim_blocks
    net, _, z, e, e_neg, t, _, _ = _aug_ref()
    s = _sampler(dev, F32)
    kw = dict(prompt_embeds=e, negative_prompt_embeds=e_neg, latents=z, num_images_per_prompt=R.AUG_N)
    got = s.get_text_cond_grad(target_steps=[0], **kw)
    ref = R.token_grad_norms(net, z.double(), t, e.double(), e_neg.double())
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"\ntoken gradient norms vs f64 restatement: max err {err:.2e} of the largest (allowed 1e-4)")
    assert tuple(got.shape) == (77,) and err <= 1e-4, err
    both, tr = s.get_text_cond_grad(target_steps=[0, 1], return_trace=True, **kw)
    assert torch.equal(_bits(tr["per_step"][0]), _bits(got))
    assert torch.equal(_bits(both), _bits(torch.stack(tr["per_step"]).mean(0))) and len(tr["per_step"]) == 2
    # the second step's latents: one DDIM step under guidance from the first, from the two predictions of the first step
    eng = s.unet.engine
    zd, n = z.to(dev), R.AUG_N
    assert torch.equal(_bits(tr["latents"][0]), _bits(zd))
    tt = torch.full((n,), R.AUG_T, dtype=torch.long, device=dev)
    u = eng.forward(zd, tt, e_neg.to(dev).repeat(n, 1, 1)).clone()
    p = eng.forward(zd, tt, e.to(dev).repeat(n, 1, 1)).clone()
    x1 = zd.clone()
    norms = torch.zeros(2, n, ddim_blocks(n, zd[0].numel()), device=dev)
    cfg_ddim_step(torch.cat([u, p]), x1, x1, s.scheduler.coeffs(R.AUG_T), 7.5, 0.0, norms)
    assert torch.equal(_bits(tr["latents"][1]), _bits(x1))
    assert not torch.equal(x1, zd)


# ================================================================ the tool, and its consumer
def test_make_aug_prompt_tool_feeds_delete_sd(dev, tmp_path):
    """tools/make_aug_prompt.py --allow-random-init on a tiny config, in a fresh process, writes a [1, 77, X] .pt; a DeleteSD run from
    config with using_augmented_prompt=true starts from that file and completes one step."""
    unet = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=[64, 128],
                down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"], up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"],
                attention_head_dim=2, cross_attention_dim=64)
    uj = tmp_path / "unet.json"
    uj.write_text(json.dumps(unet))
    out = tmp_path / "aug_prompt.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_aug_prompt.py"), "--allow-random-init", "--unet-json", str(uj),
                        "--out", str(out), "--n", "2", "--iters", "2", "--token-grads", "pretrained_model_name_or_path=/nonexistent"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    e = torch.load(str(out))
    assert tuple(e.shape) == (1, 77, 64) and e.dtype == F32 and bool(torch.isfinite(e).all())
    rec = json.load(open(str(tmp_path / "aug_prompt.json")))
    assert len(rec["noise_norm"]) == 2 and len(rec["token_grad_norms"]) == 77
    sys.path.insert(0, ROOT)
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["training_steps=1", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/out",
                     "pretrained_model_name_or_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true",
                     "using_augmented_prompt=true"])
    cfg.validation_prompts = [str(out)]
    cfg.unet = unet
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    got = task.conditioning(2, dev)["encoder_hidden_states"]
    assert torch.equal(got[0].cpu(), e[0]) and torch.equal(got[1].cpu(), e[0])
    task.run()
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"))]
    assert len(lines) == 1

"""The forget-set likelihood metric on the GPU: conv_in's data gradient, the engine's input VJP (against the f64 oracle, without any
weight-gradient product, leaving the training state alone), the class surface's sample gradient, the fused drift / divergence kernel,
the device RK45, and bits/dim end to end against the reference's composition in f64."""
import json
import math
import os

import numpy as np
import pytest
import torch

from likelihood_ref import likelihood_f64, rk45_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# config/train_tshirt_mnist.yaml's unet (widths 64, 128, 256 at 28 x 28) with one resnet per level
MNIST_TINY = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=(64, 128, 256),
                  down_block_types=("DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
                  up_block_types=("UpBlock2D", "AttnUpBlock2D", "UpBlock2D"), layers_per_block=1, attention_head_dim=8,
                  norm_num_groups=32, norm_eps=1e-5, downsample_padding=1, flip_sin_to_cos=True, freq_shift=0)
# google/ddpm-celebahq-256's block kinds at two levels: one-head attention (128 channels, 8 x 8 tokens: the fused kernels)
CELEB_TINY = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
                  down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
                  layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6, downsample_padding=0,
                  flip_sin_to_cos=False, freq_shift=1)
# an MNIST-shaped net small enough for the f64 CPU composition: two levels
MNIST_SMALL = dict(MNIST_TINY, block_out_channels=(64, 128), down_block_types=("DownBlock2D", "AttnDownBlock2D"),
                   up_block_types=("AttnUpBlock2D", "UpBlock2D"))
CASES = [("mnist", MNIST_TINY), ("celeb", CELEB_TINY)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


def _engine(kw, dtype, seed=1):
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    eng = UNetEngine(UNet2DConfig(**kw), "cuda:0", dtype=dtype)
    return eng, eng.init_random(seed=seed)


def _oracle(kw, sd):
    from oracle.unet import OracleUNet2D, UNetConfig
    net = OracleUNet2D(UNetConfig(**kw)).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    return net


def _inputs(kw, B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    c, hw = kw["in_channels"], kw["sample_size"]
    return (torch.randn(B, c, hw, hw, generator=g), torch.tensor([999, 10, 500, 3][:B]),
            torch.randn(B, kw["out_channels"], hw, hw, generator=g))


# ---------------------------------------------------------------- 1. siss_conv_in_dgrad
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cin, c0, head", [(1, 64, 0), (3, 64, 0), (1, 128, 0), (3, 128, 0), (3, 64, 128), (1, 128, 64)])
def test_conv_in_dgrad_matches_torch_conv2d_input_f64(dev, dtype, cin, c0, head):
    from siss_amd import lib
    from siss_amd.layout import Act, ActView
    N, H, W = 2, 12, 10
    kp = -(-9 * cin // 64) * 64
    g = torch.Generator().manual_seed(cin * 1000 + c0 + head)
    w = torch.randn(c0, cin, 3, 3, generator=g).to(dtype).double()          # the operand the kernel reads, exactly
    native = torch.zeros(c0, kp, dtype=torch.float64)
    native[:, :9 * cin] = w.permute(0, 2, 3, 1).reshape(c0, 9 * cin)
    cot = torch.randn(N, c0, H, W, generator=g).to(dtype)
    base = Act(N, H, W, head + c0, device=dev, dtype=dtype)
    # a column view of a wider (concat) buffer when head > 0: the other columns hold values the kernel must not read
    base.interior().copy_(torch.randn(N, H, W, head + c0, generator=g).to(dev, dtype))
    dh = ActView(base, head, c0) if head else base
    base.interior()[..., head:].copy_(cot.permute(0, 2, 3, 1).to(dev))
    dx = torch.full((N, cin, H, W), float("nan"), device=dev)
    name = "siss_conv_in_dgrad" if dtype == torch.bfloat16 else "siss_conv_in_dgrad_f32"
    lib.call(name, dh.data, head + c0, native.to(dev, dtype), kp, dx, N, cin, H, W, c0)
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_input((N, cin, H, W), w, cot.double(), padding=1)
    err = float((dx.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err


def test_conv_in_dgrad_refuses_unaligned_row_strides(dev):
    from siss_amd import lib
    x = torch.zeros(4096, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(64, device=dev)
    assert lib.call("siss_conv_in_dgrad", x, 68, x, 64, out, 1, 1, 4, 4, 64, refusable=True) == 1      # ld % 8
    assert lib.call("siss_conv_in_dgrad", x, 64, x, 64, out, 1, 1, 4, 4, 48, refusable=True) == 1      # C0 / 8 not a power of 2


# ---------------------------------------------------------------- 2. UNetEngine.input_vjp against the f64 oracle
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name, kw", CASES, ids=[c[0] for c in CASES])
def test_input_vjp_matches_the_f64_oracle(dev, name, kw, dtype):
    eng, sd = _engine(kw, dtype)
    net = _oracle(kw, sd)
    x, t, cot = _inputs(kw)
    xr = x.double().requires_grad_(True)
    ref = torch.autograd.grad(net(xr, t)[0], xr, cot.double())[0]
    eng.forward(x.to(dev), t.to(dev))
    dx = eng.input_vjp(cot.to(dev).contiguous()).double().cpu()
    scale = float(ref.abs().max())
    err = float((dx - ref).abs().max()) / scale
    cos = float((dx * ref).sum() / (dx.norm() * ref.norm()))
    print(f"\n{name} {dtype}: input VJP vs f64 oracle: max err {err:.2e} of max|dx|, cosine {cos:.6f}")
    if dtype == torch.float32:
        assert err <= 1e-4, err
    else:
        assert cos >= 0.99 and err <= 3e-2, (cos, err)


# ---------------------------------------------------------------- 3. no weight-gradient product
@pytest.mark.parametrize("name, kw", CASES, ids=[c[0] for c in CASES])
def test_bf16_input_vjp_launches_no_weight_gradient_product(dev, name, kw):
    from siss_amd import lib
    eng, _ = _engine(kw, torch.bfloat16)
    x, t, cot = _inputs(kw)
    eng.forward(x.to(dev), t.to(dev))
    torch.cuda.synchronize()
    lib.dispatch_counts(reset=True)
    eng.input_vjp(cot.to(dev).contiguous())
    torch.cuda.synchronize()
    got = lib.dispatch_counts(reset=True)
    assert got["gemm_tn_kernel<1>"] == got["gemm_tn_kernel<3>"] == got["gemm_tn_pair"] == 0, got
    # positive control: the weight-gradient backward of the same forward does land on them
    eng.zero_grad()
    eng.backward(cot.to(dev).contiguous(), nsets=1)
    torch.cuda.synchronize()
    got = lib.dispatch_counts(reset=True)
    assert got["gemm_tn_kernel<1>"] + got["gemm_tn_kernel<3>"] + got["gemm_tn_pair"] > 0, got


# ---------------------------------------------------------------- 4. the training state is left alone
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_input_vjp_and_evaluation_leave_the_training_state_bitwise(dev):
    from siss_amd import lib
    from siss_amd.likelihood import LikelihoodEvaluator, VPSDE
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.step import SISSStepper
    kw = MNIST_SMALL
    eng, _ = _engine(kw, torch.bfloat16)
    B = 2
    st = SISSStepper(eng, DDPMScheduler().alphas_cumprod, lr=1e-4, scaling_norm=5.0, train_batch_size=B, mixed_precision="bf16",
                     inf_guard=True)
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (B, 1, 28, 28)
    for _ in range(2):                                   # two steps: AdamW moments, both gradient sets and a sparse-fill plan exist
        x0, a0, noise = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
        st.step(x0, a0, noise, torch.randint(0, 1000, (B,), device=dev, generator=g), torch.rand(B, device=dev, generator=g))
    torch.cuda.synchronize()
    lib.overwrite_log()                                  # (drained: whatever the steps left)
    ps = eng.ps
    snap = [ps.flat.clone(), ps.grads.clone(), ps.shadow.clone(), st.opt.m.clone(), st.opt.v.clone()]
    fill = (eng._fill_key, eng._fill_plan, dict(eng._fill_plans), eng.wgrad_overwrite)
    assert fill[2], "the steps recorded no sparse-fill plan"

    def unchanged():
        torch.cuda.synchronize()
        for a, b in zip(snap, [ps.flat, ps.grads, ps.shadow, st.opt.m, st.opt.v]):
            assert torch.equal(_bits(a), _bits(b))
        assert (eng._fill_key, eng._fill_plan, eng.wgrad_overwrite) == (fill[0], fill[1], fill[3])
        assert eng._fill_plans.keys() == fill[2].keys() and all(eng._fill_plans[k] is v for k, v in fill[2].items())
        assert lib.overwrite_log() == []
    x, t, cot = _inputs(kw)
    eng.forward(x.to(dev), t.to(dev))
    eng.input_vjp(cot.to(dev).contiguous())
    unchanged()
    ev = LikelihoodEvaluator(VPSDE())
    bpd, _, nfe = ev.evaluate_likelihood(eng, x[:1].to(dev), generator=torch.Generator(device=dev).manual_seed(1))
    assert math.isfinite(float(bpd[0])) and nfe >= 8
    unchanged()


# ---------------------------------------------------------------- 5. the class surface
def _bitwise_or_within_rerun_spread(got, ref, rerun, what):
    """got must equal ref bitwise when the computation is bitwise reproducible (ref == rerun); otherwise within twice the
    run-to-run spread."""
    if all(torch.equal(a, b) for a, b in zip(ref, rerun)):
        for a, b in zip(got, ref):
            assert torch.equal(a, b), what
        return "bitwise"
    for a, b, c in zip(got, ref, rerun):
        assert float((a - b).abs().max()) <= 2 * float((c - b).abs().max()) + 1e-30, what
    return "within the rerun spread"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_class_surface_sample_gradient(dev, dtype):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    kw = MNIST_SMALL
    m = UNet2DModel(UNet2DConfig(**kw), device=dev, compute_dtype=dtype)
    m.engine.init_random(seed=3)
    x, t, cot = (a.to(dev) for a in _inputs(kw))
    # torch.autograd.grad with respect to the sample == input_vjp, and no parameter gradient is touched
    grads_before = m.engine.ps.grads.clone()
    xs = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(m(xs, t)[0], xs, cot)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(m.engine.ps.grads, grads_before)
    m.engine.forward(x, t)
    vjp1 = m.engine.input_vjp(cot.contiguous()).clone()
    m.engine.forward(x, t)
    vjp2 = m.engine.input_vjp(cot.contiguous()).clone()
    how = _bitwise_or_within_rerun_spread([dx], [vjp1], [vjp2], "autograd.grad vs input_vjp")
    assert torch.equal(vjp1, vjp2), "input_vjp is not bitwise reproducible"

    # .backward() with a sample that requires grad: sample.grad, and the parameter gradients of today's path -- the SAME launches
    # (plus conv_in's data gradient), so the same numbers up to the order of the atomic per-channel sums (GroupNorm gamma / beta)
    from siss_amd import lib

    def params_grads(sample_requires_grad):
        for p in m.parameters():
            p.grad = None
        s = x.clone().requires_grad_(sample_requires_grad)
        out = m(s, t)[0]
        torch.cuda.synchronize()
        lib.PROF = []
        try:
            out.backward(cot)
            torch.cuda.synchronize()
            launches = [(r[0], r[4]) for r in lib.PROF]
        finally:
            lib.PROF = None
        return [p.grad.clone() for p in m.parameters()], s.grad, launches
    today1, none, l_today = params_grads(False)
    assert none is None
    today2, _, _ = params_grads(False)
    got, sgrad, l_got = params_grads(True)
    assert [r for r in l_got if not r[0].startswith("siss_conv_in_dgrad")] == l_today
    assert sum(r[0].startswith("siss_conv_in_dgrad") for r in l_got) == 1
    for a, b, c in zip(got, today1, today2):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + float((c - b).abs().max())
    same = all(torch.equal(a, b) for a, b in zip(got, today1))
    assert torch.equal(sgrad, vjp1)
    print(f"\n{dtype}: autograd.grad vs input_vjp {how}; parameter gradients: today's launch sequence, values bitwise equal: {same}")


# ---------------------------------------------------------------- 6. siss_pflow_drift_div
@pytest.mark.parametrize("shape", [(2, 1, 28, 28), (1, 3, 64, 64), (3, 3, 5, 7)], ids=["mnist", "rgb64", "odd"])
def test_pflow_drift_is_torchs_f32_expression_and_divergence_f64(dev, shape):
    from siss_amd import lib
    from siss_amd.likelihood import VPSDE
    sde = VPSDE()
    B = shape[0]
    chw = int(np.prod(shape[1:]))
    n = B * chw
    g = torch.Generator(device=dev).manual_seed(7)
    x, pred, v = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
    eps = torch.randint(0, 2, shape, device=dev, generator=g).float() * 2 - 1
    for t in (1e-5, 0.3, 0.5004, 0.97, 1.0):
        beta, std, label = sde.coefficients(t)
        g2 = np.float32(np.sqrt(beta) * np.sqrt(beta))
        par = torch.tensor([beta, std, g2], dtype=torch.float32, device=dev)
        nblk = max(1, chw // 512)
        out = torch.full((n + B,), float("nan"), dtype=torch.float64, device=dev)
        part = torch.empty(B, nblk, dtype=torch.float64, device=dev)
        lib.call("siss_pflow_drift_div", x, pred, v, eps, par, out, part, B, chw, nblk)
        lib.call("siss_slab_rowsum_f64", part, out[n:], B, nblk)
        # the reference's expression (sde_lib.VPSDE.sde + get_score_fn + RSDE.sde, probability_flow=True), f32 on this GPU
        vec_t = torch.ones(B, device=dev) * t
        beta_t = sde.beta_0 + vec_t * (sde.beta_1 - sde.beta_0)
        drift = -0.5 * beta_t[:, None, None, None] * x
        diffusion = torch.sqrt(beta_t)
        labels = vec_t * (sde.N - 1)
        std_t = sde.sqrt_1m_alphas_cumprod.to(dev)[labels.long()]
        score = -pred / std_t[:, None, None, None]
        ref = drift - diffusion[:, None, None, None] ** 2 * score * 0.5
        assert int(labels.long()[0]) == label and float(std_t[0]) == float(std) and float(beta_t[0]) == float(beta)
        assert torch.equal(out[:n].float().view(shape), ref), t
        assert torch.equal(out[:n], out[:n].float().double())
        e, vd, b, s = eps.double(), v.double(), float(beta), float(std)
        div = (e * (-0.5 * b * e)).sum(dim=(1, 2, 3)) + (e * (0.5 * b / s * vd)).sum(dim=(1, 2, 3))
        rel = float(((out[n:] - div).abs() / div.abs()).max())
        assert rel <= 1e-6, (t, rel)


# ---------------------------------------------------------------- 7. the device RK45 on analytic ODEs
def _odes():
    rng = np.random.default_rng(0)
    A = np.array([[-0.5, 1.0, 0.0], [-1.0, -0.5, 0.2], [0.0, 0.3, -2.0]])
    lam = rng.uniform(0.1, 5.0, 5000)
    c = rng.standard_normal(5000)

    def lin(xp):
        M = xp.asarray(A) if xp is np else torch.tensor(A, dtype=torch.float64, device="cuda")
        return lambda t, y: M @ y

    def vdp(xp):
        cos = np.cos if xp is np else math.cos
        cat = (lambda a: np.array(a)) if xp is np else (lambda a: torch.stack(a))
        return lambda t, y: cat([y[1], (1 - y[0] ** 2) * y[1] - y[0], -y[2] * cos(3 * t)])

    def big(xp):      # 5000 decoupled decays driven by a label floored as the likelihood ODE's (many blocks in every kernel)
        L = lam if xp is np else torch.tensor(lam, device="cuda")
        Cc = c if xp is np else torch.tensor(c, device="cuda")
        return lambda t, y: -L * y + Cc * (int(np.float32(t) * np.float32(999)) / 999.0)
    return [("linear", lin, [1.0, -0.5, 2.0], (0.0, 4.0)), ("vdp", vdp, [2.0, 0.0, 1.0], (1e-5, 3.0)),
            ("floored-5000", big, list(rng.standard_normal(5000)), (1e-5, 1.0))]


@pytest.mark.parametrize("case", _odes(), ids=lambda c: c[0])
def test_device_rk45_matches_the_host_restatement(dev, case):
    from siss_amd.likelihood import rk45
    name, make, y0, (t0, t1) = case
    ref = rk45_host(make(np), t0, np.array(y0), t1, rtol=1e-5, atol=1e-5)
    y0d = torch.tensor(y0, dtype=torch.float64, device=dev)
    out32 = torch.zeros(len(y0), device=dev)
    got = rk45(make(torch), t0, y0d, t1, rtol=1e-5, atol=1e-5, out32=out32, n32=len(y0))
    y = got.y.cpu().numpy()
    assert got.nfev == ref.nfev and got.nfev == 2 + 6 * got.n_attempted
    # (the accepted times agree to ~1e-10 only: the error estimate is a small difference of large stage sums, so the last bits of
    #  the stage arithmetic -- device loop against numpy's dot -- reach the step size controller)
    np.testing.assert_allclose(got.t, ref.t, rtol=1e-9, atol=0)
    assert float(np.abs(y - ref.y).max() / np.abs(ref.y).max()) <= 1e-12
    assert torch.equal(out32, got.y.float())            # the last state evaluated is the result (FSAL)


# ---------------------------------------------------------------- 8. integrator isolation
def test_device_pipeline_against_the_host_integrator_on_the_same_drift(dev):
    from siss_amd.likelihood import LikelihoodEvaluator, VPSDE, bits_per_dim
    kw = MNIST_SMALL
    eng, _ = _engine(kw, torch.float32, seed=5)
    sde = VPSDE()
    ev = LikelihoodEvaluator(sde)
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(1, 1, 28, 28, device=dev, generator=g).clamp(-1, 1)
    eps = torch.randint(0, 2, x.shape, device=dev, generator=g).float() * 2 - 1
    bpd, z, nfe = ev.evaluate_likelihood(eng, x, epsilon=eps)
    ode = ev._odes[tuple(x.shape)]
    # is the f32 forward + VJP (+ drift) bitwise reproducible from run to run?  (decides the bound below)
    ode.xs.copy_(x)
    a = ode(0.4).clone()
    b = ode(0.4).clone()
    reproducible = torch.equal(a, b)
    n = ode.n

    def fun(t, y):                                       # the reference's shape: numpy state, a round trip per evaluation
        ode.xs.view(-1).copy_(torch.from_numpy(y[:n].astype(np.float32)))
        return ode(t).cpu().numpy()
    y0 = np.concatenate([x.double().cpu().reshape(-1).numpy(), np.zeros(1)])
    ref = rk45_host(fun, ev.eps, y0, 1.0, rtol=ev.rtol, atol=ev.atol)
    zr = torch.from_numpy(ref.y[:n]).float().view(x.shape)
    bpd_ref = bits_per_dim(zr, torch.from_numpy(ref.y[n:]), sde)
    gap = abs(float(bpd[0]) - float(bpd_ref[0]))
    print(f"\nforward + VJP bitwise reproducible: {reproducible}; nfe device {nfe} host {ref.nfev}; |d bpd| {gap:.2e}")
    if reproducible:
        assert nfe == ref.nfev and gap <= 1e-9
    else:
        assert abs(nfe - ref.nfev) <= 6 and gap <= 1e-5


# ---------------------------------------------------------------- 9. end to end against the f64 composition
def test_bits_per_dim_against_the_f64_reference_composition(dev):
    from siss_amd.likelihood import LikelihoodEvaluator, VPSDE
    kw = MNIST_SMALL
    eng, _ = _engine(kw, torch.float32)
    g = torch.Generator().manual_seed(2)
    sd = {n: (torch.ones(s.ref_shape) if n.endswith(("norm1.weight", "norm2.weight", "group_norm.weight", "norm_out.weight"))
              else 0.002 * torch.randn(s.ref_shape, generator=g)) for n, s in eng.ps.specs.items()}    # small-std weights
    eng.load_state_dict(sd)
    net = _oracle(kw, sd)
    sde = VPSDE()
    x = (torch.rand(1, 1, 28, 28, generator=g) * 2 - 1)
    eps = torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1
    bpd, _, nfe = LikelihoodEvaluator(sde).evaluate_likelihood(eng, x.to(dev), epsilon=eps.to(dev))
    ref, nfe_ref = likelihood_f64(net, x, eps, sde)
    gap = abs(float(bpd[0]) - float(ref[0]))
    print(f"\nbits/dim: device f32 {float(bpd[0]):.8f} ({nfe} nfe), f64 composition {float(ref[0]):.8f} ({nfe_ref} nfe), |d| {gap:.2e}")
    assert gap <= 1e-4
    # negative control: without the divergence term the number moves by far more than the bound
    ref_nodiv, _ = likelihood_f64(net, x, eps, sde, drop_divergence=True)
    assert abs(float(ref_nodiv[0]) - float(bpd[0])) > 100 * 1e-4


# ---------------------------------------------------------------- 10. the task loop
def _tshirt(tmp_path, name, extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    ["training_steps=4", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "save_final=false",
                     "mixed_precision=bf16", "+dataloader_num_workers=1", *extra])
    cfg.unet = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
                    down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"],
                    layers_per_block=1)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    return task.run(), cfg


def test_delete_tshirt_logs_the_likelihood_without_changing_the_training(dev, tmp_path):
    plain, _ = _tshirt(tmp_path, "plain", [])
    want = plain.e.ps.flat.clone()
    lk = ["+metrics.likelihood.step_frequency=2",
          "+metrics.likelihood.class_cfg._target_=metrics.likelihood.LikelihoodEvaluator",
          "+metrics.likelihood.class_cfg.sde._target_=metrics.song_likelihood.sde_lib.VPSDE"]
    st, cfg = _tshirt(tmp_path, "lk", lk)
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "likelihood_rank0.jsonl"))]
    assert [r["global_step"] for r in lines] == [0, 2, 4]
    assert all(math.isfinite(r["bpd"]) and r["nfe"] >= 8 and (r["nfe"] - 2) % 6 == 0 and r["seconds"] > 0 for r in lines)
    # (two plain runs of a task loop already differ in the last bits of some weights: the bound is 1e-6, as for DeleteSD's evaluation)
    assert float((st.e.ps.flat - want).abs().max()) <= 1e-6

"""The opt-in DPM-Solver++ (2M) sampler on HIP: the fused guidance + multistep kernel (csrc/dpm_solver.hip) against the f64 and f32
restatements of tests/dpm_solver_ref.py and against siss_cfg_ddim_step's noise norms, the SD pipeline and the pixel-space
Evaluator against torch compositions with the f64 solver, and delete_tshirt / delete_sd through main.main with pipeline.sampler set."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import dpm_solver_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _solver(order=2, steps=20, **kw):
    from siss_amd.scheduler import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=order, **{**dict(timestep_spacing="leading", steps_offset=1), **SD, **kw})
    s.set_timesteps(steps)
    return s


# ---------------------------------------------------------------- 1. the fused kernel
# (name, order, step of a real 20-step grid, first): an early order-1 step, a middle order-2 step, the final step
CASES = [("order1", 2, 0, None), ("order2", 2, 10, None), ("final", 2, 19, None)]


def _inputs(dev, n, shape, g):
    gen = torch.Generator().manual_seed(n * 7 + shape[1])
    eps = torch.randn(n, *shape, generator=gen)
    if g > 1.0:                                          # eps_text = eps_uncond + a smaller text-conditional part, as a UNet gives
        eps = torch.cat([eps, eps + 0.25 * torch.randn(n, *shape, generator=gen)])
    x = torch.randn(n, *shape, generator=gen)
    m1 = torch.randn(n, *shape, generator=gen)
    return eps.to(dev), x.to(dev), m1.to(dev)


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("shape", [(4, 64, 64), (3, 17, 19)])          # C*H*W = 16384 and an odd 969
@pytest.mark.parametrize("g", [7.5, 1.0])
def test_cfg_dpmpp_kernel(dev, n, shape, g):
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import cfg_ddim_step, cfg_dpmpp_step, ddim_blocks
    sch = _solver()
    ddim = DDIMScheduler.from_pretrained(None)
    ddim.set_timesteps(50)
    eps, x, m1 = _inputs(dev, n, shape, g)
    chw = x[0].numel()
    nblk = ddim_blocks(n, chw)
    cfg = g > 1.0
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    for name, order, i, first in CASES:
        co = sch.coeffs(i, first=first)
        assert (co[4] != 0.0) == (name == "order2") and (co[2] == 0.0) == (name == "final")
        mp = m1 if co[4] != 0.0 else None
        slab = nan(2, n, nblk) if cfg else None
        xo, mo = cfg_dpmpp_step(eps, x, mp, nan(*x.shape), nan(*x.shape), co, g, slab)
        # f64, fed the same five floats.  Bound: 1e-6 of scale (the DDIM kernel's bound), scale the largest of |c_x x|, |c_0 m|,
        # |c_1 m1| over the tensor (for m: of |m|).  The kernel takes up to 3 + 3 + 6 roundings per element; their a-priori bound
        # (dpm_solver_ref.error_bound: 2^-24 per operation on the magnitudes involved, m's error carried through c_0) is printed
        # beside it and is the smaller of the two on every case here, so 1e-6 of scale is what is asserted.
        e64, nu, nt = R.guide(eps.cpu().numpy(), n, g)
        ref_x, ref_m = R.step(e64, x.cpu().numpy(), m1.cpu().numpy(), co)
        scale = max(abs(co[2]) * x.abs().max().item(), abs(co[3]) * np.abs(ref_m).max(),
                    abs(co[4]) * m1.abs().max().item() if co[4] != 0.0 else 0.0)
        bx, bm = R.error_bound(eps.cpu().numpy(), x.cpu().numpy(), m1.cpu().numpy(), n, g, co)
        err_x, err_m = np.abs(xo.cpu().numpy() - ref_x).max(), np.abs(mo.cpu().numpy() - ref_m).max()
        print(f"\n{name} n={n} chw={chw} g={g}: x err {err_x:.3g} (1e-6 scale {1e-6 * scale:.3g}, a-priori {bx:.3g}); "
              f"m err {err_m:.3g} (1e-6 scale {1e-6 * np.abs(ref_m).max():.3g}, a-priori {bm:.3g})")
        assert bx <= 1e-6 * scale and bm <= 1e-6 * np.abs(ref_m).max()
        assert err_x <= 1e-6 * scale, (name, err_x, scale)
        assert err_m <= 1e-6 * np.abs(ref_m).max(), (name, err_m)
        # the f32 restatement of the kernel's arithmetic, fed the same five floats: the same bits
        want_x, want_m = R.step_f32(eps, x, m1, n, g, co)
        assert torch.equal(xo, want_x), (name, (xo - want_x).abs().max().item())
        assert torch.equal(mo, want_m), (name, (mo - want_m).abs().max().item())
        # repeatable, bit for bit (no atomics)
        slab2 = nan(2, n, nblk) if cfg else None
        xo2, mo2 = cfg_dpmpp_step(eps, x, mp, nan(*x.shape), nan(*x.shape), co, g, slab2)
        assert torch.equal(xo, xo2) and torch.equal(mo, mo2)
        if cfg:
            assert torch.equal(slab, slab2)
            # the norm slab: the bits siss_cfg_ddim_step leaves on the same eps, n, chw, nblk; within 1e-5 of f64
            dslab = nan(2, n, nblk)
            cfg_ddim_step(eps, x, torch.empty_like(x), ddim.coeffs(981), g, 0.0, dslab)
            assert torch.equal(slab, dslab)
            got = slab.cpu().double().sum(-1).sqrt().numpy()
            np.testing.assert_allclose(got[0], nu, rtol=1e-5, atol=0)
            np.testing.assert_allclose(got[1], nt, rtol=1e-5, atol=0)
        # in place (x_out = x, m_out = m_prev) == out of place
        xi, mi = x.clone(), m1.clone()
        cfg_dpmpp_step(eps, xi, mi if co[4] != 0.0 else None, xi, mi, co, g, nan(2, n, nblk) if cfg else None)
        assert torch.equal(xi, xo) and torch.equal(mi, mo)
        # forced grid stride: one block per sample walks the whole row -- the same x and m
        s1 = nan(2, n, 1) if cfg else None
        x1, mm1 = cfg_dpmpp_step(eps, x, mp, nan(*x.shape), nan(*x.shape), co, g, s1, nblk=1)
        assert torch.equal(x1, xo) and torch.equal(mm1, mo)
        if cfg:
            np.testing.assert_allclose(s1.cpu().double().sum(-1).sqrt().numpy()[0], nu, rtol=1e-5, atol=0)
        # c_1 == 0: m_prev is not read -- a NaN-filled one leaves a finite result
        if co[4] == 0.0:
            xn, mn = cfg_dpmpp_step(eps, x, nan(*x.shape), nan(*x.shape), nan(*x.shape), co, g, nan(2, n, nblk) if cfg else None)
            assert torch.equal(xn, xo) and torch.equal(mn, mo) and torch.isfinite(xn).all()


@pytest.mark.parametrize("g", [7.5, 1.0])
def test_misaligned_views_take_the_scalar_path(dev, g):
    """x / m one float off 16-byte alignment: the launcher takes the one-element-per-lane kernel, with the same bits."""
    from siss_amd.sd_sampler import cfg_dpmpp_step, ddim_blocks
    n, shape = 3, (4, 16, 16)
    eps, x, m1 = _inputs(dev, n, shape, g)
    co = _solver().coeffs(10)
    nblk = ddim_blocks(n, 1024)
    slab = torch.empty(2, n, nblk, device=dev)
    xo, mo = cfg_dpmpp_step(eps, x, m1, torch.empty_like(x), torch.empty_like(x), co, g, slab)

    def off(t):                                          # a contiguous copy that starts 4 bytes past an aligned address
        buf = torch.empty(t.numel() + 1, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    slab2 = torch.empty(2, n, nblk, device=dev)
    xs, ms = cfg_dpmpp_step(eps, off(x), off(m1), off(x), off(m1), co, g, slab2)
    assert torch.equal(xs, xo) and torch.equal(ms, mo)
    if g > 1.0:                                          # (other lanes sum other elements: the norms agree as f64 sums do)
        torch.testing.assert_close(slab2.double().sum(-1), slab.double().sum(-1), rtol=1e-6, atol=0)


def test_bad_arguments_are_refused_and_write_nothing(dev):
    from siss_amd.sd_sampler import cfg_dpmpp_step, ddim_blocks
    n, shape = 2, (4, 16, 16)
    eps, x, m1 = _inputs(dev, n, shape, 7.5)
    sch = _solver()
    xo, mo = torch.full_like(x, 7.0), torch.full_like(x, 9.0)
    slab = torch.full((2, n, ddim_blocks(n, 1024)), 5.0, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):         # no m_prev although c_1 != 0
        cfg_dpmpp_step(eps, x, None, xo, mo, sch.coeffs(10), 7.5, slab)
    with pytest.raises(RuntimeError, match="bad argument"):         # guidance without norms
        cfg_dpmpp_step(eps, x, m1, xo, mo, sch.coeffs(10), 7.5, None)
    torch.cuda.synchronize()
    assert (xo == 7.0).all() and (mo == 9.0).all() and (slab == 5.0).all()


def test_order_1_step_equals_the_ddim_kernel(dev):
    """One (s, t) pair both grids hold: the order-1 update and siss_cfg_ddim_step's are the same map, to f32 rounding."""
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import cfg_ddim_step, cfg_dpmpp_step, ddim_blocks
    n, shape = 2, (4, 16, 16)
    eps, x, _ = _inputs(dev, n, shape, 7.5)
    ddim = DDIMScheduler.from_pretrained(None)
    sch = _solver(order=1, steps=9)                      # 901, 801, ..., 101: the first nine of DDIM's ten "leading" timesteps
    assert ddim.set_timesteps(10)[:9] == sch.timesteps
    slab = torch.empty(2, n, ddim_blocks(n, 1024), device=dev)
    for i in range(8):
        a, _ = cfg_dpmpp_step(eps, x, None, torch.empty_like(x), torch.empty_like(x), sch.coeffs(i), 7.5, slab)
        b = cfg_ddim_step(eps, x, torch.empty_like(x), ddim.coeffs(sch.timesteps[i]), 7.5, 0.0, slab)
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


# ---------------------------------------------------------------- 2. the SD pipeline
def _torch_solver(net, emb, lat, ts, ac, g, order, start=0):
    """The same sampling with the fp32 torch UNet and the f64 solver: (latents, uncond norms [n, steps], text norms)."""
    n, dev = lat.shape[0], lat.device
    x, m1, un, tn = lat.double().cpu().numpy(), None, [], []
    for i in range(start, len(ts)):
        xt = torch.from_numpy(x).to(dev).float()
        with torch.no_grad():
            e2 = net(torch.cat([xt, xt]), torch.full((2 * n,), ts[i], device=dev), emb)[0]
        e, nu, nt = R.guide(e2.double().cpu().numpy(), n, g)
        x, m1 = R.step(e, x, m1, R.coeffs(ac, ts, i, order, first=(i == start)))
        un.append(nu)
        tn.append(nt)
    return x, np.stack(un, 1), np.stack(tn, 1)


def _close(got, ref, rel, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() + 1e-12
    err = np.abs(got - ref).max()
    print(f"\n{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g}, bound {rel})")
    assert err <= rel * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {rel})"


@pytest.fixture(scope="module")
def sd_case(dev):
    gen = torch.Generator().manual_seed(5)
    text = torch.randn(2, 77, 64, generator=gen).to(dev)
    neg = torch.randn(1, 77, 64, generator=gen).to(dev).expand(2, -1, -1)
    lat = torch.randn(2, 4, 16, 16, generator=gen).to(dev)
    return text, neg, lat


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd_sampler_with_the_solver_matches_torch_composition(dev, sd_case, dtype):
    from test_hip_sd_sampling import _tiny_models
    from siss_amd.sd_sampler import SDSampler
    unet, net, vae, _ = _tiny_models(dev, dtype)
    text, neg, lat = sd_case
    steps, g = 10, 7.5
    sch = _solver(steps=steps)
    ac = R.betas_ac("scaled_linear", SD["beta_start"], SD["beta_end"])
    ref_x, ref_u, ref_t = _torch_solver(net, torch.cat([neg, text]), lat, sch.timesteps, ac, g, 2)
    pipe = SDSampler(unet, vae=vae, scheduler=sch)
    x, st = pipe(text, negative_prompt_embeds=neg, num_inference_steps=steps, guidance_scale=g, latents=lat, output_type="latent")
    got_u, got_t = np.asarray(st["uncond_noise_norm"]), np.asarray(st["text_noise_norm"])
    assert got_u.shape == got_t.shape == (2, steps) and pipe.scheduler.timesteps == R.timesteps(steps, 1000, "leading", 1)
    if dtype == torch.float32:
        _close(x.cpu().numpy(), ref_x, 1e-4, "latents (f32 engine)")
        np.testing.assert_allclose(got_u, ref_u, rtol=1e-4, atol=0)
        np.testing.assert_allclose(got_t, ref_t, rtol=1e-4, atol=0)
    else:
        cos = torch.nn.functional.cosine_similarity(x.flatten().double().cpu(), torch.from_numpy(ref_x).flatten(), dim=0).item()
        print(f"\nbf16 engine: cosine {cos:.5f}")
        assert cos >= 0.99, cos
        np.testing.assert_allclose(got_u, ref_u, rtol=3e-2, atol=0)
        np.testing.assert_allclose(got_t, ref_t, rtol=3e-2, atol=0)
    # graph replay == eager launches, bit for bit
    x_eager, st_eager = SDSampler(unet, vae=vae, scheduler=_solver(steps=steps), use_graph=False)(
        text, negative_prompt_embeds=neg, num_inference_steps=steps, guidance_scale=g, latents=lat, output_type="latent")
    assert torch.equal(x, x_eager) and st == st_eager
    imgs, _ = pipe(text, negative_prompt_embeds=neg, num_inference_steps=steps, guidance_scale=g, latents=lat, output_type="np")
    assert imgs.shape == (2, 32, 32, 3) and imgs.dtype.name == "uint8"
    # no guidance: n-row UNet batch, no norms
    x1, st1 = pipe(text, num_inference_steps=3, guidance_scale=1.0, latents=lat, output_type="latent")
    assert x1.shape == lat.shape and torch.isfinite(x1).all() and st1["text_noise_norm"] == []
    for method in (pipe.aug_prompt, pipe.get_text_cond_grad):        # defined on the DDIM step
        with pytest.raises(NotImplementedError, match="DDIM"):
            method(prompt_embeds=text[:1], negative_prompt_embeds=neg[:1])


def test_sd_sampler_order_1_follows_the_ddim_path(dev, sd_case):
    """solver_order = 1 on "leading" with the DDIM grid's offset.  DDIM's ten timesteps are 901, 801, ..., 101, 1 and end at
    alphas_cumprod[0]; the solver's nine are 901, ..., 101 and end at sigma = 0: the grids share the eight steps 901 -> 101, over
    which the two paths are the same map.  Both loops are run over those eight steps from the same latents."""
    from test_hip_sd_sampling import _tiny_models
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import SDSampler
    unet, _, vae, _ = _tiny_models(dev, torch.float32)
    text, neg, lat = sd_case
    sol, ddim = SDSampler(unet, vae=vae, scheduler=_solver(order=1, steps=9)), SDSampler(unet, vae=vae)
    assert isinstance(ddim.scheduler, DDIMScheduler) and ddim.scheduler.set_timesteps(10)[:9] == sol.scheduler.timesteps
    emb, n = sol._embeddings(text, neg, 1, True)
    shared = sol.scheduler.timesteps[:8]
    xs, st_s = sol._denoise(lat.clone(), shared, emb, 7.5, "latent", True)
    xd, st_d = ddim._denoise(lat.clone(), shared, emb, 7.5, "latent", True)
    _close(xs.cpu().numpy(), xd.cpu().numpy(), 1e-5, "order 1 against the DDIM path after 8 shared steps")
    np.testing.assert_allclose(st_s["text_noise_norm"], st_d["text_noise_norm"], rtol=1e-5)


def test_img2img_suffix_starts_at_order_1(dev, sd_case):
    from test_hip_sd_sampling import _tiny_models
    from siss_amd.sd_sampler import SDSampler
    unet, net, vae, _ = _tiny_models(dev, torch.float32)
    text, neg, _ = sd_case
    steps, g = 10, 7.5
    pipe = SDSampler(unet, vae=vae, scheduler=_solver(steps=steps))
    image = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(8)).to(dev)
    suffix, count = pipe.get_timesteps(steps, 0.5)
    assert count == 5 and suffix == pipe.scheduler.timesteps[5:]
    seeded = lambda: torch.Generator(device=dev).manual_seed(7)
    start = pipe.prepare_latents_img2img(image, suffix[0], 2, 1, generator=seeded())
    x, st = pipe.denoise_injection(image, text, strength=0.5, negative_prompt_embeds=neg, num_inference_steps=steps,
                                   guidance_scale=g, generator=seeded(), output_type="latent")
    ac = R.betas_ac("scaled_linear", SD["beta_start"], SD["beta_end"])
    emb = torch.cat([neg, text])
    ref_x, _, ref_t = _torch_solver(net, emb, start, pipe.scheduler.timesteps, ac, g, 2, start=5)
    _close(x.cpu().numpy(), ref_x, 1e-4, "img2img suffix")
    assert np.asarray(st["text_noise_norm"]).shape == (2, 5)
    np.testing.assert_allclose(st["text_noise_norm"], ref_t, rtol=1e-4, atol=0)
    # ... and an order-2 first step (reading a previous prediction that does not exist) would be another trajectory
    ts = pipe.scheduler.timesteps
    e0 = R.guide(net(torch.cat([start, start]), torch.full((4,), ts[5], device=dev), emb)[0].detach().double().cpu().numpy(), 2, g)[0]
    s = start.double().cpu().numpy()
    first_1, _ = R.step(e0, s, None, R.coeffs(ac, ts, 5, 2, first=True))
    first_2, _ = R.step(e0, s, np.zeros_like(s), R.coeffs(ac, ts, 5, 2, first=False))
    assert np.abs(first_1 - first_2).max() > 1e-2 * np.abs(first_1).max()


# ---------------------------------------------------------------- 3. the pixel-space Evaluator
KW = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
          down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)


def test_evaluator_sample_images_with_the_solver(dev):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.sampler import Evaluator
    from siss_amd.scheduler import DDPMScheduler, DPMSolverMultistepScheduler
    from oracle.unet import OracleUNet2D, UNetConfig
    hip = UNet2DModel(UNet2DConfig(**KW), device=dev, compute_dtype=torch.float32)
    sd = hip.engine.init_random(seed=9)
    net = OracleUNet2D(UNetConfig(**KW))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    # the task's own betas reach the solver.  (beta_end = 0.002: 1 / alpha_T = 1.7 instead of the default schedule's 158, which a
    # random-init network's eps does not take back -- x would end near 700 and the images' clamp would hide all but 1 % of it)
    sched = DDPMScheduler(beta_end=0.002)
    solver = DPMSolverMultistepScheduler.from_sampler_config(dict(name="dpmsolver++"), sched)
    steps = 6
    x_T = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    keep = x_T.clone()
    ev = Evaluator()
    ev.load_model(hip, sched)
    got = ev.sample_images(2, num_inference_steps=steps, x_T=x_T, sampler=solver)
    assert got.shape == (2, 16, 16, 3) and torch.equal(x_T, keep) and solver.timesteps == R.timesteps(steps)
    ac = R.betas_ac("linear", 1e-4, 0.002)

    def eps(x, t):
        with torch.no_grad():
            out = net(torch.from_numpy(x).to(dev).float(), torch.full((2,), t, device=dev))
        return out[0].double().cpu().numpy()
    ref = R.trajectory(ac, solver.timesteps, x_T.numpy(), eps, 2)[-1]
    img = np.clip(ref / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    inside = ((img > 0) & (img < 1)).mean()
    err, tol = np.abs(got - img).max(), 1e-4 * max(1.0, np.abs(ref).max()) / 2        # images = x / 2 + 0.5: half of x's scale
    print(f"\npixel-space solver: max err {err:.3g} (bound {tol:.3g}), |x| max {np.abs(ref).max():.3g}, {inside:.0%} of pixels inside (0, 1)")
    assert inside > 0.1 and err <= tol
    # the same x_T twice: the same bytes; the generator is consumed for x_T only
    assert np.array_equal(got, ev.sample_images(2, num_inference_steps=steps, x_T=x_T, sampler=solver))
    g1, g2 = (torch.Generator(device=dev).manual_seed(3) for _ in range(2))
    a = ev.sample_images(2, num_inference_steps=steps, generator=g1, sampler=solver)
    torch.randn((2, 3, 16, 16), device=dev, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    assert np.array_equal(a, ev.sample_images(2, num_inference_steps=steps, generator=torch.Generator(device=dev).manual_seed(3),
                                              sampler=solver))
    with pytest.raises(ValueError, match="noises"):
        ev.sample_images(2, num_inference_steps=steps, x_T=x_T, noises=[x_T] * steps, sampler=solver)


# ---------------------------------------------------------------- 4. the tasks through main.main
def _main(argv):
    import main
    main.main(argv)


def _watch_evaluations(monkeypatch, cls, seen):
    """Wrap cls.evaluate: the engine's weights and their operand copies are the same bytes before and after every evaluation."""
    inner = cls.evaluate

    def evaluate(self, unet, sched, forget_image, step, device):
        e = unet.engine
        torch.cuda.synchronize()
        flat, shadow = e.ps.flat.clone(), e.ps.shadow.clone()
        inner(self, unet, sched, forget_image, step, device)
        torch.cuda.synchronize()
        assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)
        seen.append(step)
    monkeypatch.setattr(cls, "evaluate", evaluate)


def _out(tmp_path, name):
    (d,) = glob.glob(os.path.join(str(tmp_path), name, "*"))
    return d


def _lines(path):
    return [json.loads(l) for l in open(path)]


FIELDS = {"sampler": "dpmsolver++2m", "num_inference_steps": 4}


def test_delete_tshirt_with_the_solver(dev, tmp_path, monkeypatch):
    from siss_amd.tasks import DeleteTShirt
    seen = []
    _watch_evaluations(monkeypatch, DeleteTShirt, seen)
    base = ["--config-name", "delete_tshirt", "training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1",
            "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "save_final=false",
            "mixed_precision=bf16", "+dataloader_num_workers=1", "+unet.sample_size=28", "+unet.in_channels=1", "+unet.out_channels=1",
            "+unet.block_out_channels=[64,128]", "+unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
            "+unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "+unet.layers_per_block=1", "eval_every=2", "+sampling_steps=2",
            "+eval_images=4", "+eval_batch_size=2", "+pipeline.num_inference_steps=4", "+metrics.fraction_deletion=true",
            "+metrics.denoising_injections.timestep=3"]
    _main([*base, f"output_dir={tmp_path}/on", "pipeline.sampler.name=dpmsolver++"])
    out = _out(tmp_path, "on")
    assert seen == [2] and os.path.isfile(os.path.join(out, "samples_step2.png"))
    assert os.path.isfile(os.path.join(out, "denoised_forget_t3_step2.png"))
    recs = _lines(os.path.join(out, "metrics_rank0.jsonl"))
    assert [r["global_step"] for r in recs] == [0, 2]
    for r in recs:
        assert {k: r[k] for k in FIELDS} == FIELDS and 0 <= r["deletion_class_fraction"] <= 1
    _main([*base, f"output_dir={tmp_path}/off"])
    recs = _lines(os.path.join(_out(tmp_path, "off"), "metrics_rank0.jsonl"))
    assert [r["global_step"] for r in recs] == [0, 2] and seen == [2, 2]
    assert all(set(r) <= {"global_step", "deletion_class_fraction", "deletion_steps", "seconds"} for r in recs)
    with pytest.raises(ValueError, match="sampler"):                 # another name: refused before the first optimizer step
        _main([*base, f"output_dir={tmp_path}/bad", "pipeline.sampler.name=unipc"])
    assert not glob.glob(os.path.join(str(tmp_path), "bad", "*", "train_log_rank0.jsonl"))


def test_delete_sd_with_the_solver(dev, tmp_path, monkeypatch):
    from PIL import Image
    from test_hip_sd_sampling import _tiny_checkpoint
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    seen = []
    _watch_evaluations(monkeypatch, DeleteSD, seen)
    base = ["--config-name", "delete_sd", "train_batch_size=2", "gradient_accumulation_steps=1", "training_steps=1",
            f"pretrained_model_name_or_path={ckpt}", f"images_all={tmp_path}/all.pt", f"images_deletion={tmp_path}/del.pt",
            "save_final=false", f"validation_prompts=[{tmp_path}/prompt_ids.pt]", "eval_every=1", "+eval_batches=1",
            "+eval_batch_size=2", "+pipeline.num_inference_steps=4"]
    _main([*base, f"output_dir={tmp_path}/on", "pipeline.sampler.name=dpmsolver++"])
    out = _out(tmp_path, "on")
    assert seen == [1] and Image.open(os.path.join(out, "validation_p0_step1.png")).size == (32 + 4, 2 * 34 + 2)
    (rec,) = _lines(os.path.join(out, "noise_norms_rank0.jsonl"))
    assert {k: rec[k] for k in FIELDS} == FIELDS
    assert rec["timesteps"] == R.timesteps(4, 1000, "leading", 1)[::-1] == [201, 401, 601, 801]
    for k in ("text_noise_norm", "uncond_noise_norm"):               # 4 norms per image, averaged over the images
        assert len(rec[k]) == 4 and all(math.isfinite(v) and v > 0 for v in rec[k])
    _main([*base, f"output_dir={tmp_path}/off"])
    (rec,) = _lines(os.path.join(_out(tmp_path, "off"), "noise_norms_rank0.jsonl"))
    assert seen == [1, 1] and not set(FIELDS) & set(rec) and rec["timesteps"] == [1, 251, 501, 751]
    assert set(rec) == {"step", "prompt", "prompt_text", "timesteps", "text_noise_norm", "uncond_noise_norm"}

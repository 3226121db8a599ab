"""The injection check on the GPU: siss_latent_inject against float64 (tests/injection_ref.py), the img2img entry of SDSampler into
the shared DDIM loop (bitwise against __call__ from the same start latents; partial trajectories against a torch composition), the
VAE entry with its draw order, and both tasks end to end (DeleteSD's injected_mem grid + sscd_inj_<prompt>, the pixel-space
injection_rank0.jsonl)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import injection_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _close(got, ref, rel, what=""):
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {rel})"


# ---------------------------------------------------------------- 1. the kernel
SHAPES = [(1, 1, 4, 8, 8),          # base case
          (1, 3, 4, 8, 8),          # one image tiled to three
          (2, 4, 4, 5, 5),          # two images tiled to four
          (1, 5, 3, 5, 5),          # chw = 75: the scalar path (rows not 16-B aligned)
          (1, 2, 4, 24, 24),        # more than one block per sample
          (1, 70, 4, 40, 40),       # 7 blocks per sample (see _blocks below), and the grid-stride loop at forced nblk
          (1, 700, 4, 24, 24)]      # 2048 // 700 = 2 < 3: the grid cap acts, every block strides


def _blocks(n, chw):
    """The launch's blocks per sample, restated: one per 1024 elements (256 lanes x f32x4), the whole grid capped at 2048 blocks."""
    return max(1, min(-(-chw // 1024), 2048 // n, 1024))


def _inputs(shape, dtype, seed):
    m, n, C, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(m, C, h, w, generator=g)
    logvar = 3 * torch.randn(m, C, h, w, generator=g) - 2
    logvar.view(-1)[0], logvar.view(-1)[1] = -40.0, 30.0          # both clamps act (exact in bf16 too)
    moments = torch.cat([mean, logvar], dim=1).to(dtype)
    return moments, torch.randn(m, C, h, w, generator=g), torch.randn(n, C, h, w, generator=g)


def _check(got, moments, eps_z, eps_t, scaling, a, b, what):
    ref, M, S = R.inject_f64(moments, eps_z, eps_t, scaling, a, b)
    bound = 2 * R.inject_bound(M, S)
    err = (got.cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n{what}: max|d| {float(err.max()):.3e}, largest error / asserted bound {worst:.3f}")
    assert torch.isfinite(got).all() and bool((err <= bound).all()), (what, worst)
    return ref, bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_latent_inject_against_f64(dev, shape, dtype):
    """x_i = a * ((mean_j + exp(0.5 * clamp(logvar_j, -30, 20)) * eps_z_j) * scaling) + b * eps_t_i, j = i mod m, against float64
    from the same f32 / bf16 inputs and the same f32 scalars: the difference is the kernel's arithmetic alone.

    The bound, per element (U = 2^-24, one rounding to nearest; ulp(v) <= 2^-23 |v|).  The kernel rounds seven times: 0.5 * lv
    (exact, counted all the same), std * eps_z, mean + (.), (.) * scaling, a * z, b * eps_t and the final sum.  Each rounding is at
    most U relative to its own result, and every result is bounded by M = (|mean| + |std * eps_z|) * scaling * a + |b * eps_t| once
    carried to the output, so to first order the roundings add up to at most 7 U M.  expf is documented by HIP's math API at 1 ulp:
    std is off by at most 2^-23 std, which reaches the output through S = |std * eps_z| * scaling * a alone.  Derived bound:
    7 * 2^-24 * M + 2^-23 * S.  Asserted: twice that (the second-order terms are ~1e-7 of it)."""
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import ddim_blocks, latent_inject
    m, n, C, h, w = shape
    chw = C * h * w
    assert ddim_blocks(n, chw) == _blocks(n, chw)
    if shape == (1, 2, 4, 24, 24):
        assert _blocks(n, chw) == 3
    if shape == (1, 70, 4, 40, 40):                      # 7 x 1024 lanes-elements cover 6400: below the cap of 2048 // 70 = 29
        assert _blocks(n, chw) == 7 == -(-chw // 1024) < 2048 // n
    if shape == (1, 700, 4, 24, 24):                     # the cap: 2 blocks of 1024 elements per sweep for 2304 -> 2 sweeps each
        assert _blocks(n, chw) == 2048 // n == 2 < -(-chw // 1024)
    moments, eps_z, eps_t = _inputs(shape, dtype, seed=sum(shape))
    d_mom, d_ez, d_et = moments.to(dev), eps_z.to(dev), eps_t.to(dev)
    sch = DDIMScheduler.from_pretrained(None)
    scaling = R.f32(0.18215)
    big = n * chw > 1 << 20
    for t in ((500,) if big else (0, 500, 999)):
        a, b = R.scalars(sch.alphas_cumprod, t)
        got = latent_inject(d_mom, d_ez, d_et, scaling, a, b)
        ref, bound = _check(got, moments, eps_z, eps_t, scaling, a, b, f"{shape} {dtype} t={t}")
        assert torch.equal(got, latent_inject(d_mom, d_ez, d_et, scaling, a, b))          # the same bits again
        for nblk in (1, 2):                              # the grid-stride loop: an elementwise kernel gives the same bits on any grid
            assert torch.equal(got, latent_inject(d_mom, d_ez, d_et, scaling, a, b, nblk=nblk)), nblk
    if m == 2:                                           # negative control: tiled [0, 0, 1, 1] instead of [0, 1, 0, 1]
        wrong = R.inject_f64(moments, eps_z, eps_t, scaling, a, b, order="block")[0]
        away = float(((got.cpu().double() - wrong).abs() / bound.clamp_min(1e-300)).max())
        print(f"  wrong tiling: {away:.3g} asserted bounds away")
        assert away >= 1000


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_latent_inject_misaligned_views_take_the_scalar_path(dev, dtype):
    """A shape that vectorises (chw = 2304), each pointer in turn 4 bytes (2 for bf16 moments) off a 16-byte boundary: the launcher
    falls back to one element per lane, and the result is the same bits."""
    from siss_amd.sd_sampler import latent_inject
    shape = (1, 2, 4, 24, 24)
    moments, eps_z, eps_t = [v.to(dev) for v in _inputs(shape, dtype, seed=9)]
    a, b = R.f32(0.8), R.f32(0.6)
    want = latent_inject(moments, eps_z, eps_t, 0.18215, a, b)

    def off(v):
        buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=dev)
        view = buf[1:].view(v.shape)
        view.copy_(v)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    for k in range(4):
        args = [moments, eps_z, eps_t]
        out = torch.empty_like(eps_t)
        if k < 3:
            args[k] = off(args[k])
        else:
            out = off(out)
        got = latent_inject(*args, 0.18215, a, b, out=out)
        assert torch.equal(got, want), k
    _check(want, moments.cpu(), eps_z.cpu(), eps_t.cpu(), 0.18215, a, b, f"aligned {dtype}")


def test_latent_inject_refuses_bad_arguments(dev):
    from siss_amd import lib
    mom = torch.zeros(2, 8, 4, 4, device=dev)
    ez = torch.zeros(2, 4, 4, 4, device=dev)
    et = torch.zeros(3, 4, 4, 4, device=dev)
    x = torch.full((3, 4, 4, 4), float("nan"), device=dev)
    bad = [(mom, 0, ez, et, x, 2, 3, 64, 1.0, 0.8, 0.6, 1),              # n % m != 0
           (None, 0, ez, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 1), (mom, 0, None, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 1),
           (mom, 0, ez, None, x, 1, 3, 64, 1.0, 0.8, 0.6, 1), (mom, 0, ez, et, None, 1, 3, 64, 1.0, 0.8, 0.6, 1),
           (mom, 2, ez, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 1),              # no such moments type
           (mom, 0, ez, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 0), (mom, 0, ez, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 1025),
           (mom, 0, ez, et, x, 0, 3, 64, 1.0, 0.8, 0.6, 1), (mom, 0, ez, et, x, 1, 3, 0, 1.0, 0.8, 0.6, 1)]
    for args in bad:
        with pytest.raises(RuntimeError, match="status 1"):
            lib.call("siss_latent_inject", *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())                    # nothing was launched
    lib.call("siss_latent_inject", mom, 0, ez, et, x, 1, 3, 64, 1.0, 0.8, 0.6, 1)
    assert bool((x == 0).all())


# ---------------------------------------------------------------- the tiny UNet / VAE pair of tests/test_hip_sd_sampling.py
def _perturbed(module, seed=0):
    torch.manual_seed(seed)
    with torch.no_grad():
        for nm, p in module.named_parameters():
            if "norm" in nm or nm.endswith(".bias"):
                p.add_(0.05 * torch.randn_like(p))
    return module.eval()


def _tiny_models(dev, dtype):
    from sd_decoder_ref import RefVAEDecoder
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    from siss_amd.vae import VAEDecoder, VAEDecoderConfig
    from oracle.unet_cond import OracleUNet2DCondition, UNetCondConfig
    from oracle.vae import VAEConfig
    oc = UNetCondConfig.tiny()
    kw = {k: getattr(oc, k) for k in ("sample_size", "in_channels", "out_channels", "block_out_channels", "down_block_types",
                                      "up_block_types", "layers_per_block", "attention_head_dim", "cross_attention_dim",
                                      "norm_num_groups", "norm_eps", "downsample_padding", "flip_sin_to_cos", "freq_shift")}
    unet = UNet2DConditionModel(UNet2DConditionConfig(**kw), device=dev, compute_dtype=dtype)
    sd = unet.engine.init_random(seed=11)
    net = OracleUNet2DCondition(oc)
    net.load_state_dict(sd)
    vcfg = dict(block_out_channels=(64, 128), layers_per_block=1)
    torch.manual_seed(3)
    vref = _perturbed(RefVAEDecoder(VAEConfig(**vcfg)))
    vae = VAEDecoder(VAEDecoderConfig(**vcfg), dev)
    vae.load_state_dict(vref.state_dict())
    return unet, net.to(dev).eval(), vae, vref.to(dev)


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def tiny(request, dev):
    unet, net, vae, _ = _tiny_models(dev, request.param)
    g = torch.Generator().manual_seed(5)
    text = torch.randn(2, 77, 64, generator=g).to(dev)
    neg = torch.randn(1, 77, 64, generator=g).to(dev).expand(2, -1, -1)
    lat = (0.8 * torch.randn(2, 4, 16, 16, generator=g)).to(dev)
    return request.param, unet, net, vae, text, neg, lat


# ---------------------------------------------------------------- 2. the loop entry
def test_full_strength_injection_is_call_from_the_same_start(dev, tiny):
    """strength = 1.0 runs every step: denoise_injection is then __call__ from the latents prepare_latents_img2img returns for the
    same generator state -- the same loop, the same bits."""
    from siss_amd.sd_sampler import SDSampler
    _, unet, _, vae, text, neg, lat = tiny
    pipe = SDSampler(unet, vae=vae)
    ts, count = pipe.get_timesteps(4, 1.0)
    assert count == 4 and ts == pipe.scheduler.set_timesteps(4)
    x_t = pipe.prepare_latents_img2img(lat, ts[0], 2, 1, generator=torch.Generator(device=dev).manual_seed(21))
    noise = torch.randn(lat.shape, generator=torch.Generator(device=dev).manual_seed(21), device=dev)
    a, b = R.scalars(pipe.scheduler.alphas_cumprod, ts[0])
    assert torch.equal(x_t, a * lat + b * noise)         # latents in: bitwise torch's add_noise
    for g in (7.5, 1.0):
        got, st = pipe.denoise_injection(lat, text, strength=1.0, negative_prompt_embeds=neg, num_inference_steps=4,
                                         guidance_scale=g, generator=torch.Generator(device=dev).manual_seed(21),
                                         output_type="latent")
        want, st2 = pipe(text, negative_prompt_embeds=neg, num_inference_steps=4, guidance_scale=g, latents=x_t,
                         output_type="latent")
        assert torch.equal(got, want) and st == st2 and not torch.equal(got, x_t)
    img, _ = pipe.denoise_injection(lat, text, strength=1.0, negative_prompt_embeds=neg, num_inference_steps=4,
                                    generator=torch.Generator(device=dev).manual_seed(21), output_type="decoded")
    img2, _ = pipe(text, negative_prompt_embeds=neg, num_inference_steps=4, latents=x_t, output_type="decoded")
    assert img.shape == (2, 3, 32, 32) and torch.equal(img, img2)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe.denoise_injection(lat, text, negative_prompt_embeds=neg, num_inference_steps=4, eta=0.5, output_type="latent")
    with pytest.raises(ValueError, match="Cannot duplicate"):
        pipe.denoise_injection(lat, text[:1].expand(3, -1, -1), negative_prompt_embeds=neg[:1].expand(3, -1, -1),
                               num_inference_steps=4, output_type="latent")


# ---------------------------------------------------------------- 3. partial trajectories
def _torch_injection(net, text, neg, lat, noise, N, strength, g):
    """The same check with the fp32 torch UNet: float64 latent preparation, float64 guidance + DDIM over the suffix."""
    from siss_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler.from_pretrained(None)
    steps, _ = R.timesteps_ref(sch.set_timesteps(N), N, strength)
    n = lat.shape[0]
    a, b = R.scalars(sch.alphas_cumprod, steps[0])
    zero = torch.zeros_like(lat)
    x = R.inject_f64(torch.cat([lat, zero], dim=1), zero, noise, 1.0, a, b)[0].to(lat.device)
    emb = torch.cat([neg, text]) if g > 1.0 else text
    un, tn = [], []
    for t in steps:
        xin = torch.cat([x, x]) if g > 1.0 else x
        with torch.no_grad():
            e = net(xin.float(), torch.full((xin.shape[0],), t, device=x.device), emb)[0]
        x, norms = R.ddim_f64(e, x, n, g, sch.coeffs(t))
        if norms is not None:
            un.append(norms[0])
            tn.append(norms[1])
    return x.float(), (torch.stack(un, 1), torch.stack(tn, 1)) if un else None, len(steps)


@pytest.mark.parametrize("g", [7.5, 1.0])
@pytest.mark.parametrize("N,strength,executed", [(4, 0.5, 2), (7, 0.3, 2)])
def test_partial_trajectory_matches_torch_composition(dev, tiny, N, strength, executed, g):
    """The bounds of test_sd_sampler_matches_torch_composition (tests/test_hip_sd_sampling.py) for the full trajectory: f32 engine
    1e-4 of max|latent| and 1e-4 relative on the norms; bf16 engine cosine >= 0.99 and 3e-2 on the norms.  A suffix of that
    computation needs no looser bound."""
    from siss_amd.sd_sampler import SDSampler
    dtype, unet, net, vae, text, neg, lat = tiny
    pipe = SDSampler(unet, vae=vae)
    noise = torch.randn(lat.shape, generator=torch.Generator(device=dev).manual_seed(33), device=dev)
    ref_x, ref_norms, count = _torch_injection(net, text, neg, lat, noise, N, strength, g)
    assert count == executed
    x, st = pipe.denoise_injection(lat, text, strength=strength, negative_prompt_embeds=neg, num_inference_steps=N,
                                   guidance_scale=g, generator=torch.Generator(device=dev).manual_seed(33), output_type="latent")
    assert x.shape == lat.shape
    if dtype == torch.float32:
        _close(x.cpu(), ref_x.cpu(), 1e-4, "latents")
    else:
        cos = torch.nn.functional.cosine_similarity(x.flatten().double(), ref_x.flatten().double(), dim=0).item()
        print(f"\nbf16 N={N} strength={strength} g={g}: cosine {cos:.6f}")
        assert cos >= 0.99, cos
    if g > 1.0:
        got_u, got_t = torch.tensor(st["uncond_noise_norm"]), torch.tensor(st["text_noise_norm"])
        assert got_u.shape == got_t.shape == (2, executed)               # one entry per executed step
        rtol = 1e-4 if dtype == torch.float32 else 3e-2
        assert torch.allclose(got_u, ref_norms[0].cpu().float(), rtol=rtol, atol=0)
        assert torch.allclose(got_t, ref_norms[1].cpu().float(), rtol=rtol, atol=0)
    else:
        assert st == {"uncond_noise_norm": [], "text_noise_norm": []}


# ---------------------------------------------------------------- 4. the VAE entry
def test_vae_entry_samples_the_posterior_then_noises(dev):
    """A 3-channel image through the tiny VAEEncoder: prepare_latents_img2img against the restatement fed the encoder's own moments
    (the kernel and the draw order alone), at the kernel test's bound.  The posterior normals are drawn first: the expectation
    with the two draws swapped is far away."""
    from siss_amd.sd_sampler import SDSampler
    from siss_amd.vae import VAEEncoder, VAEEncoderConfig
    from oracle.vae import OracleVAEEncoder, VAEConfig
    kw = dict(block_out_channels=(64, 128), layers_per_block=1)
    torch.manual_seed(0)
    enc = VAEEncoder(VAEEncoderConfig(**kw), dev)
    enc.load_state_dict(_perturbed(OracleVAEEncoder(VAEConfig(**kw))).state_dict())
    seen = []
    inner = enc.raw_moments
    enc.raw_moments = lambda image: seen.append(inner(image)) or seen[-1]
    pipe = SDSampler(unet=None, vae_encoder=enc)
    img = (torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(dev)
    t = pipe.get_timesteps(50, 0.5)[0][0]
    x = pipe.prepare_latents_img2img(img, t, 1, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    mom = seen[0]
    assert len(seen) == 1 and mom.shape == (1, 8, 16, 16) and mom.dtype == torch.float32 and x.shape == (3, 4, 16, 16)
    mean, logvar = enc.moments(img)                      # moments() is the clamped form of its own call's raw moments
    assert len(seen) == 2 and torch.equal(mean, seen[1][:, :4]) and torch.equal(logvar, seen[1][:, 4:].clamp(-30.0, 20.0))
    g = torch.Generator(device=dev).manual_seed(8)
    eps_z = torch.randn(1, 4, 16, 16, generator=g, device=dev)
    eps_t = torch.randn(3, 4, 16, 16, generator=g, device=dev)
    a, b = R.scalars(pipe.scheduler.alphas_cumprod, t)
    _, bound = _check(x, mom, eps_z, eps_t, R.f32(0.18215), a, b, "VAE entry")
    g = torch.Generator(device=dev).manual_seed(8)       # swapped: the noise first
    eps_t2 = torch.randn(3, 4, 16, 16, generator=g, device=dev)
    eps_z2 = torch.randn(1, 4, 16, 16, generator=g, device=dev)
    wrong = R.inject_f64(mom, eps_z2, eps_t2, R.f32(0.18215), a, b)[0]
    assert float(((x.cpu().double() - wrong).abs() / bound.clamp_min(1e-300)).max()) >= 1000
    with pytest.raises(ValueError, match="vae_encoder"):
        SDSampler(unet=None).prepare_latents_img2img(img, t, 1, 1, device=dev)


# ---------------------------------------------------------------- 5. DeleteSD end to end
def _tiny_checkpoint(dev, ckpt):
    from safetensors.torch import save_file
    from sd_decoder_ref import RefVAEDecoder
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    from oracle.clip_text import CLIPTextCfg, OracleCLIPText
    from oracle.vae import OracleVAEEncoder, VAEConfig
    ucfg = UNet2DConditionConfig(sample_size=16, block_out_channels=(64, 128),
                                 down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                                 up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), attention_head_dim=2,
                                 cross_attention_dim=128)
    unet = UNet2DConditionModel(ucfg, device=dev)
    unet.engine.init_random(seed=3)
    unet.save_pretrained(str(ckpt / "unet"))
    torch.manual_seed(0)
    sd = dict(OracleVAEEncoder(VAEConfig.tiny()).state_dict())
    sd.update(RefVAEDecoder(VAEConfig.tiny()).state_dict())
    os.makedirs(ckpt / "vae")
    json.dump(dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=[64, 128], layers_per_block=1,
                   norm_num_groups=32, scaling_factor=0.18215), open(ckpt / "vae" / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ckpt / "vae" / "diffusion_pytorch_model.safetensors"))
    clip = OracleCLIPText(CLIPTextCfg(vocab_size=49408, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                      num_attention_heads=2))     # the full vocabulary: the SD v1 empty-prompt ids
    os.makedirs(ckpt / "text_encoder")
    json.dump(dict(num_attention_heads=2, layer_norm_eps=1e-5, hidden_size=128), open(ckpt / "text_encoder" / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in clip.state_dict().items()}, str(ckpt / "text_encoder" / "model.safetensors"))


def _run_sd(tmp_path, name, ckpt, overrides, prompt, hook=None):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     f"pretrained_model_name_or_path={ckpt}", f"images_all={tmp_path}/all.pt",
                     f"images_deletion={tmp_path}/del.pt", "save_final=false", *overrides])
    cfg.validation_prompts = [prompt]
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    if hook is not None:
        hook(task)
    return task, task.run(), cfg


def _weights_hook(store, name):
    """Wrap task.evaluate: the evaluation only reads the weights (bitwise), and the weights it found are kept under `name`."""
    def install(task):
        inner = task.evaluate

        def evaluate(unet, sched, forget_image, step, device):
            e = unet.engine
            torch.cuda.synchronize()
            flat, shadow = e.ps.flat.clone(), e.ps.shadow.clone()
            inner(unet, sched, forget_image, step, device)
            torch.cuda.synchronize()
            assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)
            store[name, step] = flat
        task.evaluate = evaluate
    return install


def _same_weights(store, a, b, steps, rerun):
    """The trained weights of run `a` are bitwise those of run `b` -- wherever a run is itself reproducible: the step's gradient
    kernels add with float atomics (tests/test_hip_sd_sampling.py records up to 3e-8 between two plain runs), so when the two differ
    a second run of `b` (`rerun()`, stored as "again") tells which case this machine is in, and the comparison takes that test's 1e-6."""
    if all(torch.equal(store[a, s], store[b, s]) for s in steps):
        return
    rerun()
    assert not all(torch.equal(store["again", s], store[b, s]) for s in steps), "the run is reproducible, yet the block changed it"
    for s in steps:
        assert float((store[a, s] - store[b, s]).abs().max()) <= 1e-6


def test_delete_sd_injection_end_to_end(dev, tmp_path):
    from PIL import Image
    from siss_amd import lib
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    prompt = str(tmp_path / "prompt_ids.pt")
    mem = torch.randint(0, 256, (32, 32, 3), generator=g, dtype=torch.uint8)
    Image.fromarray(mem.numpy()).save(str(tmp_path / "mem.png"))
    evals = ["training_steps=1", "eval_every=1", "+eval_batches=1", "+eval_batch_size=1", "+pipeline.num_inference_steps=4",
             "resolution=32", f"data_files.mem_img_path={tmp_path}/mem.png"]
    block = ["metrics.denoising_injections.strength=0.5", "metrics.denoising_injections.num_images=4",
             "metrics.denoising_injections.prompt=0", f"metrics.sscd.model_path={tmp_path}/missing.pt",
             "metrics.sscd.allow_random_init=true"]
    store, decoded = {}, []
    _, _, cfg0 = _run_sd(tmp_path, "plain", ckpt, evals, prompt, _weights_hook(store, "plain"))
    assert cfg0.metrics.denoising_injections is None
    plain_files = sorted(os.listdir(cfg0.output_dir))
    assert plain_files == ["noise_norms_rank0.jsonl", "train_log_rank0.jsonl", "validation_p0_step1.png"]   # no new file

    def hook(task):
        _weights_hook(store, "inj")(task)
        inner = task._validation_pipeline

        def build(unet, device):                         # keep the decoder output the injection is scored from
            pipe = inner(unet, device)
            run = pipe.denoise_injection

            def spy(*a, **kw):
                out = run(*a, **kw)
                decoded.append((out[0].clone(), kw))
                return out
            pipe.denoise_injection = spy
            return pipe
        task._validation_pipeline = build
    task, _, cfg = _run_sd(tmp_path, "inj", ckpt, evals + block, prompt, hook)
    assert sorted(os.listdir(cfg.output_dir)) == sorted(plain_files + ["injected_mem_s0.5_step1.png", "metrics_rank0.jsonl"])
    im = Image.open(os.path.join(cfg.output_dir, "injected_mem_s0.5_step1.png"))
    assert im.size == (2 * 34 + 2, 2 * 34 + 2)           # make_grid: 4 images of 32 x 32, nrow = 2, 2-pixel padding
    assert len(decoded) == 1
    img, kw = decoded[0]
    assert img.shape == (4, 3, 32, 32) and kw["strength"] == 0.5 and kw["num_inference_steps"] == 4 and kw["guidance_scale"] == 7.5
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))]
    inj = [r for r in lines if "sscd_inj_0" in r]
    assert inj == [r for r in lines if "sscd_0" not in r] and len(inj) == 1 and inj[0]["global_step"] == 1
    assert [r["global_step"] for r in lines if "sscd_0" in r] == [1]                     # the validation score is still recorded
    v = inj[0]["sscd_inj_0"]
    assert isinstance(v, float) and math.isfinite(v) and -1.0 <= v <= 1.0
    # by hand: the same decoded tensor through the same network against the memorized image's embedding
    model = task.sscd.model
    ref = model.embed_u8(mem[None].to(dev))[0]
    _, u8, scores = model.embed_decoded(img, ref=ref)
    again = float(scores.cpu().double().mean())
    print(f"\nsscd_inj_0 recorded {v:.9f}, by hand {again:.9f}")
    assert abs(v - again) <= 2.0 ** -22
    tiles = np.asarray(im)
    assert np.array_equal(tiles[2:34, 2:34], u8[0].cpu().numpy()) and np.array_equal(tiles[36:68, 36:68], u8[3].cpu().numpy())
    _same_weights(store, "inj", "plain", (1,), lambda: _run_sd(tmp_path, "again", ckpt, evals, prompt, _weights_hook(store, "again")))
    # refused before the first step
    with pytest.raises(ValueError, match="no denoising step"):
        _run_sd(tmp_path, "bad", ckpt, evals + ["metrics.denoising_injections.strength=0.2"], prompt)      # 0.2 * 4 < 1
    assert not os.path.exists(os.path.join(str(tmp_path), "bad", "train_log_rank0.jsonl"))
    assert lib.PROF is None


# ---------------------------------------------------------------- 6. the pixel-space tasks end to end
def _run_celeb(tmp_path, name, data, overrides, hook=None):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"),
                    [f"data_dir={data}", f"output_dir={tmp_path}/{name}", "training_steps=2", "train_batch_size=2",
                     "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent", "allow_random_init=true",
                     "unet.sample_size=16", "unet.block_out_channels=[64,128]",
                     "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]", "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]",
                     "unet.layers_per_block=1", "unet.attention_head_dim=null", "save_final=false",
                     "eval_every=1", "eval_batch_size=2", "pipeline.num_inference_steps=3",
                     "metrics.denoising_injections.timestep=3", *overrides])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    if hook is not None:
        hook(task)
    return task, task.run(), cfg


def test_pixel_space_injection_score_end_to_end(dev, tmp_path):
    from PIL import Image
    data = tmp_path / "celeba"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(data / f"{10000 + i}.jpg")
    sscd = [f"metrics.denoising_injections.sscd.model_path={tmp_path}/missing.pt",
            "metrics.denoising_injections.sscd.allow_random_init=true"]
    store = {}
    _, _, cfg0 = _run_celeb(tmp_path, "plain", data, [], _weights_hook(store, "plain"))
    plain_files = sorted(os.listdir(cfg0.output_dir))
    assert "injection_rank0.jsonl" not in plain_files and "denoised_forget_t3_step2.png" in plain_files
    task, _, cfg = _run_celeb(tmp_path, "sscd", data, sscd, _weights_hook(store, "sscd"))
    assert sorted(os.listdir(cfg.output_dir)) == sorted(plain_files + ["injection_rank0.jsonl"])
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "injection_rank0.jsonl"))]
    assert [r["global_step"] for r in lines] == [1, 2]   # one line per evaluation
    model = task.injection.model
    forget = np.asarray(Image.open(data / "10000.jpg").convert("RGB"), dtype=np.uint8)
    ref = model.embed_u8(torch.from_numpy(forget.copy())[None].to(dev))[0]
    for r in lines:
        assert set(r) == {"global_step", "timestep", "sscd_mean", "sscd_max", "sscd"} and r["timestep"] == 3
        png = np.asarray(Image.open(os.path.join(cfg.output_dir, f"denoised_forget_t3_step{r['global_step']}.png")))
        assert png.shape == (16, 32, 3)
        u8 = torch.from_numpy(np.stack([png[:, :16], png[:, 16:]]).copy()).to(dev)       # the bytes of the grid
        want = model.embed_u8(u8, ref=ref)[1].cpu().double()
        got = torch.tensor(r["sscd"], dtype=torch.float64)
        print(f"\nstep {r['global_step']}: recorded {r['sscd']}, from the grid {want.tolist()}")
        assert got.shape == (2,) and float((got - want).abs().max()) <= 2.0 ** -22
        assert bool((got.abs() <= 1.0 + 2.0 ** -22).all())
        f32 = torch.tensor(r["sscd"], dtype=torch.float32)
        assert r["sscd_mean"] == float(f32.double().mean()) and r["sscd_max"] == float(f32.double().max())
    # the grid is the same picture with and without the score (same seeds, same quantisation rule), to within what two runs differ
    _same_weights(store, "sscd", "plain", (1, 2), lambda: _run_celeb(tmp_path, "again", data, [], _weights_hook(store, "again")))
    # a 1-channel network is refused before the first step
    with pytest.raises(ValueError, match="in_channels=1"):
        _run_celeb(tmp_path, "mono", data, sscd + ["unet.in_channels=1", "unet.out_channels=1"])
    assert not os.path.exists(os.path.join(str(tmp_path), "mono", "train_log_rank0.jsonl"))

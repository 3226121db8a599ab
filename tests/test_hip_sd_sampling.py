"""SD validation sampling on HIP (delete_sd.py:170-340 log_validation; data/src/local_sd_pipeline.py): the fused
guidance + DDIM kernel against float64 torch, the VAE decoder against tests/sd_decoder_ref.py, the whole pipeline against a
torch composition (oracle.unet_cond + decoder reference + float64 DDIM), and DeleteSD.evaluate end to end."""
import json
import math
import os

import pytest
import torch

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


def _ddim_f64(eps, x, n, g, co, clip):
    """Float64 guidance + DDIM (eta = 0) step and the per-sample norms of eps_uncond and eps_text - eps_uncond."""
    e = eps.double()
    sa, sb, sap, sbp = co
    if g > 1.0:
        u, d = e[:n], e[n:] - e[:n]
        e = u + g * d
        norms = (u.flatten(1).norm(dim=1), d.flatten(1).norm(dim=1))
    else:
        norms = None
    x0 = (x.double() - sb * e) / sa
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    return sap * x0 + sbp * e, norms


# ---------------------------------------------------------------- 1. the fused kernel
@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("shape", [(4, 64, 64), (3, 17, 19)])          # C*H*W = 16384 and an odd 969
@pytest.mark.parametrize("g", [7.5, 1.0])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_cfg_ddim_kernel_matches_f64(dev, n, shape, g, clip):
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import cfg_ddim_step, ddim_blocks
    sch = DDIMScheduler.from_pretrained(None)
    sch.set_timesteps(50)
    gen = torch.Generator().manual_seed(n * 7 + shape[1])
    eps = torch.randn(n, *shape, generator=gen)
    if g > 1.0:                                          # eps_text = eps_uncond + a smaller text-conditional part, as a UNet gives
        eps = torch.cat([eps, eps + 0.25 * torch.randn(n, *shape, generator=gen)])
    eps = eps.to(dev)
    x = torch.randn(n, *shape, generator=gen).to(dev)
    chw = x[0].numel()
    for t in (981, 501, 1):
        co = sch.coeffs(t)
        slab = torch.full((2, n, ddim_blocks(n, chw)), float("nan"), device=dev)
        out = cfg_ddim_step(eps, x, torch.empty_like(x), co, g, clip, slab)
        ref, norms = _ddim_f64(eps.cpu(), x.cpu(), n, g, co, clip)
        _close(out.cpu().double(), ref, 1e-6, f"x_prev t={t}")
        # diffusers' own f32 operations, one rounding each (pipeline guidance, then DDIMScheduler.step): the same bits
        e = eps[:n] + g * (eps[n:] - eps[:n]) if g > 1.0 else eps
        x0 = (x - co[1] * e) / co[0]
        if clip > 0:
            x0 = x0.clamp(-clip, clip)
        want = co[2] * x0 + co[3] * e
        assert torch.equal(out, want), (t, (out - want).abs().max().item())
        out2 = cfg_ddim_step(eps, x, torch.empty_like(x), co, g, clip, slab.clone())
        assert torch.equal(out, out2)
        if g > 1.0:
            got = slab.cpu().double().sum(-1).sqrt()
            for k in range(2):
                assert torch.allclose(got[k], norms[k], rtol=1e-5, atol=0), (t, k, got[k], norms[k])
            slab2 = torch.empty_like(slab)
            cfg_ddim_step(eps, x, torch.empty_like(x), co, g, clip, slab2)
            assert torch.equal(slab, slab2)                  # no atomics: the same bits every launch
    xi = x.clone()                                            # in place (out = x)
    cfg_ddim_step(eps, xi, xi, sch.coeffs(961), g, clip, torch.empty(2, n, ddim_blocks(n, chw), device=dev))
    assert torch.equal(xi, cfg_ddim_step(eps, x, torch.empty_like(x), sch.coeffs(961), g, clip,
                                         torch.empty(2, n, ddim_blocks(n, chw), device=dev)))


# ---------------------------------------------------------------- 2. the VAE decoder
def _perturbed(module, seed=0):
    torch.manual_seed(seed)
    with torch.no_grad():
        for nm, p in module.named_parameters():
            if "norm" in nm or nm.endswith(".bias"):
                p.add_(0.05 * torch.randn_like(p))
    return module.eval()


@pytest.mark.parametrize("case", ["tiny", "sd_widths"])
def test_vae_decoder_matches_reference(dev, case):
    from sd_decoder_ref import RefVAEDecoder
    from siss_amd.vae import VAEDecoder, VAEDecoderConfig
    from oracle.vae import VAEConfig
    kw = dict(block_out_channels=(64, 128) if case == "tiny" else (128, 256, 512, 512), layers_per_block=1)
    torch.manual_seed(0)
    ref = _perturbed(RefVAEDecoder(VAEConfig(**kw)))
    dec = VAEDecoder(VAEDecoderConfig(**kw), dev)
    dec.load_state_dict(ref.state_dict())
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref(z)
    got = dec.decode(z.to(dev))
    up = 2 ** (len(kw["block_out_channels"]) - 1)
    assert got.shape == want.shape == (2, 3, 16 * up, 16 * up)
    _close(got.cpu(), want, 3e-2, f"decoder {case}")
    _close(dec.decode(z[:1].to(dev)).cpu(), want[:1], 3e-2, f"decoder {case} N=1")     # another batch reuses the engine


def test_vae_decoder_full_size(dev):
    """SD v1 decoder (49,490,179 + 20 parameters, diffusers key names): [1, 4, 64, 64] -> [1, 3, 512, 512] against the fp32
    torch reference on the same GPU."""
    from sd_decoder_ref import RefVAEDecoder
    from siss_amd.vae import VAEDecoder
    from oracle.vae import VAEConfig
    torch.manual_seed(0)
    ref = _perturbed(RefVAEDecoder(VAEConfig.sd_v1()))
    assert sum(p.numel() for p in ref.decoder.parameters()) == 49_490_179
    assert sum(p.numel() for p in ref.post_quant_conv.parameters()) == 20
    dec = VAEDecoder(device=dev)
    assert dec.diffusers_shapes() == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    dec.load_state_dict(ref.state_dict())
    z = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(2))
    ref = ref.to(dev)
    with torch.no_grad():
        want = ref(z.to(dev))
    got = dec.decode(z.to(dev))
    assert got.shape == (1, 3, 512, 512) and torch.isfinite(got).all()
    _close(got, want, 3e-2, "SD v1 decoder")
    with pytest.raises(KeyError):
        dec.load_state_dict({k: v for k, v in ref.state_dict().items() if "post_quant_conv" not in k})


# ---------------------------------------------------------------- 3. the pipeline end to end
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


def _torch_pipeline(net, vref, text, neg, lat, steps, g):
    """The same sampling with the fp32 torch UNet, f64 guidance + DDIM, and the decoder reference."""
    from siss_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler.from_pretrained(None)
    n = lat.shape[0]
    x = lat.double()
    emb = torch.cat([neg, text])
    un, tn = [], []
    for t in sch.set_timesteps(steps):
        with torch.no_grad():
            e = net(torch.cat([x, x]).float(), torch.full((2 * n,), t, device=x.device), emb)[0]
        x, (nu, nt) = _ddim_f64(e, x, n, g, sch.coeffs(t), 0.0)
        un.append(nu)
        tn.append(nt)
    with torch.no_grad():
        img = vref((x / 0.18215).float())
    return x.float(), torch.stack(un, 1), torch.stack(tn, 1), img


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd_sampler_matches_torch_composition(dev, dtype):
    from siss_amd.sd_sampler import SDSampler
    unet, net, vae, vref = _tiny_models(dev, dtype)
    gen = torch.Generator().manual_seed(5)
    text = torch.randn(2, 77, 64, generator=gen).to(dev)
    neg = torch.randn(1, 77, 64, generator=gen).to(dev)
    lat = torch.randn(2, 4, 16, 16, generator=gen).to(dev)
    steps, g = 10, 7.5
    ref_x, ref_u, ref_t, ref_img = _torch_pipeline(net, vref, text, neg.expand(2, -1, -1), lat, steps, g)
    pipe = SDSampler(unet, vae=vae)
    x, st = pipe(text, negative_prompt_embeds=neg.expand(2, -1, -1), num_inference_steps=steps, guidance_scale=g,
                 latents=lat, output_type="latent")
    got_u, got_t = torch.tensor(st["uncond_noise_norm"]), torch.tensor(st["text_noise_norm"])
    assert got_u.shape == got_t.shape == (2, steps)
    if dtype == torch.float32:
        _close(x.cpu(), ref_x.cpu(), 1e-4, "latents")
        assert torch.allclose(got_u, ref_u.cpu().float(), rtol=1e-4, atol=0)
        assert torch.allclose(got_t, ref_t.cpu().float(), rtol=1e-4, atol=0)
    else:
        cos = torch.nn.functional.cosine_similarity(x.flatten().double(), ref_x.flatten().double(), dim=0).item()
        assert cos >= 0.99, cos
        assert torch.allclose(got_u, ref_u.cpu().float(), rtol=3e-2, atol=0)
        assert torch.allclose(got_t, ref_t.cpu().float(), rtol=3e-2, atol=0)
    # graph replay == eager launches, bit for bit
    x_eager, st_eager = SDSampler(unet, vae=vae, use_graph=False)(text, negative_prompt_embeds=neg.expand(2, -1, -1),
                                                                  num_inference_steps=steps, guidance_scale=g, latents=lat,
                                                                  output_type="latent")
    assert torch.equal(x, x_eager) and st == st_eager
    # images: decode + diffusers' postprocess
    imgs, _ = pipe(text, negative_prompt_embeds=neg.expand(2, -1, -1), num_inference_steps=steps, guidance_scale=g,
                   latents=lat, output_type="np")
    assert imgs.shape == (2, 32, 32, 3) and imgs.dtype.name == "uint8"
    want = ((ref_img / 2 + 0.5).clamp(0, 1) * 255).permute(0, 2, 3, 1).cpu()
    if dtype == torch.float32:
        assert (torch.from_numpy(imgs).float() - want).abs().max() <= 0.03 * 255
    # no guidance: n-row UNet batch, no norms
    x1, st1 = pipe(text, num_inference_steps=3, guidance_scale=1.0, latents=lat, output_type="latent")
    assert x1.shape == lat.shape and torch.isfinite(x1).all() and st1["text_noise_norm"] == []
    with pytest.raises(NotImplementedError):
        pipe(text, negative_prompt_embeds=neg, num_inference_steps=3, eta=0.5, output_type="latent")


# ---------------------------------------------------------------- 4. DeleteSD.evaluate
def _tiny_checkpoint(dev, ckpt, with_vae=True):
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
    if with_vae:
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


def _run(tmp_path, name, ckpt, overrides, prompt, hook=None):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     f"pretrained_model_name_or_path={ckpt}", f"images_all={tmp_path}/all.pt",
                     f"images_deletion={tmp_path}/del.pt", "save_final=false", *overrides])
    cfg.validation_prompts = [prompt]
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    if hook is not None:
        hook(task)
    stepper = task.run()
    return task, stepper, cfg


def test_delete_sd_evaluate_writes_grids_and_noise_norms(dev, tmp_path):
    from PIL import Image
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    prompt = str(tmp_path / "prompt_ids.pt")
    _, plain, _ = _run(tmp_path, "plain", ckpt, ["training_steps=2"], prompt)
    want = plain.e.ps.flat.clone()
    seen = {}

    def hook(task):
        inner = task.evaluate

        def evaluate(unet, sched, forget_image, step, device):
            e = unet.engine
            torch.cuda.synchronize()
            flat, shadow, fill = e.ps.flat.clone(), e.ps.shadow.clone(), (e._fill_key, dict(e._fill_plans))
            if step == 2:
                seen["params"] = flat                        # after 2 steps, with an evaluation between them
            inner(unet, sched, forget_image, step, device)
            torch.cuda.synchronize()
            # the evaluation leaves the weights, their operand copies and the sparse-fill state exactly as they were
            assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)
            assert e._fill_key == fill[0] and e._fill_plans.keys() == fill[1].keys()
            assert all(e._fill_plans[k] is v for k, v in fill[1].items())
            del flat, shadow, fill                           # (only this test's own copies: seen["params"] stays from step 2 on)
            seen[f"mem{step}"] = torch.cuda.memory_allocated()
        task.evaluate = evaluate
    evals = ["training_steps=3", "eval_every=1", "+eval_batches=2", "+eval_batch_size=1", "+pipeline.num_inference_steps=3"]
    task, _, cfg = _run(tmp_path, "eval", ckpt, evals, prompt, hook)
    # the same training as without evaluations: two plain runs of this task already differ by up to 3e-8 in ~1.5 % of the weights
    # after 2 steps (measured), so the comparison across runs takes that noise; the evaluation's own effect is held to zero above
    assert (seen["params"] - want).abs().max().item() <= 1e-6
    assert seen["mem3"] <= seen["mem2"], (seen["mem2"], seen["mem3"])
    for step in (1, 2, 3):
        im = Image.open(os.path.join(cfg.output_dir, f"validation_p0_step{step}.png"))
        assert im.size == (32 + 4, 2 * 34 + 2)               # make_grid: nrow = int(sqrt(2)) = 1, 2-pixel padding
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "noise_norms_rank0.jsonl"))]
    assert [r["step"] for r in lines] == [1, 2, 3]
    for r in lines:
        assert r["timesteps"] == [1, 334, 667] and r["prompt"] == 0
        for k in ("text_noise_norm", "uncond_noise_norm"):
            assert len(r[k]) == 3 and all(math.isfinite(v) and v > 0 for v in r[k])


def test_delete_sd_evaluate_synthetic_without_vae(dev, tmp_path):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["training_steps=1", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/out",
                     "pretrained_model_name_or_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true",
                     "save_final=false", "eval_every=1", "+eval_batches=1", "+eval_batch_size=2",
                     "+pipeline.num_inference_steps=2"])
    cfg.unet = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=[64, 128],
                    down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"],
                    up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"], attention_head_dim=2, cross_attention_dim=64)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.run()
    assert not [f for f in os.listdir(cfg.output_dir) if f.endswith(".png")]
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "noise_norms_rank0.jsonl"))]
    assert len(lines) == 1 and lines[0]["timesteps"] == [1, 501]
    assert all(math.isfinite(v) for v in lines[0]["text_noise_norm"] + lines[0]["uncond_noise_norm"])

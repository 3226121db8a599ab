#!/usr/bin/env python
"""The injection check on one GPU: prints ONE JSON line.

    python tools/bench_injection.py [--reps 3] [--skip-celeb] [--skip-sd] [--skip-kernel]

  * kernel: siss_latent_inject alone (csrc/injection.hip) on SD latents (C*h*w = 4 x 64 x 64, f32 moments) for n = 4 starting
    latents of m = 1 image -- the evaluation's launch, a few hundred KB: launch-bound -- and for n = 1024 of m = 1024, where it
    streams: us per launch and achieved GB/s (3 reads of m rows, 1 read and 1 write of n rows) beside the 8 TB/s HBM figure;
  * celeb: one evaluation's injection of the CelebA-HQ task (config/delete_celeb.yaml: google/ddpm-celebahq-256's architecture,
    bf16 engine): the forget image noised to t = 250 and denoised back over 251 steps (Evaluator.denoise_images) for n = 1 and 4,
    then the score -- quantisation on the device, SSCD ResNet-50 on the n images of 256 x 256 against the forget image's embedding;
  * sd: one evaluation's injection of the SD task (SD v1.5 architecture, bf16 engine, SD v1 VAE): a 512 x 512 image through
    SDSampler.denoise_injection at strength 0.5 of 50 steps (25 steps, guidance 7.5), n = 4, to the decoder's output, and its score.
Host-synchronised wall time after one warm-up call (which also captures the forward), median of --reps.  All weights are
random-init: the times do not depend on them.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0


def _median_s(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def kernel(dev, res):
    from siss_amd.sd_sampler import latent_inject
    chw = 4 * 64 * 64
    rows = {}
    for m, n in ((1, 4), (1024, 1024)):
        mom, ez, et = torch.randn(m, 8, 64, 64, device=dev), torch.randn(m, 4, 64, 64, device=dev), torch.randn(n, 4, 64, 64, device=dev)
        out = torch.empty_like(et)
        for _ in range(10):
            latent_inject(mom, ez, et, 0.18215, 0.8, 0.6, out=out)
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(200):
            latent_inject(mom, ez, et, 0.18215, 0.8, 0.6, out=out)
        s1.record()
        torch.cuda.synchronize()
        us = s0.elapsed_time(s1) / 200 * 1e3
        nbytes = 4 * chw * (3 * m + 2 * n)
        rows[f"m{m}_n{n}"] = {"us": round(us, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (us * 1e-6) / 1e9, 1),
                              "hbm_frac": round(nbytes / (us * 1e-6) / 1e9 / HBM_GBS, 4)}
    res["kernel"] = rows


def celeb(dev, res, reps):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.sampler import Evaluator
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.sscd import InjectionScore, SSCDModel
    unet = UNet2DModel(UNet2DConfig.celebahq256(), device=dev, compute_dtype=torch.bfloat16)
    unet.engine.init_random(seed=0)
    sch = DDPMScheduler()
    g = torch.Generator().manual_seed(0)
    forget = torch.rand(3, 256, 256, generator=g).to(dev) * 2 - 1
    score = InjectionScore(SSCDModel().to(dev), "", os.devnull)
    score._ref = torch.nn.functional.normalize(torch.randn(512, generator=g), dim=0).to(dev)     # (no image file: a unit row)
    rows = {}
    for n in (1, 4):
        noise = torch.randn(n, 3, 256, 256, generator=g).to(dev)
        noisy = sch.add_noise(forget.expand(n, -1, -1, -1), noise, torch.full((n,), 250, device=dev))
        ev = Evaluator()
        ev.load_model(unet, sch)
        den = ev.denoise_images(noisy, 250)

        def scored():
            u8 = (den.clamp(0, 1) * 255).to(torch.uint8).contiguous()
            return score.score_u8(u8).cpu()
        rows[f"n{n}"] = {"denoise_251_steps_s": round(_median_s(lambda: ev.denoise_images(noisy, 250), reps), 3),
                         "score_ms": round(_median_s(scored, reps) * 1e3, 2)}
    res["celeb"] = rows


def sd(dev, res, reps):
    from oracle.vae import OracleVAEEncoder, VAEConfig
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    from siss_amd.sd_sampler import SDSampler
    from siss_amd.sscd import SSCDModel, SSCDScore
    from siss_amd.vae import VAEDecoder, VAEEncoder
    dec = VAEDecoder(device=dev)
    dec.load_state_dict({k: 0.02 * torch.randn(v) if len(v) > 1 else (torch.ones(v) if "norm" in k and k.endswith(".weight")
                                                                        else torch.zeros(v))
                         for k, v in dec.diffusers_shapes().items()})
    enc = VAEEncoder(device=dev)
    torch.manual_seed(0)
    enc.load_state_dict(OracleVAEEncoder(VAEConfig.sd_v1()).state_dict())
    unet = UNet2DConditionModel(UNet2DConditionConfig.sd15(), device=dev, compute_dtype=torch.bfloat16)
    unet.engine.init_random(seed=0)
    pipe = SDSampler(unet, vae=dec, vae_encoder=enc)
    g = torch.Generator().manual_seed(0)
    text, neg = torch.randn(1, 77, 768, generator=g).to(dev), torch.randn(1, 77, 768, generator=g).to(dev)
    img = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    gen = torch.Generator(device=dev).manual_seed(42)
    score = SSCDScore(SSCDModel().to(dev), "", os.devnull)
    score._ref = torch.nn.functional.normalize(torch.randn(512, generator=g), dim=0).to(dev)
    held = {}

    def run():
        held["img"], _ = pipe.denoise_injection(img, text, strength=0.5, negative_prompt_embeds=neg, num_inference_steps=50,
                                                guidance_scale=7.5, num_images_per_prompt=4, generator=gen, output_type="decoded")
    with pipe.holding_graphs():
        t = _median_s(run, reps)
    res["sd"] = {"n4_strength0.5_of_50_steps_s": round(t, 3),
                 "score_ms": round(_median_s(lambda: score.score_decoded(held["img"])[0].cpu(), reps) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-celeb", action="store_true")
    ap.add_argument("--skip-sd", action="store_true")
    a = ap.parse_args()
    from siss_amd import lib
    lib.load()
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_injection", "device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_gb_per_s": HBM_GBS,
           "weights": "random-init"}
    with torch.no_grad():
        if not a.skip_kernel:
            kernel(dev, res)
        if not a.skip_celeb:
            celeb(dev, res, a.reps)
        if not a.skip_sd:
            sd(dev, res, a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

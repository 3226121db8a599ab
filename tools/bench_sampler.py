#!/usr/bin/env python
"""Sampler / evaluation path throughput.  The reference's `log_metrics` runs, at `sampling_steps: 1`
(config/delete_celeb.yaml:97), ~301 UNet forwards per optimizer step: a 50-step DDPM sampling of `eval_batch_size` images
(evaluate.py:37-50, pipeline.num_inference_steps: 50) and the 251-step inject-then-denoise of the forget image
(evaluate.py:64-79, metrics.denoising_injections.timestep: 250; delete_celeb.py:376-436, :486-503).  Forward only, CelebA-HQ
256 x 256 architecture, random-init weights, synthetic inputs.

    python tools/bench_sampler.py [--batch 1 16] > profiles/rNN_sampler_celeb.json
    python tools/bench_sampler.py --sd [--sd-batch 1 4] [--sd-dtype bf16 f32]

One JSON line: per batch size, the two schedules timed end to end (captured forward replayed per denoising step vs eager launches),
images / s, UNet forwards / s, and the forward's fraction of the bf16 MFMA roof (1 x 498.35 GFLOP per sample and forward, SURVEY.md
§8d, against 2.5 PFLOP/s).

--sd: the SD v1.5 validation pipeline of delete_sd.py:170-340 instead (siss_amd/sd_sampler.py: DDIM, guidance 7.5, 512 x 512):
ms per denoising step (one replay of the captured UNet forward over the 2n batch + the fused guidance / DDIM launch) at each
--sd-batch, the fused siss_cfg_ddim_step launch alone (us), the VAE decode per 512 x 512 image (ms), and one reference-sized
validation (eval_batches 8 x eval_batch_size 1 images x 50 steps + decode, s).  Random-init weights, synthetic prompts."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from siss_amd.config import UNet2DConfig           # noqa: E402
from siss_amd.model import UNet2DModel             # noqa: E402
from siss_amd.sampler import Evaluator             # noqa: E402
from siss_amd.scheduler import DDPMScheduler       # noqa: E402

FWD_GFLOP_PER_SAMPLE = 498.35
PEAK_BF16_TFLOPS = 2500.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sd_main(a):
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    from siss_amd.scheduler import DDIMScheduler
    from siss_amd.sd_sampler import SDSampler, cfg_ddim_step, ddim_blocks
    from siss_amd.vae import VAEDecoder
    dev = torch.device("cuda:0")
    vae = VAEDecoder(device=dev)
    vae.load_state_dict({k: 0.02 * torch.randn(v) if len(v) > 1 else (torch.ones(v) if "norm" in k and k.endswith(".weight")
                                                                        else torch.zeros(v))
                         for k, v in vae.diffusers_shapes().items()})
    g = torch.Generator().manual_seed(0)
    out = {"metric": "SD v1.5 validation sampling (delete_sd.py:170-340): DDIM + CFG 7.5, 512 x 512", "data": "synthetic",
           "device": torch.cuda.get_device_name(0), "results": {}}
    # the fused guidance + DDIM launch alone: latents of one 512 x 512 image per sample
    sch = DDIMScheduler.from_pretrained(None)
    sch.set_timesteps(50)
    kern = {}
    for n in a.sd_batch:
        eps, x = torch.randn(2 * n, 4, 64, 64, device=dev), torch.randn(n, 4, 64, 64, device=dev)
        slab = torch.empty(2, n, ddim_blocks(n, 4 * 64 * 64), device=dev)
        co = sch.coeffs(501)
        for _ in range(10):
            cfg_ddim_step(eps, x, x, co, 7.5, 0.0, slab)
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(200):
            cfg_ddim_step(eps, x, x, co, 7.5, 0.0, slab)
        s1.record()
        torch.cuda.synchronize()
        kern[f"n{n}"] = round(s0.elapsed_time(s1) / 200 * 1e3, 2)
    out["results"]["cfg_ddim_step_us"] = kern
    z = torch.randn(1, 4, 64, 64, device=dev)
    vae.decode(z)
    out["results"]["decode_ms_per_512px_image"] = round(timed(lambda: [vae.decode(z) for _ in range(5)]) / 5 * 1e3, 2)
    for dt in a.sd_dtype:
        unet = UNet2DConditionModel(UNet2DConditionConfig.sd15(), device=dev,
                                    compute_dtype=torch.float32 if dt == "f32" else torch.bfloat16)
        unet.engine.init_random(seed=0)
        pipe = SDSampler(unet, vae=vae)
        neg = torch.randn(1, 77, 768, generator=g).to(dev)
        row = {}
        for n in a.sd_batch:
            text = torch.randn(n, 77, 768, generator=g).to(dev)
            with pipe.holding_graphs():
                run = lambda k: pipe(text, negative_prompt_embeds=neg.expand(n, -1, -1), num_inference_steps=k, output_type="latent")
                run(2)                                                  # the capture
                t10, t60 = timed(lambda: run(10)), timed(lambda: run(60))
            row[f"ms_per_denoising_step_n{n}"] = round((t60 - t10) / 50 * 1e3, 3)
        text = torch.randn(1, 77, 768, generator=g).to(dev)
        gen = torch.Generator(device=dev).manual_seed(42)

        def validation():
            with pipe.holding_graphs():
                for _ in range(8):
                    pipe(text, negative_prompt_embeds=neg, num_inference_steps=50, generator=gen, output_type="np")
        row["validation_8x1_images_50_steps_s"] = round(timed(validation), 3)
        out["results"][dt] = row
        del pipe, unet
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16], help="eval_batch_size (config/delete_celeb.yaml:101 ships 1)")
    ap.add_argument("--sample-steps", type=int, default=50)
    ap.add_argument("--inject-t", type=int, default=250)
    ap.add_argument("--sd", action="store_true", help="the SD v1.5 validation pipeline (DDIM + CFG + VAE decode) instead")
    ap.add_argument("--sd-batch", type=int, nargs="+", default=[1, 4], help="images per pipeline call")
    ap.add_argument("--sd-dtype", nargs="+", default=["bf16", "f32"], choices=["bf16", "f32"],
                    help="UNet engine: bf16, or f32 (mixed_precision: null, config/delete_sd.yaml)")
    a = ap.parse_args()
    if a.sd:
        return sd_main(a)
    dev = torch.device("cuda:0")
    unet = UNet2DModel(UNet2DConfig.celebahq256(), device=dev)
    unet.engine.init_random(seed=0)
    sch = DDPMScheduler()
    rows = []
    for B in a.batch:
        x = torch.randn(B, 3, 256, 256, device=dev)
        row = {"eval_batch_size": B}
        for graph in (True, False):
            ev = Evaluator(use_graph=graph)
            ev.load_model(unet, sch)
            ev.denoise_images(x, 2)                       # warm-up (and the capture)
            dt_s = timed(lambda: ev.sample_images(B, num_inference_steps=a.sample_steps))
            dt_d = timed(lambda: ev.denoise_images(x, a.inject_t))
            nd = a.inject_t + 1
            fps = (a.sample_steps + nd) * B / (dt_s + dt_d)                      # sample-forwards per second over both schedules
            row["hipgraph" if graph else "eager"] = {
                "sample_%d_steps_s" % a.sample_steps: round(dt_s, 4), "sample_images_per_s": round(B / dt_s, 3),
                "inject_denoise_%d_steps_s" % nd: round(dt_d, 4), "denoised_images_per_s": round(B / dt_d, 4),
                "ms_per_denoising_step": round(dt_d / nd * 1e3, 3), "unet_forwards_per_s": round(fps, 1),
                "forward_mfma_frac": round(fps * FWD_GFLOP_PER_SAMPLE / 1e3 / PEAK_BF16_TFLOPS, 4)}
        row["graph_vs_eager"] = round(row["eager"]["ms_per_denoising_step"] / row["hipgraph"]["ms_per_denoising_step"], 3)
        rows.append(row)
    print(json.dumps({"metric": "sampler / eval path, CelebA-HQ-256 DDPM UNet forward-only (evaluate.py:37-79)", "dtype": "bf16",
                      "data": "synthetic", "device": torch.cuda.get_device_name(0),
                      "forward_gflop_per_sample": FWD_GFLOP_PER_SAMPLE, "peak_tflops": PEAK_BF16_TFLOPS, "results": rows}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The opt-in DPM-Solver++ (2M) sampler (pipeline.sampler) beside the samplers it can replace, on the GPU.

    python tools/bench_dpm_sampler.py [--steps-old 50] [--steps-new 20] > profiles/dpm_sampler.json

(a) kernel: siss_cfg_dpmpp_step (an order-2 step: every operand read) against siss_cfg_ddim_step at the SD shape (n = 16, 4 x 64 x 64,
    guidance 7.5) and the CelebA-HQ shape (n = 16, 3 x 256 x 256, no guidance): device events around replays of 200 captured
    launches (per launch: the kernel and the gap to the next one, without the host's launch cost), the two kernels alternated window
    by window, the median window per kernel; bytes per launch from the shapes (f32 reads + writes of
    every operand once: guided 4 + 2 against 3 + 1 per element, unguided 3 + 2 against 2 + 1) and the achieved GB/s they give.
    Both work out of place on fixed inputs.  The operands of these shapes (1-13 MB each) fit the 256 MB last-level cache: the
    rates are those of a launch in a sampling loop, not of a stream from HBM.
(b) one evaluation pass: CelebA-HQ 256 x 256, B = 16 -- Evaluator.sample_images at --steps-old ancestral DDPM steps against
    --steps-new solver steps -- and SD v1.5 at 512 x 512, n = 8 under guidance 7.5 -- SDSampler at --steps-old DDIM steps against
    --steps-new solver steps (latents out, no decode).  Random-init weights, the same captured forward on both sides of a pair;
    wall seconds (host clock, synchronised) and ms per network call.  What 20 steps do to image quality is not measured here.
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from siss_amd.scheduler import SD_V1_SCHEDULER, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler   # noqa: E402
from siss_amd.sd_sampler import SDSampler, cfg_ddim_step, cfg_dpmpp_step, ddim_blocks      # noqa: E402


def window_us(fn, launches):
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(launches):
        fn()
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / launches * 1e3


def graph_of(fn, launches):
    """`launches` launches captured back to back (the launchers only enqueue): a replay times the kernels without the host's ~12 us
    per Python launch, which at these sizes is longer than either kernel."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(launches):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def kernel_pair(dev, n, shape, guidance, launches=200, windows=7):
    chw = shape[0] * shape[1] * shape[2]
    cfg = guidance > 1.0
    eps = torch.randn((2 if cfg else 1) * n, *shape, device=dev)
    x, m1 = torch.randn(n, *shape, device=dev), torch.randn(n, *shape, device=dev)
    xo, mo = torch.empty_like(x), torch.empty_like(x)
    slab = torch.empty(2, n, ddim_blocks(n, chw), device=dev) if cfg else None
    ddim = DDIMScheduler.from_pretrained(None)
    ddim.set_timesteps(50)
    sol = DPMSolverMultistepScheduler.from_pretrained(None)
    sol.set_timesteps(20)
    cd, cs = ddim.coeffs(501), sol.coeffs(10)
    assert cs[4] != 0.0
    runs = {"siss_cfg_ddim_step": lambda: cfg_ddim_step(eps, x, xo, cd, guidance, 0.0, slab),
            "siss_cfg_dpmpp_step": lambda: cfg_dpmpp_step(eps, x, m1, xo, mo, cs, guidance, slab)}
    elems = {"siss_cfg_ddim_step": (3 if cfg else 2) + 1, "siss_cfg_dpmpp_step": (4 if cfg else 3) + 2}
    graphs = {k: graph_of(fn, launches) for k, fn in runs.items()}
    for g in graphs.values():
        window_us(g.replay, 2)                              # warm-up: code objects, clocks
    times = {k: [] for k in runs}
    for _ in range(windows):                                # alternated: both kernels see the same machine state
        for k, g in graphs.items():
            times[k].append(window_us(g.replay, 5) / launches)
    out = {"n": n, "shape": list(shape), "guidance": guidance}
    for k in runs:
        us = statistics.median(times[k])
        nbytes = elems[k] * 4 * n * chw
        out[k] = {"us": round(us, 2), "us_min_max": [round(min(times[k]), 2), round(max(times[k]), 2)], "bytes": nbytes,
                  "f32_per_element": elems[k], "GBps": round(nbytes / us / 1e3, 1)}
    out["bytes_ratio"] = round(out["siss_cfg_dpmpp_step"]["bytes"] / out["siss_cfg_ddim_step"]["bytes"], 3)
    out["time_ratio"] = round(out["siss_cfg_dpmpp_step"]["us"] / out["siss_cfg_ddim_step"]["us"], 3)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pass_row(old, new, k_old, k_new, what_old, what_new):
    t_old, t_new = min(timed(old) for _ in range(2)), min(timed(new) for _ in range(2))
    return {what_old: {"steps": k_old, "wall_s": round(t_old, 4), "ms_per_network_call": round(t_old / k_old * 1e3, 3)},
            what_new: {"steps": k_new, "wall_s": round(t_new, 4), "ms_per_network_call": round(t_new / k_new * 1e3, 3)},
            "wall_ratio_new_over_old": round(t_new / t_old, 3)}


def celeb_pass(dev, k_old, k_new, B=16):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.sampler import Evaluator
    unet = UNet2DModel(UNet2DConfig.celebahq256(), device=dev)
    unet.engine.init_random(seed=0)
    sch = DDPMScheduler()
    sol = DPMSolverMultistepScheduler.from_sampler_config(dict(name="dpmsolver++"), sch)
    ev = Evaluator()
    ev.load_model(unet, sch)
    ev.sample_images(B, num_inference_steps=2)              # the capture; both sides replay this graph
    ev.sample_images(B, num_inference_steps=2, sampler=sol)
    row = pass_row(lambda: ev.sample_images(B, num_inference_steps=k_old),
                   lambda: ev.sample_images(B, num_inference_steps=k_new, sampler=sol), k_old, k_new, "ddpm", sol.label)
    return {"shape": "CelebA-HQ 256 x 256, B = %d, bf16 engine, images to the host" % B, **row}


def sd_pass(dev, k_old, k_new, n=8):
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    unet = UNet2DConditionModel(UNet2DConditionConfig.sd15(), device=dev)
    unet.engine.init_random(seed=0)
    g = torch.Generator().manual_seed(0)
    text, neg = torch.randn(n, 77, 768, generator=g).to(dev), torch.randn(1, 77, 768, generator=g).to(dev).expand(n, -1, -1)
    lat = torch.randn(n, 4, 64, 64, generator=g).to(dev)
    sol = DPMSolverMultistepScheduler.from_sampler_config(dict(name="dpmsolver++"), SD_V1_SCHEDULER, timestep_spacing="leading",
                                                          steps_offset=SD_V1_SCHEDULER["steps_offset"])
    pipes = {"ddim": SDSampler(unet), sol.label: SDSampler(unet, scheduler=sol)}
    run = lambda p, k: p(text, negative_prompt_embeds=neg, num_inference_steps=k, latents=lat, output_type="latent")
    a, b = pipes["ddim"], pipes[sol.label]
    with a.holding_graphs(), b.holding_graphs():
        run(a, 2), run(b, 2)                                # the captures
        row = pass_row(lambda: run(a, k_old), lambda: run(b, k_new), k_old, k_new, "ddim", sol.label)
    return {"shape": "SD v1.5 512 x 512, n = %d, guidance 7.5, bf16 engine, latents out" % n, **row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-old", type=int, default=50, help="pipeline.num_inference_steps of the configs")
    ap.add_argument("--steps-new", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    out = {"metric": "DPM-Solver++ (2M) sampler against the DDPM / DDIM samplers", "data": "synthetic, random-init weights",
           "device": torch.cuda.get_device_name(0),
           "kernel": [kernel_pair(dev, 16, (4, 64, 64), 7.5), kernel_pair(dev, 16, (3, 256, 256), 1.0)]}
    if not a.kernels_only:
        out["evaluation_pass"] = [celeb_pass(dev, a.steps_old, a.steps_new), sd_pass(dev, a.steps_old, a.steps_new)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The pre-training update and step on one GPU: prints ONE JSON line.

    python tools/bench_train.py [--reps 20] [--rounds 5] [--steps 30] [--skip-update] [--skip-step]

  * update: the single-set update with the EMA (FlatAdamW.launch_single: siss_grad_norm_single + siss_clip_adamw_ema, 42 bytes per
    parameter with the bf16 shadow) against the composition the library offered before it (siss_grad_norms_scale mode 2 +
    siss_recombine_clip_adamw on (g, 0), then siss_ema_step: 54 bytes per parameter), at P = 113,673,219 (CelebA-HQ) and at the
    MNIST network's P.  Device events around --reps back-to-back updates, the two forms ALTERNATING for --rounds rounds in the
    same process; the median round of each, its spread, and the achieved GB/s beside the 8 TB/s HBM figure.
  * step: milliseconds per pre-training optimizer step (siss_amd/train.py TrainStepper with the EMA) at the shipped shape of
    config/train_tshirt_mnist.yaml -- 28 x 28, B = 128, GA = 1 -- on the f32 engine (mixed_precision: null, as shipped) and on the
    bf16 engine; device events around --steps steps after 5 warm-up steps.
Weights are random-init, data synthetic: the times do not depend on them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0
P_CELEB = 113_673_219
EMA_ARGS = dict(decay=0.9999, use_ema_warmup=True, inv_gamma=1.0, power=0.75)


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:2] or None
    except Exception:
        return None


def _timed(fn, reps):
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(reps):
        fn()
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / reps * 1e3          # us per call


class _Flat:
    """what EMAModel / FlatAdamW need of a model: one flat f32 parameter buffer"""

    def __init__(self, p):
        self.engine = type("E", (), {})()
        self.engine.ps = type("PS", (), {"flat": p, "specs": {}, "total": p.numel()})()


def update(dev, res, reps, rounds, sizes):
    from siss_amd import lib
    from siss_amd.ema import EMAModel
    from siss_amd.optim import FlatAdamW
    rows = {}
    for name, n in sizes.items():
        g = torch.randn(n, device=dev) * 1e-3
        zero = torch.zeros(n, device=dev)
        p = torch.randn(n, device=dev)
        opt = FlatAdamW(p, lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, shadow=torch.zeros(n, dtype=torch.bfloat16, device=dev))
        ema = EMAModel(_Flat(p), **EMA_ARGS)
        opt._train_block()

        def fused():
            opt.launch_single(g, ema=ema)

        def composed():
            lib.call("siss_grad_norms_scale", g, zero, n, 2, 1.0, opt.max_grad_norm, opt.betas[0], opt.betas[1], opt.partials, opt.scalars)
            lib.call("siss_recombine_clip_adamw", g, zero, opt.p, opt.m, opt.v, opt.shadow, None, n, opt.lr, opt.betas[0], opt.betas[1],
                     opt.eps, opt.wd, opt.scalars)
            lib.call("siss_ema_step", opt.p, ema.flat, n, opt.train_scalars)
        for fn in (fused, composed):
            _timed(fn, 3)
        t = {"fused": [], "composed": []}
        for _ in range(rounds):
            t["fused"].append(_timed(fused, reps))
            t["composed"].append(_timed(composed, reps))
        row = {"P": n}
        for k, per in (("fused", 42), ("composed", 54)):
            us = statistics.median(t[k])
            row[k] = {"us": round(us, 1), "min_us": round(min(t[k]), 1), "max_us": round(max(t[k]), 1), "bytes": per * n,
                      "gb_per_s": round(per * n / (us * 1e-6) / 1e9, 1), "hbm_frac": round(per * n / (us * 1e-6) / 1e9 / HBM_GBS, 4)}
        row["fused_over_composed"] = round(row["fused"]["us"] / row["composed"]["us"], 4)
        rows[name] = row
        del g, zero, p, opt, ema
        torch.cuda.empty_cache()
    res["update"] = rows


def _mnist(dev, dtype):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    unet = UNet2DModel(UNet2DConfig.mnist_tshirt(), device=dev, compute_dtype=dtype)
    unet.engine.init_random(seed=0)
    return unet


def step(dev, res, steps):
    from siss_amd.ema import EMAModel
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.train import TrainStepper
    rows = {}
    for name, dtype, mp in (("f32", torch.float32, None), ("bf16", torch.bfloat16, "bf16")):
        unet = _mnist(dev, dtype)
        ema = EMAModel(unet, model_cls=type(unet), model_config=unet.config, **EMA_ARGS)
        st = TrainStepper(unet.engine, DDPMScheduler().alphas_cumprod, lr=1e-4, betas=(0.95, 0.999), weight_decay=1e-6, ema=ema,
                          mixed_precision=mp)
        g = torch.Generator(device=dev).manual_seed(0)
        x0 = torch.rand(128, 1, 28, 28, device=dev, generator=g) * 2 - 1

        def one():
            st.step(x0, torch.randn(x0.shape, device=dev, generator=g), torch.randint(0, 1000, (128,), device=dev, generator=g))
        _timed(one, 5)
        rows[name] = {"ms_per_step": round(_timed(one, steps) / 1e3, 3), "B": 128, "P": unet.engine.ps.total}
        del st, ema, unet
        torch.cuda.empty_cache()
    res["step"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-update", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    from siss_amd import lib
    lib.load()
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_train", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "hbm_gb_per_s": HBM_GBS}
    if not a.skip_update:
        p_mnist = _mnist(dev, torch.bfloat16).engine.ps.total
        torch.cuda.empty_cache()
        update(dev, res, a.reps, a.rounds, {"celebahq256": P_CELEB, "mnist": p_mnist})
    if not a.skip_step:
        step(dev, res, a.steps)
    clock = _clock()                                     # read right after the timed work
    res["sclk"] = clock if clock else "not recorded"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

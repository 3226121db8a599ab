#!/usr/bin/env python
"""The Fisher-anchor fold (csrc/ewc.hip) at the flat-buffer sizes of the two flagship UNets: writes ONE JSON (profiles/ewc.json).

    python tools/bench_ewc.py [--reps 40] [--rounds 5] [--only celebahq256|sd15] [--out profiles/ewc.json]

Per buffer size (the aligned flat parameter buffers of `google/ddpm-celebahq-256` and of the SD v1.5 UNet, computed from the
configurations), in ONE process and on the SAME buffers:

  * norms / norms_ewc      pass 1 alone: siss_grad_norms_scale against siss_grad_norms_scale_ewc;
  * pair / pair_ewc        pass 1 + siss_recombine_clip_adamw (with the bf16 shadow), without and with the fold;
  * fisher_accumulate      one siss_fisher_accumulate launch (the per-micro-batch cost of the Fisher estimate beyond its backward pass).

Every leg is timed over --reps launches between two device events, the legs interleaved, --rounds rounds, after a warm-up of every
leg: ms per call of every round are reported, and a leg's spread over the rounds is the run-to-run spread its differences are to be
read against.  The byte model (from the shapes; per float): pass 1 reads 8 B, with the fold 20 B read + 4 B written; pass 2 reads
20 B and writes 14 B (p, m, v, shadow); the accumulation reads 8 B and writes 4 B.  Achieved GB/s = model bytes over the median time
per call -- an end-to-end rate of the launch sequence (kernel gaps included), not a kernel's share of peak.  No threshold is attached
to any figure.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HP = dict(lr=1e-4, beta1=0.95, beta2=0.999, eps=1e-8, wd=1e-2)
BYTES_PER_FLOAT = dict(norms=8, norms_ewc=24, pair=42, pair_ewc=58, fisher_accumulate=12)


def buffer_floats():
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.unet import ALIGN, UNetEngine
    from siss_amd.unet_cond import UNetCondEngine
    out = {}
    for name, cls, cfg in (("celebahq256", UNetEngine, UNet2DConfig.celebahq256()), ("sd15", UNetCondEngine, UNet2DConditionConfig.sd15())):
        specs = cls.param_specs(cfg)
        out[name] = dict(floats=sum(-(-int(sp.numel) // ALIGN) * ALIGN for sp in specs.values()),
                         real_params=sum(int(sp.numel) for sp in specs.values()), tensors=len(specs))
    return out


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def spread(xs):
    return dict(ms=[round(x, 4) for x in xs], min=round(min(xs), 4), max=round(max(xs), 4), median=round(sorted(xs)[len(xs) // 2], 4))


def byte_model():
    return dict(per_float=BYTES_PER_FLOAT, note="pass 1: 8 B read (g_x, g_a); with the fold 20 B read (+ p, pstar, F) + 4 B written (g_x'); "
                "pass 2: 20 B read + 14 B written (p, m, v, bf16 shadow); fisher_accumulate: 8 B read + 4 B written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ewc.json"))
    ap.add_argument("--only", default=None, choices=[None, "celebahq256", "sd15"])
    a = ap.parse_args()
    sizes = buffer_floats()
    assert torch.cuda.is_available(), "bench_ewc.py needs a GPU (there is no CPU timing: the byte model alone says nothing about speed)"
    from siss_amd import lib
    dev = torch.device("cuda", 0)
    result = dict(reps=a.reps, rounds=a.rounds, hyper=HP, device=torch.cuda.get_device_name(0), byte_model=byte_model(), buffers={},
                  not_measured=[])
    for name, info in sizes.items():
        if a.only and name != a.only:
            result["not_measured"].append(f"{name}: left out by --only")
            continue
        n = info["floats"]
        gen = torch.Generator(device=dev).manual_seed(0)
        gx = 1e-2 * torch.randn(n, device=dev, generator=gen)
        ga = 2e-2 * torch.randn(n, device=dev, generator=gen)
        p = torch.randn(n, device=dev, generator=gen)
        pstar = p + 1e-3 * torch.randn(n, device=dev, generator=gen)
        F = torch.randn(n, device=dev, generator=gen).square_()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        shadow = p.to(torch.bfloat16)
        partials = torch.zeros(lib.query("siss_opt_partials_words"), dtype=torch.float64, device=dev)
        ewc_partials = torch.zeros(lib.query("siss_ewc_partials_words"), dtype=torch.float64, device=dev)
        scalars = torch.zeros(lib.query("siss_opt_scalars_words"), dtype=torch.float32, device=dev)

        def norms():
            lib.call("siss_grad_norms_scale", gx, ga, n, 0, 5.0, 1.0, HP["beta1"], HP["beta2"], partials, scalars)

        def norms_ewc():
            lib.call("siss_grad_norms_scale_ewc", gx, ga, p, pstar, F, n, 1.0, 0, 5.0, 1.0, HP["beta1"], HP["beta2"], partials,
                     ewc_partials, scalars)

        def pass2():
            lib.call("siss_recombine_clip_adamw", gx, ga, p, m, v, shadow, None, n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                     HP["wd"], scalars)

        legs = {"norms": norms, "norms_ewc": norms_ewc, "pair": lambda: (norms(), pass2()), "pair_ewc": lambda: (norms_ewc(), pass2()),
                "fisher_accumulate": lambda: lib.call("siss_fisher_accumulate", gx, F, n, 0.125)}
        for fn in legs.values():                           # warm every leg
            fn()
        torch.cuda.synchronize()
        times = {leg: [] for leg in legs}
        for _ in range(a.rounds):
            for leg, fn in legs.items():                   # interleaved: one timed window per leg per round
                times[leg].append(timed(fn, a.reps))
        out = dict(info)
        for leg, ts in times.items():
            s = spread(ts)
            nbytes = BYTES_PER_FLOAT[leg] * n
            out[leg] = dict(s, spread_ms=round(s["max"] - s["min"], 4), model_bytes=nbytes,
                            achieved_gb_per_s=round(nbytes / (s["median"] * 1e-3) / 1e9, 1))
        out["norms_ewc_minus_norms_ms"] = round(out["norms_ewc"]["median"] - out["norms"]["median"], 4)
        out["pair_ewc_minus_pair_ms"] = round(out["pair_ewc"]["median"] - out["pair"]["median"], 4)
        out["added_model_bytes"] = (BYTES_PER_FLOAT["norms_ewc"] - BYTES_PER_FLOAT["norms"]) * n
        result["buffers"][name] = out
        del gx, ga, p, pstar, F, m, v, shadow
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

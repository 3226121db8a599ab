#!/usr/bin/env python
"""The attribution projection (csrc/attribution.hip) at the flat-buffer sizes of the two flagship UNets: writes ONE JSON
(profiles/attribution.json).

    python tools/bench_attribution.py [--reps 5] [--rounds 3] [--only celebahq256|sd15] [--passes 3] [--out profiles/attribution.json]

Per buffer size (the aligned flat parameter buffers of `google/ddpm-celebahq-256` and of the SD v1.5 UNet, computed from the
configurations), on ONE buffer of seeded normals: siss_jl_project at k = 512 / 2048 / 4096, timed over --reps launches between two
device events, --rounds rounds after a warm-up; sign-adds per second = n * k over the median time, and its share of the 157.3 TF f32
vector peak counted as 78.65e12 adds per second (an add is half an FMA).  Beside it (--passes N > 0): the forward + backward of ONE
row's batch of 8 noisings on a random-init engine of that UNet (GradientFeatures._fill inside quiet_backward), host wall time around
a device synchronisation, per pass.  No threshold is attached to any figure.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_VECTOR_FLOPS = 157.3e12
KS = (512, 2048, 4096)
NOISINGS = 8


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


def backward_of_a_row(name, cls, cfg, passes, dev):
    """ms per forward + backward of one row's batch (8 noisings of one image) on a random-init engine."""
    from siss_amd.attribution import GradientFeatures, Projector
    from siss_amd.step import SISSStepper
    from siss_amd.variants import quiet_backward
    eng = cls(cfg, dev)
    eng.init_random(seed=42)
    g = torch.Generator(device=dev).manual_seed(1)
    if name == "sd15":
        ac = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2, 0)
        ehs = torch.randn(1, 77, cfg.cross_attention_dim, generator=g, device=dev).to(torch.bfloat16)
        cond, scale = (lambda B: {"encoder_hidden_states": ehs.repeat(B, 1, 1)}), 0.18215
    else:
        ac = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32), 0)
        cond, scale = None, 1.0
    st = SISSStepper(eng, ac, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=500.0, lambd=0.5,
                     train_batch_size=NOISINGS, mixed_precision="bf16")
    feats = GradientFeatures(st, Projector(int(eng.ps.total), 2048, device=dev), timesteps=NOISINGS, output="square", conditioning=cond)
    x = scale * torch.randn(cfg.in_channels, cfg.sample_size, cfg.sample_size, generator=g, device=dev)
    out = torch.zeros(2048, device=dev)
    feats.row(x, 0, out)                                        # warm-up: allocations, fill plans, the workspace
    torch.cuda.synchronize()
    with quiet_backward(st, "bench_attribution"):
        t0 = time.perf_counter()
        for i in range(passes):
            feats._fill(x, i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / passes
    t0 = time.perf_counter()
    for i in range(passes):
        feats.row(x, i, out)
    torch.cuda.synchronize()
    row_ms = (time.perf_counter() - t0) * 1e3 / passes
    res = dict(passes=passes, noisings=NOISINGS, forward_backward_ms=round(ms, 3), whole_row_ms_k2048=round(row_ms, 3))
    del st, eng, feats
    torch.cuda.empty_cache()
    return res


def main():
    from tools.bench_ssd import buffer_floats, engines
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3, help="timed forward + backward passes of one row's batch (0: leave it out)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribution.json"))
    ap.add_argument("--only", default=None, choices=[None, "celebahq256", "sd15"])
    a = ap.parse_args()
    sizes = buffer_floats()
    assert torch.cuda.is_available(), "bench_attribution.py needs a GPU (there is no CPU timing)"
    from siss_amd import lib
    dev = torch.device("cuda", 0)
    result = dict(reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), chunk=int(lib.query("siss_jl_chunk")),
                  f32_vector_flops=F32_VECTOR_FLOPS, adds_per_s_at_peak=F32_VECTOR_FLOPS / 2,
                  work_model="n * k sign-adds per projection; an add is counted as half an FMA of the 157.3 TF f32 vector peak",
                  buffers={}, not_measured=[])
    for name, cls, cfg in engines():
        if a.only and name != a.only:
            result["not_measured"].append(f"{name}: left out by --only")
            continue
        info = sizes[name]
        n = info["floats"]
        g = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 1e-3
        out = dict(info, k={})
        for k in KS:
            ws = torch.empty(int(lib.query("siss_jl_ws_bytes", n, k)) // 8, dtype=torch.float64, device=dev)
            row = torch.zeros(k, device=dev)
            fn = lambda: lib.call("siss_jl_project", g, n, None, 0, k, 0, ws, ws.numel() * 8, row)
            fn()
            torch.cuda.synchronize()
            first = row.clone()
            s = spread([timed(fn, a.reps) for _ in range(a.rounds)])
            rate = n * k / (s["median"] * 1e-3)
            out["k"][str(k)] = dict(s, workspace_bytes=ws.numel() * 8, sign_adds=n * k, sign_adds_per_s=round(rate / 1e12, 3),
                                    unit="1e12 / s", share_of_f32_add_peak=round(rate / (F32_VECTOR_FLOPS / 2), 3),
                                    repeatable=bool(torch.equal(first, row)),
                                    norm_ratio=round(float(row.double().square().sum() / g.double().square().sum()), 4))
            del ws
        del g
        torch.cuda.empty_cache()
        if a.passes > 0:
            out["row_batch"] = backward_of_a_row(name, cls, cfg, a.passes, dev)
            out["projection_k2048_over_forward_backward"] = round(out["k"]["2048"]["median"] / out["row_batch"]["forward_backward_ms"], 3)
        else:
            result["not_measured"].append(f"{name}: the forward + backward of a row's batch (--passes 0)")
        result["buffers"][name] = out
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

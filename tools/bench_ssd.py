#!/usr/bin/env python
"""Selective Synaptic Dampening (csrc/ssd.hip) at the flat-buffer sizes of the two flagship UNets: writes ONE JSON (profiles/ssd.json).

    python tools/bench_ssd.py [--reps 40] [--rounds 5] [--only celebahq256|sd15] [--passes 4] [--out profiles/ssd.json]

Per buffer size (the aligned flat parameter buffers of `google/ddpm-celebahq-256` and of the SD v1.5 UNet, computed from the
configurations), in ONE process and on the SAME buffers:

  * ratio / ratio_torch          siss_ssd_ratio against torch.where(ff == 0, 0, ff / fk) into a preallocated output;
  * dampen_dry / dampen          siss_ssd_dampen with apply = 0 and apply = 1 (about 1 % of the weights selected);
  * dampen_torch                 the same arithmetic in eager torch: the selection, beta, the in-place update under the mask and the
                                 seven statistics in f64 -- what the pass would cost without the kernel.

Every leg is timed over --reps launches between two device events, the legs interleaved, --rounds rounds, after a warm-up of every
leg.  The byte model (per float): the ratio reads 8 B and writes 4 B; the dampening reads 8 B and writes 4 B only in granules that
hold a selected weight (counted as 8 B read + 4 B x the fraction of such granules).  Achieved GB/s = model bytes over the median
time per call; hbm_share = that over the 8 TB/s the MI355X is specified with -- an end-to-end rate of the launch sequence (the
one-block fold of the statistics included), not a kernel's share of what a copy achieves.

--passes N > 0: one importance estimate on each UNet at random-init weights, micro-batch 1 (the per-sample Fisher): N backward passes
through variants.fisher_of_batches, host wall time around a device synchronisation, per pass.  No threshold is attached to any figure.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12
LAMBDA = 1.0


def engines():
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.unet import UNetEngine
    from siss_amd.unet_cond import UNetCondEngine
    return (("celebahq256", UNetEngine, UNet2DConfig.celebahq256()), ("sd15", UNetCondEngine, UNet2DConditionConfig.sd15()))


def buffer_floats():
    from siss_amd.unet import ALIGN
    out = {}
    for name, cls, cfg in engines():
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


def torch_dampen(p, r, thr, lam, out):
    """The arithmetic of siss_ssd_dampen (strict = 0, apply = 1) in eager torch; the statistics go to `out` (8 f64)."""
    sel = r >= thr
    beta = torch.where(r > lam, lam / r, torch.ones_like(r))
    q = torch.where(sel, p * beta, p)
    pd, qd = p.double(), q.double()
    out[0] = sel.sum()
    out[1] = (sel & (beta < 1)).sum()
    out[2] = (sel & (beta == 0)).sum()
    out[3] = torch.where(sel, beta, torch.zeros_like(beta)).double().sum()
    out[4] = (qd - pd).square().sum()
    out[5] = torch.where(sel, pd * pd, torch.zeros_like(pd)).sum()
    out[6] = (pd * pd).sum()
    p.copy_(q)


def importance_pass(name, cls, cfg, passes, dev):
    """ms per backward pass of one importance estimate (micro-batch 1) on a random-init engine."""
    from siss_amd.step import SISSStepper
    from siss_amd.variants import fisher_of_batches
    eng = cls(cfg, dev)
    eng.init_random(seed=42)
    sd = name == "sd15"
    g = torch.Generator(device=dev).manual_seed(1)
    if sd:
        ac = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2, 0)
        cond = {"encoder_hidden_states": torch.randn(1, 77, cfg.cross_attention_dim, generator=g, device=dev).to(torch.bfloat16)}
        scale = 0.18215
    else:
        ac = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32), 0)
        cond, scale = None, 1.0
    st = SISSStepper(eng, ac, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=500.0, lambd=0.5,
                     train_batch_size=1, mixed_precision="bf16")
    x = scale * torch.randn(1, cfg.in_channels, cfg.sample_size, cfg.sample_size, generator=g, device=dev)

    def batches():
        while True:
            yield x
    fisher_of_batches(st, batches(), 1, "bench_ssd", conditioning=cond, generator=g)          # warm-up: allocations, fill plans
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    F = fisher_of_batches(st, batches(), passes, "bench_ssd", conditioning=cond, generator=g)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / passes
    out = dict(passes=passes, micro_batch=1, ms_per_pass=round(ms, 3), nonzero_fraction=round(float((F != 0).float().mean()), 4))
    del st, eng, F
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=4, help="backward passes of the timed importance estimate (0: leave it out)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssd.json"))
    ap.add_argument("--only", default=None, choices=[None, "celebahq256", "sd15"])
    a = ap.parse_args()
    sizes = buffer_floats()
    assert torch.cuda.is_available(), "bench_ssd.py needs a GPU (there is no CPU timing: the byte model alone says nothing about speed)"
    from siss_amd import lib
    from siss_amd.saliency import bits_to_float, select_magnitude
    dev = torch.device("cuda", 0)
    result = dict(reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, **{"lambda": LAMBDA},
                  byte_model="ratio: 8 B read + 4 B written per float; dampen: 8 B read per float + 16 B written per granule that holds a "
                             "selected weight; the torch legs are charged the same bytes (what they move is more)", buffers={},
                  not_measured=[])
    for name, cls, cfg in engines():
        if a.only and name != a.only:
            result["not_measured"].append(f"{name}: left out by --only")
            continue
        info = sizes[name]
        n = info["floats"]
        gen = torch.Generator(device=dev).manual_seed(0)
        fk = torch.randn(n, device=dev, generator=gen).square_() * 1e-4
        ff = torch.randn(n, device=dev, generator=gen).square_() * 1e-4
        p0 = torch.randn(n, device=dev, generator=gen)
        p, r, r2 = p0.clone(), torch.empty_like(fk), torch.empty_like(fk)
        partials = torch.empty(lib.query("siss_ssd_partials_words"), dtype=torch.float64, device=dev)
        stats, tstats = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(8, dtype=torch.float64, device=dev)
        lib.call("siss_ssd_ratio", fk, ff, r, n)
        thr = bits_to_float(select_magnitude(r, max(1, n // 100))["threshold_bits"])
        granules = float((r.view(-1, 4) >= thr).any(dim=1).float().mean()) if n % 4 == 0 else None

        def torch_ratio():
            torch.where(ff == 0, torch.zeros_like(ff), ff / fk, out=r2)

        legs = {"ratio": lambda: lib.call("siss_ssd_ratio", fk, ff, r, n), "ratio_torch": torch_ratio,
                "dampen_dry": lambda: lib.call("siss_ssd_dampen", p, r, n, thr, 0, LAMBDA, 0, partials, stats),
                "dampen": lambda: lib.call("siss_ssd_dampen", p, r, n, thr, 0, LAMBDA, 1, partials, stats),
                "dampen_torch": lambda: torch_dampen(p, r, thr, LAMBDA, tstats)}
        for fn in legs.values():                           # warm every leg
            fn()
        torch.cuda.synchronize()
        same_ratio = bool(torch.equal(r, r2))
        p.copy_(p0)
        legs["dampen"]()
        mine, got = p.clone(), stats.cpu().tolist()
        p.copy_(p0)
        legs["dampen_torch"]()
        same_dampen = bool(torch.equal(mine, p)) and got[:3] == tstats.cpu().tolist()[:3]
        times = {leg: [] for leg in legs}
        for _ in range(a.rounds):
            for leg, fn in legs.items():                   # interleaved: one timed window per leg per round
                times[leg].append(timed(fn, a.reps))
        written = 4 * n * (granules if granules is not None else 0.04)
        model = {"ratio": 12 * n, "ratio_torch": 12 * n, "dampen_dry": 8 * n, "dampen": 8 * n + written, "dampen_torch": 8 * n + written}
        out = dict(info, threshold=thr, selected=int(got[0]), granules_written_fraction=granules,
                   eager_torch_gives_the_same_bits=dict(ratio=same_ratio, dampen=same_dampen))
        for leg, ts in times.items():
            s = spread(ts)
            rate = model[leg] / (s["median"] * 1e-3)
            out[leg] = dict(s, spread_ms=round(s["max"] - s["min"], 4), model_bytes=int(model[leg]),
                            achieved_gb_per_s=round(rate / 1e9, 1), hbm_share=round(rate / HBM_BYTES_PER_S, 3))
        out["ratio_torch_over_ratio"] = round(out["ratio_torch"]["median"] / out["ratio"]["median"], 2)
        out["dampen_torch_over_dampen"] = round(out["dampen_torch"]["median"] / out["dampen"]["median"], 2)
        del fk, ff, p0, p, r, r2, mine
        torch.cuda.empty_cache()
        if a.passes > 0:
            out["importance_estimate"] = importance_pass(name, cls, cfg, a.passes, dev)
        else:
            result["not_measured"].append(f"{name}: the importance estimate (--passes 0)")
        result["buffers"][name] = out
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

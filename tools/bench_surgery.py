#!/usr/bin/env python
"""The gradient-surgery update pair (csrc/surgery.hip) against the plain pair it replaces, on the real parameter tables of the two
flagship UNets: writes ONE JSON (profiles/surgery.json).

    python tools/bench_surgery.py [--window-ms 300] [--rounds 5] [--only celebahq256|sd15] [--chunks 4096,8192,16384,32768,65536]
                                  [--out profiles/surgery.json]

Per buffer (the aligned flat parameter buffers of `google/ddpm-celebahq-256` and of the SD v1.5 UNet with their REAL spec tables: the
group table of `granularity: tensor` is the tensors' own), in ONE process and on the SAME buffers, random gradients (independent draws:
about half of the tensors conflict), mode mutual:

  * pair                 siss_grad_norms_scale + siss_recombine_clip_adamw (with the bf16 shadow): the yardstick;
  * pair_tensor / pair_global   siss_grad_norms_scale_surgery + siss_recombine_clip_adamw_surgery for both granularities;
  * pass1*, pass2*       the halves of each pair on their own (where a difference sits);
  * chunk sweep          pair_tensor at every chunk length of --chunks (siss_surgery_test_config), beside `pair` in the same rounds.

Every leg is timed between two device events over as many launches as fill --window-ms (counted once, after the warm-up), the legs
interleaved, --rounds rounds: ms per call of every round are reported, and a leg's spread over the rounds is the run-to-run spread its
differences are to be read against.  The byte model (from the shapes; per float): pass 1 reads 8 B, pass 2 reads 20 B and writes 14 B
(p, m, v, shadow); the surgery adds one 24-byte row per job, the plan and the tables.  Achieved GB/s = model bytes over the median
time per call -- an end-to-end rate of the launch sequence (kernel gaps included), not a kernel's share of peak.  No threshold is
attached to any figure.
"""
import argparse
import json
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HP = dict(lr=1e-4, beta1=0.95, beta2=0.999, eps=1e-8, wd=1e-2)
BYTES_PER_FLOAT = dict(pass1=8, pass2=34, pair=42)


def spec_tables():
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.unet import ALIGN, UNetEngine
    from siss_amd.unet_cond import UNetCondEngine
    out = {}
    for name, cls, cfg in (("celebahq256", UNetEngine, UNet2DConfig.celebahq256()), ("sd15", UNetCondEngine, UNet2DConditionConfig.sd15())):
        specs, off = {}, 0
        for key, sp in cls.param_specs(cfg).items():           # (buffer order: one tensor after another, each start aligned)
            specs[key] = types.SimpleNamespace(name=key, off=off, numel=int(sp.numel))
            off += -(-int(sp.numel) // ALIGN) * ALIGN
        out[name] = (specs, off)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surgery.json"))
    ap.add_argument("--only", default=None, choices=[None, "celebahq256", "sd15"])
    ap.add_argument("--chunks", default="4096,8192,16384,32768,65536")
    a = ap.parse_args()
    tables = spec_tables()
    assert torch.cuda.is_available(), "bench_surgery.py needs a GPU (there is no CPU timing: the byte model alone says nothing about speed)"
    from siss_amd import lib
    from siss_amd.surgery import Surgery
    dev = torch.device("cuda", 0)
    default_chunk = int(lib.query("siss_surgery_chunk"))
    chunks = [int(c) for c in a.chunks.split(",") if c]
    result = dict(window_ms=a.window_ms, rounds=a.rounds, hyper=HP, device=torch.cuda.get_device_name(0), mode="mutual",
                  default_chunk=default_chunk, buffers={}, not_measured=[],
                  byte_model=dict(per_float=BYTES_PER_FLOAT, note="pass 1: 8 B read (g_x, g_a); pass 2: 20 B read + 14 B written (p, m, v, "
                                  "bf16 shadow); the surgery pair adds 24 B per job row (written, then read by the group fold), 16 B "
                                  "per job of plan, and per group 24 B of sums, 8 B of coefficients and 16 B of plan"))
    for name, (specs, n) in tables.items():
        if a.only and name != a.only:
            result["not_measured"].append(f"{name}: left out by --only")
            continue
        gen = torch.Generator(device=dev).manual_seed(0)
        gx = 1e-2 * torch.randn(n, device=dev, generator=gen)
        ga = 2e-2 * torch.randn(n, device=dev, generator=gen)
        p = torch.randn(n, device=dev, generator=gen)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        shadow = p.to(torch.bfloat16)
        partials = torch.zeros(lib.query("siss_opt_partials_words"), dtype=torch.float64, device=dev)
        scalars = torch.zeros(lib.query("siss_opt_scalars_words"), dtype=torch.float32, device=dev)
        eng = types.SimpleNamespace(ps=types.SimpleNamespace(specs=specs, total=n, flat=p), device=dev)

        def pass1():
            lib.call("siss_grad_norms_scale", gx, ga, n, 0, 5.0, 1.0, HP["beta1"], HP["beta2"], partials, scalars)

        def pass2():
            lib.call("siss_recombine_clip_adamw", gx, ga, p, m, v, shadow, None, n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                     HP["wd"], scalars)

        def halves(sg):
            def one():
                lib.call("siss_grad_norms_scale_surgery", gx, ga, n, sg.group_offsets, sg.groups, sg.plan, sg.jobs, sg.smode, 0, 5.0, 1.0,
                         HP["beta1"], HP["beta2"], sg.partials, sg.group_sums, sg.coef, scalars)

            def two():
                lib.call("siss_recombine_clip_adamw_surgery", gx, ga, p, m, v, shadow, None, n, sg.group_offsets, sg.groups, sg.plan,
                         sg.jobs, sg.coef, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], scalars)
            return one, two

        def measure(legs):
            """{leg: ms per call of every round}: warm every leg, size its window once, then the legs interleaved"""
            reps = {}
            for leg, fn in legs.items():
                fn()
                torch.cuda.synchronize()
                reps[leg] = max(3, min(2000, math.ceil(a.window_ms / max(timed(fn, 3), 1e-3))))
            times = {leg: [] for leg in legs}
            for _ in range(a.rounds):
                for leg, fn in legs.items():
                    times[leg].append(timed(fn, reps[leg]))
            return times, reps

        def report(ts, reps, leg_bytes):
            s = spread(ts)
            return dict(s, reps=reps, spread_ms=round(s["max"] - s["min"], 4), model_bytes=leg_bytes,
                        achieved_gb_per_s=round(leg_bytes / (s["median"] * 1e-3) / 1e9, 1))

        out = dict(floats=n, tensors=len(specs), real_params=sum(sp.numel for sp in specs.values()))
        sgs = {g: Surgery(eng, "mutual", g) for g in ("tensor", "global")}
        legs = {"pass1": pass1, "pass2": pass2, "pair": lambda: (pass1(), pass2())}
        extra = {}
        for g, sg in sgs.items():
            one, two = halves(sg)
            legs.update({f"pass1_{g}": one, f"pass2_{g}": two, f"pair_{g}": (lambda one=one, two=two: (one(), two()))})
            extra[g] = 40 * sg.jobs + 48 * sg.groups
            out[f"jobs_{g}"], out[f"groups_{g}"] = sg.jobs, sg.groups
        times, reps = measure(legs)
        for leg, ts in times.items():
            kind, _, g = leg.partition("_")
            out[leg] = report(ts, reps[leg], BYTES_PER_FLOAT[kind] * n + (extra[g] if g else 0))
        one, _ = halves(sgs["tensor"])
        one()
        torch.cuda.synchronize()
        out["conflicts_tensor"] = int(scalars[12].item())
        for g in sgs:
            out[f"pair_{g}_minus_pair_ms"] = round(out[f"pair_{g}"]["median"] - out["pair"]["median"], 4)
            out[f"pair_{g}_over_pair"] = round(out[f"pair_{g}"]["median"] / out["pair"]["median"], 4)
        # the chunk lengths tried: pair_tensor at each, beside the plain pair in the same rounds
        sweep = {}
        for c in chunks:
            assert lib.query("siss_surgery_test_config", c, 0) == 0
            sg = Surgery(eng, "mutual", "tensor")
            one, two = halves(sg)
            times, reps = measure({"pair": lambda: (pass1(), pass2()), "pair_tensor": (lambda one=one, two=two: (one(), two()))})
            sweep[str(c)] = dict(jobs=sg.jobs, pair=report(times["pair"], reps["pair"], BYTES_PER_FLOAT["pair"] * n),
                                 pair_tensor=report(times["pair_tensor"], reps["pair_tensor"],
                                                    BYTES_PER_FLOAT["pair"] * n + 40 * sg.jobs + 48 * sg.groups))
            del sg
        assert lib.query("siss_surgery_test_config", 0, 0) == 0
        out["chunk_sweep"] = sweep
        result["buffers"][name] = out
        del gx, ga, p, m, v, shadow, sgs, eng
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

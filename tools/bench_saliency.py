#!/usr/bin/env python
"""The saliency kernels (csrc/saliency.hip) at the flat-buffer sizes of the two flagship UNets: writes ONE JSON (profiles/saliency.json).

    python tools/bench_saliency.py [--parent-lib tools/ab/libsiss_base.so] [--reps 10] [--rounds 3] [--out profiles/saliency.json]

Per buffer size (the aligned flat parameter buffers of `google/ddpm-celebahq-256` and of the SD v1.5 UNet, computed from the
configurations):

  * select_ms, mask_ms     siss_absf_select at k = half the buffer (eight launches) and siss_saliency_mask, on a Gaussian gradient whose
                           per-tensor scales are log-uniform (exponents pile into a handful of bins, as real gradients' do);
  * the update pair        siss_grad_norms_scale + siss_recombine_clip_adamw (with the bf16 shadow) from --parent-lib -- a build of the
                           PARENT commit (the file tools/ab_bench.sh takes), or this build when none is given -- against the masked pair of
                           this build at mask densities 1.0, 0.5 and 0.03, all on the SAME buffers.

Every leg is timed over --reps launches between two device events, the legs interleaved, --rounds rounds: ms per call of every round
are reported, and the whole-buffer pair's spread over the rounds is the run-to-run spread the differences are to be read against.
Bytes: pass 1 reads 8 B per float, pass 2 reads 20 B and writes 14 B (p, m, v, shadow); the masked pair adds 1 bit per float per
pass.  No threshold is attached to any figure.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HP = dict(lr=1e-4, beta1=0.95, beta2=0.999, eps=1e-8, wd=1e-2)


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


class WholePair:
    """siss_grad_norms_scale + siss_recombine_clip_adamw of a library loaded on its own (the parent commit's build)."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        P, L, I, F = C.c_void_p, C.c_long, C.c_int, C.c_float
        self.lib.siss_grad_norms_scale.argtypes = [P, P, L, I, F, F, F, F, P, P, P]
        self.lib.siss_recombine_clip_adamw.argtypes = [P, P, P, P, P, P, P, L, F, F, F, F, F, P, P]

    def __call__(self, gx, ga, p, m, v, shadow, n, partials, scalars):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.siss_grad_norms_scale(ptr(gx), ptr(ga), n, 0, 5.0, 1.0, HP["beta1"], HP["beta2"], ptr(partials), ptr(scalars), s)
        rc |= self.lib.siss_recombine_clip_adamw(ptr(gx), ptr(ga), ptr(p), ptr(m), ptr(v), ptr(shadow), None, n, HP["lr"], HP["beta1"],
                                                 HP["beta2"], HP["eps"], HP["wd"], ptr(scalars), s)
        assert rc == 0, rc


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saliency.json"))
    ap.add_argument("--only", default=None, choices=[None, "celebahq256", "sd15"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_saliency.py needs a GPU"
    from siss_amd import lib
    from siss_amd.saliency import pack_threshold, select_magnitude
    dev = torch.device("cuda", 0)
    whole = WholePair(a.parent_lib or lib.LIB_PATH)
    result = dict(parent_lib=bool(a.parent_lib), reps=a.reps, rounds=a.rounds, hyper=HP, device=torch.cuda.get_device_name(0), buffers={})
    for name, info in buffer_floats().items():
        if a.only and name != a.only:
            continue
        n = info["floats"]
        gen = torch.Generator(device=dev).manual_seed(0)
        # per-stretch scales 2^-12 .. 2^0 over stretches of 64 Ki floats: a gradient's exponents, not a flat spectrum
        scale = torch.exp2(-12 * torch.rand(-(-n // 65536), device=dev, generator=gen)).repeat_interleave(65536)[:n]
        gx = torch.randn(n, device=dev, generator=gen) * scale
        ga = torch.randn(n, device=dev, generator=gen) * scale
        del scale
        p = torch.randn(n, device=dev, generator=gen)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        shadow = p.to(torch.bfloat16)
        partials = torch.zeros(lib.query("siss_opt_partials_words"), dtype=torch.float64, device=dev)
        scalars = torch.zeros(lib.query("siss_opt_scalars_words"), dtype=torch.float32, device=dev)
        work = torch.empty(lib.query("siss_absf_select_work_bytes"), dtype=torch.uint8, device=dev)
        res = torch.zeros(lib.query("siss_absf_select_result_words"), dtype=torch.int64, device=dev)
        k = n // 2
        sel = select_magnitude(gx, k)
        bits_sel = pack_threshold(gx, sel["threshold_bits"])
        masks = {}
        for density in (1.0, 0.5, 0.03):
            if density == 1.0:
                masks[density] = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
            else:
                masks[density] = pack_threshold(gx, select_magnitude(gx, int(density * n))["threshold_bits"])

        def masked(bits):
            lib.call("siss_grad_norms_scale_masked", gx, ga, n, bits, 0, 5.0, 1.0, HP["beta1"], HP["beta2"], partials, scalars)
            lib.call("siss_recombine_clip_adamw_masked", gx, ga, p, m, v, shadow, None, n, bits, HP["lr"], HP["beta1"], HP["beta2"],
                     HP["eps"], HP["wd"], scalars)

        legs = {"select": lambda: lib.call("siss_absf_select", gx, n, k, work, res),
                "mask": lambda: lib.call("siss_saliency_mask", gx, n, sel["threshold_bits"], bits_sel),
                "whole_pair": lambda: whole(gx, ga, p, m, v, shadow, n, partials, scalars)}
        for density, bits in masks.items():
            legs[f"masked_pair_{density}"] = (lambda b: (lambda: masked(b)))(bits)
        for fn in legs.values():                           # warm every leg
            fn()
        torch.cuda.synchronize()
        times = {leg: [] for leg in legs}
        for _ in range(a.rounds):
            for leg, fn in legs.items():                   # interleaved: one timed window per leg per round
                times[leg].append(timed(fn, a.reps))
        out = dict(info, k=k, select_result=sel, **{leg + "_ms": spread(ts) for leg, ts in times.items()})
        wp = out["whole_pair_ms"]
        out["whole_pair_spread_ms"] = round(wp["max"] - wp["min"], 4)
        for density in masks:
            mp = out[f"masked_pair_{density}_ms"]
            out[f"masked_pair_{density}_minus_whole_ms"] = round(mp["median"] - wp["median"], 4)
        out["whole_pair_bytes"] = 42 * n
        out["whole_pair_tb_per_s"] = round(42 * n / (wp["median"] * 1e-3) / 1e12, 3)
        out["select_plus_mask_ms"] = round(out["select_ms"]["median"] + out["mask_ms"]["median"], 4)
        result["buffers"][name] = out
        del gx, ga, p, m, v, shadow, masks, bits_sel
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

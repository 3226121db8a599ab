#!/usr/bin/env python
"""Unified Concept Editing (csrc/uce.hip) on the 32 cross-attention key / value matrices of the SD v1.5 UNet: writes ONE JSON
(profiles/uce.json).

    python tools/bench_uce.py [--reps 20] [--rounds 5] [--out profiles/uce.json]

The targets are read from the configuration (UNetCondEngine.param_specs of UNet2DConditionConfig.sd15(): every `attn2.to_k.weight` /
`attn2.to_v.weight`, X = 768), laid out in a flat buffer as the engine lays them out.  In ONE process and on the SAME buffers:

  * delta            siss_uce_delta: the increments of all targets in one launch (exact f32 on v_mfma_f32_16x16x4_f32);
  * apply_dry/apply  siss_uce_apply with apply = 0 and apply = 1 (the add and its four statistics);
  * pair             the two launches back to back -- what siss_amd.uce.apply issues;
  * addmm_torch      per target torch.addmm(W, W, E^T, out=W') on the same device: the f32 products of the BLAS library, not an
                     exact chain -- and pair_torch adds the statistics in eager torch (what the edit would cost without the kernels).

Every leg is timed over --reps calls between two device events, the legs interleaved, --rounds rounds, after a warm-up of every leg.
The operation count is 2 * rows * X * X per target; the bytes are 4 * (2 rows X + X X) for the products and 12 / 8 B per float for
the add (apply / dry run).  Rates are model operations (bytes) over the median time per call: end-to-end rates of the launch
sequence.  `share_of_f32_matrix_peak` is the delta launch's rate over the 157.3 TFLOP/s the MI355X is specified with for f32 matrix
operations.  No threshold is attached to any figure, and no speed claim is made in advance: the kernel's contract is an exact, grid-
independent value per element, torch.addmm's is not.  `max_abs_difference_to_addmm` says how far apart the two results are.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MATRIX_PEAK = 157.3e12
HBM_BYTES_PER_S = 8.0e12


def targets():
    """[(name, rows)] of the SD v1.5 UNet's cross-attention key / value projections, and X"""
    import re
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.uce import DEFAULT_TARGETS
    from siss_amd.unet_cond import UNetCondEngine
    cfg = UNet2DConditionConfig.sd15()
    specs = UNetCondEngine.param_specs(cfg)
    pat = re.compile(DEFAULT_TARGETS[0])
    X = int(cfg.cross_attention_dim)
    out = [(n, int(sp.native_shape[0])) for n, sp in specs.items() if pat.search(n)]
    assert out and all(specs[n].kind == "mat" and specs[n].native_shape[1] == X for n, _ in out)
    return out, X


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uce.json"))
    a = ap.parse_args(argv)
    tg, X = targets()
    assert torch.cuda.is_available(), "bench_uce.py needs a GPU (there is no CPU timing: the operation count alone says nothing about speed)"
    from types import SimpleNamespace as NS
    from siss_amd import lib
    from siss_amd.uce import job_table
    from siss_amd.unet import ALIGN
    dev = torch.device("cuda", 0)
    specs, off = {}, 0
    for n, rows in tg:
        specs[n] = NS(off=off, native_shape=(rows, X), numel=rows * X)
        off += -(-rows * X // ALIGN) * ALIGN
    names = [n for n, _ in tg]
    rec, rows = job_table(specs, names)
    jobs = (ctypes.c_char * rec.nbytes).from_buffer_copy(rec.tobytes())
    gen = torch.Generator(device=dev).manual_seed(0)
    p0 = torch.randn(off, device=dev, generator=gen) * 0.03
    E = torch.randn(X, X, device=dev, generator=gen) * (0.1 / X ** 0.5)
    p, delta = p0.clone(), torch.empty(rows * X, dtype=torch.float32, device=dev)
    partials = torch.empty(lib.query("siss_uce_partials_words", rows * X, len(names)), dtype=torch.float64, device=dev)
    stats, tstats = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    Ws = [p[specs[n].off:specs[n].off + specs[n].numel].view(specs[n].native_shape) for n in names]
    outs = [torch.empty_like(w) for w in Ws]
    ET = E.T.contiguous()

    def addmm():
        for w, o in zip(Ws, outs):
            torch.addmm(w, w, ET, out=o)

    def pair_torch():
        sd = sp = torch.zeros((), dtype=torch.float64, device=dev)
        mx = torch.zeros((), dtype=torch.float32, device=dev)
        for w, o in zip(Ws, outs):
            d = torch.mm(w, ET)
            sd, sp, mx = sd + d.double().square().sum(), sp + w.double().square().sum(), torch.maximum(mx, d.abs().max())
            torch.add(w, d, out=o)
        tstats[0], tstats[1], tstats[2], tstats[3] = sd, sp, mx.double(), float(rows * X)

    def kdelta():
        lib.call("siss_uce_delta", p, jobs, len(names), E, X, delta)

    def pair():
        kdelta()
        lib.call("siss_uce_apply", p, jobs, len(names), X, delta, 0, partials, stats)          # (dry: the buffers stay what they are)

    legs = {"delta": kdelta, "apply_dry": lambda: lib.call("siss_uce_apply", p, jobs, len(names), X, delta, 0, partials, stats),
            "apply": lambda: lib.call("siss_uce_apply", p, jobs, len(names), X, delta, 1, partials, stats), "pair": pair,
            "addmm_torch": addmm, "pair_torch": pair_torch}
    for leg, fn in legs.items():                           # warm every leg
        if leg != "apply":
            fn()
    torch.cuda.synchronize()
    diff = max(float((o - (w + delta[r0 * X:(r0 + w.shape[0]) * X].view_as(w))).abs().max())
               for o, w, r0 in zip(outs, Ws, [int(r["row_off"]) for r in rec]))
    mine, theirs = stats.cpu().tolist(), tstats.cpu().tolist()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():                       # interleaved: one timed window per leg per round
            if leg == "apply":
                p.copy_(p0)                                # (outside the window: the add accumulates otherwise)
            times[leg].append(timed(fn, a.reps if leg != "apply" else 1))
    p.copy_(p0)
    flops, floats = 2.0 * rows * X * X, rows * X
    gemm_bytes = 4.0 * (2 * floats + X * X)
    model = {"delta": (flops, gemm_bytes), "apply_dry": (0.0, 8.0 * floats), "apply": (0.0, 12.0 * floats),
             "pair": (flops, gemm_bytes + 8.0 * floats), "addmm_torch": (flops, gemm_bytes), "pair_torch": (flops, gemm_bytes + 8.0 * floats)}
    result = dict(reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), X=X, targets=len(names), rows=rows, floats=floats,
                  gflop=round(flops / 1e9, 3), f32_matrix_peak_flops=F32_MATRIX_PEAK, hbm_bytes_per_s=HBM_BYTES_PER_S,
                  note="apply (apply = 1) is timed one call per window on restored weights; every other leg over --reps calls",
                  max_abs_difference_to_addmm=diff, stats_kernel=mine, stats_torch=theirs, legs={})
    for leg, ts in times.items():
        s = spread(ts)
        ops, nbytes = model[leg]
        sec = s["median"] * 1e-3
        result["legs"][leg] = dict(s, spread_ms=round(s["max"] - s["min"], 4), model_flop=ops, model_bytes=nbytes,
                                   achieved_tflops=round(ops / sec / 1e12, 2), achieved_gb_per_s=round(nbytes / sec / 1e9, 1))
    result["share_of_f32_matrix_peak"] = round(flops / (result["legs"]["delta"]["median"] * 1e-3) / F32_MATRIX_PEAK, 3)
    result["addmm_torch_over_delta"] = round(result["legs"]["addmm_torch"]["median"] / result["legs"]["delta"]["median"], 3)
    result["pair_torch_over_pair"] = round(result["legs"]["pair_torch"]["median"] / result["legs"]["pair"]["median"], 3)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()

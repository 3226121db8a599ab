#!/usr/bin/env python
"""The dataset-wide SSCD search on one GPU against the composition a user writes today: prints ONE JSON line and writes it to
profiles/sscd_search.json.

    python tools/bench_sscd_search.py [--reps 20] [--gallery 30000] [--dims 512] [--k 5] [--out profiles/sscd_search.json]

Three cases on Gaussian unit rows (the times do not depend on the values), k = 5:
  * q64 / q1024: 64 and 1,024 queries against the gallery (siss_amd.sscd_search.topk: siss_sscd_topk);
  * all_pairs:   every row of the gallery against the gallery with its own row excluded, in query blocks of 4,096.
Per case: hip_ms (median), hip_ms_min, torch_ms / torch_ms_min for chunked `(q @ g.T).topk(k)` on the same device in the same
query blocks (its self pair masked with -inf in the all-pairs case), the peak device memory either side allocates on top of the
rows (torch.cuda.max_memory_allocated), the algorithmic rate 2 nq ng d / time against the 157.3 TF f32 MFMA peak, and whether the two
sides returned the same indices.  Device events around one whole search after two warm-up searches, --reps repeats, the two sides
alternating; the shader clock is read right after the timed work.  No threshold is asserted: this tool records."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3
BLOCK = 4096


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:2] or None
    except Exception:
        return None


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def _peak(fn):
    """Bytes fn allocates on top of what is live when it starts."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def torch_topk(q, g, k, self0=-1):
    vals, idxs = [], []
    for s in range(0, q.shape[0], BLOCK):
        sim = q[s:s + BLOCK] @ g.T
        if self0 >= 0:
            n = sim.shape[0]
            sim[torch.arange(n, device=q.device), torch.arange(self0 + s, self0 + s + n, device=q.device)] = float("-inf")
        v, i = sim.topk(k, dim=1)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gallery", type=int, default=30000)
    ap.add_argument("--dims", type=int, default=512)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sscd_search.json"))
    a = ap.parse_args()
    from siss_amd import lib, sscd_search as S
    lib.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    g = torch.nn.functional.normalize(torch.randn(a.gallery, a.dims, generator=gen), dim=1).to(dev)
    res = {"tool": "bench_sscd_search", "device": torch.cuda.get_device_name(0), "reps": a.reps, "gallery": a.gallery, "dims": a.dims,
           "k": a.k, "query_block": BLOCK, "peak_tf": PEAK_TF,
           "timing": "device events around one whole search, median (and minimum) of the repeats, the two sides alternating", "cases": {}}
    cases = [("q64", torch.nn.functional.normalize(torch.randn(64, a.dims, generator=gen), dim=1).to(dev), -1),
             ("q1024", torch.nn.functional.normalize(torch.randn(1024, a.dims, generator=gen), dim=1).to(dev), -1),
             ("all_pairs", g, 0)]
    for name, q, self0 in cases:
        hip = lambda: S.topk(q, g, a.k, self0)
        ref = lambda: torch_topk(q, g, a.k, self0)
        for _ in range(2):
            hip(), ref()
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(a.reps):
            th.append(_timed(hip)[0])
            tt.append(_timed(ref)[0])
        (hv, hi), (tv, ti) = hip(), ref()
        flops = 2.0 * q.shape[0] * g.shape[0] * a.dims
        ms = statistics.median(th)
        res["cases"][name] = {
            "queries": int(q.shape[0]), "hip_ms": round(ms, 4), "hip_ms_min": round(min(th), 4),
            "torch_ms": round(statistics.median(tt), 4), "torch_ms_min": round(min(tt), 4),
            "hip_peak_bytes": _peak(hip), "torch_peak_bytes": _peak(ref),
            "matrix_bytes": int(q.shape[0]) * int(g.shape[0]) * 4,
            "tflops": round(flops / (ms * 1e-3) / 1e12, 2), "peak_frac": round(flops / (ms * 1e-3) / 1e12 / PEAK_TF, 4),
            "same_indices": float((hi.long() == ti).float().mean()), "max_value_diff": float((hv - tv).abs().max())}
    clock = _clock()                                     # read right after the timed work
    res["sclk"] = clock if clock else "not recorded"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

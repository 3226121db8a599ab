#!/usr/bin/env python
"""The feature-set launchers (csrc/feature_sets.hip) on one GPU against the composition a user writes in torch: prints ONE JSON line
and writes it to profiles/feature_sets.json.  NOT the reference's protocol, which reports FID only.

    python tools/bench_feature_sets.py [--reps 5] [--out profiles/feature_sets.json]

Two shapes on synthetic ReLU features (the times do not depend on the values), d = 2048, k = 5:
  * full:  30,000 real / 10,000 fake rows, 100 subsets of 1,000;
  * small: 30,000 real /  1,000 fake rows, 100 subsets of 500.
Three stages per shape, each timed on both sides:
  * real_radii:  squared norms and k-th-neighbour radii of the real rows (once per run);
  * prdc_eval:   the fake rows' norms and radii and the two ball passes, the real side given (once per evaluation);
  * kid:         the 3 x 100 kernel sums.
The torch side is what a user writes on the same device: `sq[:, None] + sq[None, :] - 2 f @ g.T` in chunks of 4,096 rows with
`topk(k, largest=False)` for the radii, comparisons and `min` for the balls, and `((xs @ ys.T) / d + 1) ** 3` per subset for the sums.
Per stage: hip_ms / torch_ms (medians) with their minima, the peak device memory either side allocates on top of the rows
(torch.cuda.max_memory_allocated), the algorithmic rate 2 n m d / time, and how far the two sides' results are apart.  Device events
around one whole stage after two warm-up runs, --reps repeats, the two sides alternating; the shader clock is read right after the
timed work.  No threshold is asserted: this tool records, including a stage where torch is faster."""
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
SHAPES = {"full": dict(real=30000, fake=10000, subsets=100, subset_size=1000),
          "small": dict(real=30000, fake=1000, subsets=100, subset_size=500)}


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


# ---------------------------------------------------------------- the torch side
def torch_d2(q, sq_q, g, sq_g):
    return (sq_q[:, None] + sq_g[None, :] - 2.0 * (q @ g.T)).clamp_(min=0)


def torch_radii(x, k):
    sq = (x * x).sum(1)
    out = []
    for s in range(0, x.shape[0], BLOCK):
        d2 = torch_d2(x[s:s + BLOCK], sq[s:s + BLOCK], x, sq)
        n = d2.shape[0]
        d2[torch.arange(n, device=x.device), torch.arange(s, s + n, device=x.device)] = float("inf")
        out.append(d2.topk(k, dim=1, largest=False).values[:, k - 1])
    return sq, torch.cat(out)


def torch_ball(q, sq_q, g, sq_g, rad):
    inside, mins = [], []
    for s in range(0, q.shape[0], BLOCK):
        d2 = torch_d2(q[s:s + BLOCK], sq_q[s:s + BLOCK], g, sq_g)
        inside.append((d2 <= rad[None, :]).sum(1))
        mins.append(d2.min(1).values)
    return torch.cat(inside), torch.cat(mins)


def torch_prdc(real, sq_r, r_r, fake, k):
    sq_f, r_f = torch_radii(fake, k)
    in_f, _ = torch_ball(fake, sq_f, real, sq_r, r_r)
    in_r, min_r = torch_ball(real, sq_r, fake, sq_f, r_f)
    return torch.stack([(in_f > 0).double().mean(), (in_r > 0).double().mean(), in_f.double().sum() / (k * fake.shape[0]),
                        (min_r <= r_r).double().mean()])


def torch_kid(real, ir, fake, if_, d):
    out = []
    eye = torch.eye(ir.shape[1], device=real.device, dtype=torch.bool)
    for b in range(ir.shape[0]):
        xs, ys = real[ir[b]], fake[if_[b]]
        kxx, kyy, kxy = (((p @ q.T) / d + 1) ** 3 for p, q in ((xs, xs), (ys, ys), (xs, ys)))
        out.append(torch.stack([kxx.masked_fill(eye, 0).sum(), kyy.masked_fill(eye, 0).sum(), kxy.sum()]))
    return torch.stack(out)


# ---------------------------------------------------------------- the measurement
def stage(reps, hip, ref, flops, diff):
    for _ in range(2):
        hip(), ref()
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(reps):
        th.append(_timed(hip)[0])
        tt.append(_timed(ref)[0])
    ms, tms = statistics.median(th), statistics.median(tt)
    return {"hip_ms": round(ms, 3), "hip_ms_min": round(min(th), 3), "torch_ms": round(tms, 3), "torch_ms_min": round(min(tt), 3),
            "hip_peak_bytes": _peak(hip), "torch_peak_bytes": _peak(ref), "hip_tflops": round(flops / (ms * 1e-3) / 1e12, 2),
            "torch_tflops": round(flops / (tms * 1e-3) / 1e12, 2), "hip_peak_frac": round(flops / (ms * 1e-3) / 1e12 / PEAK_TF, 4),
            "faster": "hip" if ms < tms else "torch", "max_rel_diff": diff(hip(), ref())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--shapes", default="full,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_sets.json"))
    a = ap.parse_args()
    from siss_amd import feature_sets as F, lib
    lib.load()
    F.require_kernels()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev, d, k = torch.device("cuda", 0), a.dims, a.k
    gen = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(8, d, device=dev, generator=gen)

    def rows(n, shift):
        z = torch.randn(n, 8, device=dev, generator=gen) + shift
        return torch.relu(z @ W / 8 ** 0.5 + 0.05 * torch.randn(n, d, device=dev, generator=gen)).contiguous()

    res = {"tool": "bench_feature_sets", "device": torch.cuda.get_device_name(0), "reps": a.reps, "dims": d, "k": k, "torch_block": BLOCK,
           "peak_tf": PEAK_TF, "protocol": "NOT the reference's protocol, which reports FID only",
           "timing": "device events around one whole stage, median (and minimum) of the repeats after two warm-up runs, the two sides "
                     "alternating", "shapes": {}}
    rel = lambda x, y: float(((x.double() - y.double()).abs().max() / y.double().abs().max().clamp_min(1e-300)).cpu())
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        real, fake = rows(sh["real"], 0.0), rows(sh["fake"], 0.3)
        N, M, S, s = sh["real"], sh["fake"], sh["subsets"], sh["subset_size"]
        out = dict(sh)
        out["real_radii"] = stage(a.reps, lambda: F.knn_radius(real, F.sqnorm(real), k), lambda: torch_radii(real, k)[1],
                                  2.0 * N * N * d, rel)
        sq_r = F.sqnorm(real)
        r_r = F.knn_radius(real, sq_r, k)
        rb, fb = F.FeatureBank(d, N, dev), F.FeatureBank(d, M, dev)
        rb.append(real), fb.append(fake)
        prdc = F.PRDC(k)
        prdc.compute(rb, fb)                                  # the real side's cache

        def hip_prdc():
            fb.cache.clear()
            return torch.tensor(list(prdc.compute(rb, fb).values()), dtype=torch.float64)

        out["prdc_eval"] = stage(a.reps, hip_prdc, lambda: torch_prdc(real, sq_r, r_r, fake, k).cpu(), 2.0 * d * (M * M + 2.0 * N * M), rel)
        out["prdc_eval"]["figures"] = dict(zip(("precision", "recall", "density", "coverage"), hip_prdc().tolist()))
        ir, if_ = F.subset_tables(N, M, S, s, 0)
        ird, ifd = ir.to(dev), if_.to(dev)
        out["kid"] = stage(a.reps, lambda: F.kid_sums(real, ir, fake, if_, 1.0 / d, 1.0), lambda: torch_kid(real, ird, fake, ifd, d),
                           2.0 * d * 3.0 * S * s * s, rel)
        out["kid"]["kid_mean_std"] = [float(v) for v in F.kid_from_sums(F.kid_sums(real, ir, fake, if_, 1.0 / d, 1.0), s)]
        res["shapes"][name] = out
        del real, fake, rb, fb
        torch.cuda.empty_cache()
    clock = _clock()                                     # read right after the timed work
    res["sclk"] = clock if clock else "not recorded"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

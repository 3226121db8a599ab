#!/usr/bin/env python
"""The FID metric's device work on one GPU: prints ONE JSON line.

    python tools/bench_fid.py [--reps 10] [--sizes 1,16,64]

  * hip_ms[N] / images_per_s[N] / tflops[N] / peak_frac[N]: preprocessing + the FID Inception-v3 features (siss_amd.fid, f32,
    csrc/inception.hip) of N images of 256 x 256, against the 157.3 TF f32 MFMA peak; algorithmic flops = 2 x MACs of the 94
    convolutions;
  * stats_ms[N]: one statistics update (sum, cov_sum in f64, D = 2048) of N feature rows;
  * torch_ms[N]: the same weights in tests/fid_ref.py's module on torch-ROCm (f32, eval), its preprocessing included.
Device-event timing after warm-up, median of --reps repeats.  The weights are random-init (He-normal, BN statistics randomised): the
times do not depend on them.  An FID evaluation is bound by its sampling, not by this: 10 000 images x 50 UNet steps cost about
10^4 times the Inception pass over them.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TF = 157.3


def _median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out)


def macs_per_image():
    """MACs of one 299 x 299 image through the 94 convolutions (map sizes followed through the strides and the two stem pools)."""
    from siss_amd.fid import convs
    size = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 73}
    total = 0
    for name, cin, cout, (kh, kw), stride, (ph, pw) in convs():
        block = name.split(".")[0]
        h = size.get(name) or (35 if block.startswith("Mixed_5") or block == "Mixed_6a" else 17 if block.startswith("Mixed_6")
                               or block == "Mixed_7a" else 8)
        if block == "Mixed_6a" and name.endswith("dbl_3"):
            h = 35
        ho, wo = (h + 2 * ph - kh) // stride + 1, (h + 2 * pw - kw) // stride + 1
        total += ho * wo * cout * kh * kw * cin
    return total


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:2] or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import fid_ref as R
    from siss_amd import lib
    from siss_amd.fid import FEATURES, FrechetInceptionDistance, InceptionV3FID
    lib.load()
    dev = torch.device("cuda", 0)
    net = R.make(0)
    hip = InceptionV3FID()
    hip.load_state_dict(net.state_dict())
    hip.to(dev)
    tnet = net.to(dev).float().eval()
    macs = macs_per_image()
    res = {"tool": "bench_fid", "device": torch.cuda.get_device_name(0), "reps": a.reps, "macs_per_image": macs, "image": "256 x 256",
           "weights": "random-init (He-normal, BN statistics randomised)", "hip_ms": {}, "images_per_s": {}, "tflops": {},
           "peak_frac": {}, "stats_ms": {}, "torch_ms": {}, "torch_tflops": {}}
    clock = _clock()
    res["sclk"] = clock if clock else "not recorded"
    fc = FrechetInceptionDistance(None, FEATURES, dev)
    for n in [int(v) for v in a.sizes.split(",")]:
        x = torch.rand(n, 3, 256, 256, generator=torch.Generator().manual_seed(n)).to(dev)
        with torch.no_grad():
            ms = _median_ms(lambda: hip(x), a.reps)
            f = hip(x)
            sms = _median_ms(lambda: fc.update_features(f, real=False), a.reps)
            if not a.no_torch:
                tms = _median_ms(lambda: tnet(R.preprocess(x)), a.reps)
                res["torch_ms"][n] = round(tms, 4)
                res["torch_tflops"][n] = round(2.0 * macs * n / (tms * 1e-3) / 1e12, 2)
        tf = 2.0 * macs * n / (ms * 1e-3) / 1e12
        res["hip_ms"][n], res["images_per_s"][n] = round(ms, 4), round(n / (ms * 1e-3), 1)
        res["tflops"][n], res["peak_frac"][n], res["stats_ms"][n] = round(tf, 2), round(tf / PEAK_TF, 4), round(sms, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The SSCD score's device work on one GPU: prints ONE JSON line.

    python tools/bench_sscd.py [--reps 10] [--sizes 8,64] [--size 512] [--no-torch]

  * hip_ms[N] / images_per_s[N] / tflops[N] / peak_frac[N]: preprocessing from uint8 + the SSCD ResNet-50 embeddings
    (siss_amd.sscd, f32: csrc/metric_conv.hip's convolution, csrc/sscd.hip around it) of N images of --size x --size, in chunks of
    16, against the 157.3 TF f32 MFMA peak; algorithmic flops = 2 x MACs of the 53 convolutions and fc (the trunk);
  * torch_ms[N] / torch_tflops[N]: the same weights in tests/sscd_ref.py's module on torch-ROCm (f32, eval), its normalisation
    included, in the same chunks.
Device-event timing after warm-up, median of --reps repeats.  The weights are random-init: the times do not depend on them.  The
convolution is the 64 x 64-tile kernel written for the MNIST ResNet-18; whether a larger tile pays on these shapes is what this
tool is for.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TF = 157.3
CHUNK = 16


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


def macs_per_image(h, w):
    """MACs of one h x w image through the 53 convolutions and fc (map sizes followed through the strides and the max pool)."""
    from siss_amd.sscd import FEATURES, _convs
    total = 0
    last = block_in = None                          # the map the previous convolution wrote / the current block reads
    for name, cin, cout, k, s, p, _ in _convs():
        if name == "conv1":
            hi, wi = h, w
        elif name.endswith(".conv1"):
            hi, wi = block_in = last
        elif name.endswith("downsample.0"):          # (listed after the block's conv3; it reads the block's input)
            hi, wi = block_in
        else:
            hi, wi = last
        ho, wo = (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1
        total += ho * wo * cout * k * k * cin
        if name == "conv1":
            last = ((ho - 1) // 2 + 1, (wo - 1) // 2 + 1)                                      # the max pool
        elif not name.endswith("downsample.0"):
            last = (ho, wo)
    return total + FEATURES * 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="8,64")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import sscd_ref as R
    from siss_amd import lib
    from siss_amd.sscd import SSCDModel
    lib.load()
    dev = torch.device("cuda", 0)
    net = R.make(0)
    hip = SSCDModel(batch_size=CHUNK)
    hip.load_state_dict(net.state_dict())
    hip.to(dev)
    tnet = net.to(dev).float().eval()
    macs = macs_per_image(a.size, a.size)
    res = {"tool": "bench_sscd", "device": torch.cuda.get_device_name(0), "reps": a.reps, "macs_per_image": macs,
           "image": f"{a.size} x {a.size}", "chunk": CHUNK, "weights": "random-init", "hip_ms": {}, "images_per_s": {}, "tflops": {},
           "peak_frac": {}, "torch_ms": {}, "torch_tflops": {}}
    m = torch.tensor(R.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    s = torch.tensor(R.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    for n in [int(v) for v in a.sizes.split(",")]:
        u8 = torch.randint(0, 256, (n, a.size, a.size, 3), generator=torch.Generator().manual_seed(n), dtype=torch.uint8).to(dev)

        def torch_side():
            return torch.cat([tnet((u8[i:i + CHUNK].permute(0, 3, 1, 2).float() / 255 - m) / s) for i in range(0, n, CHUNK)])
        with torch.no_grad():
            ms = _median_ms(lambda: hip.embed_u8(u8, R.IMAGENET_MEAN, R.IMAGENET_STD), a.reps)
            if not a.no_torch:
                tms = _median_ms(torch_side, a.reps)
                res["torch_ms"][n] = round(tms, 4)
                res["torch_tflops"][n] = round(2.0 * macs * n / (tms * 1e-3) / 1e12, 2)
        tf = 2.0 * macs * n / (ms * 1e-3) / 1e12
        res["hip_ms"][n], res["images_per_s"][n] = round(ms, 4), round(n / (ms * 1e-3), 1)
        res["tflops"][n], res["peak_frac"][n] = round(tf, 2), round(tf / PEAK_TF, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

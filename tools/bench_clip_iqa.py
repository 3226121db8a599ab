#!/usr/bin/env python
"""The CLIP-IQA score's device work on one GPU: prints ONE JSON line.

    python tools/bench_clip_iqa.py [--reps 10] [--sizes 8,64] [--size 512]

  * hip_ms[N] / images_per_s[N] / tflops[N] / peak_frac[N]: preprocessing from uint8 + the CLIP RN50 image tower + the score
    (siss_amd.clip_iqa, f32: csrc/metric_conv.hip's convolution, csrc/clip_iqa.hip around it) of N images of --size x --size, in
    chunks of 16, against the 157.3 TF f32 MFMA peak; algorithmic flops = 2 x MACs of the convolutions and the FOLDED attention pool;
  * trunk_ms[N] / attnpool_ms[N]: the same chunks split into the trunk (preprocessing .. layer4) and the attention pool (mean token
    .. c_proj), each timed on its own; attnpool_unfolded_macs is what projecting every token through k_proj and v_proj would cost.
Device-event timing after warm-up, median of --reps repeats.  The weights are random-init: the times do not depend on them.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def macs_per_image(model, h, w):
    """(trunk MACs, folded attention-pool MACs, unfolded attention-pool MACs) of one h x w image."""
    from siss_amd.clip_iqa import visual_convs
    trunk, H, W = 0, h, w
    for name, cin, cout, k, s, p, _, pool in visual_convs(model.layers, model.width):
        if name.endswith("downsample.0"):
            trunk += (Hb // pool) * (Wb // pool) * cout * cin
            continue
        if name.endswith(".conv1"):
            Hb, Wb = H, W                               # the block's input: what its shortcut reads
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        trunk += Ho * Wo * cout * k * k * cin
        H, W = Ho // pool, Wo // pool
    E, T, out = model.embed, H * W + 1, model.output_dim
    folded = E * E + E * E + T * E * model.heads + T * E * model.heads + E * E + E * out     # q, fold, logits, pooling, value, c_proj
    unfolded = E * E + 2 * T * E * E + 2 * T * E + E * out
    return trunk, folded, unfolded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="8,64")
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    from siss_amd import lib
    from siss_amd.clip_iqa import CLIPIQAModel
    lib.load()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    hip = CLIPIQAModel(batch_size=CHUNK, text_layers=1).to(dev)              # (the text tower is not timed: the anchors are given)
    anchors = torch.nn.functional.normalize(torch.randn(2, hip.output_dim), dim=1).to(dev)
    trunk, folded, unfolded = macs_per_image(hip, a.size, a.size)
    macs = trunk + folded
    res = {"tool": "bench_clip_iqa", "device": torch.cuda.get_device_name(0), "reps": a.reps, "trunk_macs_per_image": trunk,
           "attnpool_macs_per_image": folded, "attnpool_unfolded_macs_per_image": unfolded, "image": f"{a.size} x {a.size}",
           "chunk": CHUNK, "weights": "random-init", "hip_ms": {}, "images_per_s": {}, "tflops": {}, "peak_frac": {}, "trunk_ms": {},
           "attnpool_ms": {}}
    fh, fw = hip._shapes(1, a.size, a.size)[0]
    for n in [int(v) for v in a.sizes.split(",")]:
        u8 = torch.randint(0, 256, (n, a.size, a.size, 3), generator=torch.Generator().manual_seed(n), dtype=torch.uint8).to(dev)
        pooled = hip.attention_pool
        maps = []

        def keep_map(h, N, HW):                          # the trunk alone: stop in front of the attention pool
            maps.append(h)
            return torch.empty(N, hip.output_dim, device=dev)
        with torch.no_grad():
            ms = _median_ms(lambda: hip.scores_u8(u8, anchors), a.reps)
            hip.attention_pool = keep_map
            try:
                tms = _median_ms(lambda: (maps.clear(), hip.embed_u8(u8)), a.reps)
            finally:
                hip.attention_pool = pooled
            pms = _median_ms(lambda: [pooled(h, h.shape[0], fh * fw) for h in maps], a.reps)
        tf = 2.0 * macs * n / (ms * 1e-3) / 1e12
        res["hip_ms"][n], res["images_per_s"][n] = round(ms, 4), round(n / (ms * 1e-3), 1)
        res["tflops"][n], res["peak_frac"][n] = round(tf, 2), round(tf / PEAK_TF, 4)
        res["trunk_ms"][n], res["attnpool_ms"][n] = round(tms, 4), round(pms, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

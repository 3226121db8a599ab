#!/usr/bin/env python
"""Membership loss on one GPU, CelebA-HQ 256 x 256, bf16, RANDOM-INIT weights, synthetic images: prints ONE JSON line.

    python tools/bench_membership.py [--images 8] [--noises 8] [--min-seconds 1.0] [--rounds 2]

One forget image (every shipped delete config), timesteps [200, 900].  Per items-per-forward b in {4, 16, 32}:
  * fused_graph / fused_eager: siss_amd.membership.MembershipLoss (siss_pair_noise -> forward -> siss_pair_sqerr per forward), the
    forward replayed from the captured hipGraph / launched eagerly, dedupe off: 2 * I * J work items per timestep;
  * fused_graph_dedupe: the same with dedupe on (I * J + J items per timestep), and dedupe_ratio = its time / the dedupe-off time
    against the ideal (I * J + J) / (2 * I * J);
  * plain: the composition a user writes without the metric -- the reference's loop body (metrics/class_membership.py:75-116)
    through the class surface: three expanded tensors, sched.add_noise twice, unet(x, t, return_dict=False)[0] on batches of b for
    both groups, torch.sum, torch.cat + mean per timestep; one host read at the end.
Every number is `items / s` over the 2 * I * J * len(timesteps) pairs an evaluation reports (so dedupe shows as more pairs per second),
plus ms per forward.  Timing: a synchronised host clock around whole evaluations (host-side launch work is part of what is compared); every shape is warmed (graphs captured) first; each measurement repeats the evaluation
until --min-seconds have passed; the paths are alternated --rounds times in one call and the median is reported with the spread
between identical runs (max - min over rounds, relative).
"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TIMESTEPS = [200, 900]


def plain_composition(unet, sched, images_all, images_del, noise, timesteps, b):
    """metrics/class_membership.py:75-130 as it stands, on this package's class surface."""
    I, J, dev = images_all.shape[0], noise.shape[0], images_all.device
    out = []
    for t in timesteps:
        xa = images_all.unsqueeze(1).expand(-1, J, -1, -1, -1)
        xd = images_del.unsqueeze(1).expand(-1, J, -1, -1, -1)
        nz = noise.unsqueeze(0).expand(I, -1, -1, -1, -1)
        xa, xd, nz = (v.reshape(-1, *v.shape[2:]) for v in (xa, xd, nz))
        tt = torch.full((xa.shape[0],), t, device=dev)
        na, nd = sched.add_noise(xa, nz, tt), sched.add_noise(xd, nz, tt)
        la, ld = [], []
        with torch.no_grad():
            for i in range(0, na.shape[0], b):
                bn = nz[i:i + b]
                bt = tt[:bn.shape[0]]
                oa = unet(na[i:i + b], bt, return_dict=False)[0]
                od = unet(nd[i:i + b], bt, return_dict=False)[0]
                la.append(torch.sum((oa - bn) ** 2, dim=[1, 2, 3]))
                ld.append(torch.sum((od - bn) ** 2, dim=[1, 2, 3]))
        a, d = torch.mean(torch.cat(la)), torch.mean(torch.cat(ld))
        out.append([a, d])
    return torch.stack([torch.stack(p) for p in out]).cpu()      # one host read per evaluation, as the fused path's caller makes


def measure(fn, min_seconds):
    """Seconds per call of fn (a whole evaluation, host-synchronised), repeated until min_seconds have passed."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--noises", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--small", action="store_true", help="a 64 x 64 two-level UNet instead of CelebA-HQ 256 (a quick check of the tool)")
    a = ap.parse_args()
    from siss_amd.config import UNet2DConfig
    from siss_amd.data import SyntheticImages
    from siss_amd.membership import MembershipLoss
    from siss_amd.model import UNet2DModel
    from siss_amd.scheduler import DDPMScheduler
    dev = torch.device("cuda", 0)
    cfg = UNet2DConfig.celebahq256()
    if a.small:
        cfg = UNet2DConfig(sample_size=64, in_channels=3, out_channels=3, block_out_channels=(64, 128),
                           down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
                           layers_per_block=1, attention_head_dim=None)
    unet = UNet2DModel(cfg, device=dev, compute_dtype=torch.bfloat16)
    unet.engine.init_random(seed=0)
    sched = DDPMScheduler()
    shape = (cfg.in_channels, cfg.sample_size, cfg.sample_size)
    ds_all, ds_del = SyntheticImages(256, shape, seed=1), SyntheticImages(1, shape, seed=2)
    I, J, T = a.images, a.noises, len(TIMESTEPS)
    pairs = 2 * I * J * T
    res = {"metric": "membership_loss", "model": "small64" if a.small else "celebahq256", "dtype": "bf16", "weights": "random-init",
           "images": I, "noises": J, "timesteps": TIMESTEPS, "forget_images": 1, "pairs_per_evaluation": pairs,
           "ideal_dedupe_ratio": round((I * J + J) / (2 * I * J), 4), "device": torch.cuda.get_device_name(0), "sizes": {}}
    for b in a.sizes:
        def metric(**kw):
            m = MembershipLoss(ds_all, ds_del, sched, unet, I, J, b, dev, **kw)
            random.seed(0)
            m.sample_images()
            m.sample_noises(generator=torch.Generator(device=dev).manual_seed(0))
            return m
        ms = {"fused_graph": metric(dedupe=False), "fused_eager": metric(dedupe=False, use_graph=False), "fused_graph_dedupe": metric()}
        ref = ms["fused_graph"]
        paths = {k: (lambda m=m: m.compute_membership_losses(TIMESTEPS)) for k, m in ms.items()}
        paths["plain"] = lambda: plain_composition(unet, sched, ref.all_sampled_images, ref.deletion_sampled_images, ref.noise, TIMESTEPS, b)
        for fn in paths.values():                               # every shape warmed, every graph captured
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.rounds):                               # alternated: fused, plain, ... in one call
            for k in ("fused_graph", "plain", "fused_graph_dedupe", "fused_eager"):
                times[k].append(measure(paths[k], a.min_seconds))
        # the two paths report the same numbers (bf16: not the same bits -- other batch slots, another schedule of the noising)
        got = torch.stack([torch.stack(p) for p in ms["fused_graph"].compute_membership_losses(TIMESTEPS)]).cpu()
        want = paths["plain"]()
        out = {"means_rel_diff_vs_plain": float(((got - want).abs() / want.abs()).max())}
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
            forwards = ms[k].forwards if k in ms else 2 * T * -(-I * J // b)
            out[k] = {"eval_s": round(med, 4), "pairs_per_s": round(pairs / med, 1), "ms_per_forward": round(1e3 * med / forwards, 3),
                      "forwards": forwards, "spread": round((ts[-1] - ts[0]) / med, 4)}
        out["fused_graph_over_plain"] = round(out["plain"]["eval_s"] / out["fused_graph"]["eval_s"], 4)
        out["dedupe_ratio"] = round(out["fused_graph_dedupe"]["eval_s"] / out["fused_graph"]["eval_s"], 4)
        res["sizes"][str(b)] = out
        del ms, paths
    print(json.dumps(res))


if __name__ == "__main__":
    main()

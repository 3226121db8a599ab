#!/usr/bin/env python
"""The SD task's front end on one GPU, with and without the latent cache: prints ONE JSON line.

    python tools/bench_latent_cache.py [--reps-encode 10] [--reps-warm 200]

SD v1 VAE shapes (512 x 512 images -> 4 x 64 x 64 latents, the 34.2 M-parameter encoder, random-init weights: the times do not
depend on them), per batch size B = 1 (config/delete_sd.yaml's train_batch_size) and B = 16:

  * encode_ms: ``VAEEncoder.encode(x, generator=g)`` of B images already on the device -- what DeleteSD.prepare_batch runs per
    micro-batch and batch with the cache off (the decode and the host-to-device copy of the images are NOT in it: the Prefetcher hides
    them);
  * warm_ms: ``LatentCache.latents(indices, g)`` of B cached images -- host-side lookup, the index copy, the normals, one
    siss_latent_sample launch;
  * cold_ms: the same call on an empty cache -- B images stacked from host tensors, copied, encoded in one raw_moments call, their
    rows written, then sampled (one call, host clock around a synchronise: it is taken once per image and run).

encode_ms and warm_ms: device events on the launch stream around `reps` back-to-back calls after 3 warm-up calls of the same shape,
so a call's host work counts where it is what the device waits for.  The shader clock is read once after the timed work.  No
threshold is attached to any of it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:2] or None
    except Exception:
        return None


def _timed_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(reps):
        fn()
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps-encode", type=int, default=10)
    ap.add_argument("--reps-warm", type=int, default=200)
    ap.add_argument("--images", type=int, default=32, help="dataset size (host tensors of 512 x 512)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_latent_cache.py needs a GPU"
    from oracle.vae import OracleVAEEncoder, VAEConfig
    from siss_amd import lib
    from siss_amd.data import TensorImages
    from siss_amd.latent_cache import LatentCache
    from siss_amd.vae import VAEEncoder
    lib.load()
    dev = torch.device("cuda", 0)
    enc = VAEEncoder(device=dev)
    torch.manual_seed(0)
    enc.load_state_dict(OracleVAEEncoder(VAEConfig.sd_v1()).state_dict())
    ds = TensorImages(torch.rand(a.images, 3, 512, 512, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    g = torch.Generator(device=dev).manual_seed(42)
    res = {"tool": "bench_latent_cache", "device": torch.cuda.get_device_name(0), "weights": "random-init",
           "image": [3, 512, 512], "latent": [4, 64, 64], "dataset_images": a.images,
           "reps": {"encode": a.reps_encode, "warm": a.reps_warm, "cold": 1, "warmup": 3},
           "timing": "device events on the launch stream around back-to-back calls (cold: host clock around one synchronised call)"}
    rows = {}
    with torch.no_grad():
        for B in (1, 16):
            idx = list(range(B))
            x = ds.t[:B].to(dev)
            encode = _timed_ms(lambda: enc.encode(x, generator=g), a.reps_encode)        # (warms the encoder at this shape too)
            cache = LatentCache(enc, ds, (4, 64, 64))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cache.latents(idx, g)
            torch.cuda.synchronize()
            cold = (time.perf_counter() - t0) * 1e3
            assert cache.encoded == B
            warm = _timed_ms(lambda: cache.latents(idx, g), a.reps_warm)
            assert cache.encoded == B                    # nothing encoded since
            rows[f"b{B}"] = {"encode_ms": round(encode, 4), "warm_ms": round(warm, 4), "cold_ms": round(cold, 3),
                             "encode_over_warm": round(encode / warm, 1)}
    res["rows"] = rows
    clock = _clock()                                     # read right after the timed work
    res["sclk"] = clock if clock else "not recorded"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

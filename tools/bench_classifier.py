#!/usr/bin/env python
"""The T-shirt experiment's quality metrics on one GPU: prints ONE JSON line.

    python tools/bench_classifier.py [--reps 20] [--no-eval]

  * hip_ms[N] / tflops[N] / peak_frac[N]: the MNIST ResNet-18 logits (siss_amd.classifier, f32, csrc/metric_conv.hip) at
    N = 128, 1024, 4096 images of 28 x 28, against the 157.3 TF f32 MFMA peak; algorithmic flops = 2 x MACs of the convolutions
    and fc;
  * torch_ms[N]: the same weights in tests/classifier_ref.py's module on torch-ROCm (f32, eval);
  * eval: one T-shirt evaluation at the reference's settings on the MNIST UNet (config/train_tshirt_mnist.yaml, its f32 engine,
    RANDOM-INIT weights): 128 images x 50 DDPM steps for the fraction, 1024 images x 50 steps for the Inception Score, split into
    sampling and classifier seconds.
Device-event timing after warm-up, median of --reps repeats.  The classifier weights are random-init (reference init, BN statistics
randomised): the times do not depend on them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TF = 157.3


def _median_ms(fn, reps, warmup=3):
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


def _block_macs(hw=28, cin=1, classes=10):
    """MACs of one image through the network (conv1, the BasicBlocks with their shortcuts, fc)."""
    h = (hw + 6 - 7) // 2 + 1
    total = h * h * 64 * 49 * cin
    h = (h - 1) // 2 + 1
    c = 64
    for i, w in enumerate((64, 128, 256, 512)):
        for j in range(2):
            s = 2 if (i > 0 and j == 0) else 1
            ho = (h + 2 - 3) // s + 1
            total += ho * ho * w * 9 * c + ho * ho * w * 9 * w
            if s != 1 or c != w:
                total += ho * ho * w * c
            h, c = ho, w
    return total + 512 * classes


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:2] or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-eval", action="store_true")
    a = ap.parse_args()
    import classifier_ref as R
    from siss_amd import lib
    from siss_amd.classifier import resnet18
    lib.load()
    dev = torch.device("cuda", 0)
    net = R.make(10, True, seed=0)
    hip = resnet18(10, True)
    hip.load_state_dict(net.state_dict())
    hip.to(dev)
    tnet = net.to(dev).float().eval()
    macs = _block_macs()
    res = {"tool": "bench_classifier", "device": torch.cuda.get_device_name(0), "reps": a.reps, "macs_per_image": macs,
           "weights": "random-init (reference init, BN statistics randomised)", "hip_ms": {}, "tflops": {}, "peak_frac": {},
           "torch_ms": {}, "torch_tflops": {}}
    clock = _clock()
    res["sclk"] = clock if clock else "not recorded"
    for n in (128, 1024, 4096):
        x = torch.rand(n, 1, 28, 28, generator=torch.Generator().manual_seed(n)).to(dev)
        with torch.no_grad():
            ms = _median_ms(lambda: hip(x), a.reps)
            tms = _median_ms(lambda: tnet(x), a.reps)
        tf = 2.0 * macs * n / (ms * 1e-3) / 1e12
        res["hip_ms"][n], res["tflops"][n], res["peak_frac"][n] = round(ms, 4), round(tf, 2), round(tf / PEAK_TF, 4)
        res["torch_ms"][n] = round(tms, 4)
        res["torch_tflops"][n] = round(2.0 * macs * n / (tms * 1e-3) / 1e12, 2)
    if not a.no_eval:
        res["eval"] = _evaluation(dev, hip)
    print(json.dumps(res))


def _evaluation(dev, hip):
    """One T-shirt evaluation at the reference's settings: sampling and classifier seconds."""
    import numpy as np
    from siss_amd import hydra_lite as H
    from siss_amd.classifier import Classifier, InceptionScore, TShirtClassifier
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.sampler import Evaluator
    from siss_amd.scheduler import DDPMScheduler
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"), [])
    ucfg = {k: v for k, v in cfg.unet.items() if not k.startswith("_")}
    unet = UNet2DModel(UNet2DConfig.from_dict(ucfg), device=dev, compute_dtype=torch.float32)
    unet.engine.init_random(seed=0)
    sched = DDPMScheduler(num_train_timesteps=1000, beta_schedule="linear", beta_start=1e-4, beta_end=0.02)
    ev = Evaluator(cfg)
    ev.load_model(unet, sched)
    gen = torch.Generator(device=dev).manual_seed(0)
    tshirt = torch.rand(1, 28, 28, generator=torch.Generator().manual_seed(1)).to(dev)
    clf = Classifier.__new__(Classifier)
    clf.classifier, clf.transform = hip, None

    def sample(n, bs):
        out = [ev.sample_images(min(bs, n - s), num_inference_steps=50, generator=gen) for s in range(0, n, bs)]
        return torch.from_numpy(np.concatenate(out)).permute(0, 3, 1, 2).to(dev)

    out = {"unet": "config/train_tshirt_mnist.yaml, f32 engine, random-init", "steps": 50}
    for n in (128, 1024):                              # warm-up: the captured forward of both batch shapes
        ev.sample_images(n, num_inference_steps=1, generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    imgs = sample(128, 128)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    frac, _ = TShirtClassifier.get_tshirt_frequency(imgs, tshirt)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out.update(fraction_images=128, fraction_sampling_s=round(t1 - t0, 4), fraction_match_s=round(t2 - t1, 5))
    t0 = time.perf_counter()
    imgs = sample(1024, 1024)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _, m = TShirtClassifier.get_tshirt_frequency(imgs, tshirt)
    ic = InceptionScore(clf, splits=10)
    ic.update(imgs[~m])
    mean, std = ic.compute(generator=torch.Generator().manual_seed(0))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out.update(is_images=1024, is_sampling_s=round(t1 - t0, 4), is_classifier_s=round(t2 - t1, 5),
               is_mean=float(mean), fraction=frac)
    return out


if __name__ == "__main__":
    main()

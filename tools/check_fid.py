#!/usr/bin/env python
"""The HIP FID path against torchmetrics on the REAL Inception weights, for whoever has both (this repository has seen neither):

    python tools/check_fid.py /path/to/pt_inception-2015-12-05-6726825d.pth [--images DIR] [--n 32] [--size 256]

Loads the state dict strictly into siss_amd.fid.InceptionV3FID and into torchmetrics' own feature extractor
(torchmetrics.image.fid.NoTrainInceptionV3 over torch-fidelity's FeatureExtractorInceptionV3, f32 on the same GPU), runs the same
images through both -- the files of --images (jpg / png, ToTensor), or seeded uniform noise plus a darker, smoother second set when
no directory is given -- and compares
  * the [N, 2048] features: max |d| <= 1e-3 of max |reference| (two f32 stacks of ~100 layers in different summation orders), and
  * the FID of the two halves of the images: FIDEvaluator-style statistics here against torchmetrics'
    FrechetInceptionDistance(normalize=True) fed the same halves, within 1e-3 relative.
Exit status 0 when both hold.  Needs torchmetrics and torch-fidelity importable: their absence is an error, not a skip.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _images(a):
    if a.images:
        from siss_amd.data import CelebAHQ, ToTensor
        ds = CelebAHQ("all", a.images, [], ToTensor())
        n = min(len(ds), a.n)
        if n < 4:
            raise SystemExit(f"{a.images}: {len(ds)} images, at least 4 are needed (two per side)")
        return torch.stack([ds[i] for i in range(n)])
    g = torch.Generator().manual_seed(0)
    first = torch.rand(a.n // 2, 3, a.size, a.size, generator=g)
    second = torch.nn.functional.avg_pool2d(torch.rand(a.n - a.n // 2, 3, a.size, a.size, generator=g), 3, 1, 1) * 0.6
    return torch.cat([first, second])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--images")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    from torchmetrics.image.fid import FrechetInceptionDistance as TMFid, NoTrainInceptionV3
    from siss_amd.fid import FrechetInceptionDistance, InceptionV3FID
    dev = torch.device("cuda", 0)
    sd = torch.load(a.checkpoint, map_location="cpu")
    hip = InceptionV3FID()
    hip.load_state_dict(sd)
    hip.to(dev).eval()
    ref_net = NoTrainInceptionV3(name="inception-v3-compat", features_list=["2048"], feature_extractor_weights_path=a.checkpoint)
    ref_net = ref_net.to(dev).eval()
    imgs = _images(a).to(dev)
    half = imgs.shape[0] // 2
    with torch.no_grad():
        got = hip(imgs)
        want = ref_net((imgs * 255).byte())
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    ok_f = err <= 1e-3 * scale
    print(f"features [{imgs.shape[0]}, 2048]: max|d| {err:.3e} = {err / scale:.2e} of max|reference| {scale:.3e}  {'ok' if ok_f else 'FAIL'}")
    ours = FrechetInceptionDistance(hip, 2048, dev)
    ours.update(imgs[:half], real=True)
    ours.update(imgs[half:], real=False)
    theirs = TMFid(feature=ref_net, normalize=True).to(dev)
    theirs.update(imgs[:half], real=True)
    theirs.update(imgs[half:], real=False)
    a_, b_ = float(ours.compute()), float(theirs.compute())
    ok_d = abs(a_ - b_) <= 1e-3 * abs(b_)
    print(f"FID {half} + {imgs.shape[0] - half}: {a_:.6f} here, {b_:.6f} torchmetrics: {abs(a_ - b_) / abs(b_):.2e}  {'ok' if ok_d else 'FAIL'}")
    return 0 if ok_f and ok_d else 1


if __name__ == "__main__":
    sys.exit(main())

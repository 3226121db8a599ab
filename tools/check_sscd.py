#!/usr/bin/env python
"""The HIP SSCD path against TorchScript on the REAL checkpoint, for whoever has it (this repository has not seen the file):

    python tools/check_sscd.py /path/to/sscd_disc_mixup.torchscript.pt [--images DIR] [--n 8] [--size 512]

Loads the file both ways -- `torch.jit.load` as the reference does (f32 on the same GPU, no autocast), and
`siss_amd.sscd.SSCDModel.load`, which is strict over the key names: a file whose trunk is not torchvision-layout is refused
here with the missing and unexpected keys -- embeds the same images with both (the files of --images, jpg / png, at their own size
one by one; or seeded uniform noise with a smoothed second half when no directory is given), Normalize(ImageNet)(ToTensor(.)) in
front of each, and prints
  * the [N, dims] embeddings: max |d| and the smallest cosine between the two embeddings of an image, and
  * the scores of every image against the first one, both ways.
Exit status 0 when max |d| <= 1e-4 (two f32 stacks of 53 layers in different summation orders, on unit rows).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _images(a):
    """A list of uint8 [1, H, W, 3] tensors."""
    if a.images:
        from PIL import Image
        names = sorted(f for f in os.listdir(a.images) if f.lower().endswith((".jpg", ".jpeg", ".png")))[:a.n]
        if len(names) < 2:
            raise SystemExit(f"{a.images}: {len(names)} images, at least 2 are needed")
        return [torch.from_numpy(np.asarray(Image.open(os.path.join(a.images, f)).convert("RGB")).copy())[None] for f in names]
    g = torch.Generator().manual_seed(0)
    x = torch.rand(a.n, 3, a.size, a.size, generator=g)
    x[a.n // 2:] = torch.nn.functional.avg_pool2d(x[a.n // 2:], 5, 1, 2) * 0.8
    return list((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().split(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--images")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    from siss_amd.data import Normalize
    from siss_amd.sscd import SSCDModel
    dev = torch.device("cuda", 0)
    hip = SSCDModel.load(a.checkpoint).to(dev).eval()
    ref_net = torch.jit.load(a.checkpoint, map_location="cpu").to(dev).eval()
    norm = Normalize(MEAN, STD)
    got, want = [], []
    with torch.no_grad():
        for u8 in _images(a):
            u8 = u8.to(dev)
            got.append(hip.embed_u8(u8, MEAN, STD))
            want.append(ref_net(norm((u8.permute(0, 3, 1, 2).float().cpu() / 255).to(dev))).float())     # ToTensor divides on the host
    got, want = torch.cat(got).double(), torch.cat(want).double()
    err = float((got - want).abs().max())
    cos = float((got * want).sum(1).min())
    ok = err <= 1e-4
    print(f"embeddings [{got.shape[0]}, {got.shape[1]}]: max|d| {err:.3e}, smallest cosine {cos:.8f}  {'ok' if ok else 'FAIL'}")
    print("scores against image 0, here:       ", [round(float(v), 6) for v in got @ got[0]])
    print("scores against image 0, TorchScript:", [round(float(v), 6) for v in want @ want[0]])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""The HIP CLIP-IQA path against torchmetrics on the REAL checkpoint, for whoever has both (this repository has seen neither the
OpenAI RN50 file nor torchmetrics / piq: this script has NOT been run on them):

    python tools/check_clip_iqa.py /path/to/RN50.pt --tokenizer /path/to/clip/tokenizer [--images DIR] [--n 8] [--size 512]

Loads the file with `siss_amd.clip_iqa.CLIPIQAModel.load` (strict over the OpenAI key names), builds
`siss_amd.clip_iqa.CLIPImageQualityAssessment(model, tokenizer=...)` and torchmetrics' `CLIPImageQualityAssessment()` (its
defaults: model "clip_iqa", data_range 1.0, prompts ("quality",); f32 on the same GPU, no autocast -- it fetches its own copy of the
weights through piq), scores the same images with both (the files of --images, jpg / png, at their own size one by one; or seeded
uniform noise with a smoothed second half when no directory is given) and prints both score lists and their largest deviation.
Exit status 0 when it is <= 1e-3 (two f32 stacks of ~70 layers in different summation orders behind a softmax over 100 x cosines).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _images(a):
    """A list of float [1, 3, H, W] tensors in [0, 1] (ToTensor of uint8 images)."""
    if a.images:
        from PIL import Image
        names = sorted(f for f in os.listdir(a.images) if f.lower().endswith((".jpg", ".jpeg", ".png")))[:a.n]
        if not names:
            raise SystemExit(f"{a.images}: no images")
        u8 = [torch.from_numpy(np.asarray(Image.open(os.path.join(a.images, f)).convert("RGB")).copy())[None] for f in names]
    else:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(a.n, 3, a.size, a.size, generator=g)
        x[a.n // 2:] = torch.nn.functional.avg_pool2d(x[a.n // 2:], 5, 1, 2) * 0.8
        u8 = list((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().split(1))
    return [t.permute(0, 3, 1, 2).float() / 255 for t in u8]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--tokenizer", required=True, help="a transformers CLIPTokenizer directory")
    ap.add_argument("--images")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    from torchmetrics.multimodal import CLIPImageQualityAssessment as Reference
    from siss_amd.clip_iqa import CLIPImageQualityAssessment, CLIPIQAModel
    dev = torch.device("cuda", 0)
    here = CLIPImageQualityAssessment(model=CLIPIQAModel.load(a.checkpoint).to(dev).eval(), tokenizer=a.tokenizer)
    ref = Reference().to(dev)
    got, want = [], []
    with torch.no_grad():
        for img in _images(a):
            got.append(here(img.to(dev)).reshape(-1))
            want.append(ref(img.to(dev)).float().reshape(-1))
    got, want = torch.cat(got).double().cpu(), torch.cat(want).double().cpu()
    err = float((got - want).abs().max())
    ok = err <= 1e-3
    print("scores, here:        ", [round(float(v), 6) for v in got])
    print("scores, torchmetrics:", [round(float(v), 6) for v in want])
    print(f"max|d| {err:.3e}  {'ok' if ok else 'FAIL'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

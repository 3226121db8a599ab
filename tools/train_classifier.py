#!/usr/bin/env python
"""Produce `checkpoints/classifiers/mnist.pt`, the trained MNIST ResNet-18 that `metrics.classifier_cfg` of delete_tshirt.yaml reads
(T-shirt fraction, class frequencies, Inception Score) and that the reference trains in notebooks/cnn-resnet18-mnist.ipynb: Adam
(lr 1e-3), batch 128, 10 epochs, seed 1, images in [0, 1] through ToTensor alone, train-mode BatchNorm, cross-entropy -- here on the
HIP kernels (siss_amd.classifier_train.ResNet18Trainer).

    python tools/train_classifier.py --data DIR [--split train] [--test-split test] [--remove-class 10] [--epochs 10]
        [--batch-size 128] [--lr 1e-3] [--seed 1] --out checkpoints/classifiers/mnist.pt [--allow-synthetic]

DIR/<split>.npz holds `image` (uint8 [N, H, W]) and `label` ([N]) as siss_amd.data.HFDataset reads them; the images whose label is
--remove-class (the T-shirt label 10 of delete_tshirt.yaml; `none` keeps every image) are left out.  Each epoch prints the loss every
50 batches and the train accuracy in eval mode; at the end the test accuracy when DIR/<test-split>.npz exists.  Beside --out,
metrics.json holds the per-epoch loss and accuracy, every step's loss, the arguments and the seed.

--allow-synthetic replaces the dataset by a seeded synthetic one (10 fixed prototype images plus noise, --synthetic-images of them):
it exists for the tests, and nothing falls back to it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Synthetic:
    """n images of 10 classes: a fixed uint8 prototype per class (drawn from `seed` alone) plus noise drawn from (seed, split);
    the labels cycle 0 .. 9.  `images` / `labels` as HFDataset's."""

    def __init__(self, n, seed, split, hw=28):
        protos = np.random.default_rng([int(seed), 0]).integers(0, 256, (10, hw, hw)).astype(np.float64)
        noise = np.random.default_rng([int(seed), 1 + (split != "train")]).normal(0.0, 32.0, (n, hw, hw))
        self.labels = np.arange(n, dtype=np.int64) % 10
        self.images = np.clip(np.rint(protos[self.labels] + noise), 0, 255).astype(np.uint8)

    def __len__(self):
        return len(self.images)


def remove_class(text):
    """--remove-class: an integer label, or `none`."""
    return None if str(text).lower() == "none" else int(text)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", default=None)
    ap.add_argument("--split", default="train")
    ap.add_argument("--test-split", default="test")
    ap.add_argument("--remove-class", type=remove_class, default=10)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", required=True)
    ap.add_argument("--allow-synthetic", action="store_true")
    ap.add_argument("--synthetic-images", type=int, default=640)
    a = ap.parse_args(argv)
    if a.epochs < 1 or a.batch_size < 2:
        ap.error("--epochs >= 1 and --batch-size >= 2 are needed")
    if not a.allow_synthetic and not a.data:
        ap.error("--data DIR is needed (or --allow-synthetic)")
    return a


def load_split(a, split):
    """The dataset of one split: HFDataset over DIR/<split>.npz without the removed class (FileNotFoundError when the file is
    missing), or the synthetic one with --allow-synthetic."""
    if a.allow_synthetic:
        return Synthetic(a.synthetic_images, a.seed, split)
    from siss_amd.data import HFDataset
    if a.remove_class is None:
        return HFDataset("all", a.data, split)
    return HFDataset("nondeletion", a.data, split, class_to_remove=a.remove_class)


def batch_of(ds, idx):
    """(images [n, 1, H, W] f32 in [0, 1], labels [n] int64) of the items idx: siss_amd.data.ToTensor's arithmetic (uint8 -> f32,
    / 255) on the whole batch at once."""
    import torch
    imgs = ds.images[np.asarray(idx)]
    if imgs.ndim != 3:
        raise ValueError(f"grayscale images [N, H, W] are needed, got {ds.images.shape}")
    x = torch.from_numpy(imgs.astype(np.float32) / np.float32(255.0)).unsqueeze(1)
    return x, torch.from_numpy(np.asarray(ds.labels)[np.asarray(idx)].astype(np.int64))


def accuracy(trainer, ds, batch_size=2048):
    """Share of ds that eval-mode logits classify right (one host read at the end)."""
    import torch
    right = torch.zeros((), device=trainer.device, dtype=torch.int64)
    for s in range(0, len(ds), batch_size):
        x, y = batch_of(ds, range(s, min(s + batch_size, len(ds))))
        right += (trainer.eval_logits(x).argmax(-1) == y.to(trainer.device)).sum()
    return int(right) / len(ds)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from siss_amd.classifier_train import ResNet18Trainer
    from siss_amd.data import EpochSampler
    train = load_split(a, a.split)
    if len(train) < 2:
        raise ValueError(f"{len(train)} training images")
    if int(np.asarray(train.labels).max()) >= 10 or int(np.asarray(train.labels).min()) < 0:
        raise ValueError("labels outside 0 .. 9 remain after --remove-class: the network has 10 classes")
    trainer = ResNet18Trainer(num_classes=10, grayscale=True, device="cuda", lr=a.lr, seed=a.seed)
    sampler = EpochSampler(len(train), a.batch_size, a.seed, a.epochs)
    nb = len(sampler)
    epochs, step_losses, losses = [], [], []

    def close_epoch(e):
        vals = torch.stack(losses).cpu().tolist()
        losses.clear()
        step_losses.extend(vals)
        acc = accuracy(trainer, train)
        epochs.append({"epoch": e + 1, "loss": float(np.mean(vals)), "train_acc": acc})
        print(f"Epoch: {e + 1:03d}/{a.epochs:03d} | loss {np.mean(vals):.4f} | train acc {100 * acc:.3f} %", flush=True)

    for e, pos, idx in sampler:
        if pos == 0 and e > 0:
            close_epoch(e - 1)
        if len(idx) < 2:                                         # (a last batch of one image: train-mode BN over one value)
            continue
        x, y = batch_of(train, idx)
        losses.append(trainer.step(x, y))
        if pos % 50 == 0:
            print(f"Epoch: {e + 1:03d}/{a.epochs:03d} | Batch {pos:04d}/{nb:04d} | loss {float(losses[-1]):.4f}", flush=True)
    close_epoch(a.epochs - 1)
    test_acc = None
    if a.allow_synthetic or os.path.isfile(os.path.join(str(a.data), f"{a.test_split}.npz")):
        test_acc = accuracy(trainer, load_split(a, a.test_split))
        print(f"test acc {100 * test_acc:.3f} %", flush=True)
    out = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    trainer.save(out)
    rec = {"args": {k: v for k, v in sorted(vars(a).items())}, "seed": a.seed, "images": len(train), "epochs": epochs,
           "step_losses": step_losses, "test_acc": test_acc}
    with open(os.path.join(os.path.dirname(out), "metrics.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {out} and metrics.json beside it")
    return rec


if __name__ == "__main__":
    main()

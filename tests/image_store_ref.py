"""Reference of the image store (siss_amd/image_store.py, csrc/image_store.hip): the HOST TRANSFORM, nothing else.  The store claims
the bits of ``torch.stack([dataset[i] for i in idx])``, so every comparison against what is here is torch.equal -- there is no
tolerance to derive.  Also the tiny datasets the tests write: a PNG directory for CelebAHQ, an npz for HFDataset."""
import os

import numpy as np
import torch

CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)


def transforms(C):
    """{name: transform} the store recognises for C channels: ToTensor alone, Normalize(0.5, 0.5) of length 1 (broadcast) and, for
    C = 3, of length 3 and CIFAR's per-channel triple."""
    from siss_amd.data import Compose, Normalize, ToTensor
    out = {"totensor": ToTensor(), "half1": Compose([ToTensor(), Normalize([0.5], [0.5])])}
    if C == 3:
        out["half3"] = Compose([ToTensor(), Normalize([0.5] * 3, [0.5] * 3)])
        out["cifar"] = Compose([ToTensor(), Normalize(CIFAR_MEAN, CIFAR_STD)])
    return out


def table_pixel_by_pixel(transform, C):
    """[C, 256] f32: the transform applied to 256 one-pixel images, one per byte value (every channel holding that value)."""
    out = torch.empty(C, 256, dtype=torch.float32)
    for v in range(256):
        px = np.full((1, 1) if C == 1 else (1, 1, C), v, dtype=np.uint8)
        t = transform(px)
        assert tuple(t.shape) == (C, 1, 1) and t.dtype == torch.float32
        out[:, v] = t[:, 0, 0]
    return out


def lookup(table, raw):
    """numpy table lookup: out[c, y, x] = table[c][raw[c, y, x]] for a uint8 [C, H, W] image."""
    tab = table.numpy()
    return torch.from_numpy(np.stack([tab[c][raw[c]] for c in range(raw.shape[0])]))


def gather(store, idx, table, out_dtype=torch.float32):
    """What siss_image_gather writes, on the host: out[i, c] = table[c][store[idx[i], c]] (bf16: torch's cast of the f32 table
    value, round to nearest even); an index outside [0, rows) gives a NaN row."""
    rows, C = store.shape[:2]
    out = torch.full((len(idx), *store.shape[1:]), float("nan"), dtype=torch.float32)
    for i, r in enumerate(idx):
        if 0 <= r < rows:
            for c in range(C):
                out[i, c] = table[c][store[r, c].long()]
    return out.to(out_dtype)


def all_bytes_store(rows, C, H, W, seed=0):
    """uint8 [rows, C, H, W] whose every channel holds every byte value: a ramp modulo 256 over the channel's rows * H * W >= 256
    bytes, shuffled, with its own shuffle per channel."""
    g = torch.Generator().manual_seed(seed + 131 * C + H)
    n = rows * H * W
    assert n >= 256
    out = torch.empty(C, n, dtype=torch.uint8)
    for c in range(C):
        out[c] = (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8)
    store = out.view(C, rows, H, W).permute(1, 0, 2, 3).contiguous()
    assert all(len(torch.unique(store[:, c])) == 256 for c in range(C))
    return store


def write_png_dir(path, n, H, W, seed=0, gray=(), size_of=None):
    """n PNG files 000.png ... under `path`: RGB noise, the indices in `gray` single-channel (mode L) files that convert("RGB")
    expands; size_of {index: (H, W)} gives single files another size.  Returns the uint8 arrays written."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    written = []
    for i in range(n):
        h, w = (size_of or {}).get(i, (H, W))
        a = rng.integers(0, 256, (h, w) if i in gray else (h, w, 3), dtype=np.uint8)
        Image.fromarray(a, mode="L" if i in gray else "RGB").save(os.path.join(str(path), f"{i:03d}.png"))
        written.append(a)
    return written


def write_npz(path, n, H, W, C=None, seed=0, split="train", labels=None):
    """<path>/<split>.npz with `image` uint8 [n, H, W] (C None) or [n, H, W, C] and `label` [n] (i % 11 unless given)."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (n, H, W) if C is None else (n, H, W, C), dtype=np.uint8)
    label = np.arange(n) % 11 if labels is None else np.asarray(labels)
    np.savez(os.path.join(str(path), f"{split}.npz"), image=image, label=label)
    return image, label

"""Latent cache of the Stable Diffusion unlearning loop (OPT-IN: ``latent_cache.enabled`` of config/delete_sd.yaml).

``DeleteSD.prepare_batch`` runs the frozen VAE encoder on every micro-batch, for the keep batch and again for the forget batch
(delete_sd.py:879-888 of the reference: ``vae.encode(x).latent_dist.sample() * vae.config.scaling_factor``).  The encoder is
frozen and the transform is fixed, so an image's posterior moments never change; only the normals of ``sample()`` do.  A
``LatentCache`` keeps the moments of a dataset on the device -- one row per image, filled the first time the image is drawn -- and
turns a batch of dataset INDICES into latents with one launch (csrc/latent_cache.hip ``siss_latent_sample``), drawing the normals
exactly as ``VAEEncoder.encode`` draws them: the loop's generator stream is the same with the cache on or off.

There is no fallback: a dataset whose cache does not fit ``max_bytes`` is refused at construction, a cache file that does not
belong to (encoder, dataset, transform, latent shape) is not used and the reason printed.
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import lib
from .data import IndexBatch, index_batches      # (they live in data.py: the image store carries them too)  # noqa: F401

DEFAULT_MAX_BYTES = 8 << 30
DEFAULT_CHUNK = 16
MAX_BATCH = 65535               # grid.y of the launch
FORMAT = 1


def sample_blocks(n, chw):
    """Blocks per sample of siss_latent_sample: one per 1024 elements (one f32x4 sweep of 256 lanes), the grid capped at 2048
    blocks; the rest is grid-strided (the streaming grid of sd_sampler.ddim_blocks)."""
    return max(1, min(-(-chw // 1024), 2048 // n, 1024))


def latent_sample(cache, idx, eps, scaling, out_dtype=torch.float32, out=None, nblk=None):
    """out[i] = (mean[r] + exp(0.5 * clamp(logvar[r], -30, 20)) * eps[i]) * scaling, r = idx[i]: cache [rows, 2C, h, w] f32 (the mean
    first, the unclamped log-variance second: VAEEncoder.raw_moments), idx [n] int64 ON THE DEVICE, eps [n, C, h, w] f32; out f32 or
    bf16.  An index outside [0, rows) is not read: its output row is NaN (LatentCache validates on the host before it launches)."""
    n, chw = eps.shape[0], int(np.prod(eps.shape[1:]))
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype {out_dtype}: f32 or bf16 are written")
    if not 0 < n <= MAX_BATCH:
        raise ValueError(f"{n} samples in one launch: 1..{MAX_BATCH} are taken")
    assert cache.dtype == eps.dtype == torch.float32 and idx.dtype == torch.int64
    assert cache.is_contiguous() and idx.is_contiguous() and eps.is_contiguous()
    assert cache.dim() >= 2 and cache[0].numel() == 2 * chw and idx.numel() == n and idx.device == cache.device == eps.device
    out = torch.empty(eps.shape, dtype=out_dtype, device=eps.device) if out is None else out
    assert out.dtype == out_dtype and out.is_contiguous() and out.shape == eps.shape and out.device == eps.device
    lib.call("siss_latent_sample", cache, idx, eps, out, int(out_dtype == torch.bfloat16), cache.shape[0], n, chw, float(scaling),
             sample_blocks(n, chw) if nblk is None else int(nblk))
    return out


# ---------------------------------------------------------------- fingerprint
def _unwrap(ds):
    from .data import ImagesOnly
    while isinstance(ds, ImagesOnly):
        ds = ds.dataset
    return ds


def transform_repr(ds):
    """repr of the dataset's transform; a transform without a stable repr (the default `<... object at 0x...>`) cannot be
    fingerprinted and is refused."""
    r = repr(getattr(_unwrap(ds), "transform", None))
    if " at 0x" in r:
        raise TypeError(f"latent cache fingerprint: the transform {r} has no stable repr")
    return r


def image_entries(ds):
    """[(relative name, sha256 of the content)] per image of a dataset, in index order: the files of an image directory (SDData:
    img_dir + img_names; CelebAHQ: paths), or the rows of a tensor stack (TensorImages)."""
    ds = _unwrap(ds)

    def file_hash(path):
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for block in iter(lambda: f.read(1 << 20), b""):
                h.update(block)
        return h.hexdigest()

    if hasattr(ds, "img_names") and hasattr(ds, "img_dir"):
        return [(str(n), file_hash(str(ds.img_dir) + str(n))) for n in ds.img_names]
    if hasattr(ds, "paths"):
        return [(os.path.basename(p), file_hash(p)) for p in ds.paths]
    if hasattr(ds, "t") and torch.is_tensor(ds.t):
        t = ds.t.detach().cpu().contiguous()
        return [(str(i), hashlib.sha256(t[i].numpy().tobytes()).hexdigest()) for i in range(t.shape[0])]
    raise TypeError(f"latent cache fingerprint: no rule for a dataset of type {type(ds).__name__} (image files or a tensor stack)")


def encoder_bytes(encoder):
    """The encoder's flat f32 parameter buffer as bytes (ParamStore.flat: every parameter, in declaration order)."""
    flat = encoder.ps.flat
    return flat.detach().cpu().contiguous().numpy().tobytes()


def fingerprint(encoder, dataset, latent_shape):
    """sha256 over the encoder's flat parameter bytes, each image's relative name and content hash, the transform's repr and the
    latent shape: what a cached moment depends on."""
    h = hashlib.sha256()
    h.update(b"siss_amd.latent_cache/%d\0" % FORMAT)
    h.update(hashlib.sha256(encoder_bytes(encoder)).digest())
    for name, digest in image_entries(dataset):
        h.update(name.encode() + b"\0" + digest.encode() + b"\0")
    h.update(transform_repr(dataset).encode() + b"\0")
    h.update(repr(tuple(int(v) for v in latent_shape)).encode())
    return h.hexdigest()


# ---------------------------------------------------------------- the cache
class LatentCache:
    """Posterior moments of `dataset` under `encoder`, [N, 2C, h, w] f32 on the device, filled lazily.

    encoder: a VAEEncoder (raw_moments(x) -> [k, 2C, h, w] f32; cfg.latent_channels, cfg.scaling_factor; ps.flat for the
    fingerprint).  dataset: items are image tensors [3, H, W] on the host.  latent_shape: (C, h, w) of one latent.  chunk: the
    most images one raw_moments call takes.  max_bytes: the budget the FULL cache must fit -- refused otherwise, with the count."""

    def __init__(self, encoder, dataset, latent_shape, device=None, max_bytes=None, chunk=None, name="latent cache"):
        self.encoder, self.dataset, self.name = encoder, dataset, name
        self.latent_shape = tuple(int(v) for v in latent_shape)
        C, h, w = self.latent_shape
        if C != int(encoder.cfg.latent_channels):
            raise ValueError(f"{name}: latent shape {self.latent_shape} with an encoder of {encoder.cfg.latent_channels} latent channels")
        self.n = len(dataset)
        self.max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
        self.chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
        if self.n <= 0 or self.chunk <= 0:
            raise ValueError(f"{name}: {self.n} images, chunk {self.chunk}: positive counts are needed")
        self.nbytes = self.n * 2 * C * h * w * 4
        if self.nbytes > self.max_bytes:
            raise MemoryError(f"{name}: the moments of {self.n} images x {2 * C} x {h} x {w} f32 take {self.nbytes} bytes, more than "
                              f"latent_cache.max_bytes = {self.max_bytes}; raise the budget or run with the cache off")
        self.device = torch.device(device if device is not None else encoder.device)
        self.moments = torch.zeros((self.n, 2 * C, h, w), dtype=torch.float32, device=self.device)
        self.filled = np.zeros(self.n, dtype=bool)            # host side: a lookup never asks the device
        self.encoded = 0                                      # images that went through the encoder in this process

    # -- host-side checks
    def _indices(self, indices):
        """The indices as a host int64 array, validated: integers (a list / IndexBatch, a numpy array or a HOST tensor of an integer
        type) within [0, N).  A device tensor is refused: reading it would synchronise."""
        if torch.is_tensor(indices):
            if indices.device.type != "cpu":
                raise TypeError(f"{self.name}: indices on {indices.device}: host indices are needed (the misses are looked up on the "
                                "host, without a device synchronisation)")
            if indices.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
                raise TypeError(f"{self.name}: indices of dtype {indices.dtype}: integers are needed")
            arr = indices.numpy()
        else:
            arr = np.asarray(indices)
        if arr.ndim != 1 or arr.size == 0:
            raise ValueError(f"{self.name}: a non-empty one-dimensional batch of indices is needed, got shape {arr.shape}")
        if arr.dtype.kind not in "iu":
            raise TypeError(f"{self.name}: indices of dtype {arr.dtype}: integers are needed")
        arr = arr.astype(np.int64)
        bad = arr[(arr < 0) | (arr >= self.n)]
        if bad.size:
            raise IndexError(f"{self.name}: indices {bad[:8].tolist()} outside [0, {self.n})")
        return arr

    def misses(self, arr):
        """The distinct indices of `arr` that are not filled yet, in order of first appearance."""
        seen, out = set(), []
        for i in arr.tolist():
            if not self.filled[i] and i not in seen:
                seen.add(i)
                out.append(i)
        return out

    def _to_device(self, host):
        if self.device.type == "cuda":
            return host.pin_memory().to(self.device, non_blocking=True)
        return host.to(self.device)

    # -- filling
    @torch.no_grad()
    def fill(self, indices):
        """Decode and encode the images of `indices` that are not cached yet -- each once, the misses of the call together in
        raw_moments calls of at most `chunk` images -- and write their rows.  Returns the misses."""
        miss = self.misses(self._indices(indices))
        C, h, w = self.latent_shape
        for lo in range(0, len(miss), self.chunk):
            part = miss[lo:lo + self.chunk]
            x = self._to_device(torch.stack([self.dataset[i] for i in part]).float())
            mom = self.encoder.raw_moments(x)
            if tuple(mom.shape) != (len(part), 2 * C, h, w) or mom.dtype != torch.float32:
                raise ValueError(f"{self.name}: images {tuple(x.shape)} encode to moments {tuple(mom.shape)} {mom.dtype}, the cache was "
                                 f"built for {(2 * C, h, w)} f32 per image")
            rows = self._to_device(torch.tensor(part, dtype=torch.int64))
            self.moments.index_copy_(0, rows, mom.to(self.device))
            self.filled[part] = True
            self.encoded += len(part)
        return miss

    # -- the front end of a micro-batch
    @torch.no_grad()
    def latents(self, indices, generator=None, out_dtype=torch.float32):
        """``vae.encode(dataset[indices]).latent_dist.sample() * scaling_factor`` [n, C, h, w] from the cached moments: the misses
        are encoded first (fill), the normals are drawn as VAEEncoder.encode draws them -- torch.randn((n, C, h, w), device=...,
        generator=generator), f32 -- and one launch samples the rows."""
        arr = self._indices(indices)
        if arr.size > MAX_BATCH:
            raise ValueError(f"{self.name}: {arr.size} indices in one batch: at most {MAX_BATCH}")
        self.fill(arr)
        if not self.filled[arr].all():
            raise RuntimeError(f"{self.name}: indices {arr[~self.filled[arr]][:8].tolist()} are not filled after the miss pass")
        idx = self._to_device(torch.from_numpy(arr))
        eps = torch.randn((arr.size, *self.latent_shape), device=self.device, generator=generator)
        return latent_sample(self.moments, idx, eps, float(self.encoder.cfg.scaling_factor), out_dtype)

    # -- persistence
    def fingerprint(self):
        return fingerprint(self.encoder, self.dataset, self.latent_shape)

    def save(self, path):
        """The filled rows as safetensors (`moments` [K, 2C, h, w] f32 in index order, `filled` [N] uint8) with the JSON metadata
        {format, fingerprint, n, latent_shape} in the file's header.  Written beside `path` first, then moved over it."""
        from safetensors.torch import save_file
        rows = np.flatnonzero(self.filled)
        mom = self.moments[torch.from_numpy(rows).to(self.device)].cpu().contiguous()
        meta = dict(format=FORMAT, fingerprint=self.fingerprint(), n=self.n, latent_shape=list(self.latent_shape))
        d = os.path.dirname(os.path.abspath(str(path)))
        os.makedirs(d, exist_ok=True)
        tmp = f"{path}.tmp{os.getpid()}"
        save_file({"moments": mom, "filled": torch.from_numpy(self.filled.astype(np.uint8))}, tmp,
                  metadata={"latent_cache": json.dumps(meta)})
        os.replace(tmp, str(path))
        return len(rows)

    def load(self, path):
        """Take the rows of a file save() wrote, when it belongs to this (encoder, dataset, transform, latent shape).  A missing
        file, or one that does not belong, is not used: the reason is printed and False returned."""
        from safetensors import safe_open
        path = str(path)

        def refuse(why):
            print(f"[siss_amd] {self.name}: {path} is not used: {why}")
            return False

        if not os.path.isfile(path):
            return refuse("no such file (it is written at the end of the run)")
        try:
            with safe_open(path, framework="pt", device="cpu") as f:
                meta = json.loads((f.metadata() or {}).get("latent_cache") or "null")
                if not isinstance(meta, dict):
                    return refuse("no latent_cache metadata in its header")
                if meta.get("format") != FORMAT:
                    return refuse(f"format {meta.get('format')!r}, this build reads {FORMAT}")
                if meta.get("n") != self.n or tuple(meta.get("latent_shape") or ()) != self.latent_shape:
                    return refuse(f"it holds {meta.get('n')} images of latent shape {meta.get('latent_shape')}, the dataset has "
                                  f"{self.n} of {list(self.latent_shape)}")
                want = self.fingerprint()
                if meta.get("fingerprint") != want:
                    return refuse(f"fingerprint {str(meta.get('fingerprint'))[:16]}... differs from {want[:16]}... (the encoder's "
                                  "weights, an image file, the transform or the latent shape changed)")
                filled, mom = f.get_tensor("filled").numpy().astype(bool), f.get_tensor("moments")
        except Exception as e:                               # a truncated / foreign file: not used, loudly
            return refuse(f"{type(e).__name__}: {e}")
        rows = np.flatnonzero(filled)
        if filled.shape != (self.n,) or tuple(mom.shape) != (len(rows), *self.moments.shape[1:]) or mom.dtype != torch.float32:
            return refuse(f"moments {tuple(mom.shape)} {mom.dtype} for {len(rows)} filled rows of {filled.shape[0]}")
        if len(rows):
            self.moments.index_copy_(0, torch.from_numpy(rows).to(self.device), mom.to(self.device))
        self.filled |= filled
        print(f"[siss_amd] {self.name}: {len(rows)} of {self.n} rows read from {path}")
        return True

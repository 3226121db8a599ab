"""Image store of the pixel-space tasks (OPT-IN: ``image_store.enabled`` of config/delete_celeb.yaml, delete_tshirt.yaml and
train_tshirt_mnist.yaml).

The pixel-space loops pay for their input on the host at every micro-batch: a decode per image, ToTensor / Normalize in numpy /
torch, a stack of f32 images and a host-to-device copy of 4 bytes per sub-pixel.  An image's bytes never change and the transform
of these datasets is a fixed per-channel map of a byte, so an ``ImageStore`` keeps the dataset on the device as uint8 -- one planar
row per image, a file dataset filled the first time an image is drawn -- and turns a batch of dataset INDICES into the batch of
training images with one launch (csrc/image_store.hip ``siss_image_gather``) through a [C, 256] table.  The table is the dataset's
OWN transform object applied to every byte value on the host, so the batch has the bits of ``torch.stack([dataset[i] for i in
idx])`` by construction; the data path draws no random numbers, so the loop's generator stream does not move either.

There is no fallback: a dataset without a rule for its raw bytes or a transform that is not a per-channel byte map is refused
(TypeError), a dataset that does not fit ``max_bytes`` is refused at construction.  The host logic (raw_u8, byte_table,
parse_config, host_indices) needs no GPU.
"""
import numpy as np
import torch

from . import lib
from .data import CelebAHQ, Compose, HFDataset, ImagesOnly, IndexBatch, Normalize, ToTensor, index_batches  # noqa: F401

DEFAULT_MAX_BYTES = 8 << 30     # as the latent cache's
DEFAULT_WORKERS = 4
STAGING_ROWS = 16               # first size of the pinned staging buffer, in images; it grows to the largest miss batch seen
MAX_BATCH = 65535               # grid.y of the launch
MAX_CHANNELS = 32               # the table is held in LDS, 1 KB per channel
CONFIG_KEYS = ("enabled", "max_bytes", "workers")


# ---------------------------------------------------------------- the launch
def gather_blocks(n, chw):
    """Blocks per sample of siss_image_gather: one per 4096 elements (four dword sweeps of 256 lanes: the block's C KB table fill is
    paid once per 4 KB read and 16 KB written), the grid capped at 2048 blocks as latent_cache.sample_blocks caps it; the rest is
    grid-strided."""
    return max(1, min(-(-chw // 4096), 2048 // n, 1024))


def image_gather(store, idx, table, out_dtype=torch.float32, out=None, nblk=None):
    """out[i, c] = table[c][store[idx[i], c]]: store [rows, C, H, W] uint8 (a contiguous view may start at any byte), idx [n] int64
    ON THE DEVICE, table [C, 256] f32; out [n, C, H, W] f32 or bf16 (the table value rounded to nearest even).  An index outside
    [0, rows) is not read: its output row is NaN (ImageStore validates on the host before it launches)."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype {out_dtype}: f32 or bf16 are written")
    n = idx.numel()
    if not 0 < n <= MAX_BATCH:
        raise ValueError(f"{n} samples in one launch: 1..{MAX_BATCH} are taken")
    assert store.dtype == torch.uint8 and idx.dtype == torch.int64 and table.dtype == torch.float32
    assert store.dim() == 4 and store.is_contiguous() and idx.is_contiguous() and table.is_contiguous() and idx.dim() == 1
    rows, C, H, W = store.shape
    assert tuple(table.shape) == (C, 256) and idx.device == store.device == table.device
    if not 0 < C <= MAX_CHANNELS:
        raise ValueError(f"{C} channels: 1..{MAX_CHANNELS} are taken (the table is held in LDS)")
    out = torch.empty((n, C, H, W), dtype=out_dtype, device=store.device) if out is None else out
    assert out.dtype == out_dtype and out.is_contiguous() and tuple(out.shape) == (n, C, H, W) and out.device == store.device
    lib.call("siss_image_gather", store, idx, table, out, int(out_dtype == torch.bfloat16), rows, n, C, H * W,
             gather_blocks(n, C * H * W) if nblk is None else int(nblk))
    return out


# ---------------------------------------------------------------- host logic (no GPU)
def _unwrap(ds):
    while isinstance(ds, ImagesOnly):
        ds = ds.dataset
    return ds


def has_rule(ds):
    """Whether raw_u8 knows the dataset (after ImagesOnly): image files decoded to RGB bytes, or one uint8 array in memory."""
    return isinstance(_unwrap(ds), (CelebAHQ, HFDataset))


def source_name(ds, i):
    """What image i is called in an error message: its file, or its row."""
    ds = _unwrap(ds)
    return ds.paths[i] if isinstance(ds, CelebAHQ) else f"row {i} of {type(ds).__name__}"


def raw_u8(ds, i):
    """Image i of the dataset as its transform receives it, as a uint8 [C, H, W] array: CelebAHQ -- the RGB image CelebAHQ.load
    opens (the call __getitem__ makes); HFDataset -- images[i], a 2-D image with C = 1; ImagesOnly is looked through.  A dataset
    whose items are not bytes (SyntheticImages, TensorImages, SDData's float images, anything else) has no rule: TypeError."""
    ds = _unwrap(ds)
    if isinstance(ds, CelebAHQ):
        a = np.asarray(ds.load(int(i)))
    elif isinstance(ds, HFDataset):
        a = ds.images[int(i)]
    else:
        raise TypeError(f"image store: no rule for the raw bytes of a dataset of type {type(ds).__name__} (CelebAHQ image files or "
                        "an HFDataset uint8 array)")
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise TypeError(f"image store: {source_name(ds, int(i))} is {a.dtype} {a.shape}, a uint8 [H, W] or [H, W, C] image is needed")
    if a.ndim == 2:
        a = a[:, :, None]
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def byte_table(transform, C):
    """[C, 256] f32: table[c, v] = the transform of byte value v in channel c, computed by applying the transform OBJECT to a uint8
    image that holds every byte value in every channel -- nothing is re-derived, so whatever the transform rounds, the table rounds
    alike.  Recognised, because they are per-channel maps of a byte: ToTensor() alone and Compose([ToTensor(), Normalize(mean,
    std)]) with mean / std of length 1 or C.  Anything else, None included, raises TypeError with the transform's repr."""
    C = int(C)

    def refuse(why):
        return TypeError(f"image store: the transform {transform!r} {why}; ToTensor() or Compose([ToTensor(), Normalize(mean, std)]) "
                         f"with mean / std of length 1 or {C} are taken")

    members = transform.transforms if type(transform) is Compose else [transform]
    if not 1 <= len(members) <= 2 or type(members[0]) is not ToTensor or (len(members) == 2 and type(members[1]) is not Normalize):
        raise refuse("is not a per-channel map of a byte this store knows")
    if len(members) == 2:
        norm = members[1]
        if len(norm.mean) != len(norm.std) or len(norm.mean) not in (1, C):
            raise refuse(f"normalises {len(norm.mean)} / {len(norm.std)} channels, the images have {C}")
    if not 0 < C <= MAX_CHANNELS:
        raise ValueError(f"image store: {C} channels: 1..{MAX_CHANNELS} are taken")
    ramp = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 1, C)))     # HWC, H = 256
    t = transform(ramp[:, :, 0] if C == 1 else ramp)
    if not torch.is_tensor(t) or tuple(t.shape) != (C, 256, 1) or t.dtype != torch.float32:
        raise refuse(f"maps a [256, 1, {C}] uint8 image to {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return t.reshape(C, 256).contiguous()


def parse_config(block):
    """The `image_store` block of a config: None when it is null or not enabled, else {max_bytes, workers} (None = the default).
    Anything but null or a mapping of enabled / max_bytes / workers raises."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"image_store={block!r}: null or a mapping {{enabled, max_bytes, workers}} is needed")
    unknown = sorted(set(block) - set(CONFIG_KEYS))
    if unknown:
        raise ValueError(f"image_store: unknown keys {unknown} (enabled, max_bytes, workers)")
    if not block.get("enabled"):
        return None
    return dict(max_bytes=block.get("max_bytes"), workers=block.get("workers"))


def host_indices(indices, n, name="image store"):
    """The indices as a host int64 array, validated: integers (a list / IndexBatch, a numpy array or a HOST tensor of an integer
    type) within [0, n).  A device tensor is refused: reading it would synchronise."""
    if torch.is_tensor(indices):
        if indices.device.type != "cpu":
            raise TypeError(f"{name}: indices on {indices.device}: host indices are needed (the misses are looked up on the host, "
                            "without a device synchronisation)")
        arr = indices.numpy()
    else:
        arr = np.asarray(indices)
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError(f"{name}: a non-empty one-dimensional batch of indices is needed, got shape {arr.shape}")
    if arr.dtype.kind not in "iu":
        raise TypeError(f"{name}: indices of dtype {arr.dtype}: integers are needed")
    arr = arr.astype(np.int64)
    bad = arr[(arr < 0) | (arr >= n)]
    if bad.size:
        raise IndexError(f"{name}: indices {bad[:8].tolist()} outside [0, {n})")
    return arr


# ---------------------------------------------------------------- the store
class ImageStore:
    """The raw images of `dataset`, [N, C, H, W] uint8 on the device, and the [C, 256] table of its transform.

    An HFDataset (one uint8 array in memory) is uploaded whole at construction.  A file dataset is filled lazily: the misses of a
    batch are decoded on `workers` threads into a pinned staging buffer, copied and scattered into their rows on the current stream
    (the first image is decoded at construction, for the shape, and kept).  max_bytes: the budget the FULL store must fit -- refused
    otherwise, with the count.  out_dtype: f32 (what the loops take) or bf16.  Counters: `decoded` images that went through raw_u8 in
    this process, `launches` of siss_image_gather."""

    def __init__(self, dataset, device="cuda", max_bytes=None, workers=None, out_dtype=torch.float32, name="image store"):
        from concurrent.futures import ThreadPoolExecutor
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{name}: out_dtype {out_dtype}: f32 or bf16 are written")
        self.dataset, self.name, self.out_dtype = dataset, name, out_dtype
        self.n = len(dataset)
        if self.n <= 0:
            raise ValueError(f"{name}: an empty dataset")
        base = _unwrap(dataset)
        self.decoded = self.launches = 0
        whole = isinstance(base, HFDataset)
        if whole:
            (H, W), C = base.images.shape[1:3], (base.images.shape[3] if base.images.ndim == 4 else 1)
        else:
            first = raw_u8(base, 0)                           # (a dataset without a rule raises here, naming its type)
            C, H, W = first.shape
        self.shape = (int(C), int(H), int(W))
        self.table_host = byte_table(getattr(base, "transform", None), C)
        self.max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
        self.nbytes = self.n * C * H * W
        if self.nbytes > self.max_bytes:
            raise MemoryError(f"{name}: {self.n} images x {C} x {H} x {W} uint8 take {self.nbytes} bytes, more than "
                              f"image_store.max_bytes = {self.max_bytes}; raise the budget or run with the store off")
        self.device = torch.device(device)
        self.workers = DEFAULT_WORKERS if workers is None else int(workers)
        if self.workers <= 0:
            raise ValueError(f"{name}: workers = {self.workers}: a positive count is needed")
        self.table = self.table_host.to(self.device)
        self.filled = np.zeros(self.n, dtype=bool)            # host side: a lookup never asks the device
        self.pool = self.staging = self._staged = None
        if whole:
            a = base.images if base.images.ndim == 4 else base.images[:, :, :, None]
            self.store = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(self.device)
            self.filled[:] = True
        else:
            # The rows are this object's own allocation, made once and kept for its lifetime, and every batch is allocated and
            # consumed on the current stream: no block changes hands between streams, so the hazard Prefetcher.__next__ guards
            # against with record_stream (a raw-pointer kernel reading a block its pool already took back) does not arise here.
            self.store = torch.zeros((self.n, C, H, W), dtype=torch.uint8, device=self.device)
            self.pool = ThreadPoolExecutor(max_workers=self.workers)
            self._stage([0], [first])
            self.decoded = 1

    # -- filling
    def _decode_into(self, job):
        slot, i = job
        a = raw_u8(self.dataset, i)
        if a.shape != self.shape:
            raise ValueError(f"{self.name}: {source_name(self.dataset, i)} is {a.shape[1]} x {a.shape[2]} with {a.shape[0]} channels, "
                             f"the store holds {self.shape[1]} x {self.shape[2]} with {self.shape[0]} (all images of a dataset must "
                             "share one shape)")
        self._staging_np[slot] = a

    def _staging(self, m):
        """The pinned staging buffer with room for m images, free to be written: the copy that last read it has completed."""
        if self._staged is not None:
            self._staged.synchronize()                        # the buffer is not reused (or dropped) before its copy is done
            self._staged = None
        if self.staging is None or self.staging.shape[0] < m:
            rows = max(STAGING_ROWS, 1 << (m - 1).bit_length())
            self.staging = torch.empty((rows, *self.shape), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
            self._staging_np = self.staging.numpy()
        return self.staging

    def _stage(self, rows, images=None):
        """Decode the images of `rows` (or take them from `images`) into the staging buffer, copy them and scatter them into their
        rows on the current stream; an event marks the end of the copy."""
        m = len(rows)
        staging = self._staging(m)
        if images is None:
            list(self.pool.map(self._decode_into, enumerate(rows)))       # (list: a worker's exception surfaces here)
            self.decoded += m
        else:
            for slot, a in enumerate(images):
                self._staging_np[slot] = a
        dev = staging[:m].to(self.device, non_blocking=True)
        where = torch.tensor(rows, dtype=torch.int64)
        if self.device.type == "cuda":
            where = where.pin_memory()
        self.store.index_copy_(0, where.to(self.device, non_blocking=True), dev)
        if self.device.type == "cuda":
            self._staged = torch.cuda.Event()
            self._staged.record(torch.cuda.current_stream(self.device))
        self.filled[rows] = True

    def misses(self, arr):
        """The distinct indices of `arr` that are not filled yet, in order of first appearance."""
        seen, out = set(), []
        for i in arr.tolist():
            if not self.filled[i] and i not in seen:
                seen.add(i)
                out.append(i)
        return out

    @torch.no_grad()
    def fill(self, indices):
        """Decode the images of `indices` that are not stored yet, each once, and write their rows.  Returns the misses."""
        miss = self.misses(host_indices(indices, self.n, self.name))
        if miss:
            self._stage(miss)
        return miss

    # -- the front end of a micro-batch
    @torch.no_grad()
    def images(self, indices):
        """``torch.stack([dataset[i] for i in indices])`` on the device, [n, C, H, W] in out_dtype, the same bits: the indices are
        validated on the host, the misses filled, the indices copied, and one launch gathers the rows through the table."""
        arr = host_indices(indices, self.n, self.name)
        if arr.size > MAX_BATCH:
            raise ValueError(f"{self.name}: {arr.size} indices in one batch: at most {MAX_BATCH}")
        miss = self.misses(arr)
        if miss:
            self._stage(miss)
        idx = torch.from_numpy(arr)
        if self.device.type == "cuda":
            idx = idx.pin_memory()
        out = image_gather(self.store, idx.to(self.device, non_blocking=True), self.table, self.out_dtype)
        self.launches += 1
        return out

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=False, cancel_futures=True)

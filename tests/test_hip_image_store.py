"""The image store on the GPU: siss_image_gather (csrc/image_store.hip) against the host transform (tests/image_store_ref.py), its
grid / alignment / bad-index / refusal behaviour, ImageStore on a file dataset (what is decoded when, one launch per batch, the
bits of the stacked batch), and DeleteTShirt / TrainUnconditional end to end with the store off and on.  The reference is the host
transform and every comparison is torch.equal: there are no tolerances in the kernel and store tests."""
import json
import os

import pytest
import torch

import image_store_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _table(C):
    """Per-channel rows that differ (CIFAR's triple for C = 3), from the transform object, as the store builds it."""
    from siss_amd.image_store import byte_table
    return byte_table(R.transforms(C)["cifar" if C == 3 else "half1"], C)


def _idx(values, dev):
    return torch.tensor(values, dtype=torch.int64, device=dev)


def _index_vectors(rows):
    """{name: indices}: n = 1, 5 and one larger than rows; a constant (the forget batch), a reversed range, repeats."""
    r = rows
    return {"n=1": [r - 1], "constant": [r // 2] * 5, "reversed": [(r - 1 - k) % r for k in range(5)],
            "repeats": [0, r - 1, 0, r // 2, r - 1], "n>rows": [(3 * k + 1) % r for k in range(r + 3)]}


# ---------------------------------------------------------------- 1. the kernel
@DTYPES
@pytest.mark.parametrize("C,H,W,rows", [(1, 5, 7, 8), (3, 6, 6, 8), (1, 32, 32, 3), (3, 32, 32, 3), (3, 32, 32, 1)],
                         ids=["odd", "mult4", "aligned1", "aligned3", "onerow"])
def test_image_gather_is_the_host_transform(dev, C, H, W, rows, out_dtype):
    """out[i, c] = table[c][store[idx[i], c]] against the host lookup through the table the transform object produced; bf16 against
    torch's cast of it.  chw = 35 (odd: one element per lane), 108 (a multiple of 4, not of 16: quads that straddle two channels,
    hw = 36), 1024 and 3072 (aligned); every byte value in every channel of the store."""
    from siss_amd.image_store import image_gather
    store, table = R.all_bytes_store(rows, C, H, W), _table(C)
    assert (C * H * W) % 4 == (3 if (C, H, W) == (1, 5, 7) else 0) and ((C * H * W) % 16 != 0) == (H < 32)
    d_store, d_table = store.to(dev), table.to(dev)
    for name, idx in _index_vectors(rows).items():
        got = image_gather(d_store, _idx(idx, dev), d_table, out_dtype)
        want = R.gather(store, idx, table, out_dtype)
        assert got.dtype == out_dtype and tuple(got.shape) == (len(idx), C, H, W), name
        assert torch.equal(got.cpu(), want), name
    if rows > 1:                                         # negative control: the rows taken in order instead of through idx
        wrong = R.gather(store, list(range(5)), table, out_dtype)
        assert not torch.equal(image_gather(d_store, _idx(_index_vectors(rows)["reversed"], dev), d_table, out_dtype).cpu(), wrong)


@DTYPES
def test_image_gather_same_bits_for_every_grid(dev, out_dtype):
    """chw = 3 * 40 * 40 = 4800: two blocks per sample by default; 1 block (5 sweeps of the loop), 3, 7 and 1024 give the same."""
    from siss_amd.image_store import gather_blocks, image_gather
    store, table = R.all_bytes_store(4, 3, 40, 40).to(dev), _table(3).to(dev)
    idx = _idx([3, 0, 0, 2, 1], dev)
    assert gather_blocks(5, 4800) == 2 and gather_blocks(16, 3 * 256 * 256) == 48 and gather_blocks(128, 1024) == 1
    want = image_gather(store, idx, table, out_dtype)
    assert torch.equal(want.cpu(), R.gather(store.cpu(), [3, 0, 0, 2, 1], table.cpu(), out_dtype))
    for nblk in (1, 3, 7, 1024):
        assert torch.equal(want, image_gather(store, idx, table, out_dtype, nblk=nblk)), nblk


@DTYPES
def test_image_gather_misaligned_views_take_the_scalar_path(dev, out_dtype):
    """A shape that vectorises (chw = 3072): the store's base pointer 1, 2 and 3 bytes off, then out one element off its 16-B
    (bf16: 8-B) alignment: the launcher takes one element per lane, and the bits are the same."""
    from siss_amd.image_store import image_gather
    store, table = R.all_bytes_store(3, 3, 32, 32).to(dev), _table(3).to(dev)
    idx = _idx([2, 0, 0, 2, 1], dev)
    want = image_gather(store, idx, table, out_dtype)
    assert store.data_ptr() % 4 == 0 and want.data_ptr() % 16 == 0
    for k in (1, 2, 3):
        buf = torch.empty(store.numel() + 4, dtype=torch.uint8, device=dev)
        view = buf[k:k + store.numel()].view(store.shape)
        view.copy_(store)
        assert view.data_ptr() % 4 == k and view.is_contiguous()
        assert torch.equal(image_gather(view, idx, table, out_dtype), want), k
    obuf = torch.empty(want.numel() + 1, dtype=out_dtype, device=dev)
    out = obuf[1:].view(want.shape)
    assert out.data_ptr() % (8 if out_dtype == torch.bfloat16 else 16) != 0
    got = image_gather(store, idx, table, out_dtype, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)


@DTYPES
@pytest.mark.parametrize("C,H,W", [(3, 8, 8), (1, 5, 7)], ids=["vec", "scalar"])
def test_image_gather_bad_indices_give_nan_rows_and_touch_nothing_else(dev, C, H, W, out_dtype):
    """idx = -1 and idx = rows are not dereferenced: their output rows are NaN, the other rows are what they are without them, and
    the guard regions around out are unchanged.  The store sits inside a larger buffer whose bytes before and after it map to
    finite table values, so a read of the row before or after the store would show as a finite value instead of NaN."""
    from siss_amd.image_store import image_gather
    rows, n, chw = 8, 5, C * H * W
    store, table = R.all_bytes_store(rows, C, H, W).to(dev), _table(C).to(dev)
    pad = 4 * chw                                        # whole rows on either side; a multiple of 4 bytes when chw is
    sbuf = torch.full((2 * pad + store.numel(),), 7, dtype=torch.uint8, device=dev)
    sview = sbuf[pad:pad + store.numel()].view(store.shape)
    sview.copy_(store)
    obuf = torch.full((2 * pad + n * chw,), 5.0, device=dev).to(out_dtype)
    out = obuf[pad:pad + n * chw].view(n, C, H, W)
    good = image_gather(sview, _idx([2, 0, 0, 7, 1], dev), table, out_dtype)
    before_s, before_o = sbuf.clone(), obuf.clone()
    got = image_gather(sview, _idx([2, -1, 0, rows, 1], dev), table, out_dtype, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(got[3]).all())
    for i in (0, 2, 4):
        assert torch.equal(got[i], good[i]) and bool(torch.isfinite(got[i].float()).all()), i
    assert torch.equal(sbuf, before_s)
    assert torch.equal(obuf[:pad], before_o[:pad]) and torch.equal(obuf[pad + n * chw:], before_o[pad + n * chw:])
    far = image_gather(sview, _idx([1 << 40, -(1 << 40), 0, 0, 0], dev), table, out_dtype)
    assert bool(torch.isnan(far[:2]).all()) and torch.equal(far[2], got[2])


def test_image_gather_row_offsets_past_2_31_bytes(dev):
    """A store of 11000 rows of the CelebA shape (2.16 GB): rows whose byte offset is past 2^31 and the last row are read where
    they are.  Only the rows that are read are written; the output is three images."""
    from siss_amd.image_store import image_gather
    C, H, W, rows = 3, 256, 256, 11000
    assert 10923 * C * H * W > 1 << 31
    table = _table(3)
    store = torch.empty((rows, C, H, W), dtype=torch.uint8, device=dev)
    some = R.all_bytes_store(3, C, H, W)
    store[0], store[10923], store[rows - 1] = some[0].to(dev), some[1].to(dev), some[2].to(dev)
    got = image_gather(store, _idx([rows - 1, 10923, 0], dev), table.to(dev))
    assert torch.equal(got.cpu(), R.gather(some, [2, 1, 0], table))


def test_image_gather_refusals_leave_out_untouched(dev):
    from siss_amd import lib
    from siss_amd.image_store import image_gather
    store = torch.zeros(3, 2, 4, 4, dtype=torch.uint8, device=dev)
    table = torch.ones(2, 256, device=dev)
    idx = _idx([0, 1], dev)
    out = torch.full((2, 2, 4, 4), float("nan"), device=dev)
    ok = (store, idx, table, out, 0, 3, 2, 2, 16, 1)      # store, idx, table, out, out_bf16, rows, n, C, hw, nblk
    assert lib.PARAMS["siss_image_gather"] == ("store", "idx", "table", "out", "out_bf16", "rows", "n", "C", "hw", "nblk", "stream")
    bad = {"store": (None, *ok[1:]), "idx": (store, None, *ok[2:]), "table": (*ok[:2], None, *ok[3:]), "out": (*ok[:3], None, *ok[4:]),
           "out_bf16": (*ok[:4], 2, *ok[5:]), "rows = 0": (*ok[:5], 0, *ok[6:]), "rows < 0": (*ok[:5], -3, *ok[6:]),
           "n = 0": (*ok[:6], 0, *ok[7:]), "n < 0": (*ok[:6], -1, *ok[7:]), "n > 65535": (*ok[:6], 65536, *ok[7:]),
           "C = 0": (*ok[:7], 0, *ok[8:]), "C > 32": (*ok[:7], 33, *ok[8:]), "hw = 0": (*ok[:8], 0, ok[9]),
           "hw < 0": (*ok[:8], -16, ok[9]), "C * hw > 2^30": (*ok[:8], (1 << 29) + 1, ok[9]), "nblk = 0": (*ok[:9], 0),
           "nblk > 1024": (*ok[:9], 1025), "out off its element": (*ok[:3], out.data_ptr() + 2, *ok[4:])}
    for what, args in bad.items():
        with pytest.raises(RuntimeError, match="status 1"):
            lib.call("siss_image_gather", *args)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), what        # nothing was launched
    with pytest.raises(ValueError, match="65535"):
        image_gather(store, _idx([], dev), table)
    with pytest.raises(TypeError, match="f32 or bf16"):
        image_gather(store, idx, table, out_dtype=torch.float16)
    lib.call("siss_image_gather", *ok)
    assert bool((out == 1).all())


# ---------------------------------------------------------------- 2. ImageStore on a file dataset
@DTYPES
def test_image_store_decodes_each_drawn_image_once_and_launches_once_per_batch(dev, tmp_path, out_dtype):
    """A CelebAHQ directory of 40 PNGs of 9 x 7 (chw = 189: the scalar path; one single-channel file), its open function counted.
    Batches that share indices: each drawn image is opened exactly once by the store, there is one launch per batch, a batch is
    torch.stack([ds[i] for i in idx]) on the device, and a batch of 21 distinct misses outgrows the staging buffer's first size."""
    from siss_amd.data import CelebAHQ
    from siss_amd.image_store import STAGING_ROWS, ImageStore
    R.write_png_dir(tmp_path / "img", 40, 9, 7, gray={5})
    ds = CelebAHQ("all", str(tmp_path / "img"), [], transform=R.transforms(3)["cifar"])
    opened = []
    inner = ds._open
    ds._open = lambda p: opened.append(os.path.basename(p)) or inner(p)
    store = ImageStore(ds, device=dev, workers=3, out_dtype=out_dtype)
    assert store.shape == (3, 9, 7) and store.store.device.type == "cuda" and store.staging.shape[0] == STAGING_ROWS == 16
    assert opened == ["000.png"] and store.decoded == 1 and store.filled.sum() == 1       # the shape probe, kept
    batches = [[0, 3, 3, 5], [5] * 6, [3, 0, 7, 5], list(range(19, 40)), [39, 8, 0, 21], [7]]
    seen = 0
    for k, idx in enumerate(batches):
        got = store.images(idx)
        seen = len(opened)
        want = torch.stack([ds[i] for i in idx]).to(out_dtype)           # (opens the files again: not the store's doing)
        del opened[seen:]
        assert got.dtype == out_dtype and got.device.type == "cuda" and torch.equal(got.cpu(), want), k
        assert store.launches == k + 1
    drawn = sorted({i for b in batches for i in b})
    assert sorted(opened) == [f"{i:03d}.png" for i in drawn] and store.decoded == len(drawn)          # once each
    assert store.filled.tolist() == [i in drawn for i in range(40)]
    assert store.staging.shape[0] == 32                  # grew for the 21 misses of the fourth batch
    assert bool((store.store[1] == 0).all())             # a row that was never drawn
    with pytest.raises(IndexError):
        store.images([0, 40])
    with pytest.raises(TypeError, match="host indices"):
        store.images(torch.tensor([0], device=dev))
    assert store.launches == len(batches) and len(opened) == len(drawn)
    store.close()


def test_image_store_uploads_an_in_memory_dataset_whole(dev, tmp_path):
    from siss_amd.data import HFDataset, IndexBatch
    from siss_amd.image_store import ImageStore
    R.write_npz(tmp_path / "ds", 20, 28, 28)
    ds = HFDataset("all", str(tmp_path / "ds"), "train", transform=R.transforms(1)["half1"])
    store = ImageStore(ds, device=dev)
    assert store.filled.all() and store.decoded == 0 and store.pool is None and tuple(store.store.shape) == (20, 1, 28, 28)
    idx = IndexBatch([19, 0, 7, 7, 3])
    assert torch.equal(store.images(idx).cpu(), torch.stack([ds[i] for i in idx])) and store.launches == 1 and store.decoded == 0


# ---------------------------------------------------------------- 3. the task loops end to end
UNET = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
            down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"], layers_per_block=1)


def _record(monkeypatch, cls, fed):
    """Every micro_step of `cls` appends clones of its tensor arguments (x0, a0, noise, t, u -- or x0, noise, t) to `fed`."""
    inner = cls.micro_step

    def micro_step(self, *args, **kw):
        fed.append([a.clone() for a in args if torch.is_tensor(a)])
        return inner(self, *args, **kw)
    monkeypatch.setattr(cls, "micro_step", micro_step)


def _lines(cfg):
    return [{k: v for k, v in json.loads(l).items() if k != "elapsed_s"}
            for l in open(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"))]


def _compare(fed_on, fed_off, on, off, exact_keys):
    """What the store can change is what the loop hands the step, and that is asserted BITWISE, micro-batch by micro-batch.  The
    logged scalars are compared only as far as one run agrees with itself: the step does not reproduce its own scalars from equal
    inputs (its gradient kernels add with float atomics -- DESIGN.md says the same of the latent cache, whose test measured
    differences of one ulp between two runs of the same configuration), so the counters are asserted exactly, the rest is held to
    parity_util.SCALAR_RTOL, and whether they were equal is printed."""
    from parity_util import SCALAR_RTOL
    assert len(fed_on) == len(fed_off) > 0
    for k, (a, b) in enumerate(zip(fed_on, fed_off)):
        assert len(a) == len(b)
        for j, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, j)
    assert len(on) == len(off) > 0
    print(f"\nevery logged scalar equal with the store on and off: {on == off}")
    for a, b in zip(on, off):
        assert set(a) == set(b) and all(a[k] == b[k] for k in exact_keys)
        for k in set(a) - set(exact_keys):
            assert a[k] == b[k] or (isinstance(b[k], float) and abs(a[k] - b[k]) <= SCALAR_RTOL * abs(b[k])), (k, a[k], b[k])


def _delete_tshirt(tmp_path, name, extra):
    from siss_amd import hydra_lite as H
    ds = ["_target_=data.src.hf_dataset.HFDataset", f"name={tmp_path}/ds", "split=train", "class_to_remove=10"]
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    ["training_steps=3", "train_batch_size=4", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "save_final=false", "mixed_precision=bf16",
                     "+dataloader_num_workers=1", *[f"+dataset_all.{o}" for o in ds], "+dataset_all.filter=all",
                     *[f"+dataset_deletion.{o}" for o in ds], "+dataset_deletion.filter=deletion", *extra])
    cfg.unet = dict(UNET)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.run()
    return task, cfg


def test_delete_tshirt_image_store_end_to_end(dev, tmp_path, monkeypatch):
    """DeleteTShirt on an npz of 30 images (two of the forget class, fewer than the batch: the forget batch is one image repeated),
    three optimizer steps of one micro-batch of four (one accumulation step keeps the test short; the data path does not know
    about accumulation), store off and on: x0, a0, noise, t and u of every micro-batch bitwise."""
    from siss_amd.image_store import ImageStore
    from siss_amd.step import SISSStepper
    R.write_npz(tmp_path / "ds", 30, 28, 28, labels=[10 if i in (4, 17) else i % 10 for i in range(30)])
    fed_off, fed_on = [], []
    _record(monkeypatch, SISSStepper, fed_off)
    t_off, c_off = _delete_tshirt(tmp_path, "off", [])
    monkeypatch.undo()
    _record(monkeypatch, SISSStepper, fed_on)
    t_on, c_on = _delete_tshirt(tmp_path, "on", ["+image_store.enabled=true"])
    assert t_off.keep_store is None and t_off.forget_store is None
    assert isinstance(t_on.keep_store, ImageStore) and isinstance(t_on.forget_store, ImageStore)
    assert t_on.keep_store.n == 30 and t_on.forget_store.n == 2 and t_on.keep_store.launches == t_on.forget_store.launches == 3
    assert len(fed_on) == 3 and [len(f) for f in fed_on] == [5] * 3 and fed_on[0][0].shape == (4, 1, 28, 28)
    assert fed_on[0][0].dtype == torch.float32 and not torch.equal(fed_on[0][0], fed_on[1][0])
    assert torch.equal(fed_on[0][1][0], fed_on[0][1][3])                  # the forget batch: one image repeated
    _compare(fed_on, fed_off, _lines(c_on), _lines(c_off), ("global_step", "lr"))


def _train(tmp_path, name, extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"),
                    [f"dataset.name={tmp_path}/ds", "num_epochs=2", "train_batch_size=4", f"output_dir={tmp_path}/{name}",
                     "mixed_precision=bf16", "sampling_steps=null", "checkpointing_steps=null", "lr_warmup_steps=2", *extra])
    cfg.unet = dict(UNET)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.run()
    return task, cfg


def test_train_unconditional_image_store_end_to_end(dev, tmp_path, monkeypatch):
    """TrainUnconditional on an npz of 10 images, two epochs of batches 4, 4 and a short last one of 2, store off and on: x0, noise
    and t of every micro-batch bitwise."""
    from siss_amd.train import TrainStepper
    R.write_npz(tmp_path / "ds", 10, 28, 28)
    fed_off, fed_on = [], []
    _record(monkeypatch, TrainStepper, fed_off)
    t_off, c_off = _train(tmp_path, "off", [])
    monkeypatch.undo()
    _record(monkeypatch, TrainStepper, fed_on)
    t_on, c_on = _train(tmp_path, "on", ["+image_store.enabled=true", "+image_store.max_bytes=7840"])
    assert t_off.train_store is None and t_on.train_store.launches == 6 and t_on.train_store.nbytes == 7840
    assert [f[0].shape[0] for f in fed_on] == [4, 4, 2, 4, 4, 2] and [len(f) for f in fed_on] == [3] * 6
    _compare(fed_on, fed_off, _lines(c_on), _lines(c_off), ("step", "epoch"))


def test_delete_sd_refuses_image_store(dev, tmp_path):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"), [f"output_dir={tmp_path}/sd", "+image_store.enabled=true"])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    with pytest.raises(NotImplementedError, match="latent_cache"):
        task.run()
    assert task.keep_store is None and task.keep_cache is None

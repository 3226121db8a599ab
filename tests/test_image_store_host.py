"""Host logic of the image store (siss_amd/image_store.py), no GPU: byte_table against the transform pixel by pixel, raw_u8 + a numpy
lookup against dataset[i], the refusals, the config block, and index_batches against batches.  Every comparison is bitwise."""
import itertools
import os

import numpy as np
import pytest
import torch

import image_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- byte_table
@pytest.mark.parametrize("C", [1, 3])
def test_byte_table_is_the_transform_pixel_by_pixel(C):
    from siss_amd.image_store import byte_table
    seen = []
    for name, tr in R.transforms(C).items():
        got = byte_table(tr, C)
        want = R.table_pixel_by_pixel(tr, C)
        assert got.dtype == torch.float32 and tuple(got.shape) == (C, 256) and got.is_contiguous(), name
        assert torch.equal(got, want), name
        seen.append(got)
    assert not torch.equal(seen[0], seen[1])             # ToTensor alone against Normalize(0.5, 0.5): different tables
    if C == 3:                                           # a per-channel triple gives per-channel rows; a broadcast one does not
        assert torch.equal(seen[1], seen[2]) and not torch.equal(seen[3][0], seen[3][1])
        assert torch.equal(seen[1][0], seen[1][2])


def test_byte_table_refusals():
    from siss_amd.data import Compose, Normalize, ToTensor
    from siss_amd.image_store import byte_table

    class Flip:
        def __call__(self, x):
            return x.flip(-1)

        def __repr__(self):
            return "Flip()"

    with pytest.raises(TypeError, match="None"):
        byte_table(None, 3)
    with pytest.raises(TypeError, match=r"Flip\(\)"):
        byte_table(Compose([ToTensor(), Flip()]), 3)
    with pytest.raises(TypeError, match=r"Flip\(\)"):
        byte_table(Compose([ToTensor(), Normalize([0.5], [0.5]), Flip()]), 3)
    with pytest.raises(TypeError, match=r"Normalize\("):
        byte_table(Normalize([0.5], [0.5]), 1)           # without ToTensor in front
    for C, k in ((1, 3), (3, 2), (3, 4)):                # a Normalize of the wrong length
        with pytest.raises(TypeError, match=f"the images have {C}"):
            byte_table(Compose([ToTensor(), Normalize([0.5] * k, [0.5] * k)]), C)
    with pytest.raises(TypeError, match="the images have 3"):
        byte_table(Compose([ToTensor(), Normalize([0.5] * 3, [0.5])]), 3)


# ---------------------------------------------------------------- raw_u8 + lookup == dataset[i]
def test_raw_u8_and_lookup_equal_celebahq_items(tmp_path):
    """Four 6 x 5 PNGs, one of them a single-channel file that convert("RGB") expands; raw_u8 goes through CelebAHQ.load, the call
    __getitem__ makes (the dataset's open function is counted)."""
    from siss_amd.data import CelebAHQ, ImagesOnly
    from siss_amd.image_store import byte_table, has_rule, raw_u8
    written = R.write_png_dir(tmp_path / "img", 4, 6, 5, gray={2})
    for name, tr in R.transforms(3).items():
        ds = CelebAHQ("all", str(tmp_path / "img"), [], transform=tr)
        opened = []
        inner = ds._open
        ds._open = lambda p: opened.append(p) or inner(p)
        table = byte_table(tr, 3)
        assert has_rule(ds) and len(ds) == 4
        for i in range(4):
            raw = raw_u8(ds, i)
            assert raw.dtype == np.uint8 and raw.shape == (3, 6, 5) and raw.flags["C_CONTIGUOUS"]
            a = written[i] if i != 2 else np.repeat(written[i][:, :, None], 3, axis=2)
            assert np.array_equal(raw, a.transpose(2, 0, 1))
            assert torch.equal(R.lookup(table, raw), ds[i]), (name, i)
        assert opened == [p for p in ds.paths for _ in range(2)]         # once by raw_u8, once by __getitem__
    sub = CelebAHQ("deletion", str(tmp_path / "img"), ["001.png"], transform=tr)
    assert len(sub) == 1 and np.array_equal(raw_u8(sub, 0), written[1].transpose(2, 0, 1))
    assert not has_rule(ImagesOnly(torch.zeros(2, 1, 2, 2)))


@pytest.mark.parametrize("C", [None, 3], ids=["2d", "hwc"])
def test_raw_u8_and_lookup_equal_hfdataset_items_also_through_images_only(tmp_path, C):
    from siss_amd.data import HFDataset, ImagesOnly
    from siss_amd.image_store import byte_table, has_rule, raw_u8
    image, label = R.write_npz(tmp_path / "ds", 12, 7, 5, C=C)
    ch = 1 if C is None else C

    class Labelled(HFDataset):                           # items (image, label): what ImagesOnly is for
        def __getitem__(self, i):
            return super().__getitem__(i), int(self.labels[int(i)])

    for name, tr in R.transforms(ch).items():
        table = byte_table(tr, ch)
        ds = HFDataset("nondeletion", str(tmp_path / "ds"), "train", class_to_remove=10, transform=tr)
        assert len(ds) == 11 and has_rule(ds)
        for i in (0, 5, 10):
            raw = raw_u8(ds, i)
            assert raw.dtype == np.uint8 and raw.shape == (ch, 7, 5)
            assert torch.equal(R.lookup(table, raw), ds[i]), (name, i)
        only = ImagesOnly(Labelled("all", str(tmp_path / "ds"), "train", transform=tr))
        assert has_rule(only)
        for i in (1, 11):
            assert torch.equal(R.lookup(table, raw_u8(only, i)), only[i]), (name, i)
            assert np.array_equal(raw_u8(only, i), image[i][None] if C is None else image[i].transpose(2, 0, 1))


def test_float_valued_datasets_have_no_rule():
    from siss_amd.data import ImagesOnly, SyntheticImages, TensorImages
    from siss_amd.image_store import ImageStore, has_rule, raw_u8
    for ds in (SyntheticImages(4, (1, 8, 8)), TensorImages(torch.zeros(2, 3, 4, 4)), ImagesOnly(SyntheticImages(4, (1, 8, 8)))):
        assert not has_rule(ds)
        with pytest.raises(TypeError, match="no rule"):
            raw_u8(ds, 0)
        with pytest.raises(TypeError, match="no rule"):
            ImageStore(ds, device="cpu")


# ---------------------------------------------------------------- ImageStore's refusals (on the host: nothing is launched)
def test_max_bytes_is_refused_with_the_byte_count(tmp_path):
    from siss_amd.data import CelebAHQ, HFDataset
    from siss_amd.image_store import DEFAULT_MAX_BYTES, ImageStore
    tr = R.transforms(3)["half3"]
    R.write_npz(tmp_path / "ds", 12, 7, 5, C=3)
    ds = HFDataset("all", str(tmp_path / "ds"), "train", transform=tr)
    need = 12 * 3 * 7 * 5
    with pytest.raises(MemoryError, match=f"{need} bytes.*max_bytes = {need - 1}"):
        ImageStore(ds, device="cpu", max_bytes=need - 1)
    store = ImageStore(ds, device="cpu", max_bytes=need)                 # it fits exactly: uploaded whole
    assert store.nbytes == need and store.filled.all() and store.decoded == 0
    assert tuple(store.store.shape) == (12, 3, 7, 5) and store.store.dtype == torch.uint8
    assert np.array_equal(store.store.numpy(), ds.images.transpose(0, 3, 1, 2))
    assert DEFAULT_MAX_BYTES == 8 << 30 and ImageStore(ds, device="cpu").max_bytes == 8 << 30
    R.write_png_dir(tmp_path / "img", 3, 6, 5)
    files = CelebAHQ("all", str(tmp_path / "img"), [], transform=tr)
    with pytest.raises(MemoryError, match=f"{3 * 3 * 6 * 5} bytes"):
        ImageStore(files, device="cpu", max_bytes=100)
    with pytest.raises(TypeError, match="f32 or bf16"):
        ImageStore(ds, device="cpu", out_dtype=torch.float16)


def test_mismatched_image_shapes_raise_naming_the_file(tmp_path):
    from siss_amd.data import CelebAHQ
    from siss_amd.image_store import ImageStore
    R.write_png_dir(tmp_path / "img", 4, 6, 5, size_of={2: (6, 4)})
    ds = CelebAHQ("all", str(tmp_path / "img"), [], transform=R.transforms(3)["totensor"])
    store = ImageStore(ds, device="cpu", workers=2)
    assert store.shape == (3, 6, 5) and store.filled.tolist() == [True, False, False, False] and store.decoded == 1
    assert store.fill([0, 1, 1]) == [1] and store.decoded == 2
    with pytest.raises(ValueError, match=r"002\.png is 6 x 4 .* the store holds 6 x 5"):
        store.fill([3, 2])
    assert not store.filled[2]
    with pytest.raises(IndexError, match=r"\[4\] outside \[0, 4\)"):
        store.fill([4])
    with pytest.raises(IndexError):
        store.fill([-1])
    with pytest.raises(TypeError, match="integers"):
        store.fill([0.5])
    store.close()


def test_image_store_config_block():
    from siss_amd import hydra_lite as H
    from siss_amd.image_store import parse_config
    from siss_amd.tasks import DeleteSD
    assert parse_config(None) is None and parse_config({"enabled": False, "max_bytes": 5}) is None and parse_config({}) is None
    assert parse_config({"enabled": True}) == dict(max_bytes=None, workers=None)
    assert parse_config({"enabled": True, "max_bytes": 1 << 20, "workers": 2}) == dict(max_bytes=1 << 20, workers=2)
    with pytest.raises(ValueError, match=r"unknown keys \['path'\]"):
        parse_config({"enabled": True, "path": "x"})
    with pytest.raises(ValueError, match="unknown keys"):
        parse_config({"enabled": False, "chunk": 4})         # also when it is off
    with pytest.raises(ValueError, match="mapping"):
        parse_config(True)
    for name in ("delete_celeb", "delete_tshirt", "train_tshirt_mnist"):
        assert "image_store" in H.compose(name, os.path.join(ROOT, "config")) and \
            H.compose(name, os.path.join(ROOT, "config")).image_store is None                 # shipped off
        on = H.compose(name, os.path.join(ROOT, "config"), ["+image_store.enabled=true", "+image_store.workers=2"])
        assert parse_config(on.image_store) == dict(max_bytes=None, workers=2)
    sd = H.compose("delete_sd", os.path.join(ROOT, "config"))
    assert "image_store" not in sd
    DeleteSD(sd).check_supported()
    with pytest.raises(NotImplementedError, match="latent_cache"):
        DeleteSD(H.compose("delete_sd", os.path.join(ROOT, "config"), ["+image_store.enabled=true"])).check_supported()


def test_open_image_stores_leaves_synthetic_datasets_alone(capsys):
    from siss_amd import hydra_lite as H
    from siss_amd.data import SyntheticImages
    from siss_amd.tasks import DeleteTShirt
    ds = SyntheticImages(4, (1, 8, 8))
    off = DeleteTShirt(H.compose("delete_tshirt", os.path.join(ROOT, "config")))
    off.open_image_stores(ds, ds, "cpu")
    assert off.keep_store is None and off.forget_store is None and capsys.readouterr().out == ""
    on = DeleteTShirt(H.compose("delete_tshirt", os.path.join(ROOT, "config"), ["+image_store.enabled=true"]))
    on.open_image_stores(ds, ds, "cpu")
    said = capsys.readouterr().out
    assert on.keep_store is None and on.forget_store is None
    assert said.count("\n") == 1 and "image_store.enabled is set but unused" in said and "SyntheticImages" in said
    bad = DeleteTShirt(H.compose("delete_tshirt", os.path.join(ROOT, "config"), ["+image_store.enabled=true", "+image_store.path=x"]))
    with pytest.raises(ValueError, match="unknown keys"):
        bad.open_image_stores(ds, ds, "cpu")


# ---------------------------------------------------------------- index_batches
def test_index_batches_yield_the_index_order_of_batches():
    """On the same sampler: the k-th IndexBatch names the items of the k-th stacked batch (items that carry their own index)."""
    from siss_amd.data import IndexBatch, InfiniteSampler, RepeatedSampler, TensorImages, batches, index_batches
    from siss_amd import latent_cache
    assert latent_cache.IndexBatch is IndexBatch and latent_cache.index_batches is index_batches      # one definition
    ds = TensorImages(torch.arange(10.0).view(10, 1, 1, 1))
    for make in (lambda: InfiniteSampler(ds, seed=3), lambda: InfiniteSampler(ds, rank=1, num_replicas=3),
                 lambda: InfiniteSampler(ds, shuffle=False), lambda: RepeatedSampler(ds, 4)):
        want = list(itertools.islice(batches(ds, make(), 4), 7))
        tag = object()
        got = list(itertools.islice(index_batches(make(), 4, tag), 7))
        assert [b.view(-1).long().tolist() for b in want] == [list(b) for b in got]
        assert all(isinstance(b, IndexBatch) and b.cache is tag and b.to("cuda", non_blocking=True) is b for b in got)

"""CPU tests of the latent cache's host side (siss_amd/latent_cache.py, its wiring in siss_amd/tasks.py): miss bookkeeping, the budget
refusal, index validation, the fingerprint, the save / load round trip with a mismatching file ignored loudly, the index batches'
order, the default batch hooks of _DeleteBase, and the binding's table entries.  A fake encoder stands in for the VAE: its moments
are a fixed function of the image, on the host."""
import os
import types

import numpy as np
import pytest
import torch

import latent_cache_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEncoder:
    """raw_moments(x) [k, 3, H, W] -> [k, 8, H/2, W/2]: a fixed function of each image ALONE, with the calls recorded."""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.cfg = types.SimpleNamespace(latent_channels=4, scaling_factor=0.18215, block_out_channels=(8, 8))
        self.ps = types.SimpleNamespace(flat=torch.randn(64, generator=g))
        self.device = torch.device("cpu")
        self.calls = []

    def raw_moments(self, x):
        self.calls.append(int(x.shape[0]))
        x = x.float()                                                             # elementwise: the same bits in any batch
        pooled = (x[:, :, 0::2, 0::2] + x[:, :, 1::2, 1::2]) * 0.5                # [k, 3, h, w]
        return (pooled[:, [0, 1, 2, 0, 1, 2, 0, 1]] * self.ps.flat[:8].view(1, 8, 1, 1)).contiguous()


def _dataset(n=6, hw=8, seed=1):
    from siss_amd.data import TensorImages
    return TensorImages(torch.rand(n, 3, hw, hw, generator=torch.Generator().manual_seed(seed)) * 2 - 1)


def _cache(n=6, enc=None, ds=None, **kw):
    from siss_amd.latent_cache import LatentCache
    enc = enc or FakeEncoder()
    ds = ds if ds is not None else _dataset(n)
    return LatentCache(enc, ds, (4, 4, 4), device="cpu", **kw), enc, ds


def test_reference_f32_chain_is_within_its_own_bound_of_f64():
    """The two restatements against each other: numpy's f32 chain is within the a-priori bound of the f64 form (clamps acting)."""
    g = torch.Generator().manual_seed(0)
    cache = torch.randn(3, 8, 4, 4, generator=g)
    cache[:, 4:] = 3 * cache[:, 4:] - 2
    cache[0, 4, 0, 0], cache[0, 4, 0, 1] = -40.0, 30.0
    eps = torch.randn(5, 4, 4, 4, generator=g)
    idx = [2, 0, 0, 2, 1]
    got = R.sample_f32(cache.numpy(), idx, eps.numpy(), R.f32(0.18215))
    ref, M, S = R.sample_f64(cache, idx, eps, R.f32(0.18215))
    assert got.dtype == np.float32 and got.shape == (5, 4, 4, 4)
    assert bool(((torch.from_numpy(got).double() - ref).abs() <= 2 * R.sample_bound(M, S)).all())
    # the clamps: exp(0.5 * -30) and exp(0.5 * 20), not exp(-20) / exp(15)
    assert abs(float(ref[1, 0, 0, 0]) - (float(cache[0, 0, 0, 0]) + np.exp(-15.0) * float(eps[1, 0, 0, 0])) * R.f32(0.18215)) < 1e-12
    assert abs(float(ref[1, 0, 0, 1]) / ((float(cache[0, 0, 0, 1]) + np.exp(10.0) * float(eps[1, 0, 0, 1])) * R.f32(0.18215)) - 1) < 1e-12


def test_miss_bookkeeping_encodes_each_image_once_and_only_when_drawn():
    cache, enc, ds = _cache()
    assert cache.moments.shape == (6, 8, 4, 4) and not cache.filled.any() and cache.nbytes == 6 * 8 * 16 * 4
    assert cache.fill([0, 1]) == [0, 1] and enc.calls == [2]
    assert cache.fill([1, 2]) == [2] and enc.calls == [2, 1]
    assert cache.fill([0, 2]) == [] and enc.calls == [2, 1]
    assert cache.fill([0] * 4) == [] and enc.calls == [2, 1]                      # the forget draw: one image repeated
    assert cache.filled.tolist() == [True, True, True, False, False, False] and cache.encoded == 3
    want = FakeEncoder().raw_moments(ds.t[:3])
    assert torch.equal(cache.moments[:3], want) and bool((cache.moments[3:] == 0).all())
    # repeated misses within one call are encoded once, in order of first appearance; chunks of at most `chunk`
    c2, e2, _ = _cache(chunk=2)
    assert c2.fill([5, 3, 5, 3, 4, 0, 5]) == [5, 3, 4, 0] and e2.calls == [2, 2]
    assert torch.equal(c2.moments[[5, 3, 4, 0]], FakeEncoder().raw_moments(ds.t[[5, 3, 4, 0]]))
    c3, e3, _ = _cache(chunk=3)
    c3.fill(torch.arange(6))
    assert e3.calls == [3, 3] and c3.filled.all()
    c3.fill(np.arange(6, dtype=np.int32))
    assert e3.calls == [3, 3]


def test_over_budget_dataset_is_refused_with_the_byte_count():
    from siss_amd.latent_cache import DEFAULT_MAX_BYTES, LatentCache
    assert DEFAULT_MAX_BYTES == 8 << 30
    need = 6 * 8 * 16 * 4
    with pytest.raises(MemoryError, match=rf"{need} bytes.*max_bytes = {need - 1}"):
        _cache(max_bytes=need - 1)
    cache, _, _ = _cache(max_bytes=need)
    assert cache.nbytes == need
    # the SD shapes: 8 GiB hold 65536 images' moments exactly, one more is refused -- before any allocation

    class Many:
        def __len__(self):
            return 65537
    with pytest.raises(MemoryError, match=str(65537 * 8 * 64 * 64 * 4)):
        LatentCache(FakeEncoder(), Many(), (4, 64, 64), device="cpu")
    with pytest.raises(ValueError, match="latent channels"):
        LatentCache(FakeEncoder(), _dataset(), (3, 4, 4), device="cpu")


def test_index_validation_errors():
    cache, enc, _ = _cache()
    for bad in ([6], [-1], [0, 1, 7], torch.tensor([0, 6])):
        with pytest.raises(IndexError, match=r"outside \[0, 6\)"):
            cache.fill(bad)
    for bad in ([0.0, 1.0], torch.tensor([0.0]), np.array([1.5]), torch.tensor([True])):
        with pytest.raises(TypeError, match="integers are needed"):
            cache.fill(bad)
    for bad in ([], [[0, 1]], torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="one-dimensional"):
            cache.fill(bad)
    with pytest.raises(TypeError, match="host indices"):
        cache.fill(torch.empty(2, dtype=torch.int64, device="meta"))           # not on the host: reading it would synchronise
    with pytest.raises(IndexError):
        cache.latents([9])                               # refused before anything is drawn or launched
    assert enc.calls == [] and not cache.filled.any()


def test_fingerprint_follows_image_bytes_transform_encoder_and_shape(tmp_path):
    import json
    from PIL import Image
    from siss_amd.data import Compose, ImagesOnly, Normalize, SDData
    from siss_amd.latent_cache import fingerprint, image_entries, transform_repr
    rng = np.random.default_rng(0)
    d = str(tmp_path) + "/"
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)).save(d + f"im_{i:03d}.png")
    json.dump({f"im_{i:03d}.png": int(i == 2) for i in range(3)}, open(tmp_path / "labels.json", "w"))

    def ds(mean=127.5, flt="all"):
        return ImagesOnly(SDData(d, str(tmp_path / "labels.json"), flt, transform=Compose([Normalize([mean], [127.5])])))
    enc = FakeEncoder()
    base = fingerprint(enc, ds(), (4, 4, 4))
    assert base == fingerprint(FakeEncoder(), ds(), (4, 4, 4)) and len(base) == 64          # a function of the content alone
    assert [n for n, _ in image_entries(ds())] == ["im_000.png", "im_001.png", "im_002.png"]
    assert transform_repr(ds()) == "Compose([Normalize(mean=[127.5], std=[127.5])])"
    assert fingerprint(enc, ds(mean=127.0), (4, 4, 4)) != base                              # the transform
    assert fingerprint(enc, ds(flt="nondeletion"), (4, 4, 4)) != base                       # the set of images
    assert fingerprint(enc, ds(), (4, 8, 8)) != base                                        # the latent shape
    enc2 = FakeEncoder()
    enc2.ps.flat[17] += 1e-3                                                                 # one encoder parameter
    assert fingerprint(enc2, ds(), (4, 4, 4)) != base
    raw = bytearray(open(d + "im_001.png", "rb").read())
    raw[-1] ^= 1                                                                             # one image byte
    open(d + "im_001.png", "wb").write(bytes(raw))
    assert fingerprint(enc, ds(), (4, 4, 4)) != base
    # a tensor stack: one element of one image
    t = _dataset()
    ft = fingerprint(enc, t, (4, 4, 4))
    t2 = _dataset()
    t2.t[3, 1, 2, 2] += 1e-3
    assert fingerprint(enc, t2, (4, 4, 4)) != ft == fingerprint(enc, _dataset(), (4, 4, 4))
    with pytest.raises(TypeError, match="no stable repr"):
        transform_repr(types.SimpleNamespace(transform=object()))
    with pytest.raises(TypeError, match="no rule"):
        image_entries([1, 2])


def test_save_load_round_trip_and_mismatching_file_ignored(tmp_path, capsys):
    from safetensors import safe_open
    cache, enc, ds = _cache()
    cache.fill([4, 1])
    path = tmp_path / "sub" / "keep.safetensors"
    assert cache.save(path) == 2
    with safe_open(str(path), framework="pt") as f:
        assert sorted(f.keys()) == ["filled", "moments"] and "latent_cache" in f.metadata()
        assert f.get_tensor("moments").shape == (2, 8, 4, 4) and f.get_tensor("filled").tolist() == [0, 1, 0, 0, 1, 0]
    assert os.listdir(tmp_path / "sub") == ["keep.safetensors"]                    # no temporary left behind
    fresh, enc2, _ = _cache()
    assert fresh.load(path) is True
    assert "2 of 6 rows read" in capsys.readouterr().out
    assert fresh.filled.tolist() == cache.filled.tolist() and torch.equal(fresh.moments, cache.moments)
    assert fresh.fill([1, 4]) == [] and enc2.calls == [] and fresh.encoded == 0    # nothing to encode
    assert fresh.fill([1, 2]) == [2] and enc2.calls == [1]
    # files that do not belong: another encoder, another dataset, another shape, no file, not a safetensors file
    other = FakeEncoder(seed=5)
    for what, c in (("encoder", _cache(enc=other)[0]), ("dataset", _cache(ds=_dataset(seed=9))[0])):
        assert c.load(path) is False and not c.filled.any() and bool((c.moments == 0).all()), what
        out = capsys.readouterr().out
        assert "is not used" in out and "fingerprint" in out, (what, out)
    c = _cache(n=5)[0]
    assert c.load(path) is False and "it holds 6 images" in capsys.readouterr().out
    assert _cache()[0].load(tmp_path / "nothing.safetensors") is False and "no such file" in capsys.readouterr().out
    (tmp_path / "junk.safetensors").write_bytes(b"not a safetensors file")
    assert _cache()[0].load(tmp_path / "junk.safetensors") is False and "is not used" in capsys.readouterr().out


def test_index_batches_follow_the_samplers_and_stay_on_the_host():
    from siss_amd.data import InfiniteSampler, RepeatedSampler, batches
    from siss_amd.latent_cache import IndexBatch, index_batches
    ds = _dataset(7)
    tag = object()
    for sampler in (lambda: InfiniteSampler(ds, rank=1, num_replicas=2), lambda: InfiniteSampler(ds, shuffle=False),
                    lambda: RepeatedSampler(ds, 5)):
        it, ref = index_batches(sampler(), 3, tag), batches(ds, sampler(), 3)
        for _ in range(6):
            b = next(it)
            assert isinstance(b, IndexBatch) and len(b) == 3 and b.cache is tag and b.to("cuda", non_blocking=True) is b
            assert torch.equal(ds.t[list(b)], next(ref))                              # the images today's iterator stacks
    it.close()


def test_default_hooks_return_todays_iterators_and_the_cache_applies_to_encoded_images_only(capsys):
    from siss_amd import hydra_lite as H
    from siss_amd.data import Prefetcher, batches
    from siss_amd.tasks import DeleteCeleb, DeleteSD
    cfgdir = os.path.join(ROOT, "config")
    ds = _dataset(5)
    for cls, name, ov in ((DeleteCeleb, "delete_celeb", []), (DeleteSD, "delete_sd", []),
                          (DeleteSD, "delete_sd", ["+latent_cache.enabled=false"]),
                          (DeleteSD, "delete_sd", ["+latent_cache.enabled=true"])):       # enabled, but no images are encoded
        task = cls(H.compose(name, cfgdir, ov))
        keep = task.keep_batches(ds, 2, 0, 1, "cpu")
        forget = task.forget_batches(ds, 2, "cpu")
        try:
            assert type(keep) is Prefetcher and keep.batch_size == 2 and type(keep.sampler).__name__ == "InfiniteSampler"
            assert type(forget) is type(batches(ds, [], 1))                               # the generator of data.batches
            assert torch.equal(next(forget), ds.t[:2])                                    # deletion_sampler: in order
            assert next(keep).shape == (2, 3, 8, 8)
        finally:
            keep.close()
    assert capsys.readouterr().out.count("the cache does not apply") == 1
    assert H.compose("delete_sd", cfgdir, []).get("latent_cache") is None                 # the shipped default: off
    task = DeleteSD(H.compose("delete_sd", cfgdir, ["+latent_cache.enabled=true", "+latent_cache.size=3"]))
    with pytest.raises(ValueError, match=r"unknown keys \['size'\]"):
        task.latent_cache_cfg()
    with pytest.raises(ValueError, match="a mapping"):
        DeleteSD(H.compose("delete_sd", cfgdir, ["latent_cache=true"])).latent_cache_cfg()
    task = DeleteSD(H.compose("delete_sd", cfgdir, ["+latent_cache.enabled=true", "+latent_cache.chunk=4"]))
    task.encodes_images = True
    assert dict(task.latent_cache_cfg()) == {"enabled": True, "chunk": 4}


def test_binding_and_build_entries():
    from siss_amd import lib
    from siss_amd.build import EXACT
    assert {"injection.hip", "latent_cache.hip"} <= EXACT                                  # no contraction into an fma in either
    assert "siss_latent_sample" in lib.F32_SAME
    assert lib.PARAMS["siss_latent_sample"] == ("cache", "idx", "eps", "out", "out_bf16", "rows", "n", "chw", "scaling", "nblk",
                                                "stream")
    src = os.path.join(ROOT, "siss_amd", "csrc")
    for f in ("injection.hip", "latent_cache.hip"):                                        # one statement of the expression
        text = open(os.path.join(src, f)).read()
        assert '#include "latent_sample.h"' in text and "posterior_sample(" in text and "expf(" not in text, f
    assert open(os.path.join(src, "latent_sample.h")).read().count("expf(") == 1

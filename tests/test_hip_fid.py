"""The FID metric on the GPU (csrc/inception.hip behind siss_amd/fid.py; the convolution and the max pool it shares with the other
metric networks are held in tests/test_hip_metric_conv.py): the average pools and the preprocessing against torch / the restatement, the whole Inception-v3 against the f64
restatement (tests/fid_ref.py) with negative controls and determinism, the f64 statistics, FIDEvaluator end to end, and the metric
in the delete_celeb task loop."""
import copy
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import fid_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The f32 restatement against the f64 restatement on the CPU, the network test's two images: max |f32 - f64| / max |f64| = 3.13e-07.
# The GPU sums in another order and splits K over ~100 layers: 8 x that; a wrong tap or pool lands at 0.3 of max |f64|.
E32 = 3.13e-7
NET_BOUND = 8 * E32
# The same for the end-to-end FID of the 6 + 6 images below: |FID(f32 features) - FID(f64 features)| / FID(f64) = 3.74e-07
# (FID 36.396291 against 36.396305); 8 x that, with a floor of 1e-7.
FID_E32 = 3.74e-7
FID_BOUND = max(8 * FID_E32, 1e-7)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref12():
    """The shared reference, computed once: the restatement make(0), 6 real images (8-bit values, as a decoded file has them) and 6
    fake ones of 64 x 64, and their f64 features [12, 2048]."""
    net = R.make(0)
    g = torch.Generator().manual_seed(1)
    real = torch.randint(0, 256, (6, 3, 64, 64), generator=g).float() / 255
    fake = torch.rand(6, 3, 64, 64, generator=g) * 0.7 + 0.2
    feats = R.features(net, torch.cat([real, fake]), torch.float64)
    return dict(net=net, real=real, fake=fake, feats=feats)


def _inception(net, dev):
    from siss_amd.fid import InceptionV3FID
    m = InceptionV3FID()
    m.load_state_dict(net.state_dict())
    return m.to(dev).eval()


# ---------------------------------------------------------------- pools
def _nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw(y):
    return y.permute(0, 3, 1, 2).cpu()


def test_pools_against_torch(dev):
    from siss_amd import fid
    g = torch.Generator().manual_seed(4)
    # average pool: corners (4 taps), edges (6) and the interior (9) of a 5 x 5 x 48 map, negative values included
    x = torch.randn(2, 48, 5, 5, generator=g)
    ref = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)
    got = _nchw(fid.avg_pool3(_nhwc(x, dev))).double()
    # 1e-6 relative PER ELEMENT, over a floor for the averages that cancel: n in-map taps summed in f32 are within (n - 1) 2^-24 of
    # the sum of their magnitudes (n <= 9), so the average is within 8 * 2^-24 * avg|x| of exact
    floor = 8 * 2.0 ** -24 * F.avg_pool2d(x.double().abs(), 3, 1, 1, count_include_pad=False)
    assert bool(((got - ref).abs() <= 1e-6 * ref.abs() + floor).all()), float(((got - ref).abs() / ref.abs()).max())
    # the global average over 8 x 8
    x = torch.randn(3, 2048, 8, 8, generator=g)
    ref = x.double().mean(dim=(2, 3))
    got = fid.global_avg(_nhwc(x, dev)).cpu().double()
    floor = 63 * 2.0 ** -24 * x.double().abs().mean(dim=(2, 3))      # the same reasoning for 64 terms
    assert got.shape == (3, 2048) and bool(((got - ref).abs() <= 1e-6 * ref.abs() + floor).all())


# ---------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("H, W", [(32, 32), (256, 256), (299, 299), (512, 384)])
def test_preprocessing_against_the_restatement(dev, H, W):
    from siss_amd import fid
    g = torch.Generator().manual_seed(H)
    x = torch.rand(2, 3, H, W, generator=g)
    # values exactly at k / 255 and one ulp below: the truncation's edges
    k = torch.randint(0, 256, (2, 3, H, W), generator=g).float() / 255
    where = torch.rand(2, 3, H, W, generator=g)
    x = torch.where(where < 0.25, k, x)
    x = torch.where((where >= 0.25) & (where < 0.5), torch.nextafter(k, torch.zeros(())), x)
    x[0, :, 0, 0], x[1, :, -1, -1] = 0.0, 1.0
    ref = R.preprocess(x)
    got = fid.preprocess(x.to(dev)).cpu()
    assert got.shape == (2, 299, 299, 3)
    got = got.permute(0, 3, 1, 2)
    err = float((got - ref).abs().max())
    print(f"\npreprocess {H}x{W}: max|d| {err:.3e} (bitwise equal: {torch.equal(got, ref)})")
    assert float(ref.min()) == -1.0 and 0.5 < float(ref.max()) < 1.0
    assert err <= 2e-6


# ---------------------------------------------------------------- the whole network
def test_network_against_the_f64_restatement(dev, ref12):
    net, imgs, ref = ref12["net"], ref12["real"][:2], ref12["feats"][:2]
    model = _inception(net, dev)
    got = model(imgs.to(dev))
    assert got.shape == (2, 2048) and got.dtype == torch.float32
    scale = float(ref.abs().max())
    # the reference is a test of the network: most features alive and different between the two images
    assert int(((ref[0] != 0) & (ref[1] != 0) & (ref[0] != ref[1])).sum()) >= 1024
    err = float((got.cpu().double() - ref).abs().max())
    print(f"\nInception-v3 N=2 64x64: max|d| {err:.3e} = {err / scale:.2e} of max|f64| {scale:.3e} (bound {NET_BOUND:.2e}, e32 {E32:.2e})")
    assert err <= NET_BOUND * scale
    # negative controls, each at least 100 bounds away: the BN statistics reset; Mixed_7c's max pool taken as the average pool
    ctl = R.reset_bn(copy.deepcopy(net))
    assert float((R.features(ctl, imgs) - got.cpu().double()).abs().max()) >= 100 * NET_BOUND * scale
    ctl = copy.deepcopy(net)
    ctl.Mixed_7c.pool = "avg"
    assert float((R.features(ctl, imgs) - got.cpu().double()).abs().max()) >= 100 * NET_BOUND * scale
    # the same call twice: equal bits
    assert torch.equal(got, model(imgs.to(dev)))
    assert model(imgs[:0].to(dev)).shape == (0, 2048)
    with pytest.raises(ValueError, match="3, H, W"):
        model(torch.zeros(2, 1, 64, 64, device=dev))


# ---------------------------------------------------------------- statistics
def test_statistics_against_f64_torch(dev):
    from siss_amd.fid import FrechetInceptionDistance
    D, n = 2048, 70                                               # 70 rows: not a multiple of the 16-row walk
    f = torch.randn(n, D, generator=torch.Generator().manual_seed(2)) * 0.5 + 0.5
    _, want_sum, want_cov = R.statistics(f)
    one = FrechetInceptionDistance(None, D, dev)
    one.update_features(f.to(dev), real=True)
    assert one.real_features_num_samples == n and one.fake_features_num_samples == 0 and not one.fake_features_cov_sum.any()
    assert one.real_features_sum.dtype == torch.float64 and one.real_features_cov_sum.is_cuda
    es = float((one.real_features_sum.cpu() - want_sum).abs().max() / want_sum.abs().max())
    ec = float((one.real_features_cov_sum.cpu() - want_cov).abs().max() / want_cov.abs().max())
    print(f"\nstatistics D={D} n={n}: sum {es:.2e}, cov_sum {ec:.2e} of the largest entry")
    assert es <= 1e-12 and ec <= 1e-12
    two = FrechetInceptionDistance(None, D, dev)
    two.update_features(f[:30].to(dev), real=True)
    two.update_features(f[30:].to(dev), real=True)
    assert two.real_features_num_samples == n
    assert float((two.real_features_sum - one.real_features_sum).abs().max()) <= 1e-12 * float(want_sum.abs().max())
    assert float((two.real_features_cov_sum - one.real_features_cov_sum).abs().max()) <= 1e-12 * float(want_cov.abs().max())
    again = FrechetInceptionDistance(None, D, dev)
    again.update_features(f.to(dev), real=True)
    assert torch.equal(again.real_features_cov_sum, one.real_features_cov_sum)      # no atomics: the same bits


def test_compute_on_synthetic_features(dev):
    from siss_amd.fid import FrechetInceptionDistance
    D = 256
    g = torch.Generator().manual_seed(3)
    mix = torch.randn(D, D, generator=g) / D ** 0.5
    f1 = torch.randn(600, D, generator=g) @ mix + 0.5
    f2 = (torch.randn(600, D, generator=g) @ mix) * 1.2 + 0.4
    fc = FrechetInceptionDistance(None, D, dev)
    for s in range(0, 600, 200):
        fc.update_features(f1[s:s + 200].to(dev), real=True)
        fc.update_features(f2[s:s + 200].to(dev), real=False)
    want = float(R.fid_from_features(f1, f2))
    # in f64, before the result's f32 rounding
    from siss_amd.fid import frechet_distance
    n = 600
    m1, m2 = fc.real_features_sum / n, fc.fake_features_sum / n
    c1 = (fc.real_features_cov_sum - n * torch.outer(m1, m1)) / (n - 1)
    c2 = (fc.fake_features_cov_sum - n * torch.outer(m2, m2)) / (n - 1)
    got64 = float(frechet_distance(m1, c1, m2, c2))
    print(f"\nFID D={D} 600 + 600: {got64:.12f} against {want:.12f}: {abs(got64 - want) / want:.2e}")
    assert want > 1.0 and abs(got64 - want) <= 1e-9 * want
    got = fc.compute()
    assert got.dtype == torch.float32 and float(got) == float(torch.tensor(got64, dtype=torch.float64).float())


# ---------------------------------------------------------------- end to end
class _Stub:
    """A classifier that calls an image class 1 when its first pixel is above 0.95."""

    def compute_logits(self, imgs):
        m = (imgs[:, 0, 0, 0] > 0.95).float()
        return torch.stack([1 - m, m], dim=1)


def test_evaluator_end_to_end(dev, ref12, tmp_path):
    import numpy as np
    from PIL import Image
    from siss_amd.fid import FIDEvaluator
    net, real, fake, feats = ref12["net"], ref12["real"], ref12["fake"], ref12["feats"]
    data = tmp_path / "real"
    data.mkdir()
    for i, im in enumerate(real):
        Image.fromarray((im * 255).round().byte().permute(1, 2, 0).numpy()).save(data / f"{i:05d}.png")
    stats = tmp_path / "real_stats.npz"

    def evaluator(**kw):
        ev = FIDEvaluator(4, dev, allow_random_init=True, inception_ckpt=str(tmp_path / "absent.pth"), data_path=str(data), **kw)
        ev.fid_computer.inception.load_state_dict(net.state_dict())
        return ev

    ev = evaluator(real_stats_path=str(stats))
    ev.load_celeb()                                              # 6 files in batches of 4 + 2; writes the statistics file
    assert ev.fid_computer.real_features_num_samples == 6 and stats.is_file()
    ev.add_fake_images(fake.to(dev))
    assert ev.fid_computer.fake_features_num_samples == 6
    got = ev.compute(reset=True)
    want = float(R.fid_from_features(feats[:6], feats[6:]))
    rel = abs(float(got) - want) / want
    print(f"\nFID 6 + 6: {float(got):.6f} against {want:.6f}: {rel:.2e} (bound {FID_BOUND:.2e})")
    assert got.dtype == torch.float32 and want > 1.0
    assert rel <= FID_BOUND
    assert ev.fid_computer.fake_features_num_samples == 0 and ev.fid_computer.real_features_num_samples == 6     # reset: the fake side
    # the statistics file: the next evaluator starts from the same real side without reading an image
    ev2 = evaluator(real_stats_path=str(stats), classifier=_Stub(), remove_class=1)
    ev2.data_path = str(tmp_path / "nodir")
    ev2.load_celeb()
    assert torch.equal(ev2.fid_computer.real_features_cov_sum, ev.fid_computer.real_features_cov_sum)
    assert torch.equal(ev2.fid_computer.real_features_sum, ev.fid_computer.real_features_sum)
    # remove_class: the two images the stub flags are left out
    marked = fake.clone()
    marked[:, 0, 0, 0] = 0.5
    marked[1, 0, 0, 0] = marked[4, 0, 0, 0] = 1.0
    ev2.add_fake_images(marked.to(dev))
    assert ev2.fid_computer.fake_features_num_samples == 4
    ev3 = evaluator()
    ev3.add_fake_images(marked[[0, 2, 3, 5]].to(dev))
    assert torch.equal(ev3.fid_computer.fake_features_sum, ev2.fid_computer.fake_features_sum)
    assert torch.equal(ev3.fid_computer.fake_features_cov_sum, ev2.fid_computer.fake_features_cov_sum)
    ev4 = evaluator(classifier=_Stub(), remove_class=1, filter_fake=False)
    ev4.add_fake_images(marked.to(dev))
    assert ev4.fid_computer.fake_features_num_samples == 6


# ---------------------------------------------------------------- the task
SMALL = ["unet.sample_size=16", "unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
         "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1", "unet.attention_head_dim=null",
         "training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent",
         "allow_random_init=true", "allow_synthetic=true", "save_final=false", "pipeline.num_inference_steps=2"]


def test_fid_in_the_delete_celeb_loop(dev, tmp_path):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    import main as entry
    data = tmp_path / "real"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i in range(4):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(data / f"{i}.jpg")
    out = tmp_path / "with"
    entry.main(["--config-name=delete_celeb", f"data_dir={tmp_path}/nodata", f"output_dir={out}", *SMALL,
                "+metrics.fid.class_cfg._target_=metrics.fid.FIDEvaluator", "+metrics.fid.class_cfg.inception_batch_size=4",
                "+metrics.fid.class_cfg.allow_random_init=true", f"+metrics.fid.class_cfg.data_path={data}",
                "+metrics.fid.step_frequency=1", "+metrics.fid.num_imgs_to_generate=4", "+metrics.fid.batch_size=2"])
    run = os.listdir(out)[0]
    lines = [json.loads(l) for l in open(out / run / "fid_rank0.jsonl")]
    print("\n", lines)
    assert [l["global_step"] for l in lines] == [0, 1, 2]
    for l in lines:
        assert set(l) == {"global_step", "fid", "fake_images", "real_images", "seconds"}
        assert l["fid"] is not None and l["fid"] == l["fid"] and 0.0 <= l["fid"] < float("inf")
        assert l["fake_images"] == 4 and l["real_images"] == 4
    assert len([json.loads(l) for l in open(out / run / "train_log_rank0.jsonl")]) == 2
    # the same run without the block: no such file
    out = tmp_path / "without"
    entry.main(["--config-name=delete_celeb", f"data_dir={tmp_path}/nodata", f"output_dir={out}", *SMALL])
    run = os.listdir(out)[0]
    assert os.path.exists(out / run / "train_log_rank0.jsonl") and not os.path.exists(out / run / "fid_rank0.jsonl")

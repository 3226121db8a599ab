"""The SD SSCD copy-detection score on the GPU (csrc/sscd.hip behind siss_amd/sscd.py): the preprocessing bitwise against torch's f32
chain, GeM pooling and the normalisation / score against f64, the whole ResNet-50 against the f64 restatement (tests/sscd_ref.py)
with negative controls and determinism, one full-size image, the checkpoint loader's round trip, and the metric in the delete_sd
task loop."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sscd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0                    # of the restatement's weights: its controls deviate by > 10,000 bounds on the CPU (asserted below too)
HALF = (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def net():
    return R.make(SEED)


@pytest.fixture(scope="module")
def model(net, dev):
    from siss_amd.sscd import SSCDModel
    m = SSCDModel()
    m.load_state_dict(net.state_dict())
    return m.to(dev).eval()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- preprocessing
def _u8_images(n, h, w, seed):
    """uint8 [n, h, w, 3] (n h w >= 256) in which every channel holds all 256 values, in a shuffled order per channel."""
    g = torch.Generator().manual_seed(seed)
    count = n * h * w
    cols = [(torch.arange(count) % 256).to(torch.uint8)[torch.randperm(count, generator=g)] for _ in range(3)]
    return torch.stack(cols, 1).reshape(n, h, w, 3).contiguous()


def _preprocess(dev, src, form, mean, std, want_u8=False):
    from siss_amd import lib
    n = src.shape[0]
    h, w = (src.shape[1], src.shape[2]) if form == 0 else (src.shape[2], src.shape[3])
    y = torch.full((n, 3, h, w), float("nan"), device=dev)
    u8 = torch.full((n, h, w, 3), 7, device=dev, dtype=torch.uint8) if want_u8 else None
    lib.call("siss_sscd_preprocess", src, form, n, h, w, *[float(v) for v in mean], *[float(v) for v in std], u8, y)
    return y, u8


def _torch_u8(img):
    """sd_sampler.py:147 / diffusers' postprocess on the decoder's output, in its own dtype: uint8 [n, H, W, 3]."""
    return ((img / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("mean, std", [(R.IMAGENET_MEAN, R.IMAGENET_STD), (HALF, HALF)], ids=["imagenet", "half"])
@pytest.mark.parametrize("h, w", [(5, 7), (64, 64)])
def test_preprocess_from_uint8_is_bitwise_torch(dev, h, w, mean, std):
    """Form (a).  n = 2 at 3 x 5 x 7 holds 70 bytes per channel, so that shape runs four times over shifted value ranges and the four
    runs together cover all 256 values in every channel; 3 x 64 x 64 covers them in one.  The chain is taken on the GPU in f32 with
    the division by 255 as a tensor-by-tensor division: `t / 255` with a Python scalar multiplies by the rounded reciprocal on the
    GPU (torch's documented shortcut, one bit off for some bytes), while the reference's ToTensor divides on the host -- the host
    chain is asserted as well, so the kernel is held to the true division both ways."""
    from siss_amd.data import Normalize
    n = 2
    if n * h * w >= 256:
        cases = [_u8_images(n, h, w, seed=h)]
    else:
        base = torch.arange(n * h * w * 3).reshape(n, h, w, 3)
        cases = [((base * 11 + 64 * k) % 256).to(torch.uint8) for k in range(4)]
    seen = torch.zeros(3, 256, dtype=torch.bool)
    for u8 in cases:
        for c in range(3):
            seen[c, u8[..., c].reshape(-1).long()] = True
        d = u8.to(dev)
        want = Normalize(mean, std)(d.permute(0, 3, 1, 2).float() / torch.tensor(255.0, device=dev).expand(1, 1, 1, 1))
        got, _ = _preprocess(dev, d, 0, mean, std)
        assert got.shape == want.shape == (n, 3, h, w) and want.is_cuda and want.dtype == torch.float32
        host = R.normalise(u8, mean, std)                     # Normalize(ToTensor(.)) as the reference's host code rounds it
        print(f"\npreprocess {h}x{w}: {int((_bits(got) != _bits(want)).sum())} words off the GPU chain, "
              f"{int((_bits(got.cpu()) != _bits(host)).sum())} off the host chain")
        assert torch.equal(_bits(got), _bits(want))
        assert torch.equal(_bits(got.cpu()), _bits(host))
    assert bool(seen.all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("h, w", [(5, 7), (64, 64)])
def test_preprocess_from_decoded_matches_torch_bytes_and_form_a(dev, h, w, dtype):
    """Form (b): decoder output with rounding ties ((2 k + 1) / 255 - 1 and its neighbours: x.5 before the rint) and values outside
    [-1, 1]; the bytes are torch's chain in the tensor's dtype, the f32 output is form (a) on those bytes, bit for bit."""
    n = 2
    g = torch.Generator().manual_seed(h)
    x = torch.rand(n, 3, h, w, generator=g) * 2.6 - 1.3
    k = torch.randint(0, 255, (n, 3, h, w), generator=g).float()
    tie = (2 * k + 1) / 255 - 1
    where = torch.rand(n, 3, h, w, generator=g)
    x = torch.where(where < 0.2, tie, x)
    x = torch.where((where >= 0.2) & (where < 0.3), torch.nextafter(tie, torch.full((), 2.0)), x)
    x = torch.where((where >= 0.3) & (where < 0.4), torch.nextafter(tie, torch.full((), -2.0)), x)
    x[0, :, 0, 0], x[1, :, -1, -1], x[0, :, 0, 1], x[1, :, 0, 0] = -1.0, 1.0, 5.0, -7.0
    x = x.to(dev).to(dtype)
    want_u8 = _torch_u8(x)
    assert int(want_u8.min()) == 0 and int(want_u8.max()) == 255 and float(x.float().max()) > 1 and float(x.float().min()) < -1
    for mean, std in ((R.IMAGENET_MEAN, R.IMAGENET_STD), (HALF, HALF)):
        got, u8 = _preprocess(dev, x, 2 if dtype == torch.bfloat16 else 1, mean, std, want_u8=True)
        assert torch.equal(u8, want_u8)
        a, _ = _preprocess(dev, want_u8, 0, mean, std)
        assert torch.equal(_bits(got), _bits(a))
        nobytes, _ = _preprocess(dev, x, 2 if dtype == torch.bfloat16 else 1, mean, std)        # the optional output left out
        assert torch.equal(_bits(nobytes), _bits(a))


def test_preprocess_refuses_bad_arguments(dev):
    from siss_amd import lib
    u8 = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    y = torch.empty(1, 3, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_sscd_preprocess", u8, 3, 1, 4, 4, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None, y)          # no such form
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_sscd_preprocess", u8, 0, 1, 4, 4, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, None, y)          # a zero std
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_sscd_gem", y, y, 1, 16, 3, 0.0, 1e-6)                                               # p = 0


# ---------------------------------------------------------------- GeM
def _ulp32(ref64):
    """One f32 ulp at each f64 reference value (the spacing of f32 numbers in its binade)."""
    r32 = ref64.float().abs()
    return (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()


@pytest.mark.parametrize("p", [3.0, 1.0])
@pytest.mark.parametrize("N, HW, C", [(3, 1, 64), (2, 6, 2048), (1, 256, 128)])
def test_gem_within_one_ulp_of_f64(dev, N, HW, C, p):
    from siss_amd import lib
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(N, HW, C, generator=g)
    x = torch.where(torch.rand(N, HW, C, generator=g) < 0.3, torch.zeros(()), x)                # a ReLU's zeros; negatives stay
    x[0, :, 0] = 0.0                                                                             # a channel clamped everywhere
    x[0, :, 1] = -1.0
    assert bool((x == 0).any()) and bool((x < 0).any())
    clamped = x.clamp(min=1e-6)                                                                  # in f32, at (float)1e-6
    ref = clamped.double().pow(p).mean(1).pow(1 / p)
    y = torch.full((N, C), float("nan"), device=dev)
    lib.call("siss_sscd_gem", x.to(dev), y, N, HW, C, p, 1e-6)
    got = y.cpu().double()
    err = ((got - ref).abs() / _ulp32(ref)).max().item()
    print(f"\nGeM [{N}, {HW}, {C}] p = {p}: {err:.3f} f32 ulp of the f64 value")
    assert torch.isfinite(got).all() and err <= 1.0
    assert float(got[0, 0]) == pytest.approx(1e-6, rel=1e-6) and float(got[0, 1]) == pytest.approx(1e-6, rel=1e-6)
    y2 = torch.full((N, C), float("nan"), device=dev)
    lib.call("siss_sscd_gem", x.to(dev), y2, N, HW, C, p, 1e-6)
    assert torch.equal(_bits(y), _bits(y2))


# ---------------------------------------------------------------- normalise / score
@pytest.mark.parametrize("D", [512, 96])
def test_normalize_and_score_against_f64(dev, D):
    from siss_amd import lib
    N = 5
    g = torch.Generator().manual_seed(D)
    e = torch.randn(N, D, generator=g) * torch.tensor([1e-3, 1.0, 40.0, 1.0, 1.0]).view(N, 1)
    e[3] = 0.0                                                                                   # an all-zero row
    r = torch.nn.functional.normalize(torch.randn(D, generator=g).double(), dim=0).float()
    e[4] = r * 3.0                                                                               # parallel to the reference row
    ref = e.double() / e.double().norm(dim=1, keepdim=True).clamp(min=1e-12)
    out = torch.full((N, D), float("nan"), device=dev)
    score = torch.full((N,), float("nan"), device=dev)
    lib.call("siss_sscd_normalize_score", e.to(dev), N, D, 1e-12, r.to(dev), out, score)
    got, sc = out.cpu().double(), score.cpu().double()
    print(f"\nnormalise D = {D}: rows {float((got - ref).abs().max()):.2e}, scores {float((sc - ref @ r.double()).abs().max()):.2e}")
    assert not torch.isnan(got).any() and not torch.isnan(sc).any()
    assert float((got - ref).abs().max()) <= 2.0 ** -23
    assert float((sc - ref @ r.double()).abs().max()) <= 2.0 ** -22
    assert not got[3].any() and float(sc[3]) == 0.0
    assert abs(float(sc[4]) - 1.0) <= 2.0 ** -22
    # a unit row scored against itself
    unit = out[1].clone()
    s1 = torch.full((1,), float("nan"), device=dev)
    o1 = torch.empty(1, D, device=dev)
    lib.call("siss_sscd_normalize_score", unit, 1, D, 1e-12, unit, o1, s1)
    assert abs(float(s1) - 1.0) <= 2.0 ** -22
    # without a reference row the scores are not touched; in place; the same bits again
    inplace = e.to(dev).clone()
    keep = torch.full((N,), 3.0, device=dev)
    lib.call("siss_sscd_normalize_score", inplace, N, D, 1e-12, None, inplace, keep)
    assert torch.equal(_bits(inplace), _bits(out)) and bool((keep == 3.0).all())


# ---------------------------------------------------------------- the whole network
def _images(shape, seed):
    n, _, h, w = shape
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, R.normalise(u8, R.IMAGENET_MEAN, R.IMAGENET_STD)


def _against_f64(net, model, dev, shape, seed):
    u8, x = _images(shape, seed)
    ref = R.embed(net, x, torch.float64)
    e32 = float((R.embed(net, x, torch.float32) - ref).abs().max())        # the same restatement in f32 against f64, measured here
    bound = 8 * e32
    got = model(x.to(dev))
    assert got.shape == (shape[0], 512) and got.dtype == torch.float32 and got.is_cuda
    err = float((got.cpu().double() - ref).abs().max())
    print(f"\nSSCD ResNet-50 {shape}: max|d| {err:.3e}, bound {bound:.3e} (f32 restatement {e32:.3e}), max|f64| {float(ref.abs().max()):.3e}")
    assert e32 > 0 and torch.allclose(ref.norm(dim=1), torch.ones(shape[0], dtype=torch.float64), atol=1e-12)
    assert err <= bound
    assert torch.equal(_bits(model(x.to(dev))), _bits(got))                 # the same call, the same bits
    return u8, x, ref, got, bound


@pytest.mark.parametrize("shape", [(3, 3, 64, 64), (1, 3, 96, 64)], ids=["3x64x64", "1x96x64"])
def test_network_against_the_f64_restatement(dev, net, model, shape):
    """N = 3 at 64 x 64 (the layer4 map is 2 x 2) and N = 1 at 96 x 64 (non-square, split-K on the late layers)."""
    from siss_amd.metric_net import conv_splits
    u8, x, ref, got, bound = _against_f64(net, model, dev, shape, seed=shape[2])
    n, _, h, w = shape
    assert (h // 32, w // 32) == ((2, 2) if h == 64 else (3, 2))
    assert conv_splits(n * (h // 32) * (w // 32), 2048, 512) > 1           # layer4's conv3 at this shape goes through split-K
    # negative controls, each at least 100 bounds away, on the CPU with the restatement alone and against the GPU's result
    for name, ctl in (("stride on conv1", R.variant(net, stride_on_conv1=True)), ("average pooling", R.variant(net, gem=False)),
                      ("BN statistics reset", R.reset_bn(net))):
        c = R.embed(ctl, x)
        away, away_gpu = float((c - ref).abs().max()), float((c - got.cpu().double()).abs().max())
        print(f"  control {name}: {away / bound:.0f} bounds from the restatement, {away_gpu / bound:.0f} from the GPU")
        assert away >= 100 * bound and away_gpu >= 100 * bound
    # the fused paths: from the bytes, and from a decoder output that quantises to those bytes
    e8 = model.embed_u8(u8.to(dev), R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert torch.equal(_bits(e8), _bits(got))
    dec = (u8.to(dev).permute(0, 3, 1, 2).float() / 255 * 2 - 1).contiguous()
    ed, bytes_ = model.embed_decoded(dec, R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert torch.equal(bytes_, _torch_u8(dec))
    assert torch.equal(_bits(ed), _bits(model.embed_u8(bytes_, R.IMAGENET_MEAN, R.IMAGENET_STD)))
    # the score is the f64 dot product with a unit row; chunks of one image give the same rows
    rows, scores = model.embed_u8(u8.to(dev), R.IMAGENET_MEAN, R.IMAGENET_STD, ref=got[0])
    assert torch.equal(_bits(rows), _bits(got))
    assert float((scores.cpu().double() - got.cpu().double() @ got[0].cpu().double()).abs().max()) <= 2.0 ** -22
    assert abs(float(scores[0]) - 1.0) <= 2.0 ** -22


def test_full_size_image(dev, net, model):
    """N = 1 at 3 x 512 x 512, the size the reference feeds: the 65,536-row grids of the stem and the HW = 256 GeM rows.  The f64
    anchor runs on the host (well under a second)."""
    _against_f64(net, model, dev, (1, 3, 512, 512), seed=512)
    assert model.max_elements(1, 512, 512) == 256 * 256 * 64 and model.max_elements(16, 512, 512) < 1 << 31
    with pytest.raises(ValueError, match="2\\^31"):
        model._features(torch.empty(512, 3, 512, 512, device="meta"))


def test_loader_round_trip(dev, net, model, tmp_path):
    from siss_amd.sscd import SSCDModel
    torch.jit.script(net).save(str(tmp_path / "sscd.torchscript.pt"))
    loaded = SSCDModel.load(tmp_path / "sscd.torchscript.pt").to(dev)
    _, x = _images((2, 3, 64, 48), seed=3)
    assert torch.equal(_bits(loaded(x.to(dev))), _bits(model(x.to(dev))))


# ---------------------------------------------------------------- DeleteSD
def _crop(path, k, size=32, cols=1, pad=2):
    from PIL import Image
    a = np.asarray(Image.open(path))
    r, q = divmod(k, cols)
    return a[r * (size + pad) + pad:r * (size + pad) + pad + size, q * (size + pad) + pad:q * (size + pad) + pad + size]


NORMALIZE = ("{_target_: torchvision.transforms.Compose, transforms: [{_target_: torchvision.transforms.Normalize, "
             "mean: [0.485, 0.456, 0.406], std: [0.229, 0.224, 0.225]}]}")


def _mean_score(model, u8, ref):
    """The f64 mean of the images' scores against `ref`, one image per call as the task's eval_batch_size = 1 embeds them."""
    scores = [model.embed_u8(u8[k:k + 1], R.IMAGENET_MEAN, R.IMAGENET_STD, ref=ref)[1] for k in range(u8.shape[0])]
    return float(torch.cat(scores).cpu().double().mean())


def test_delete_sd_sscd_end_to_end(dev, net, model, tmp_path):
    from PIL import Image
    from test_hip_sd_sampling import _run, _tiny_checkpoint
    from siss_amd import lib
    from siss_amd.kmeans import KMeansClassifier
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    prompt = str(tmp_path / "prompt_ids.pt")
    torch.jit.script(net).save(str(tmp_path / "sscd.torchscript.pt"))
    mem = torch.randint(0, 256, (32, 32, 3), generator=g, dtype=torch.uint8)
    Image.fromarray(mem.numpy()).save(str(tmp_path / "mem.png"))
    evals = ["training_steps=2", "eval_every=1", "+eval_batches=2", "+eval_batch_size=1", "+pipeline.num_inference_steps=3", "resolution=32"]
    sscd = [f"metrics.sscd.model_path={tmp_path}/sscd.torchscript.pt", f"metrics.sscd.data_transforms={NORMALIZE}",
            f"data_files.mem_img_path={tmp_path}/mem.png"]
    weights = {}

    def hook(name):
        def install(task):
            inner = task.evaluate

            def evaluate(unet, sched, forget_image, step, device):
                e = unet.engine
                torch.cuda.synchronize()
                flat, shadow = e.ps.flat.clone(), e.ps.shadow.clone()
                inner(unet, sched, forget_image, step, device)
                torch.cuda.synchronize()
                assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)      # evaluation only reads the weights
                weights[name, step] = flat
            task.evaluate = evaluate
        return install

    # without the metric: the files of before
    _, _, cfg0 = _run(tmp_path, "plain", ckpt, evals, prompt, hook("plain"))
    assert cfg0.metrics.sscd is None and not os.path.exists(os.path.join(cfg0.output_dir, "metrics_rank0.jsonl"))
    task, _, cfg = _run(tmp_path, "sscd", ckpt, evals + sscd, prompt, hook("sscd"))
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))]
    print("\nsscd", lines)
    assert [r["global_step"] for r in lines] == [1, 2] and all(set(r) == {"global_step", "sscd_0"} for r in lines)
    assert sorted(os.listdir(cfg.output_dir)) == sorted(os.listdir(cfg0.output_dir) + ["metrics_rank0.jsonl"])
    # the recorded value is the score of the tiles of the written grid against the memorized image, recomputed here
    ref = model.embed_u8(mem[None].to(dev), R.IMAGENET_MEAN, R.IMAGENET_STD)[0]
    for r in lines:
        v = r["sscd_0"]
        assert isinstance(v, float) and np.isfinite(v) and -1.0 <= v <= 1.0
        path = os.path.join(cfg.output_dir, f"validation_p0_step{r['global_step']}.png")
        tiles = torch.from_numpy(np.stack([_crop(path, k) for k in (0, 1)]).copy()).to(dev)
        again = _mean_score(model, tiles, ref)
        print(f"  step {r['global_step']}: recorded {v:.9f}, from the grid {again:.9f}")
        assert abs(v - again) <= 1e-6
    # the trained weights are bitwise those of the run without the metric -- wherever that run is itself reproducible.  The step's
    # gradient kernels add with float atomics, and tests/test_hip_sd_sampling.py records that two plain runs of this very task differ
    # by up to 3e-8 in ~1.5 % of the weights after two steps; a second plain run tells which case this machine is in.  Reproducible:
    # bit for bit, as the issue asks.  Not reproducible: the bound that test holds the same comparison to (1e-6).  What the
    # evaluation itself does to the weights is held to zero, bit for bit, inside every run above.
    _run(tmp_path, "plain2", ckpt, evals, prompt, hook("plain2"))
    reproducible = all(torch.equal(weights["plain2", step], weights["plain", step]) for step in (1, 2))
    for step in (1, 2):
        own = float((weights["plain2", step] - weights["plain", step]).abs().max())
        d = float((weights["sscd", step] - weights["plain", step]).abs().max())
        print(f"  weights at step {step}: max|d| against the run without the metric {d:.3e}; two runs without it {own:.3e}")
        if reproducible:
            assert torch.equal(weights["sscd", step], weights["plain", step])
        else:
            assert d <= 1e-6
    # with the k-means fraction on as well: both records; the labels are those of the fraction alone (the construction of
    # tests/test_hip_kmeans.py: the images' own centre is the memorized one, so every label is 1)
    own = _crop(os.path.join(cfg0.output_dir, "validation_p0_step1.png"), 0).reshape(-1).astype(np.float32)
    far = np.where(own < 128, 255.0, 0.0).astype(np.float32)
    KMeansClassifier(np.stack([far, own])).save(str(tmp_path / "km.npz"))
    seen = []

    def spy(task):
        inner = task.evaluate

        def evaluate(*a):                            # (the classifier is loaded by run(), after this hook: wrap it at the evaluation)
            fused = task.kmeans.from_decoded

            def from_decoded(img):                   # the labels, and what the classifier alone makes of the bytes SSCD was given
                u8, labels, dist = fused(img)
                seen.append((labels.clone(), task.kmeans.predict(u8)[1].clone(), u8.clone()))
                return u8, labels, dist
            task.kmeans.from_decoded = from_decoded
            try:
                inner(*a)
            finally:
                task.kmeans.from_decoded = fused
        task.evaluate = evaluate

    _, _, cfg_b = _run(tmp_path, "both", ckpt, evals + [f"metrics.fraction_deletion.classifier_path={tmp_path}/km.npz"] + sscd, prompt, spy)
    both = [json.loads(l) for l in open(os.path.join(cfg_b.output_dir, "metrics_rank0.jsonl"))]
    print("  both", both)
    assert len(seen) == 4 and all(torch.equal(a, b) and a.tolist() == [1] for a, b, _ in seen)
    frac = [r for r in both if "deletion_fraction_0" in r]
    assert frac == [{"global_step": 1, "deletion_fraction_0": 1.0}, {"global_step": 2, "deletion_fraction_0": 1.0}]
    rest = [r for r in both if "deletion_fraction_0" not in r]
    assert [r["global_step"] for r in rest] == [1, 2] and all(set(r) == {"global_step", "sscd_0"} for r in rest)
    for r, pair in zip(rest, (seen[:2], seen[2:])):                 # the score is that of the classifier's bytes
        again = _mean_score(model, torch.cat([u8 for _, _, u8 in pair]), ref)
        assert abs(r["sscd_0"] - again) <= 1e-6 and -1.0 <= r["sscd_0"] <= 1.0
    # refused before the first step, with what is missing in the message
    with pytest.raises(FileNotFoundError, match="mem_img_path"):
        _run(tmp_path, "bad", ckpt, ["training_steps=1"] + sscd[:2], prompt)
    assert not os.path.exists(os.path.join(str(tmp_path), "bad", "train_log_rank0.jsonl"))
    assert lib.PROF is None

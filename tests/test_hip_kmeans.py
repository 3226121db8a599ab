"""The SD k-means deletion fraction on HIP (csrc/kmeans.hip, siss_amd/kmeans.py): the fused decoder-output -> uint8 + distances
launch against torch's own chain (bitwise) and float64 sums, Lloyd's fit against the scikit-learn results recorded in
tests/golden/kmeans_ref.npz, and DeleteSD's opt-in metric end to end.

Distance bound.  A term is (float(u8) - c)^2 with the difference and the square each rounded to f32: relative error below
(1 + 2^-24)^3 - 1 < 3 * 2^-24 + 2^-46.  Terms are non-negative and are added in f64 (lane, wave, block, slab: at most D + 64 * K
additions of relative error 2^-53, D <= 2^20: < 1.2e-10), so every distance is within DIST_BOUND = 3 * 2^-24 + 1e-9 = 1.8e-7
(relative) of the exact sum -- the 1e-9 also covers the float64 reference's own rounding.  The fixtures' labels need 1e-3."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from kmeans_ref import relative_gap  # noqa: E402

DIST_BOUND = 3 * 2.0 ** -24 + 1e-9
CENTRE_TOL = 2.0 ** -17 + 1e-9
assert DIST_BOUND <= 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "kmeans_ref.npz"))
    return z, [str(c) for c in z["cases"]]


def _torch_u8(img):
    """sd_sampler.py:144, on the device, in img's dtype."""
    return ((img / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _f64_dist(rows, centres):
    """[N, K] exact-to-f64 squared distances of uint8 rows to f32 centres, on the rows' device."""
    x, c = rows.reshape(rows.shape[0], -1).double(), centres.double()
    return torch.stack([((x - c[k]) ** 2).sum(1) for k in range(c.shape[0])], 1)


def _within(got, ref, what=""):
    err = ((got - ref).abs() / ref.clamp_min(1e-300)).max().item()
    print(f"{what}: max relative distance error {err:.3g} (bound {DIST_BOUND:.3g})")
    assert ((got - ref).abs() <= DIST_BOUND * ref).all(), (what, err)


def _decoder_like(n, h, w, dtype, dev, seed):
    """Values a decoder gives and the awkward ones: rounding ties of the chain (0 -> 127.5; k / 255 * 2 - 1 neighbours), the clamp's
    ends and values outside [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(n, 3, h, w, generator=g) * 0.8
    flat = img.view(-1)
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 7.0, -7.0, 1.0 - 2 ** -20, -1.0 + 2 ** -20, 2 ** -30, 1 / 255, -1 / 255,
                            0.00392, 0.0117647, 0.5, -0.5, 0.25, 0.99609375, -0.99609375, 0.0078125, 0.00390625])
    ks = torch.arange(0, 255, dtype=torch.float64)
    ties = ((ks + 0.5) / 255 * 2 - 1).float()                        # where x / 2 + 0.5 lands next to (k + 0.5) / 255
    vals = torch.cat([special, ties, torch.nextafter(ties, torch.tensor(2.0)), torch.nextafter(ties, torch.tensor(-2.0))])
    vals = vals[: flat.numel() // 2]
    flat[torch.randperm(flat.numel(), generator=g)[: vals.numel()]] = vals
    return img.to(dev).to(dtype).contiguous()


# ---------------------------------------------------------------- 1. the fused decoded -> uint8 + distances launch
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,h,w", [(3, 8, 8), (2, 5, 7), (4, 32, 32), (1, 64, 48)])          # 5 x 7: the unvectorised path
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_decoded_u8_is_bitwise_torch_and_distances_are_bounded(dev, dtype, n, h, w, k):
    from siss_amd.kmeans import KMeansClassifier
    img = _decoder_like(n, h, w, dtype, dev, seed=h * 31 + k)
    g = torch.Generator().manual_seed(k)
    centres = torch.rand(k, h * w * 3, generator=g) * 255
    clf = KMeansClassifier(centres)
    u8, labels, dist = clf.from_decoded(img)
    want = _torch_u8(img)
    assert u8.dtype == torch.uint8 and u8.shape == (n, h, w, 3) and torch.equal(u8, want), (u8.int() - want.int()).abs().max().item()
    ref = _f64_dist(want, clf.centres(dev))
    _within(dist, ref, f"decoded {dtype} {n}x{h}x{w} K={k}")
    assert torch.equal(labels.long(), dist.argmin(1)) and labels.dtype == torch.int32
    u8b, labelsb, distb = clf.from_decoded(img)
    assert torch.equal(dist, distb) and torch.equal(u8, u8b) and torch.equal(labels, labelsb)            # bitwise repeatable
    # stored images: the uint8 path gives the SAME distances up to the bound, and its own repeat the same bits
    rows, labels2, dist2 = clf.predict(u8)
    _within(dist2, ref, "assign")
    assert rows.shape == (n, h * w * 3) and torch.equal(clf.predict(u8.cpu().numpy())[2], dist2)
    assert torch.equal(labels2.long(), dist2.argmin(1))


def test_argmin_takes_the_lowest_index_on_ties(dev):
    from siss_amd.kmeans import KMeansClassifier
    c = torch.full((3, 48), 100.0)
    c[0] += 3                                                       # centres 1 and 2 identical and nearest
    rows = torch.full((5, 48), 99, dtype=torch.uint8)
    _, labels, dist = KMeansClassifier(c).predict(rows)
    assert labels.tolist() == [1] * 5 and torch.equal(dist[:, 1], dist[:, 2])


def test_launch_counts(dev):
    """One fused launch plus one finalize per classified batch; a stored batch is one launcher call (distance pass + finalize)."""
    from siss_amd import lib
    from siss_amd.kmeans import KMeansClassifier
    clf = KMeansClassifier(torch.rand(2, 3 * 16 * 16) * 255)
    img = torch.randn(4, 3, 16, 16, device=dev)
    clf.from_decoded(img)                                            # (centres uploaded before the count)
    lib.PROF = []
    try:
        for _ in range(3):
            u8, _, _ = clf.from_decoded(img)
        names = [r[0] for r in lib.PROF]
        assert names == ["siss_kmeans_decoded", "siss_kmeans_finalize"] * 3
        lib.PROF.clear()
        clf.predict(u8)
        assert [r[0] for r in lib.PROF] == ["siss_kmeans_assign"]
    finally:
        lib.PROF = None


# ---------------------------------------------------------------- 2. the fit against recorded scikit-learn
def test_fit_matches_recorded_sklearn(dev, golden):
    from siss_amd.kmeans import fit
    z, cases = golden
    for c in cases:
        X, init = torch.from_numpy(z[c + "_X"]).to(dev), z[c + "_init"]
        k = init.shape[0]
        m = fit(X, n_clusters=k, init=init)
        print(f"{c}: n_iter {m.n_iter_} (sklearn {int(z[c + '_n_iter'])}), inertia {m.inertia_!r} (sklearn {float(z[c + '_inertia'])!r})")
        assert m.n_iter_ == int(z[c + "_n_iter"]), c
        assert np.array_equal(m.labels_.cpu().numpy(), z[c + "_labels"]), c
        assert abs(m.inertia_ - float(z[c + "_inertia"])) <= 1e-5 * float(z[c + "_inertia"]), c
        err = np.abs(m.cluster_centers_.astype(np.float64) - z[c + "_centres"]).max()
        print(f"{c}: max centre error {err:.3g} (tolerance {CENTRE_TOL:.3g})")
        assert err <= CENTRE_TOL, (c, err)
        _, held, _ = m.predict(z[c + "_held"])
        assert np.array_equal(held.cpu().numpy(), z[c + "_held_labels"]), c
        m2 = fit(X, n_clusters=k, init=init)                        # bitwise repeatable
        assert np.array_equal(m.cluster_centers_, m2.cluster_centers_) and m.inertia_ == m2.inertia_
        assert torch.equal(m.labels_, m2.labels_)


@pytest.mark.parametrize("n,d,k", [(500, 192, 2), (333, 105, 5), (700, 64, 16), (64, 3072, 3), (9, 7, 1)])
def test_update_gives_the_correctly_rounded_integer_means(dev, n, d, k):
    from siss_amd.kmeans import update
    g = torch.Generator().manual_seed(n + d)
    rows = torch.randint(0, 256, (n, d), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, k, (n,), generator=g).int()
    labels[::7] = -1                                                 # rows that belong to no cluster are left out
    centres = torch.full((k, d), -5.0)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    c_dev = centres.to(dev)
    counts = update(rows.to(dev), labels.to(dev), c_dev, status)
    empty = 0
    for j in range(k):
        members = rows[labels == j].double()
        assert int(counts[j]) == len(members)
        if len(members) == 0:
            empty += 1
            assert (c_dev[j] == -5).all()
            continue
        want = (members.sum(0) / len(members)).float()               # integer sums are exact in f64; one division, one rounding to f32
        assert torch.equal(c_dev[j].cpu(), want), (j, (c_dev[j].cpu() - want).abs().max().item())
    assert int(status.item()) >> 32 == empty and int(status.item()) & 0xFFFFFFFF == 0


def test_fit_refuses_what_it_does_not_do(dev):
    from siss_amd.kmeans import fit
    rows = torch.randint(100, 140, (40, 48), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    far = np.stack([rows.double().mean(0).numpy(), np.full(48, 255.0)])
    with pytest.raises(RuntimeError, match="empty"):
        fit(rows, n_clusters=2, init=far)
    with pytest.raises(ValueError, match="1 <= K <= 16"):
        fit(rows, n_clusters=17)
    with pytest.raises(ValueError, match="init"):
        fit(rows, n_clusters=2, init="random")
    with pytest.raises(TypeError, match="uint8"):
        fit(rows.float(), n_clusters=2)
    m = fit(rows, n_clusters=2, init=rows[:2].double().numpy(), max_iter=1)      # stopped by max_iter: labels still match the centres
    _, labels, _ = m.predict(rows)
    assert m.n_iter_ == 1 and torch.equal(labels, m.labels_)


def test_wrong_feature_order_changes_labels(dev):
    """Negative control: centres flattened CHW instead of HWC are a different classifier."""
    from siss_amd.kmeans import KMeansClassifier
    g = torch.Generator().manual_seed(5)
    h = w = 16
    proto = torch.randint(0, 256, (2, h, w, 3), generator=g)                                   # two images, HWC
    which = torch.arange(32) % 2
    imgs = (proto[which] + torch.randint(-20, 21, (32, h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    right = KMeansClassifier(proto.flatten(1).float())
    wrong = KMeansClassifier(proto.permute(0, 3, 1, 2).flatten(1).float())
    _, l_right, d_right = right.predict(imgs)
    _, l_wrong, d_wrong = wrong.predict(imgs)
    assert l_right.cpu().tolist() == which.tolist()
    ref_wrong = _f64_dist(imgs.to(dev), wrong.centres(dev))
    assert relative_gap(ref_wrong.cpu().numpy()).min() >= 1e-3
    assert torch.equal(l_wrong.long(), ref_wrong.argmin(1))                                    # it computes what it was given ...
    assert not torch.equal(l_wrong, l_right)                                                   # ... which is not the right answer


def test_kmeans_plusplus_seeding(dev, golden):
    from siss_amd.kmeans import fit, kmeans_plusplus
    z, cases = golden
    X = torch.from_numpy(z[cases[3] + "_X"]).to(dev)
    rows = {bytes(r) for r in z[cases[3] + "_X"]}
    for k in (1, 2, 3, 8):
        c = kmeans_plusplus(X, k, torch.Generator().manual_seed(11)).cpu()
        assert c.shape == (k, 192) and all(bytes(r.to(torch.uint8).numpy()) in rows for r in c) and torch.equal(c, c.round())
        assert len({bytes(r.numpy()) for r in c}) == k                                        # distinct rows
        assert torch.equal(c, kmeans_plusplus(X, k, torch.Generator().manual_seed(11)).cpu())  # deterministic under the seed
    assert not torch.equal(kmeans_plusplus(X, 3, torch.Generator().manual_seed(11)).cpu(),
                           kmeans_plusplus(X, 3, torch.Generator().manual_seed(12)).cpu())
    a = fit(X, n_clusters=3, n_init=3, generator=torch.Generator().manual_seed(4))
    b = fit(X, n_clusters=3, n_init=3, generator=torch.Generator().manual_seed(4))
    one = fit(X, n_clusters=3, n_init=1, generator=torch.Generator().manual_seed(4))
    assert np.array_equal(a.cluster_centers_, b.cluster_centers_) and a.inertia_ == b.inertia_ and a.inertia_ <= one.inertia_


# ---------------------------------------------------------------- 3. full size
def test_full_size_against_f64_on_the_gpu(dev):
    """n = 8 decoder outputs of 3 x 512 x 512 (D = 786,432), centres = two random images; each input is a noisy copy of one of them,
    so the two distances of a row differ by far more than the fixtures' 1e-3 -- asserted."""
    from siss_amd.kmeans import KMeansClassifier, fit
    g = torch.Generator(device=dev).manual_seed(9)
    proto = torch.randint(0, 256, (2, 512, 512, 3), generator=g, device=dev, dtype=torch.uint8)
    which = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=dev)
    noisy = proto[which].float() + 30 * torch.randn(8, 512, 512, 3, generator=g, device=dev)
    img = (noisy / 255 * 2 - 1).permute(0, 3, 1, 2).contiguous()                               # what a decoder returns: [n, 3, H, W]
    clf = KMeansClassifier(proto.flatten(1).float())
    for dtype in (torch.float32, torch.bfloat16):
        x = img.to(dtype)
        u8, labels, dist = clf.from_decoded(x)
        want = _torch_u8(x)
        assert torch.equal(u8, want)
        ref = _f64_dist(want, clf.centres(dev))
        gap = relative_gap(ref.cpu().numpy()).min()
        assert gap >= 1e-3, gap
        _within(dist, ref, f"full size {dtype}")
        assert torch.equal(labels.long(), ref.argmin(1)) and labels.tolist() == which.tolist()
        _, labels2, dist2 = clf.predict(u8)
        _within(dist2, ref, "full size assign")
        assert torch.equal(labels2, labels)
    m = fit(u8.flatten(1), n_clusters=2, init=u8.flatten(1)[:2].float().cpu().numpy())         # rows 0 and 1: one of each group
    assert m.labels_.tolist() == which.tolist() and m.n_iter_ == 2
    for j in (0, 1):
        want_c = (u8.flatten(1)[which == j].double().sum(0) / int((which == j).sum())).float()
        assert torch.equal(torch.from_numpy(m.cluster_centers_[j]).to(dev), want_c)


# ---------------------------------------------------------------- 4. DeleteSD
def _crop(path, k, size=32, cols=1, pad=2):
    from PIL import Image
    a = np.asarray(Image.open(path))
    r, q = divmod(k, cols)
    return a[r * (size + pad) + pad:r * (size + pad) + pad + size, q * (size + pad) + pad:q * (size + pad) + pad + size]


def test_delete_sd_fraction_end_to_end(dev, tmp_path):
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
    evals = ["training_steps=3", "eval_every=1", "+eval_batches=2", "+eval_batch_size=1", "+pipeline.num_inference_steps=3", "resolution=32"]
    # the key null (the shipped default): the files of before, nothing else
    _, _, cfg0 = _run(tmp_path, "plain", ckpt, evals, prompt)
    assert cfg0.metrics.fraction_deletion is None
    assert sorted(os.listdir(cfg0.output_dir)) == sorted(["train_log_rank0.jsonl", "noise_norms_rank0.jsonl"] +
                                                         [f"validation_p0_step{s}.png" for s in (1, 2, 3)])
    # one centre from what the seeded pipeline itself produces, the other far away
    own = _crop(os.path.join(cfg0.output_dir, "validation_p0_step1.png"), 0).reshape(-1).astype(np.float32)
    far = np.where(own < 128, 255.0, 0.0).astype(np.float32)
    KMeansClassifier(np.stack([far, own])).save(str(tmp_path / "own_is_memorized.npz"))
    KMeansClassifier(np.stack([own, far])).save(str(tmp_path / "far_is_memorized.npz"))
    seen, chain = {}, {}

    def hook(task):
        inner = task.evaluate

        def evaluate(unet, sched, forget_image, step, device):
            e = unet.engine
            torch.cuda.synchronize()
            flat, shadow = e.ps.flat.clone(), e.ps.shadow.clone()
            fused = task.kmeans.from_decoded

            def from_decoded(img):                       # what torch's chain makes of the SAME decoder output, per classified batch
                chain.setdefault(step, []).extend(_torch_u8(img).cpu().numpy())
                return fused(img)
            task.kmeans.from_decoded = from_decoded
            try:
                inner(unet, sched, forget_image, step, device)
            finally:
                task.kmeans.from_decoded = fused
            torch.cuda.synchronize()
            assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)      # evaluation only reads the weights
            seen[step] = True
        task.evaluate = evaluate

    for name, want_frac in (("own_is_memorized", 1.0), ("far_is_memorized", 0.0)):
        seen.clear()
        chain.clear()
        _, _, cfg = _run(tmp_path, name, ckpt, evals + [f"metrics.fraction_deletion.classifier_path={tmp_path}/{name}.npz"], prompt, hook)
        assert seen == {1: True, 2: True, 3: True}
        lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))]
        print(name, lines)
        assert [r["global_step"] for r in lines] == [1, 2, 3]
        assert all(r["deletion_fraction_0"] == want_frac for r in lines)
        steps = [r["deletion_steps_0"] for r in lines if "deletion_steps_0" in r]
        assert steps == ([1] if want_frac == 0 else [])                                    # once, at the first zero, never otherwise
        assert sorted(os.listdir(cfg.output_dir)) == sorted(os.listdir(cfg0.output_dir) + ["metrics_rank0.jsonl"])
        assert len(open(os.path.join(cfg.output_dir, "noise_norms_rank0.jsonl")).readlines()) == 3
        # the grid is made of the fused launch's uint8 images: bit for bit torch's chain on the decoder output of THIS run (two runs
        # of this task are not bitwise alike -- their weights differ by ~3e-8 after two steps and the sampled pixels by a grey level
        # here and there -- so the plain run's grids are compared by size only)
        for s in (1, 2, 3):
            path = os.path.join(cfg.output_dir, f"validation_p0_step{s}.png")
            assert len(chain[s]) == 2
            for k in (0, 1):
                assert np.array_equal(_crop(path, k), chain[s][k]), (s, k)
            assert Image.open(path).size == Image.open(os.path.join(cfg0.output_dir, f"validation_p0_step{s}.png")).size
    # refused before the first step
    with pytest.raises(ValueError, match="features"):
        _run(tmp_path, "bad", ckpt, ["training_steps=1", "resolution=64",
                                     f"metrics.fraction_deletion.classifier_path={tmp_path}/own_is_memorized.npz"], prompt)
    assert not os.path.exists(os.path.join(str(tmp_path), "bad", "train_log_rank0.jsonl"))
    assert lib.PROF is None


def test_sampler_decoded_output_type(dev):
    from test_hip_sd_sampling import _tiny_models
    from siss_amd.sd_sampler import SDSampler
    unet, _, vae, _ = _tiny_models(dev, torch.bfloat16)
    gen = torch.Generator().manual_seed(5)
    text, neg = torch.randn(2, 77, 64, generator=gen).to(dev), torch.randn(1, 77, 64, generator=gen).to(dev)
    lat = torch.randn(2, 4, 16, 16, generator=gen).to(dev)
    pipe = SDSampler(unet, vae=vae)
    kw = dict(negative_prompt_embeds=neg.expand(2, -1, -1), num_inference_steps=3, guidance_scale=7.5, latents=lat)
    raw, st = pipe(text, output_type="decoded", **kw)
    u8, st2 = pipe(text, output_type="np", **kw)
    assert raw.is_cuda and raw.shape == (2, 3, 32, 32) and raw.dtype in (torch.float32, torch.bfloat16) and st == st2
    assert np.array_equal(_torch_u8(raw).cpu().numpy(), u8)
    with pytest.raises(ValueError, match="decoded"):
        pipe(text, output_type="tensor", **kw)

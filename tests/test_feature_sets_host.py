"""CPU tests of siss_amd/feature_sets.py on the emulated launchers of tests/feature_sets_ref.py: the reference itself against
scikit-learn, the estimator arithmetic of KernelInceptionDistance and PRDC against the reference, the subset tables, every refusal,
FeatureBank's file, and the fid_rank0.jsonl record with and without `metrics.fid.sets`."""
import json
import os

import numpy as np
import pytest
import torch

import feature_sets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def emulated(monkeypatch):
    """The module's three doors to the library answered by the reference's emulation."""
    from siss_amd import feature_sets as F

    def launch(name, *a):
        rc = R.call(name, *a)
        assert rc is not None, name
        if rc:
            raise RuntimeError(f"{name} failed with status {rc} (bad argument)")
        return 0

    def ws(name, *a):
        n = R.ws_bytes(name, *a)
        if n < 0:
            raise ValueError(f"{name}{a} refused its arguments")
        return n

    monkeypatch.setattr(F, "_launch", launch)
    monkeypatch.setattr(F, "_ws_bytes", ws)
    monkeypatch.setattr(F, "require_kernels", lambda: None)
    return F


def gauss(n, d, seed, shift=0.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) + shift).astype(np.float32)


# ---------------------------------------------------------------- the reference against scikit-learn
def test_reference_against_scikit_learn():
    from sklearn.metrics import pairwise_distances
    from sklearn.metrics.pairwise import polynomial_kernel
    from sklearn.neighbors import NearestNeighbors
    real, fake, d = gauss(70, 16, 0), gauss(45, 16, 1, 0.3), 16
    r64, f64 = real.astype(np.float64), fake.astype(np.float64)
    for k in (1, 5, 16):
        dist, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(r64).kneighbors(r64)
        want = dist[:, k] ** 2
        got = R.radii(R.d2_64(real, real), k)
        assert np.abs(got - want).max() <= 1e-9 * want.max()
        # the ball decisions, on data without ties: no distance within 1e-9 of a radius
        pd = pairwise_distances(f64, r64) ** 2
        assert np.abs(pd - got[None, :]).min() > 1e-9
        inside, mn, arg = R.ball(R.d2_64(fake, real), got)
        assert (inside == (pd <= want[None, :]).sum(1)).all() and (arg == pd.argmin(1)).all()
        assert np.abs(mn - pd.min(1)).max() <= 1e-9 * pd.max()
    assert np.isinf(R.radii(R.d2_64(real[:5], real[:5]), 5)).all() and np.isfinite(R.radii(R.d2_64(real[:6], real[:6]), 5)).all()
    # the kernel sums
    g = torch.Generator().manual_seed(0)
    ix = torch.stack([torch.randperm(70, generator=g)[:20] for _ in range(3)]).numpy()
    iy = torch.stack([torch.randperm(45, generator=g)[:20] for _ in range(3)]).numpy()
    got = R.kernel_sums(real, ix, fake, iy, 1.0 / d, 1.0)
    for b in range(3):
        xs, ys = r64[ix[b]], f64[iy[b]]
        kxx, kyy, kxy = (polynomial_kernel(p, q, degree=3, gamma=1.0 / d, coef0=1) for p, q in ((xs, xs), (ys, ys), (xs, ys)))
        want = np.array([kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()])
        assert np.abs(got[b] - want).max() <= 1e-12 * np.abs(want).max()


def test_bound_holds_for_the_emulated_distance():
    """b(a, b) of the reference against the emulation's f32 distance (the kernel's arithmetic, restated) on the issue's recipe at a
    small size; and the recipe's f64 figures at k = 5 as the issue states them."""
    real, fake = R.realistic(40, 24, 2048, 0)
    v, nan = R.d2_32(R.chain_sims(fake, real), R.sq32(fake), R.sq32(real))
    assert not nan.any()
    err, b = np.abs(v.astype(np.float64) - R.d2_64(fake, real)), R.bound(fake, real)
    assert (err <= b).all() and err.max() > 0
    print(f"\nworst error / bound: {(err / b).max():.3f}")


def test_the_recipe_has_the_stated_f64_figures():
    real, fake = R.realistic()
    got = R.prdc(real, fake, 5)
    assert (round(got["precision"], 3), round(got["density"], 3), round(got["coverage"], 3)) == (0.940, 0.917, 0.653)
    assert 0.05 < got["recall"] < 0.95


# ---------------------------------------------------------------- the estimators on the emulation
def test_prdc_arithmetic_against_the_reference(emulated):
    F = emulated
    real, fake = R.exact_rows(61, 20, 0), R.exact_rows(37, 20, 1)          # exact data: the emulation's distances ARE the f64 ones
    rb, fb = F.FeatureBank(20, 80, "cpu"), F.FeatureBank(20, 40, "cpu")
    rb.append(torch.from_numpy(real[:30])); rb.append(torch.from_numpy(real[30:]))
    fb.append(torch.from_numpy(fake))
    assert len(rb) == 61 and rb.rows.shape == (61, 20) and len(fb) == 37
    for k in (1, 5):
        got = F.PRDC(k).compute(rb, fb)
        want = R.prdc(real, fake, k, dist=R.exact_d2)
        assert got == pytest.approx(want, abs=1e-15), (k, got, want)
        assert list(got) == ["precision", "recall", "density", "coverage"]
    # the real side's norms and radii are cached on the bank, and dropped when its rows change
    assert set(rb.cache) == {"sq", ("prdc", 1), ("prdc", 5)}
    kept = rb.cache["sq"]
    F.PRDC(5).compute(rb, fb)
    assert rb.cache["sq"] is kept
    rb.append(torch.from_numpy(real[:1]))
    assert rb.cache == {}
    with pytest.raises(ValueError, match="at least 6 rows"):
        fb5 = F.FeatureBank(20, 5, "cpu")
        fb5.append(torch.from_numpy(fake[:5]))
        F.PRDC(5).compute(rb, fb5)


def test_kid_arithmetic_and_tables(emulated):
    F = emulated
    real, fake, d = gauss(50, 12, 3), gauss(40, 12, 4, 0.2), 12
    kid = F.KernelInceptionDistance(subsets=4, subset_size=17, seed=7)
    kid.update_features(torch.from_numpy(real[:20]), real=True)
    kid.update_features(torch.from_numpy(real[20:]), real=True)
    kid.update_features(torch.from_numpy(fake), real=False)
    mean, std = kid.compute()
    ir, if_ = F.subset_tables(50, 40, 4, 17, 7)
    # the tables are torchmetrics' draws, reproducible from the seed
    g = torch.Generator().manual_seed(7)
    for b in range(4):
        assert torch.equal(ir[b], torch.randperm(50, generator=g)[:17]) and torch.equal(if_[b], torch.randperm(40, generator=g)[:17])
    again = F.subset_tables(50, 40, 4, 17, 7)
    assert torch.equal(again[0], ir) and torch.equal(again[1], if_) and not torch.equal(F.subset_tables(50, 40, 4, 17, 8)[0], ir)
    sums = R.kernel_sums(real, ir.numpy(), fake, if_.numpy(), 1.0 / d, 1.0)
    wm, ws = R.kid(sums, 17)
    tol = 1e-6 * abs(sums).max() / 17 ** 2                     # f32 dots against f64 dots
    assert abs(float(mean) - wm) <= tol and abs(float(std) - ws) <= tol
    vals = torch.from_numpy(R.kid_values(sums, 17))
    assert ws == pytest.approx(float(vals.std(unbiased=False)), rel=1e-12)          # torchmetrics' population std
    m2, s2 = kid.compute()
    assert float(m2) == float(mean) and float(s2) == float(std)                     # the same tables at every compute()
    kid.reset()                                                                      # the fake side only
    with pytest.raises(ValueError, match="Argument `subset_size` should be smaller than the number of samples"):
        kid.compute()
    kid.update_features(torch.from_numpy(fake), real=False)
    assert float(kid.compute()[0]) == float(mean)
    # gamma and coef reach the launcher
    k2 = F.KernelInceptionDistance(subsets=2, subset_size=9, gamma=0.5, coef=2.0, seed=1)
    k2.update_features(torch.from_numpy(real), True); k2.update_features(torch.from_numpy(fake), False)
    ir, if_ = F.subset_tables(50, 40, 2, 9, 1)
    wm, _ = R.kid(R.kernel_sums(real, ir.numpy(), fake, if_.numpy(), 0.5, 2.0), 9)
    assert float(k2.compute()[0]) == pytest.approx(wm, rel=1e-5)


# ---------------------------------------------------------------- refusals
def test_refusals_by_message(emulated):
    F = emulated
    K = F.KernelInceptionDistance
    with pytest.raises(ValueError, match="only the cubic kernel"):
        K(degree=2)
    with pytest.raises(ValueError, match="`subsets`"):
        K(subsets=0)
    with pytest.raises(ValueError, match="`subset_size`"):
        K(subset_size=1)
    with pytest.raises(ValueError, match="`gamma`"):
        K(gamma=-1.0)
    with pytest.raises(ValueError, match="`coef`"):
        K(coef=0.0)
    with pytest.raises(ValueError, match="`seed`"):
        K(seed=1.5)
    kid = K(subsets=1, subset_size=10)
    kid.update_features(torch.zeros(12, 8), True); kid.update_features(torch.zeros(9, 8), False)
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        kid.compute()
    for k in (0, 17, True, 2.0):
        with pytest.raises(ValueError, match="1 .. 16"):
            F.PRDC(k)
    x = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="d % 4 == 0"):
        F.sqnorm(torch.zeros(3, 6))
    with pytest.raises(ValueError, match="d % 4 == 0"):
        F.sqnorm(torch.zeros(3, 4100))
    with pytest.raises(ValueError, match="f32 rows"):
        F.sqnorm(torch.zeros(0, 8))
    with pytest.raises(ValueError, match="f32 rows"):
        F.sqnorm(torch.zeros(3, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="1 .. 16"):
        F.knn_radius(x, torch.zeros(6), 17)
    with pytest.raises(ValueError, match="rows of 8"):
        F.ball_stats(torch.zeros(2, 12), torch.zeros(2), x, torch.zeros(6))
    with pytest.raises(ValueError, match="outside 0 .. 5"):
        F.kid_sums(x, torch.tensor([[0, 6]]), x, torch.tensor([[0, 1]]), 1.0, 1.0)
    with pytest.raises(ValueError, match="one shape"):
        F.kid_sums(x, torch.tensor([[0, 1]]), x, torch.tensor([[0, 1, 2]]), 1.0, 1.0)
    with pytest.raises(ValueError, match="capacity"):
        F.FeatureBank(8, 0, "cpu")
    bank = F.FeatureBank(8, 4, "cpu")
    with pytest.raises(ValueError, match="do not fit the capacity"):
        bank.append(torch.zeros(5, 8))
    with pytest.raises(ValueError, match=r"\[N, 8\] features"):
        bank.append(torch.zeros(2, 12))


def test_launcher_refusals_of_the_emulation():
    """What the launchers refuse (status 1), as the emulation restates it: d outside 4 .. 4096 or d % 4, no rows, k outside 1 .. 16, a
    missing or too-small work buffer; and the *_ws_bytes queries' -1."""
    x, sq, big = torch.zeros(6, 8), torch.zeros(6), torch.zeros(1 << 12, dtype=torch.int64)
    r, i32 = torch.zeros(6), torch.zeros(6, dtype=torch.int32)
    assert R.call("siss_feat_sqnorm", x, 6, 8, sq) == 0
    assert R.call("siss_feat_sqnorm", torch.zeros(6, 6), 6, 6, sq) == 1 and R.call("siss_feat_sqnorm", torch.zeros(6, 4100), 6, 4100, sq) == 1
    assert R.call("siss_feat_sqnorm", torch.zeros(0, 8), 0, 8, sq) == 1
    assert R.call("siss_feat_knn_radius", x, 6, 8, sq, 5, r, big, big.numel() * 8) == 0
    for k in (0, 17):
        assert R.call("siss_feat_knn_radius", x, 6, 8, sq, k, r, big, big.numel() * 8) == 1 and R.ws_bytes("siss_feat_knn_ws_bytes", 6, k) == -1
    assert R.call("siss_feat_knn_radius", x, 6, 8, sq, 5, r, None, 0) == 1
    assert R.call("siss_feat_knn_radius", x, 6, 8, sq, 5, r, big, R.ws_bytes("siss_feat_knn_ws_bytes", 6, 5) - 1) == 1
    assert R.call("siss_feat_ball_stats", x, 6, sq, x, 6, sq, r, 8, -1, i32, r.clone(), i32.clone(), big, big.numel() * 8) == 0
    assert R.call("siss_feat_ball_stats", x, 6, sq, x, 6, sq, r, 8, -1, i32, r.clone(), i32.clone(), big, 8) == 1
    assert R.call("siss_feat_ball_stats", x, 6, sq, x, 6, sq, r, 8, -1, i32, r.clone(), i32.clone(), None, 0) == 1
    assert R.ws_bytes("siss_feat_ball_ws_bytes", 0, 5) == -1 and R.ws_bytes("siss_feat_ball_ws_bytes", 5, 0) == -1
    ix, out = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.float64)
    assert R.call("siss_kid_sums", x, 6, ix, x, 6, ix, 8, 2, 3, 0.125, 1.0, out, big, big.numel() * 8) == 0
    assert R.call("siss_kid_sums", x, 6, ix, x, 6, ix, 8, 2, 3, 0.125, 1.0, out, big, 8) == 1
    assert R.ws_bytes("siss_kid_ws_bytes", 0, 3) == -1 and R.ws_bytes("siss_kid_ws_bytes", 2, 0) == -1
    # the work buffers are linear in rows x pieces: 30,000 rows against themselves need megabytes, not 3.6 GB
    assert R.ws_bytes("siss_feat_knn_ws_bytes", 30000, 16) <= 30000 * R.MAX_PIECES * 16 * 4
    assert R.ws_bytes("siss_feat_knn_ws_bytes", 30000, 5) < 16 << 20 and R.ws_bytes("siss_feat_ball_ws_bytes", 30000, 10000) < 16 << 20
    assert R.ws_bytes("siss_kid_ws_bytes", 100, 1000) < 1 << 20


def test_no_fall_back_without_the_entry_points(monkeypatch):
    from siss_amd import feature_sets as F, lib
    monkeypatch.setattr(lib, "has", lambda name: name != "siss_kid_sums")
    with pytest.raises(RuntimeError, match="no siss_kid_sums"):
        F.sqnorm(torch.zeros(4, 8))
    monkeypatch.setattr(F, "require_kernels", lambda: None)
    with pytest.raises(RuntimeError, match="device only"):
        F._launch("siss_feat_sqnorm", torch.zeros(4, 8), 4, 8, torch.zeros(4))


# ---------------------------------------------------------------- the bank's file
def test_feature_bank_save_load_and_fingerprint(tmp_path):
    from siss_amd import feature_sets as F
    f = torch.from_numpy(gauss(9, 16, 5))
    bank = F.FeatureBank(16, 12, "cpu")
    bank.append(f)
    imgs = []
    for i in range(2):
        p = tmp_path / f"{i}.jpg"
        p.write_bytes(b"x" * (i + 1))
        imgs.append(str(p))

    class Net:
        def __init__(self, w):
            self.w = w

        def state_dict(self):
            return {"a.weight": self.w}

    fp = F.real_fingerprint(Net(torch.ones(3)), imgs)
    assert set(fp) == {"model", "files", "n"} and fp["n"] == 2
    path = tmp_path / "sub" / "real.safetensors"
    assert not F.FeatureBank.exists(path)
    bank.save(path, fp)
    assert F.FeatureBank.exists(path) and F.FeatureBank.matches(path, fp)
    back = F.FeatureBank.load(path, fp, "cpu", capacity=20)
    assert len(back) == 9 and back.capacity == 20 and torch.equal(back.rows, f)
    # other weights, or a file that changed size: another fingerprint, refused
    other = F.real_fingerprint(Net(torch.zeros(3)), imgs)
    assert other["model"] != fp["model"] and not F.FeatureBank.matches(path, other)
    with pytest.raises(ValueError, match="another fingerprint"):
        F.FeatureBank.load(path, other)
    (tmp_path / "0.jpg").write_bytes(b"xyz")
    changed = F.real_fingerprint(Net(torch.ones(3)), imgs)
    assert changed["files"] != fp["files"]
    with pytest.raises(ValueError, match="another fingerprint"):
        F.FeatureBank.load(path, changed)
    bank.clear()
    assert len(bank) == 0 and bank.rows.shape == (0, 16)


# ---------------------------------------------------------------- the key and the record
def test_parse_config_refusals():
    from siss_amd import feature_sets as F
    P = F.parse_config
    assert P(None, 100) is None
    got = P({"kid": {"subsets": 3, "subset_size": 8}, "prdc": {"k": 2}}, 12)
    assert got == {"kid": {"subsets": 3, "subset_size": 8, "seed": 0}, "prdc": {"k": 2}, "real_features_path": None, "max_bytes": 2_000_000_000}
    assert P({"kid": None, "prdc": {"k": 5}}, 12)["kid"] is None and P({"kid": {"subset_size": 10}}, 12)["prdc"] is None
    for bad, msg in (({"kidd": {}}, "unknown field"), ({"kid": {"size": 3}}, "unknown field"), ({"prdc": {"kk": 3}}, "unknown field"),
                     ("on", "a mapping"), ({"prdc": {"k": 0}}, "1 .. 16"), ({"prdc": {"k": 17}}, "1 .. 16"),
                     ({"prdc": {"k": 12}}, "no 12-th other neighbour"), ({"kid": {"subset_size": 13}}, "larger than metrics.fid.num_imgs_to_generate"),
                     ({"kid": {"degree": 2}}, "unknown field"), ({"kid": {"subsets": 0}}, "`subsets`"),
                     ({"max_bytes": 0}, "max_bytes"), ({"prdc": {"k": 2}, "max_bytes": 1000}, "does not fit")):
        with pytest.raises(ValueError, match=msg):
            P(bad, 12)


def _task(extra, tmp_path):
    from siss_amd import hydra_lite as H
    data = tmp_path / "real"
    data.mkdir(exist_ok=True)
    base = {"class_cfg._target_": "metrics.fid.FIDEvaluator", "class_cfg.inception_batch_size": 8, "class_cfg.allow_random_init": "true",
            "class_cfg.data_path": str(data), "step_frequency": 5, "num_imgs_to_generate": 16, "batch_size": 4}
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), [*(f"+metrics.fid.{k}={v}" for k, v in base.items()), *extra])
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


def test_check_metrics_refuses_a_sets_block_that_cannot_run(tmp_path):
    _task(["+metrics.fid.sets={kid:{subsets:100,subset_size:16,seed:0},prdc:{k:5},real_features_path:null,max_bytes:2000000000}"],
          tmp_path).check_metrics()
    _task(["+metrics.fid.sets={kid:null,prdc:{k:5}}"], tmp_path).check_metrics()
    _task(["+metrics.fid.sets=null"], tmp_path).check_metrics()
    for bad, msg in (("{kid:{subset_size:17}}", "larger than"), ("{prdc:{k:16}}", "no 16-th"), ("{prdc:{k:17}}", "1 .. 16"),
                     ("{prcd:{k:5}}", "unknown field"), ("{prdc:{k:5},max_bytes:4096}", "does not fit")):
        with pytest.raises(ValueError, match=msg):
            _task([f"+metrics.fid.sets={bad}"], tmp_path).check_metrics()
    # the real features need the images: a statistics file does not stand in for them
    stats = tmp_path / "stats.npz"
    stats.write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="metrics.fid.sets"):
        _task([f"+metrics.fid.class_cfg.data_path={tmp_path}/nodir", f"+metrics.fid.class_cfg.real_stats_path={stats}",
               "+metrics.fid.sets={prdc:{k:5}}"], tmp_path).check_metrics()
    # the key is absent from the YAML
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), [])
    assert "fid" not in (cfg.get("metrics") or {})


class _Stats:
    """FrechetInceptionDistance without its launcher: counts, and the sink."""

    def __init__(self, sink=None):
        self.real_features_num_samples, self.fake_features_num_samples, self.sink = 0, 0, sink

    def reset(self):
        self.fake_features_num_samples = 0

    def update_features(self, f, real):
        if real:
            self.real_features_num_samples += len(f)
        else:
            self.fake_features_num_samples += len(f)
        if self.sink is not None:
            self.sink(f, real)


class _Evaluator:
    def __init__(self, sink=None, keep=None):
        self.fid_computer, self.keep = _Stats(sink), keep

    def add_fake_images(self, f):
        self.fid_computer.update_features(f if self.keep is None else f[:self.keep], real=False)

    def compute(self, reset=True):
        return torch.tensor(1.5)


TODAY = ["global_step", "fid", "fake_images", "real_images", "seconds"]


def _run(tmp_path, name, sets, keep=None):
    from siss_amd.fid import FIDTracker
    fake = torch.from_numpy(R.exact_rows(12, 16, 2))
    ev = _Evaluator(sets, keep)
    if sets is not None:
        sets.open_real(20)
    ev.fid_computer.update_features(torch.from_numpy(R.exact_rows(20, 16, 1)), real=True)
    tr = FIDTracker(ev, str(tmp_path / name), lambda n, s=[0]: (fake[s[0]:s[0] + n], s.__setitem__(0, (s[0] + n) % 12))[0], 2, 12, 4, sets=sets)
    assert tr(1) is None
    tr(0), tr(2)
    return [json.loads(l) for l in open(tmp_path / name)], fake


def test_record_without_the_key_is_todays(tmp_path):
    lines, _ = _run(tmp_path, "plain.jsonl", None)
    assert len(lines) == 2 and all(list(l) == TODAY for l in lines)
    assert lines[0]["fid"] == 1.5 and lines[0]["fake_images"] == 12 and lines[0]["real_images"] == 20
    # and the classes take no sink unless one is given
    import inspect
    from siss_amd.fid import FIDEvaluator, FIDTracker, FrechetInceptionDistance
    assert inspect.signature(FrechetInceptionDistance.__init__).parameters["sink"].default is None
    assert inspect.signature(FIDEvaluator.__init__).parameters["feature_sets"].default is None
    assert inspect.signature(FIDTracker.__init__).parameters["sets"].default is None


def test_record_with_the_key_and_the_skipped_path(tmp_path, emulated):
    F = emulated
    settings = F.parse_config({"kid": {"subsets": 3, "subset_size": 8}, "prdc": {"k": 2}}, 12, 16)
    lines, fake = _run(tmp_path, "sets.jsonl", F.FeatureSets(settings, 12, "cpu", 16))
    real = R.exact_rows(20, 16, 1)
    want = R.prdc(real, fake.numpy(), 2, dist=R.exact_d2)
    ir, if_ = F.subset_tables(20, 12, 3, 8, 0)
    wm, ws = R.kid(R.kernel_sums(real, ir.numpy(), fake.numpy(), if_.numpy(), 1.0 / 16, 1.0), 8)
    assert len(lines) == 2
    for l in lines:
        assert list(l) == TODAY + list(F.RECORD_FIELDS)
        assert (l["kid_subsets"], l["kid_subset_size"], l["prdc_k"]) == (3, 8, 2) and l["sets_seconds"] >= 0
        assert {k: l[k] for k in want} == pytest.approx(want, abs=1e-15)
        assert l["kid_mean"] == pytest.approx(wm, rel=1e-12, abs=1e-15) and l["kid_std"] == pytest.approx(ws, rel=1e-9, abs=1e-15)
    # filter_fake left 1 of every 4 generated rows: 3 < subset_size and 3 = k + 1 -> KID null with the reason, PRDC computed
    lines, _ = _run(tmp_path, "few.jsonl", F.FeatureSets(settings, 12, "cpu", 16), keep=1)
    for l in lines:
        assert l["fake_images"] == 3 and l["kid_mean"] is None and l["kid_std"] is None and l["precision"] is not None
        assert "kid: 3 generated rows are fewer than subset_size=8" in l["sets_skipped"] and "prdc" not in l["sets_skipped"]
    s2 = F.parse_config({"prdc": {"k": 3}}, 12, 16)
    lines, _ = _run(tmp_path, "fewer.jsonl", F.FeatureSets(s2, 12, "cpu", 16), keep=1)
    for l in lines:
        assert all(l[k] is None for k in ("precision", "recall", "density", "coverage")) and l["prdc_k"] == 3
        assert l["sets_skipped"] == "prdc: 3 generated rows are fewer than k + 1 = 4" and "kid_mean" not in l
    # the real side is checked when it is loaded
    with pytest.raises(ValueError, match="larger than the real set of 5"):
        F.FeatureSets(settings, 12, "cpu", 16).open_real(5)
    with pytest.raises(ValueError, match="do not fit max_bytes"):
        F.FeatureSets(F.parse_config({"prdc": {"k": 2}, "max_bytes": 1024}, 12, 16), 12, "cpu", 16).open_real(20)

"""Host side of the SD k-means deletion fraction (siss_amd/kmeans.py, data.SDData, DeleteSD's opt-in metric, tools/make_sd_clusters.py):
the float64 Lloyd restatement against the scikit-learn results recorded in tests/golden/kmeans_ref.npz (tests/make_kmeans_golden.py),
loaders, dataset, config plumbing, refusals and the deletion_steps tracker.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from kmeans_ref import distances, host_fit, lloyd_f64, relative_gap, synthetic_set  # noqa: E402

CENTRE_TOL = 2.0 ** -17 + 1e-9        # half an f32 ulp below 256 (centres are grey levels), plus f64 noise of the reference


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "kmeans_ref.npz"))
    return z, [str(c) for c in z["cases"]]


def test_golden_cases_are_the_documented_ones(golden):
    z, cases = golden
    assert len(cases) == 6 and sum(c.startswith("k2_") for c in cases) == 3 and sum(c.startswith("k3_") for c in cases) == 3
    for k in (2, 3):
        assert max(int(z[c + "_n_iter"]) for c in cases if c.startswith(f"k{k}_")) >= 5
    for c in cases:
        k, seed = int(c[1]), int(c.split("_s")[1])
        X, held, init = synthetic_set(k, seed)                       # the file holds exactly what the generator draws
        assert np.array_equal(X, z[c + "_X"]) and np.array_equal(held, z[c + "_held"]) and np.array_equal(init, z[c + "_init"])
        assert z[c + "_X"].dtype == np.uint8 and z[c + "_X"].shape == (160, 192) and float(z[c + "_min_gap"]) >= 1e-3


def test_host_lloyd_reproduces_recorded_sklearn(golden):
    z, cases = golden
    for c in cases:
        r = lloyd_f64(z[c + "_X"], z[c + "_init"])
        assert r["n_iter"] == int(z[c + "_n_iter"]), c
        assert np.array_equal(r["labels"], z[c + "_labels"]), c
        assert r["min_gap"] >= 1e-3, (c, r["min_gap"])
        err = np.abs(r["centres"].astype(np.float32).astype(np.float64) - z[c + "_centres"]).max()
        assert err <= CENTRE_TOL, (c, err)
        assert abs(r["inertia"] - float(z[c + "_inertia"])) <= 1e-9 * float(z[c + "_inertia"]), c
        d = distances(z[c + "_held"], r["centres"])
        assert np.array_equal(d.argmin(1), z[c + "_held_labels"]) and relative_gap(d).min() >= 1e-3, c


def test_host_lloyd_against_live_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    for k, seed in ((2, 7), (3, 8), (4, 9)):
        X, held, init = synthetic_set(k, seed)
        km = cluster.KMeans(n_clusters=k, init=init, n_init=1, tol=0, algorithm="lloyd").fit(X.astype(np.float64))
        r = lloyd_f64(X, init)
        if r["min_gap"] < 1e-9:
            continue                                                  # (a tie: the two distance forms may order it differently)
        assert np.array_equal(r["labels"], km.labels_) and r["n_iter"] == km.n_iter_, (k, seed)
        assert np.abs(r["centres"] - km.cluster_centers_).max() <= 1e-9


def test_uint8_equals_the_reference_feature_for_all_values():
    """delete_sd.py:271 feeds 255 * ToTensor(PIL) in f32: f32(f32(v / 255) * 255) == v for all 256 values, so the integer is the feature."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal((v.float() / 255.0) * 255.0, v.float())
    from siss_amd.data import ToTensor
    assert torch.equal(255 * ToTensor()(v.numpy().reshape(16, 16, 1)).flatten(), v.float())


def test_classifier_files_round_trip(tmp_path):
    from siss_amd.kmeans import KMeansClassifier
    c = np.random.RandomState(0).rand(2, 48).astype(np.float32) * 255
    clf = KMeansClassifier(c)
    assert clf.n_clusters == 2 and clf.n_features == 48 and clf.cluster_centers_.dtype == np.float32
    back = KMeansClassifier.load(clf.save(str(tmp_path / "c.npz")))
    assert np.array_equal(back.cluster_centers_, c)
    np.savez(tmp_path / "other.npz", centres=c)
    with pytest.raises(KeyError, match="cluster_centers"):
        KMeansClassifier.load(tmp_path / "other.npz")
    with pytest.raises(ValueError, match="npz"):
        clf.save(str(tmp_path / "c.joblib"))
    with pytest.raises(ValueError, match="joblib"):
        KMeansClassifier.load(tmp_path / "c.txt")
    with pytest.raises(ValueError, match="1 <= K <= 16"):
        KMeansClassifier(np.zeros((17, 4), np.float32))
    with pytest.raises(ValueError):
        KMeansClassifier(np.zeros(4, np.float32))


def test_classifier_loads_a_pickled_sklearn_kmeans(tmp_path, golden):
    cluster = pytest.importorskip("sklearn.cluster")
    joblib = pytest.importorskip("joblib")
    from siss_amd.kmeans import KMeansClassifier
    z, cases = golden
    c = cases[0]
    km = cluster.KMeans(n_clusters=2, init=z[c + "_init"], n_init=1, tol=0, algorithm="lloyd").fit(z[c + "_X"].astype(np.float64))
    for ext in (".joblib", ".pkl"):
        joblib.dump(km, tmp_path / ("km" + ext))
        clf = KMeansClassifier.load(tmp_path / ("km" + ext))
        assert np.array_equal(clf.cluster_centers_, km.cluster_centers_.astype(np.float32))


def test_pickled_classifier_without_sklearn_is_a_clear_import_error(tmp_path, monkeypatch):
    from siss_amd.kmeans import KMeansClassifier
    (tmp_path / "km.joblib").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "joblib", None)                  # `import joblib` now raises ImportError
    with pytest.raises(ImportError, match="scikit-learn"):
        KMeansClassifier.load(tmp_path / "km.joblib")


def _png_dir(tmp_path, names, size=(6, 4), seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    d = tmp_path / "images"
    d.mkdir(parents=True, exist_ok=True)
    arrays = {}
    for n in names:
        arrays[n] = rng.randint(0, 256, size=(size[1], size[0], 3), dtype=np.uint8)
        Image.fromarray(arrays[n]).save(d / n)
    return str(d) + os.sep, arrays


def test_sddata_names_order_labels_and_items(tmp_path):
    from siss_amd.data import Compose, Normalize, SDData
    labels = {"x_003.png": 1, "x_000.png": 0, "x_002.png": 1, "x_001.png": 0, "x_004.png": 0}       # the FILE's order, not sorted
    img_dir, arrays = _png_dir(tmp_path, labels)
    lp = tmp_path / "kmeans_labels.json"
    json.dump(labels, open(lp, "w"))
    want = {"all": list(labels), "deletion": ["x_003.png", "x_002.png"], "nondeletion": ["x_000.png", "x_001.png", "x_004.png"]}
    for flt, names in want.items():
        ds = SDData(img_dir, str(lp), flt)
        assert ds.img_names == names and len(ds) == len(names)
        assert ds.img_labels.tolist() == [labels[n] for n in names]
        for i, n in enumerate(names):
            img, lab = ds[i]
            assert img.dtype == torch.float32 and img.shape == (3, 4, 6) and int(lab) == labels[n]
            assert torch.equal(img, torch.from_numpy(arrays[n]).permute(2, 0, 1).float())               # 0..255 before the transform
    tr = Compose([Normalize([127.5], [127.5])])
    img, _ = SDData(img_dir, str(lp), "deletion", transform=tr)[0]
    assert torch.equal(img, (torch.from_numpy(arrays["x_003.png"]).permute(2, 0, 1).float() - 127.5) / 127.5)
    with pytest.raises(ValueError, match="Invalid filter"):
        SDData(img_dir, str(lp), "some")


def _cfg(tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    return H.compose("delete_sd", os.path.join(ROOT, "config"), [f"base_dir={tmp_path}", f"output_dir={tmp_path}/out", *overrides])


def test_config_keys_remap_and_dataset_branch(tmp_path):
    from siss_amd import hydra_lite as H
    from siss_amd.data import ImagesOnly, SDData
    from siss_amd.tasks import DeleteSD
    assert H.TARGET_REMAP["data.src.sd_dataset.SDData"] == "siss_amd.data.SDData"
    cfg = _cfg(tmp_path)
    assert cfg.metrics.fraction_deletion is None and cfg.data_files.mem_img_path is None and cfg.deletion.frac_deletion is None
    assert cfg.data_files.labels_path == f"{tmp_path}/kmeans_labels.json"
    assert cfg.data_files.clustering_info_path == f"{tmp_path}/clustering_info.json" and cfg.data_files.img_dir == f"{tmp_path}/images/"
    labels = {"a_001.png": 0, "a_000.png": 1, "a_002.png": 0}
    _png_dir(tmp_path, labels)
    json.dump(labels, open(cfg.data_files.labels_path, "w"))
    tr = H.instantiate(cfg.data_transforms)
    kw = dict(img_dir=cfg.data_files.img_dir, labels_fpath=cfg.data_files.labels_path, transform=tr)     # delete_sd.py:681-682
    ds_all, ds_mem = H.instantiate(cfg.all_data, **kw), H.instantiate(cfg.memorized_data, **kw)
    assert isinstance(ds_all, SDData) and ds_all.img_names == ["a_001.png", "a_002.png"] and ds_mem.img_names == ["a_000.png"]
    assert -1.0 <= float(ds_mem[0][0].min()) and float(ds_mem[0][0].max()) <= 1.0
    # the task takes that branch only with a VAE; without one the later branches decide as before
    task = DeleteSD(cfg)
    with pytest.raises(FileNotFoundError, match="allow_synthetic"):
        task.datasets((4, 8, 8))
    task.vae = object()
    a, m = task.datasets((4, 8, 8))
    assert isinstance(a, ImagesOnly) and len(a) == 2 and len(m) == 1 and torch.is_tensor(m[0]) and m[0].shape == (3, 4, 6)


def test_fill_cfg(tmp_path):
    from siss_amd.tasks import DeleteSD
    cfg = _cfg(tmp_path)
    DeleteSD(cfg).fill_cfg()                                          # no clustering_info.json: the placeholders stay null
    assert cfg.deletion.frac_deletion is None and cfg.data_files.mem_img_path is None
    json.dump({"frac_deletion": 0.375, "mem_idx": 7}, open(cfg.data_files.clustering_info_path, "w"))
    DeleteSD(cfg).fill_cfg()
    assert cfg.deletion.frac_deletion == 0.375
    assert cfg.data_files.mem_img_path == os.path.join(f"{tmp_path}/images/", "sylvester_stallone_007.png")
    cfg2 = _cfg(tmp_path, "deletion.frac_deletion=0.5")               # set by hand: the file is not consulted
    DeleteSD(cfg2).fill_cfg()
    assert cfg2.deletion.frac_deletion == 0.5 and cfg2.data_files.mem_img_path is None


def test_fraction_deletion_refusals(tmp_path):
    from siss_amd.kmeans import KMeansClassifier
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    (ckpt / "vae").mkdir(parents=True)
    good = KMeansClassifier(np.zeros((2, 3 * 8 * 8), np.float32)).save(str(tmp_path / "good.npz"))
    three = KMeansClassifier(np.zeros((3, 3 * 8 * 8), np.float32)).save(str(tmp_path / "three.npz"))
    base = [f"pretrained_model_name_or_path={ckpt}", "resolution=8"]
    check = lambda *ov: DeleteSD(_cfg(tmp_path, *ov)).check_fraction_deletion()
    assert check(*base) is None                                                       # key null (the shipped default)
    cfg = _cfg(tmp_path, *base)
    del cfg["metrics"]
    assert DeleteSD(cfg).check_fraction_deletion() is None                            # no metrics block at all
    clf = check(*base, f"metrics.fraction_deletion.classifier_path={good}")
    assert clf.n_clusters == 2 and clf.n_features == 192
    with pytest.raises(ValueError, match="classifier_path"):
        check(*base, "metrics.fraction_deletion=true")
    with pytest.raises(ValueError, match="classifier_path"):
        check(*base, "metrics.fraction_deletion.other=1")
    with pytest.raises(FileNotFoundError, match="not a file"):
        check(*base, f"metrics.fraction_deletion.classifier_path={tmp_path}/missing.npz")
    with pytest.raises(FileNotFoundError, match="vae"):
        check("resolution=8", f"pretrained_model_name_or_path={tmp_path}/nowhere", f"metrics.fraction_deletion.classifier_path={good}")
    with pytest.raises(ValueError, match="features"):
        check(f"pretrained_model_name_or_path={ckpt}", "resolution=16", f"metrics.fraction_deletion.classifier_path={good}")
    with pytest.raises(ValueError, match="3 clusters"):
        check(*base, f"metrics.fraction_deletion.classifier_path={three}")
    # check_metrics is where run() meets it, before the first step
    task = DeleteSD(_cfg(tmp_path, *base, f"metrics.fraction_deletion.classifier_path={good}"))
    task.check_metrics()
    assert task.kmeans is not None and task.kmeans.n_features == 192


def test_deletion_steps_is_written_once_and_only_at_zero(tmp_path):
    from siss_amd.kmeans import DeletionFraction
    out = tmp_path / "metrics_rank0.jsonl"
    tr = DeletionFraction(None, str(out))
    tr.record(0, torch.tensor([1, 1, 0, 1], dtype=torch.int32), 1)
    tr.record(1, torch.tensor([0, 0, 0, 0], dtype=torch.int32), 1)
    tr.record(0, torch.tensor([0, 0, 0, 0], dtype=torch.int32), 2)
    tr.record(0, torch.tensor([0, 1, 0, 0], dtype=torch.int32), 3)
    tr.record(0, torch.tensor([0, 0, 0, 0], dtype=torch.int32), 4)
    lines = [json.loads(l) for l in open(out)]
    assert lines == [{"global_step": 1, "deletion_fraction_0": 0.75},
                     {"global_step": 1, "deletion_fraction_1": 0.0, "deletion_steps_1": 1},
                     {"global_step": 2, "deletion_fraction_0": 0.0, "deletion_steps_0": 2},
                     {"global_step": 3, "deletion_fraction_0": 0.25},
                     {"global_step": 4, "deletion_fraction_0": 0.0}]
    assert tr.deletion_steps == {0: 2, 1: 1}


def test_new_entry_points_are_declared_and_bound():
    from siss_amd import lib
    names = ("siss_kmeans_decoded", "siss_kmeans_assign", "siss_kmeans_finalize", "siss_kmeans_update", "siss_kmeans_decoded_blocks",
             "siss_kmeans_assign_blocks", "siss_kmeans_update_segments")
    for n in names:
        assert n in lib.SIGNATURES, n
    assert lib.PARAMS["siss_kmeans_decoded"][-1] == "stream" and "stream" not in lib.PARAMS["siss_kmeans_assign_blocks"]
    from siss_amd.build import EXACT
    assert "kmeans.hip" in EXACT


def test_make_sd_clusters_from_dir(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_sd_clusters as M
    finally:
        sys.path.pop(0)
    from siss_amd.kmeans import KMeansClassifier
    rng = np.random.RandomState(3)
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    mem = rng.randint(0, 256, size=(4, 4, 3))
    other = rng.randint(0, 256, size=(4, 4, 3))
    dup = {1, 4, 5, 8, 10}                                            # near-duplicates of one image among a looser group
    arrays = []
    for i in range(12):
        a = mem + rng.randint(-2, 3, size=mem.shape) if i in dup else other + np.rint(25 * rng.randn(*other.shape)).astype(int)
        arrays.append(np.clip(a, 0, 255).astype(np.uint8))
        Image.fromarray(arrays[-1]).save(img_dir / f"sylvester_stallone_{i:03d}.png")
    Image.fromarray(arrays[0]).save(img_dir / "unrelated.png")       # not <images_name>_NNN.png: ignored
    args = ["--from-dir", f"base_dir={tmp_path}"]
    labels, info, clf_path = M.main(args, fit=host_fit)
    assert clf_path == f"{tmp_path}/kmeans_classifier.npz"
    assert labels == json.load(open(tmp_path / "kmeans_labels.json")) and info == json.load(open(tmp_path / "clustering_info.json"))
    assert list(labels) == [f"sylvester_stallone_{i:03d}.png" for i in range(12)]
    assert {int(n[-7:-4]) for n, l in labels.items() if l == 1} == dup
    assert info["frac_deletion"] == 5 / 12 and info["mem_idx"] in dup
    clf = KMeansClassifier.load(clf_path)
    rows = np.stack([a.reshape(-1) for a in arrays]).astype(np.float64)
    assert np.allclose(clf.cluster_centers_[1], rows[sorted(dup)].mean(0), atol=1e-4)                   # centre 1 = memorized
    assert np.allclose(clf.cluster_centers_[0], rows[[i for i in range(12) if i not in dup]].mean(0), atol=1e-4)
    d1 = ((rows - clf.cluster_centers_[1].astype(np.float64)) ** 2).sum(1)
    assert info["mem_idx"] == int(d1.argmin())
    # --mem-image names the memorized cluster instead: an image of the looser group makes THAT one label 1
    labels2, info2, _ = M.main(args + ["--mem-image", str(img_dir / "sylvester_stallone_000.png")], fit=host_fit)
    assert {int(n[-7:-4]) for n, l in labels2.items() if l == 1} == set(range(12)) - dup and info2["frac_deletion"] == 7 / 12
    # the files feed the task: fill_cfg reads the info, SDData the labels
    from siss_amd.data import SDData
    from siss_amd.tasks import DeleteSD
    cfg = _cfg(tmp_path)
    DeleteSD(cfg).fill_cfg()
    assert cfg.deletion.frac_deletion == 7 / 12 and os.path.isfile(cfg.data_files.mem_img_path)
    assert len(SDData(cfg.data_files.img_dir, cfg.data_files.labels_path, "deletion")) == 7

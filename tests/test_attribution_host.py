"""siss_amd/attribution.py and tests/attribution_ref.py on the host (no GPU).

* The counter hash of csrc/attribution.hip, restated by attribution_ref.signs, is a usable Rademacher matrix: column sums, row sums,
  column correlations and norm preservation within the stated conditions at n = 4096, k = 256 for three seeds; rows far down the buffer
  (the SD length, and past 2^32) are no copies of the first rows.
* The timestep table and the per-index seeding of GradientFeatures.
* Attributor (store on the CPU) against a dense f64 numpy.linalg.solve at 1e-10 relative, N = 48, k = 64; the damping rule.
* Every refusal by message; the store's round trip; the forget list read back by data.CelebAHQ.
"""
import os
import sys

import numpy as np
import pytest
import torch

import attribution_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 12345)
N, K = 4096, 256


# ================================================================ 1. the hash
@pytest.mark.parametrize("seed", SEEDS)
def test_hash_is_a_usable_rademacher_matrix(seed):
    s = R.signs(seed, 0, N, K)
    assert s.shape == (N, K) and s.dtype == np.int8 and set(np.unique(s)) == {-1, 1}
    f = s.astype(np.float64)
    col, row = np.abs(f.sum(0)).max(), np.abs(f.sum(1)).max()
    corr = f.T @ f / N
    off = np.abs(corr - np.diag(np.diag(corr))).max()
    rng = np.random.default_rng(seed)
    vecs = [rng.standard_normal(N) for _ in range(100)]
    vecs += [np.ones(N), np.where(np.arange(N) % 2 == 0, 1.0, -1.0), np.eye(1, N, 1234)[0]]
    ratio = np.array([np.sum((v @ f / np.sqrt(K)) ** 2) / np.sum(v * v) for v in vecs])
    print(f"[attribution] seed {seed}: max |column sum| {col / np.sqrt(N):.2f} sqrt(n), max |row sum| {row / np.sqrt(K):.2f} sqrt(k), "
          f"max off-diagonal correlation {off * np.sqrt(N):.2f} / sqrt(n), norm ratio in [{ratio.min():.3f}, {ratio.max():.3f}]")
    assert col <= 5 * np.sqrt(N)
    assert row <= 5 * np.sqrt(K)
    assert off <= 6 / np.sqrt(N)
    assert ratio.min() >= 0.7 and ratio.max() <= 1.3


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("i0", [860_000_000, 1 << 32])
def test_far_rows_are_no_copies_of_the_first_rows(seed, i0):
    a, b = R.signs(seed, 0, 64, 64), R.signs(seed, i0, 64, 64)
    agree = float(np.mean(a == b))
    print(f"[attribution] seed {seed}: rows at {i0} agree with rows at 0 in {agree:.3f} of a 64 x 64 block")
    assert abs(agree - 0.5) <= 0.1


def test_seeds_give_other_matrices_and_the_index_is_the_flat_offset():
    a = R.signs(0, 0, 64, 64)
    assert abs(float(np.mean(a == R.signs(1, 0, 64, 64))) - 0.5) <= 0.1
    assert np.array_equal(R.signs(7, 100, 50, 32), R.signs(7, 0, 150, 32)[100:])


# ================================================================ 2. timesteps and seeds
def test_timestep_table_and_row_seeds():
    from siss_amd.attribution import row_seed, timestep_table
    assert timestep_table(10, 1000) == [50, 150, 250, 350, 450, 550, 650, 750, 850, 950]
    assert timestep_table(4, 1000) == [125, 375, 625, 875]
    assert timestep_table(1, 1000) == [500] and timestep_table(3, 10) == [1, 5, 8]
    assert timestep_table(1000, 1000) == list(range(1000))
    for S, T in ((7, 1000), (3, 10), (64, 1000)):
        assert timestep_table(S, T) == [int(np.floor((s + 0.5) * T / S)) for s in range(S)]
    for bad in (0, -1, 1001, 2.5, True):
        with pytest.raises(ValueError, match="timesteps"):
            timestep_table(bad, 1000)
    seeds = {row_seed(s, i) for s in range(4) for i in range(64)}
    assert len(seeds) == 256 and all(0 <= v < 1 << 63 for v in seeds)
    assert row_seed(3, 5) == row_seed(3, 5) != row_seed(5, 3)
    with pytest.raises(ValueError, match="row_seed"):
        row_seed(0, -1)


# ================================================================ 3. the attributor
def _store(n, k, seed):
    from siss_amd.attribution import FeatureStore
    g = torch.Generator().manual_seed(seed)
    st = FeatureStore(n, k, [f"{i:05d}.jpg" for i in range(n)], device="cpu", fingerprint=dict(weights="w0", timesteps=4))
    st.rows.copy_(torch.randn(n, k, generator=g) * torch.logspace(-1, 1, k)[None, :])
    return st


def test_attributor_against_a_dense_f64_solve():
    from siss_amd.attribution import Attributor
    st = _store(48, 64, 3)
    phi = st.rows.double().numpy()
    q = torch.randn(5, 64, generator=torch.Generator().manual_seed(4)).double().numpy()
    att = Attributor(st, damping=1e-2)
    want, v = R.scores_f64(phi, q, 1e-2)
    got_v = att.precondition(torch.from_numpy(q))
    assert np.abs(got_v - v).max() <= 1e-10 * np.abs(v).max()
    got = got_v @ phi.T
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    K, lam = R.preconditioner(phi, 1e-2)
    si = np.array([p @ np.linalg.solve(K, p) for p in phi])
    assert np.abs(att.self_influence() - si).max() <= 1e-10 * si.max()
    # the f32 scores the class hands out: the preconditioned queries rounded once, then f32 dot products
    s32 = att.scores(torch.from_numpy(q)).double().numpy()
    bound = (64 + 2) * R.U * (np.abs(v) @ np.abs(phi).T)
    assert s32.shape == (5, 48) and np.all(np.abs(s32 - want) <= bound)


def test_damping_rule():
    from siss_amd.attribution import Attributor, damping_term
    st = _store(48, 64, 5)
    phi = st.rows.double().numpy()
    mean_diag = float(np.mean(np.sum(phi * phi, 0) / 48))
    for d in (1e-2, 0.5, 3.0):
        att = Attributor(st, damping=d)
        assert att.damping == d and abs(att.mean_diag - mean_diag) <= 1e-12 * mean_diag
        assert att.lam == damping_term(d, att.mean_diag) == d * att.mean_diag
        assert abs(att.lam - R.preconditioner(phi, d)[1]) <= 1e-12 * att.lam
    # more rows than columns or fewer: the damped matrix is positive definite either way
    few = _store(8, 64, 6)
    assert np.all(np.isfinite(Attributor(few, 1e-3).self_influence()))


# ================================================================ 4. refusals
@pytest.mark.parametrize("k", [0, 16, 31, 48, 8192 + 32, 100, 2048.0, True])
def test_k_off_the_rule_is_refused(k):
    from siss_amd.attribution import FeatureStore, Projector
    with pytest.raises(ValueError, match="a multiple of 32 in 32 .. 8192"):
        Projector(1024, k)
    with pytest.raises(ValueError, match="a multiple of 32 in 32 .. 8192"):
        FeatureStore(4, k, device="cpu")


def test_projector_refusals():
    from siss_amd.attribution import Projector
    from siss_amd.trainable import Subset
    p = Projector(1024, 64, seed=3)
    assert p.fingerprint() == dict(hash="rademacher/lowbias32-v1", k=64, seed=3, total=1024, stretches=None)
    buf = torch.zeros(1024 + 4)
    assert buf.data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="g is not 16-byte aligned"):
        p.project(buf[1:1025], torch.zeros(64))
    out = torch.zeros(64 + 4)
    with pytest.raises(ValueError, match="out_row is not 16-byte aligned"):
        p.project(buf[:1024], out[1:65])
    with pytest.raises(ValueError, match="contiguous f32 vector of 1024"):
        p.project(buf[:1000], out[:64])
    with pytest.raises(ValueError, match="contiguous f32 vector of 64"):
        p.project(buf[:1024], out[:32])
    with pytest.raises(RuntimeError, match="runs on the device only"):
        p.project(buf[:1024], out[:64])
    for seed in (-1, 1 << 32, 1.5):
        with pytest.raises(ValueError, match="seed"):
            Projector(1024, 64, seed=seed)
    with pytest.raises(ValueError, match="total"):
        Projector(0, 64)
    import collections
    Spec = collections.namedtuple("Spec", "off numel")
    sub = Subset({"a": Spec(0, 64), "b": Spec(64, 64)}, ["b"], 128, 64)
    with pytest.raises(ValueError, match="a buffer of 128 floats"):
        Projector(1024, 64, subset=sub)
    a, b = Projector(128, 64, subset=sub).fingerprint(), Projector(128, 64).fingerprint()
    assert a["stretches"] is not None and b["stretches"] is None


@pytest.mark.parametrize("damping", [0, 0.0, -1e-3, float("nan"), float("inf"), None, "0.01", True])
def test_damping_refusals(damping):
    from siss_amd.attribution import Attributor
    with pytest.raises(ValueError, match="a finite number > 0 is needed"):
        Attributor(_store(8, 32, 1), damping=damping)


def test_store_max_bytes():
    from siss_amd.attribution import FeatureStore
    with pytest.raises(ValueError, match=r"100 rows of 64 take 25600 bytes, more than max_bytes = 25599"):
        FeatureStore(100, 64, device="cpu", max_bytes=25599)
    st = FeatureStore(100, 64, device="cpu", max_bytes=25600)
    assert st.rows.shape == (100, 64) and st.rows.dtype == torch.float32 and int(st.rows.count_nonzero()) == 0
    assert st.names == [str(i) for i in range(100)]
    with pytest.raises(ValueError, match="100 rows, 3 names"):
        FeatureStore(100, 64, ["a", "b", "c"], device="cpu")


# ================================================================ 5. the files
def test_store_round_trip_and_foreign_fingerprints(tmp_path):
    from siss_amd.attribution import META_FILE, ROWS_FILE, FeatureStore
    fp = dict(format=1, weights="abc", layout=dict(total=1024, tensors=3, real_params=1000),
              projector=dict(hash="rademacher/lowbias32-v1", k=64, seed=0, total=1024, stretches=None), timesteps=4, output="square", seed=0,
              names="n0")
    st = _store(12, 64, 9)
    st.fingerprint = dict(fp)
    d = st.save(tmp_path / "store")
    assert sorted(os.listdir(d)) == sorted([ROWS_FILE, META_FILE])
    back = FeatureStore.load(d, expect=fp)
    assert torch.equal(back.rows.view(torch.int32), st.rows.view(torch.int32)) and back.names == st.names and back.fingerprint == fp
    assert FeatureStore.read_meta(d)["names"] == st.names
    assert torch.equal(FeatureStore.load(d).rows, st.rows)                      # nothing expected: nothing compared
    for key, other in (("weights", "abd"), ("layout", dict(total=2048, tensors=3, real_params=1000)), ("timesteps", 10), ("output", "loss"),
                       ("seed", 1), ("projector", dict(fp["projector"], seed=1)), ("names", "n1")):
        with pytest.raises(ValueError, match=f"the store's {key} is"):
            FeatureStore.load(d, expect=dict(fp, **{key: other}))


def test_forget_list_is_what_the_dataset_takes(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import attribute
    from siss_amd.data import CelebAHQ
    data = tmp_path / "images"
    data.mkdir()
    names = [f"{i:05d}.jpg" for i in range(6)]
    for i, n in enumerate(names):
        Image.fromarray(np.full((8, 8, 3), 40 * i, np.uint8)).save(data / n)
    path = tmp_path / "forget.txt"
    listed = attribute.write_forget_list(path, ["00004.jpg", "00001.jpg", "00004.jpg"])
    assert listed == ["00004.jpg", "00001.jpg"] and open(path).read() == "00004.jpg\n00001.jpg\n"
    remove = attribute.read_forget_list(path)
    assert remove == listed
    forget, keep = CelebAHQ("deletion", str(data), remove), CelebAHQ("nondeletion", str(data), remove)
    assert [os.path.basename(p) for p in forget.paths] == ["00001.jpg", "00004.jpg"]
    assert [os.path.basename(p) for p in keep.paths] == [n for n in names if n not in remove]
    assert attribute.dataset_names(forget) == ["00001.jpg", "00004.jpg"]

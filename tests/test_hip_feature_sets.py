"""csrc/feature_sets.hip on the GPU (behind siss_amd/feature_sets.py): radii, ball counts, minima and kernel sums bit for bit on exact
integer data (ties, self exclusion, the split into pieces), within the a-priori bounds of tests/feature_sets_ref.py on realistic rows,
and `metrics.fid.sets` in the delete_celeb task loop."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import feature_sets_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REAL, N_FAKE, PADDED = 131, 67, 8300


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import feature_sets as F
    F.require_kernels()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def realistic(dev):
    """The shared realistic case, computed once: the issue's rows on the host and on the device, with the device's norms."""
    from siss_amd import feature_sets as F
    real, fake = R.realistic()
    tr, tf = torch.from_numpy(real).to(dev), torch.from_numpy(fake).to(dev)
    return dict(real=real, fake=fake, tr=tr, tf=tf, sq_r=F.sqnorm(tr), sq_f=F.sqnorm(tf))


def host(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float32:
        assert np.array_equal(R.bits(got), R.bits(want.astype(np.float32))), f"{what}: rows {np.flatnonzero(R.bits(got) != R.bits(want.astype(np.float32)))[:8].tolist()} differ"
    else:
        assert np.array_equal(got, want), f"{what}: rows {np.flatnonzero(got != want)[:8].tolist()} differ"


def padded(x, d):
    """x with far-away rows (all ones: every distance to them is still exact in f32) up to PADDED rows: more than one piece."""
    return np.concatenate([x, np.ones((PADDED - len(x), d), np.float32)])


# ---------------------------------------------------------------- exact data
@pytest.mark.parametrize("d", [4, 20, 64, 2048])
def test_exact_radii_and_balls(dev, d):
    from siss_amd import feature_sets as F
    real, fake = R.exact_rows(N_REAL, d, 10 + d), R.exact_rows(N_FAKE, d, 20 + d)
    rr, ff, fr = R.exact_d2(real, real), R.exact_d2(fake, fake), R.exact_d2(fake, real)
    tr, tf = torch.from_numpy(real).to(dev), torch.from_numpy(fake).to(dev)
    trp, tfp = torch.from_numpy(padded(real, d)).to(dev), torch.from_numpy(padded(fake, d)).to(dev)
    sq_r, sq_f, sq_rp, sq_fp = F.sqnorm(tr), F.sqnorm(tf), F.sqnorm(trp), F.sqnorm(tfp)
    same_bits(sq_r.cpu().numpy(), (real.astype(np.float64) ** 2).sum(1), "sqnorm")
    assert torch.equal(sq_rp[:N_REAL], sq_r) and bool((sq_rp[N_REAL:] == d).all())
    for k in (1, 5, 16):
        r_r, r_f = F.knn_radius(tr, sq_r, k), F.knn_radius(tf, sq_f, k)
        same_bits(r_r.cpu().numpy(), R.radii(rr, k), f"radius real k={k}")
        same_bits(r_f.cpu().numpy(), R.radii(ff, k), f"radius fake k={k}")
        for (q, sq_q, g, sq_g, rad, m, what) in ((tf, sq_f, tr, sq_r, r_r, fr, "fake in real"), (tr, sq_r, tf, sq_f, r_f, fr.T, "real in fake")):
            inside, mn, arg = host(*F.ball_stats(q, sq_q, g, sq_g, rad))
            wi, wm, wa = R.ball(m, rad.cpu().numpy().astype(np.float64))
            same_bits(inside, wi, f"inside {what} k={k}")
            same_bits(mn, wm, f"min_d2 {what} k={k}")
            same_bits(arg, wa, f"argmin {what} k={k}")
            assert int((m == wm[:, None]).sum(1).max()) > 1 or d > 64, "the data has no tie for the argmin rule to decide"
        # the same rows with the gallery padded by far-away rows: more than one piece, the same values
        r_rp, r_fp = F.knn_radius(trp, sq_rp, k), F.knn_radius(tfp, sq_fp, k)
        assert torch.equal(r_rp[:N_REAL], r_r) and torch.equal(r_fp[:N_FAKE], r_f) and bool((r_rp[N_REAL:] == 0).all())
        a = F.ball_stats(tf, sq_f, trp, sq_rp, r_rp)
        b = F.ball_stats(tf, sq_f, tr, sq_r, r_r)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f"k={k}: the padded gallery changed a result"
        a = F.ball_stats(tr, sq_r, tfp, sq_fp, r_fp)
        b = F.ball_stats(tr, sq_r, tf, sq_f, r_f)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f"k={k}: the padded gallery changed a result"
    # the self pair is left out by index: the set against itself, as a slice of the padded gallery
    inside, mn, arg = host(*F.ball_stats(tr[3:], sq_r[3:], trp, sq_rp, None, self0=3))
    wi, wm, wa = R.ball(rr[3:], None, self0=3)
    assert inside is None and wi is None
    same_bits(mn, wm, "min_d2 self0")
    same_bits(arg, wa, "argmin self0")
    # without the exclusion every row finds itself (or an equal row before it) at distance 0
    _, mn0, arg0 = host(*F.ball_stats(tr, sq_r, tr, sq_r))
    assert (mn0 == 0).all() and (arg0 <= np.arange(N_REAL)).all()
    # the same call twice: the same bits
    assert torch.equal(F.knn_radius(trp, sq_rp, 5), F.knn_radius(trp, sq_rp, 5))


def test_exact_edge_shapes(dev):
    from siss_amd import feature_sets as F
    d = 20
    real, fake = R.exact_rows(9, d, 1), R.exact_rows(7, d, 2)
    tr, tf = torch.from_numpy(real).to(dev), torch.from_numpy(fake).to(dev)
    sq_r, sq_f = F.sqnorm(tr), F.sqnorm(tf)
    # n - 1 < k: +inf; n - 1 == k: finite
    assert bool(torch.isinf(F.knn_radius(tr, sq_r, 9)).all()) and bool(torch.isinf(F.knn_radius(tr[:1], sq_r[:1], 1)).all())
    same_bits(F.knn_radius(tr, sq_r, 8).cpu().numpy(), R.radii(R.exact_d2(real, real), 8), "radius k = n - 1")
    rad = F.knn_radius(tr, sq_r, 2)
    fr = R.exact_d2(fake, real)
    # nq = 1
    inside, mn, arg = host(*F.ball_stats(tf[2:3], sq_f[2:3], tr, sq_r, rad))
    wi, wm, wa = R.ball(fr[2:3], rad.cpu().numpy().astype(np.float64))
    same_bits(inside, wi, "inside nq=1"); same_bits(mn, wm, "min nq=1"); same_bits(arg, wa, "argmin nq=1")
    # ng = 1
    inside, mn, arg = host(*F.ball_stats(tf, sq_f, tr[4:5], sq_r[4:5], rad[4:5]))
    wi, wm, wa = R.ball(fr[:, 4:5], rad[4:5].cpu().numpy().astype(np.float64))
    same_bits(inside, wi, "inside ng=1"); same_bits(mn, wm, "min ng=1"); same_bits(arg, wa, "argmin ng=1")
    # one row against itself, excluded: no candidate
    inside, mn, arg = host(*F.ball_stats(tr[:1], sq_r[:1], tr[:1], sq_r[:1], rad[:1], self0=0))
    assert inside.tolist() == [0] and np.isinf(mn).all() and arg.tolist() == [-1]
    # NaN distances are never selected and never counted
    bad = tr.clone()
    bad[5, 3] = float("nan")
    sq_b = F.sqnorm(bad)
    assert bool(torch.isnan(sq_b[5])) and int(torch.isnan(sq_b).sum()) == 1
    m = R.exact_d2(real, real)
    m[5, :], m[:, 5] = np.inf, np.inf                            # row 5 has no candidate and is nobody's candidate
    same_bits(F.knn_radius(bad, sq_b, 7).cpu().numpy(), R.radii(m, 7), "radius beside a NaN row")     # 7 candidates are left: finite
    assert np.isfinite(R.radii(m, 7)[0]) and bool(torch.isinf(F.knn_radius(bad, sq_b, 8)).all())
    inside, mn, arg = host(*F.ball_stats(tf, sq_f, bad, sq_b, torch.full_like(sq_b, float("inf"))))
    assert (inside == 8).all() and (arg != 5).all() and np.isfinite(mn).all()


def test_launcher_refusals_write_nothing(dev):
    """Status 1 from the library itself, before any launch: d outside 4 .. 4096 or d % 4, no rows, k outside 1 .. 16, a missing or
    too-small work buffer; -1 from the size queries."""
    from siss_amd import lib
    x = torch.zeros(8, 4100, device=dev)
    sq, rad = torch.full((8,), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    i32, out = torch.full((8,), 7, device=dev, dtype=torch.int32), torch.full((2, 3), 7.0, device=dev, dtype=torch.float64)
    ws = torch.zeros(1 << 14, device=dev, dtype=torch.int64)
    nb = ws.numel() * 8
    call = lambda *a: lib.call(*a, refusable=True)
    for d in (0, 2, 6, 4100):
        assert call("siss_feat_sqnorm", x, 8, d, sq) == 1
        assert call("siss_feat_knn_radius", x, 8, d, sq, 5, rad, ws, nb) == 1
        assert call("siss_feat_ball_stats", x, 8, sq, x, 8, sq, rad, d, -1, i32, rad, i32, ws, nb) == 1
        assert call("siss_kid_sums", x, 8, i32, x, 8, i32, d, 2, 3, 0.5, 1.0, out, ws, nb) == 1
    assert call("siss_feat_sqnorm", x, 0, 8, sq) == 1 and call("siss_feat_knn_radius", x, 0, 8, sq, 5, rad, ws, nb) == 1
    assert call("siss_feat_ball_stats", x, 0, sq, x, 8, sq, rad, 8, -1, i32, rad, i32, ws, nb) == 1
    assert call("siss_feat_ball_stats", x, 8, sq, x, 0, sq, rad, 8, -1, i32, rad, i32, ws, nb) == 1
    assert call("siss_kid_sums", x, 8, i32, x, 8, i32, 8, 0, 3, 0.5, 1.0, out, ws, nb) == 1
    assert call("siss_kid_sums", x, 8, i32, x, 8, i32, 8, 2, 0, 0.5, 1.0, out, ws, nb) == 1
    for k in (0, 17):
        assert call("siss_feat_knn_radius", x, 8, 8, sq, k, rad, ws, nb) == 1 and lib.query("siss_feat_knn_ws_bytes", 8, k) == -1
    assert call("siss_feat_knn_radius", x, 8, 8, sq, 5, rad, None, nb) == 1
    assert call("siss_feat_knn_radius", x, 8, 8, sq, 5, rad, ws, lib.query("siss_feat_knn_ws_bytes", 8, 5) - 1) == 1
    assert call("siss_feat_ball_stats", x, 8, sq, x, 8, sq, rad, 8, -1, i32, rad, i32, None, nb) == 1
    assert call("siss_feat_ball_stats", x, 8, sq, x, 8, sq, rad, 8, -1, i32, rad, i32, ws, lib.query("siss_feat_ball_ws_bytes", 8, 8) - 1) == 1
    assert call("siss_kid_sums", x, 8, i32, x, 8, i32, 8, 2, 3, 0.5, 1.0, out, None, nb) == 1
    assert call("siss_kid_sums", x, 8, i32, x, 8, i32, 8, 2, 3, 0.5, 1.0, out, ws, lib.query("siss_kid_ws_bytes", 2, 3) - 1) == 1
    assert lib.query("siss_feat_ball_ws_bytes", 0, 8) == -1 and lib.query("siss_kid_ws_bytes", 0, 3) == -1 and lib.query("siss_kid_ws_bytes", 2, 0) == -1
    # the size queries agree with the reference's restatement
    for a in ((8, 5), (131, 16), (8300, 5), (30000, 5)):
        assert lib.query("siss_feat_knn_ws_bytes", *a) == R.ws_bytes("siss_feat_knn_ws_bytes", *a)
    for a in ((67, 8300), (30000, 10000), (1, 1)):
        assert lib.query("siss_feat_ball_ws_bytes", *a) == R.ws_bytes("siss_feat_ball_ws_bytes", *a)
    for a in ((100, 1000), (1, 157), (3, 33)):
        assert lib.query("siss_kid_ws_bytes", *a) == R.ws_bytes("siss_kid_ws_bytes", *a)
    torch.cuda.synchronize()
    assert bool((sq == 7).all()) and bool((rad == 7).all()) and bool((i32 == 7).all()) and bool((out == 7).all())


# ---------------------------------------------------------------- realistic data
def test_realistic_radii_balls_and_figures(dev, realistic):
    from siss_amd import feature_sets as F
    c, k = realistic, 5
    real, fake = c["real"], c["fake"]
    rr, ff, fr = R.d2_64(real, real), R.d2_64(fake, fake), R.d2_64(fake, real)
    brr, bff, bfr = R.bound(real, real), R.bound(fake, fake), R.bound(fake, real)
    r_r, r_f = F.knn_radius(c["tr"], c["sq_r"], k), F.knn_radius(c["tf"], c["sq_f"], k)
    r64_r, B_r = R.accept_radius(r_r.cpu().numpy(), rr, brr, k)
    r64_f, B_f = R.accept_radius(r_f.cpu().numpy(), ff, bff, k)
    in_f, mn_f, arg_f = host(*F.ball_stats(c["tf"], c["sq_f"], c["tr"], c["sq_r"], r_r))
    in_r, mn_r, arg_r = host(*F.ball_stats(c["tr"], c["sq_r"], c["tf"], c["sq_f"], r_f))
    _, _, band1 = R.accept_ball(in_f, mn_f, arg_f, fr, bfr, r64_r, B_r)
    _, _, band2 = R.accept_ball(in_r, mn_r, arg_r, fr.T, bfr.T, r64_f, B_f)
    print(f"\nundecided bands: fake in real {band1:.2e}, real in fake {band2:.2e} of the pairs (cap {R.BAND_SHARE:.0e})")
    # the four figures, through the public class on two banks
    rb, fb = F.FeatureBank(2048, len(real), dev), F.FeatureBank(2048, len(fake), dev)
    rb.append(c["tr"]); fb.append(c["tf"])
    got = F.PRDC(k).compute(rb, fb)
    want = R.prdc(real, fake, k)
    iv = R.prdc_intervals(real, fake, k)
    print("figures", got, "f64", want, "intervals", iv)
    R.assert_in(got, iv)
    assert all(0.05 < want[n] < 0.99 for n in want), "a degenerate figure tests nothing"
    assert torch.equal(rb.cache[("prdc", k)], r_r) and torch.equal(fb.cache["sq"], c["sq_f"])
    # the distance is one value per pair: the two directions agree bit for bit
    _, mn_t, _ = F.ball_stats(c["tr"][:64], c["sq_r"][:64], c["tf"], c["sq_f"])
    assert torch.equal(mn_t.cpu(), torch.from_numpy(mn_r[:64]))


# ---------------------------------------------------------------- KID
def _tables(nx, ny, S, s, seed):
    g = torch.Generator().manual_seed(seed)
    ix = torch.stack([torch.randperm(nx, generator=g)[:s] for _ in range(S)])
    iy = torch.stack([torch.randperm(ny, generator=g)[:s] for _ in range(S)])
    return ix, iy


@pytest.mark.parametrize("d", [20, 2048])
def test_kid_sums_exact(dev, d):
    from siss_amd import feature_sets as F
    x, y = R.exact_rows(211, d, 30 + d), R.exact_rows(157, d, 40 + d)
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    for S, s in ((7, 96), (3, 33), (1, 157)):
        ix, iy = _tables(211, 157, S, s, S)
        if S > 1:
            ix[1], iy[S - 1] = ix[0], iy[0]                     # the same rows in two subsets
        got = F.kid_sums(tx, ix, ty, iy, 1.0 / d, 1.0)
        assert got.dtype == torch.float64 and got.shape == (S, 3)
        want = R.kernel_sums(x, ix.numpy(), y, iy.numpy(), 1.0 / d, 1.0, dots=R.exact_sims)
        n = np.array([s * (s - 1), s * (s - 1), s * s], np.float64)
        err = np.abs(got.cpu().numpy() - want)
        assert (want > 0).all() and (err <= n * 2.0 ** -53 * want).all(), (S, s, (err / (n * 2.0 ** -53 * want)).max())
        if S > 1:
            assert got[1, 0] == got[0, 0] and got[S - 1, 1] == got[0, 1]
        assert torch.equal(F.kid_sums(tx, ix, ty, iy, 1.0 / d, 1.0), got)         # the same tables: the same bits


def test_kid_realistic(dev, realistic):
    from siss_amd import feature_sets as F
    c, S, s, gam = realistic, 3, 200, 1.0 / 2048
    kid = F.KernelInceptionDistance(subsets=S, subset_size=s, seed=5)
    kid.update_features(c["tr"][:1000], real=True); kid.update_features(c["tr"][1000:], real=True)
    kid.update_features(c["tf"], real=False)
    mean, std = (float(v) for v in kid.compute())
    ir, if_ = F.subset_tables(len(c["real"]), len(c["fake"]), S, s, 5)
    got = F.kid_sums(c["tr"], ir, c["tf"], if_, gam, 1.0).cpu().numpy()
    want = R.kernel_sums(c["real"], ir.numpy(), c["fake"], if_.numpy(), gam, 1.0)
    b = R.kernel_sum_bounds(c["real"], ir.numpy(), c["fake"], if_.numpy(), gam, 1.0)
    err = np.abs(got - want)
    print(f"\nkernel sums: worst error / bound {(err / b).max():.3f}; relative bound {(b / want).max():.2e}")
    assert (err <= b).all()
    e = (b[:, 0] + b[:, 1]) / (s * (s - 1)) + 2 * b[:, 2] / (s * s)              # what the bounds leave of each subset's value
    wm, ws = R.kid(want, s)
    assert wm > 10 * e.max(), "the KID of the shifted set must stand clear of its own bound"
    assert abs(mean - wm) <= e.mean() and abs(std - ws) <= e.max()              # (the population std is 1-Lipschitz in the sup norm)
    kid.reset()
    with pytest.raises(ValueError, match="subset_size"):
        kid.compute()


# ---------------------------------------------------------------- the task
SMALL = ["unet.sample_size=16", "unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
         "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1", "unet.attention_head_dim=null",
         "training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent",
         "allow_random_init=true", "allow_synthetic=true", "save_final=false", "pipeline.num_inference_steps=2"]


def test_sets_in_the_delete_celeb_loop(dev, tmp_path, monkeypatch):
    from PIL import Image
    from siss_amd import feature_sets as F
    sys.path.insert(0, ROOT)
    import main as entry
    data = tmp_path / "real"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i in range(12):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(data / f"{i:02d}.jpg")
    fid = ["+metrics.fid.class_cfg._target_=metrics.fid.FIDEvaluator", "+metrics.fid.class_cfg.inception_batch_size=4",
           "+metrics.fid.class_cfg.allow_random_init=true", f"+metrics.fid.class_cfg.data_path={data}",
           "+metrics.fid.step_frequency=2", "+metrics.fid.num_imgs_to_generate=12", "+metrics.fid.batch_size=6",
           # the two runs' FIDs are compared bit for bit below, at step 0 AND after the two training steps.  The f32 training step is
           # not bitwise repeatable from run to run (the same command without the key gave FID 339.42111 once and 339.41974 once at
           # step 2, with equal bits at step 0), so the steps run at lr = 0: the weights stay, the evaluations still draw new samples
           "optimizer.lr=0"]
    seen = []
    evaluate = F.FeatureSets.evaluate

    def keeping(self):
        seen.append((self.real.rows.cpu().numpy().copy(), self.fake.rows.cpu().numpy().copy()))
        return evaluate(self)

    monkeypatch.setattr(F.FeatureSets, "evaluate", keeping)
    feats = tmp_path / "real_features.safetensors"
    out = tmp_path / "with"
    entry.main(["--config-name=delete_celeb", f"data_dir={tmp_path}/nodata", f"output_dir={out}", *SMALL, *fid,
                "+metrics.fid.sets={kid:{subsets:3,subset_size:8},prdc:{k:2},real_features_path:" + str(feats) + "}"])
    lines = [json.loads(l) for l in open(out / os.listdir(out)[0] / "fid_rank0.jsonl")]
    print("\n", lines)
    assert [l["global_step"] for l in lines] == [0, 2] and len(seen) == 2 and F.FeatureBank.exists(feats)
    for l, (real, fake) in zip(lines, seen):
        assert real.shape == (12, 2048) and fake.shape == (12, 2048) and "sets_skipped" not in l
        assert list(l)[-len(F.RECORD_FIELDS):] == list(F.RECORD_FIELDS)
        assert (l["kid_subsets"], l["kid_subset_size"], l["prdc_k"]) == (3, 8, 2)
        R.assert_in(l, R.prdc_intervals(real, fake, 2))
        ir, if_ = F.subset_tables(12, 12, 3, 8, 0)
        want = R.kernel_sums(real, ir.numpy(), fake, if_.numpy(), 1.0 / 2048, 1.0)
        b = R.kernel_sum_bounds(real, ir.numpy(), fake, if_.numpy(), 1.0 / 2048, 1.0)
        e = (b[:, 0] + b[:, 1]) / (8 * 7) + 2 * b[:, 2] / 64
        wm, ws = R.kid(want, 8)
        assert abs(l["kid_mean"] - wm) <= e.mean() and abs(l["kid_std"] - ws) <= e.max()
    # the same run without the key: the same FID bit for bit, none of the new fields
    monkeypatch.setattr(F.FeatureSets, "evaluate", evaluate)
    out2 = tmp_path / "without"
    entry.main(["--config-name=delete_celeb", f"data_dir={tmp_path}/nodata", f"output_dir={out2}", *SMALL, *fid])
    plain = [json.loads(l) for l in open(out2 / os.listdir(out2)[0] / "fid_rank0.jsonl")]
    assert [p["fid"] for p in plain] == [l["fid"] for l in lines]
    for p in plain:
        assert set(p) == {"global_step", "fid", "fake_images", "real_images", "seconds"}

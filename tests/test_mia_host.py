"""CPU tests of the membership inference attacks (siss_amd/mia.py): the statistics against brute-force pair counting, the FPR cap,
the transfer coefficients, the f64 reference chains of tests/mia_ref.py on the exact denoiser of point-mass data, the config key and
every refusal, and the wiring of the new entry points."""
import math
import os

import numpy as np
import pytest
import torch

import mia_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPR = (0.01, 0.001, 0.05, 0.29)


# ---------------------------------------------------------------------------------------------------------------- statistics
def _cases():
    """(member, holdout, forget) score lists: continuous, heavy ties (a few integer values), n_h below and above 1 / alpha."""
    rng = np.random.default_rng(0)
    out = []
    for n_m, n_h, n_f, ties in ((7, 5, 1, False), (40, 100, 3, False), (33, 250, 4, True), (12, 9, 2, True), (25, 1000, 5, True),
                                (1, 1, 1, False), (64, 101, 9, False)):
        draw = (lambda n, lo: rng.integers(lo, lo + 6, n).astype(np.float64)) if ties else (lambda n, lo: rng.normal(lo, 2.0, n))
        out.append((draw(n_m, 0).tolist(), draw(n_h, 1).tolist(), draw(n_f, 0).tolist()))
    return out


@pytest.mark.parametrize("case", range(7))
def test_statistics_equal_brute_force_pair_counting(case):
    from siss_amd.mia import forget_stats, fpr_key, roc_stats
    member, holdout, forget = _cases()[case]
    roc, fg = roc_stats(member, holdout, FPR), forget_stats(forget, holdout, FPR)
    assert roc["auc"] == R.brute_auc(member, holdout)
    assert fg["forget_auc"] == R.brute_auc(forget, holdout)
    assert fg["forget_percentile"] == R.brute_percentile(forget, holdout)
    for a in FPR:
        tpr, realised = R.brute_flagged(member, holdout, a)
        assert roc[f"tpr_at_fpr_{fpr_key(a)}"] == tpr
        assert fg[f"forget_flagged_at_fpr_{fpr_key(a)}"] == R.brute_flagged(forget, holdout, a)[0]
        assert realised <= a + 1e-12, (a, realised)                                    # the cap, ties included


@pytest.mark.parametrize("case", range(7))
def test_the_realised_fpr_never_exceeds_the_level(case):
    """The holdout images flagged at the operating point, counted directly from operating_threshold."""
    from siss_amd.mia import operating_threshold
    _, holdout, _ = _cases()[case]
    h = np.asarray(holdout)
    for a in FPR:
        thr = operating_threshold(holdout, a)
        assert int((h < thr).sum()) <= a * h.size + 1e-9
        if h.size < 1 / a:
            assert thr == h.min() and int((h < thr).sum()) == 0                      # "below every holdout score"


def test_statistics_edge_cases():
    from siss_amd.mia import forget_stats, roc_stats
    same = roc_stats([3.0] * 6, [3.0] * 11, (0.01, 0.2))
    assert same == {"auc": 0.5, "tpr_at_fpr_0.01": 0.0, "tpr_at_fpr_0.2": 0.0}          # all equal: chance, nothing flagged
    fg = forget_stats([3.0], [3.0] * 11, (0.2,))
    assert fg == {"forget_auc": 0.5, "forget_flagged_at_fpr_0.2": 0.0, "forget_percentile": 0.5}
    apart = roc_stats([0.1, 0.2, 0.3], [1.0, 2.0], (0.01,))
    assert apart == {"auc": 1.0, "tpr_at_fpr_0.01": 1.0}                                # disjoint, members below
    assert roc_stats([5.0, 6.0], [1.0, 2.0], (0.01,)) == {"auc": 0.0, "tpr_at_fpr_0.01": 0.0}
    assert forget_stats([0.0], [1.0, 2.0], (0.5,)) == {"forget_auc": 1.0, "forget_flagged_at_fpr_0.5": 1.0, "forget_percentile": 0.0}
    # tensors (the device's f64 scores) are taken as they are
    assert roc_stats(torch.tensor([0.1, 0.2], dtype=torch.float64), torch.tensor([1.0]))["auc"] == 1.0
    for bad in ([], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            roc_stats(bad, [1.0])
    with pytest.raises(ValueError, match="fpr"):
        roc_stats([1.0], [1.0], (1.0,))


# ---------------------------------------------------------------------------------------------------------------- coefficients
def _ab():
    from siss_amd.scheduler import DDPMScheduler
    return DDPMScheduler().alphas_cumprod


def test_transfer_coefficients_are_the_f64_formula_rounded_once():
    from siss_amd.mia import transfer_coefficients
    ab = _ab()
    assert ab.dtype == torch.float32
    ab64 = ab.double().numpy()
    for a, c in ((0, 10), (10, 20), (90, 100), (100, 110), (110, 100), (0, 999), (999, 0), (500, 500)):
        cx, ce = transfer_coefficients(ab, "transfer", a, c)
        wx, we = R.coefficients(ab64, a, c)
        assert cx == float(np.float32(wx)) and ce == float(np.float32(we)), (a, c)
        assert np.float32(cx) == cx and np.float32(ce) == ce                           # f32 values
    for t in (0, 200, 999):
        cx, ce = transfer_coefficients(ab.numpy(), "noise", None, t)
        assert cx == float(np.float32(math.sqrt(ab64[t]))) and ce == float(np.float32(math.sqrt(1 - ab64[t])))
    assert transfer_coefficients(ab, "transfer", 500, 500) == (1.0, 0.0)
    with pytest.raises(ValueError, match="kind"):
        transfer_coefficients(ab, "ddim", 0, 1)


def test_a_transfer_and_its_inverse_with_one_eps_return_x():
    ab = _ab().double().numpy()
    g = torch.Generator().manual_seed(0)
    x, e = torch.randn(3, 50, generator=g, dtype=torch.float64), torch.randn(3, 50, generator=g, dtype=torch.float64)
    for a, c in ((0, 10), (100, 110), (300, 900)):
        back = R.transfer(R.transfer(x, e, ab, a, c), e, ab, c, a)
        assert float((back - x).abs().max()) <= 1e-12 * max(1.0, 1.0 / math.sqrt(ab[c]))


# ---------------------------------------------------------------------------------------------------------------- point mass
@pytest.mark.parametrize("p", [2, 4])
def test_reference_chains_on_the_exact_denoiser_of_point_mass_data(p):
    """Data concentrated at mu: SecMI's round trip closes for every input (one eps serves a whole DDIM trajectory), PIA and the
    loss give the closed forms -- zero for the member mu itself."""
    ab = _ab().double().numpy()
    g = torch.Generator().manual_seed(3)
    mu = torch.rand(1, 3, 4, 4, generator=g, dtype=torch.float64) * 2 - 1
    x0 = torch.cat([mu, torch.rand(4, 3, 4, 4, generator=g, dtype=torch.float64) * 2 - 1])          # the member, four non-members
    noise = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64)
    eps = R.point_mass_eps(ab, mu)
    d = (x0 - mu).reshape(5, -1)
    s = R.secmi(eps, ab, x0, 100, 10)
    assert float(s.max()) <= 1e-20 * 48, s
    for t in (100, 200):
        ratio = ab[t] / (1 - ab[t])
        got, want = R.pia(eps, ab, x0, t, p), ratio ** (p / 2) * (d.abs() ** p).sum(1)
        # (the member: zero up to the rounding of eps*(mu, 0), a few 2^-53 over sqrt(1 - ab_0) ~ 0.01 per element: < 1e-13, squared)
        assert float(got[0]) <= 48 * 1e-26 * ratio and float(((got - want).abs() / want.clamp_min(1e-300))[1:].max()) <= 1e-9
        got, want = R.loss(eps, ab, x0, noise, t, per_noise=True), (ratio * (d ** 2).sum(1))[:, None].expand(-1, 2)
        assert float(got[0].abs().max()) <= 1e-20 and float(((got - want).abs() / want.clamp_min(1e-300))[1:].max()) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- the config key
def _task(config, extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose(config, os.path.join(ROOT, "config"), list(extra))
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


MIA = "+metrics.mia={step_frequency: 5}"


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt"])
def test_the_key_is_parsed_with_its_defaults_and_absent_means_nothing(config):
    t = _task(config, [])
    t.check_metrics()
    assert t.mia is None and t.mia_metric(None, None, None, None, "cpu") is None
    t = _task(config, ["+metrics.mia=null"])
    t.check_metrics()
    assert t.mia is None
    t = _task(config, [MIA])
    t.check_metrics()
    assert t.mia == dict(step_frequency=5, num_members=64, num_forget=16, batch_size=16, seed=0, attacks=("secmi", "pia", "loss"),
                         settings={"secmi": dict(t_sec=100, stride=10), "pia": dict(t=200, p=4), "loss": dict(t=100, noises=4)},
                         fpr=[0.01, 0.001], holdout=None)
    t = _task(config, ["+metrics.mia={step_frequency: 2, attacks: [pia], pia: {p: 2}, fpr: [0.05], num_members: 8, seed: 4, "
                       "holdout: {limit: 12}}", "allow_synthetic=true"])
    t.check_metrics()
    assert t.mia["attacks"] == ("pia",) and t.mia["settings"]["pia"] == dict(t=200, p=2) and t.mia["holdout"] == dict(path=None, limit=12)
    assert t.mia["fpr"] == [0.05] and t.mia["num_members"] == 8 and t.mia["seed"] == 4


@pytest.mark.parametrize("bad,exc,match", [
    ("+metrics.mia=5", ValueError, "mapping"),
    ("+metrics.mia={step_frequency: 5, frequency: 2}", ValueError, "unknown field"),
    ("+metrics.mia={attacks: [pia]}", ValueError, "step_frequency"),
    ("+metrics.mia={step_frequency: 0}", ValueError, "step_frequency"),
    ("+metrics.mia={step_frequency: 5, num_members: 0}", ValueError, "num_members"),
    ("+metrics.mia={step_frequency: 5, num_forget: true}", ValueError, "num_forget"),
    ("+metrics.mia={step_frequency: 5, batch_size: -1}", ValueError, "batch_size"),
    ("+metrics.mia={step_frequency: 5, seed: x}", ValueError, "seed"),
    ("+metrics.mia={step_frequency: 5, attacks: [lira]}", ValueError, "attacks"),
    ("+metrics.mia={step_frequency: 5, attacks: []}", ValueError, "attacks"),
    ("+metrics.mia={step_frequency: 5, attacks: pia}", ValueError, "attacks"),
    ("+metrics.mia={step_frequency: 5, secmi: {t_sec: 95}}", ValueError, "secmi"),
    ("+metrics.mia={step_frequency: 5, secmi: {t_sec: 990}}", ValueError, "secmi"),
    ("+metrics.mia={step_frequency: 5, secmi: {steps: 3}}", ValueError, "unknown field"),
    ("+metrics.mia={step_frequency: 5, pia: {t: 1000}}", ValueError, r"pia\.t"),
    ("+metrics.mia={step_frequency: 5, pia: {t: -1}}", ValueError, r"pia\.t"),
    ("+metrics.mia={step_frequency: 5, pia: {p: 3}}", ValueError, r"pia\.p"),
    ("+metrics.mia={step_frequency: 5, loss: {t: 1000}}", ValueError, r"loss\.t"),
    ("+metrics.mia={step_frequency: 5, loss: {noises: 0}}", ValueError, "noises"),
    ("+metrics.mia={step_frequency: 5, fpr: [0.0]}", ValueError, "fpr"),
    ("+metrics.mia={step_frequency: 5, fpr: 0.01}", ValueError, "fpr"),
    ("+metrics.mia={step_frequency: 5, holdout: {dir: x}}", ValueError, "unknown field"),
    ("+metrics.mia={step_frequency: 5, holdout: {limit: 0}}", ValueError, "limit"),
    ("+metrics.mia={step_frequency: 5, holdout: {limit: 8}}", ValueError, "holdout.path"),       # (no allow_synthetic)
    ("+metrics.mia={step_frequency: 5, holdout: {path: /nonexistent/holdout}}", FileNotFoundError, "holdout.path"),
])
def test_a_bad_key_is_refused_before_anything_is_loaded(bad, exc, match):
    with pytest.raises(exc, match=match):
        _task("delete_tshirt", [bad]).check_metrics()


def test_sd_and_the_pretraining_task_refuse_the_key_by_message():
    with pytest.raises(NotImplementedError, match="metrics.mia.*latent-space"):
        _task("delete_sd", [MIA]).check_metrics()
    with pytest.raises(NotImplementedError, match="metrics.mia.*pre-training"):
        _task("train_tshirt_mnist", [MIA]).check_supported()
    _task("train_tshirt_mnist", []).check_supported()
    from siss_amd.tasks import DeleteCeleb, DeleteSD, DeleteTShirt
    assert DeleteCeleb.mia_supported and DeleteTShirt.mia_supported and not DeleteSD.mia_supported


def test_the_key_is_in_no_shipped_config():
    for f in os.listdir(os.path.join(ROOT, "config")):
        assert "mia" not in open(os.path.join(ROOT, "config", f)).read(), f


# ---------------------------------------------------------------------------------------------------------------- groups and files
def test_members_come_from_a_generator_of_their_own_and_forget_indices_are_scored_once():
    import random
    from siss_amd.mia import draw_members, unique_in_order
    random.seed(1)
    torch.manual_seed(1)
    state, tstate = random.getstate(), torch.get_rng_state()
    a, b = draw_members(100, 8, 3), draw_members(100, 8, 3)
    assert a == b and len(set(a)) == 8 and all(0 <= i < 100 for i in a) and a != draw_members(100, 8, 4)
    assert len(draw_members(5, 8, 0)) == 5
    assert random.getstate() == state and torch.equal(torch.get_rng_state(), tstate)
    assert unique_in_order([0, 0, 0]) == [0] and unique_in_order([4, 2, 4, 9, 2]) == [4, 2, 9]


def test_holdout_images_are_read_through_the_tasks_transform(tmp_path):
    from PIL import Image
    from siss_amd.data import Compose, Normalize, ToTensor
    from siss_amd.mia import load_holdout
    tf = Compose([ToTensor(), Normalize([0.5], [0.5])])
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, (5, 28, 28), dtype=np.uint8)
    np.savez(tmp_path / "test.npz", image=imgs, label=np.arange(5))
    got = load_holdout(str(tmp_path / "test.npz"), 3, tf, 1)
    assert got.shape == (3, 1, 28, 28) and torch.equal(got, torch.stack([tf(i) for i in imgs[:3]]))
    d = tmp_path / "dir"
    d.mkdir()
    for k in (2, 0, 1):
        Image.fromarray(imgs[k]).save(d / f"{k}.png")
    got = load_holdout(str(d), 9, tf, 1)
    assert torch.equal(got, torch.stack([tf(i) for i in imgs[:3]]))                       # sorted by name, L for one channel
    assert load_holdout(str(d), 2, Compose([ToTensor()]), 3).shape == (2, 3, 28, 28)
    with pytest.raises(FileNotFoundError):
        load_holdout(str(tmp_path / "none"), 2, tf, 1)


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_the_new_entry_points_are_declared_and_built_exact():
    from siss_amd import build, lib
    import tools.gen_header as gen_header
    names = ("siss_mia_gather", "siss_mia_transfer", "siss_mia_transfer_sqerr", "siss_mia_powdiff")
    for n in names:
        assert n in lib.SIGNATURES and lib.PARAMS[n][-1] == "stream" and n in lib.F32_SAME, n
    assert lib.RESTYPE["siss_mia_partials_words"] is lib.L
    assert "mia.hip" in build.EXACT and "mia.hip" in build.sources() and "mia.hip" in gen_header.ORDER
    header, _ = gen_header.generate()
    assert header == open(os.path.join(ROOT, "include", "siss_hip.h")).read()


def test_the_settings_of_the_class_are_checked_on_the_host():
    from siss_amd.mia import MembershipAttack, check_settings
    from siss_amd.scheduler import DDPMScheduler
    m = MembershipAttack(None, DDPMScheduler(), "cpu", secmi=dict(t_sec=30, stride=10), loss=dict(noises=3))
    assert [m.forwards_per_image(a) for a in m.attacks] == [5, 2, 3]
    with pytest.raises(ValueError, match="batch_size"):
        MembershipAttack(None, DDPMScheduler(), "cpu", batch_size=0)
    attacks, s = check_settings(("pia",), 1000, pia=dict(p=2))
    assert attacks == ("pia",) and s["pia"] == dict(t=200, p=2) and s["secmi"] == dict(t_sec=100, stride=10)
    for kw in (dict(secmi=dict(t_sec=30, stride=20)), dict(secmi=dict(t_sec=0, stride=10)), dict(secmi=dict(t_sec=990, stride=10)),
               dict(pia=dict(p=1)), dict(loss=dict(t=1000))):
        with pytest.raises(ValueError):
            check_settings(("secmi", "pia", "loss"), 1000, **kw)

"""CPU tests of the opt-in DPM-Solver++ (2M) sampler's host side: DPMSolverMultistepScheduler (siss_amd/scheduler.py) against the
f64 restatement tests/dpm_solver_ref.py -- timestep tables, order 1 = DDIM, exact solutions on a point mass, the order of convergence
on Gaussian data --, its refusals and loaders, the pipeline.sampler key of the four YAMLs and the record fields."""
import json
import os

import numpy as np
import pytest
import torch

import dpm_solver_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
LIN = dict(beta_start=1e-4, beta_end=0.02, beta_schedule="linear")


def _sch(**kw):
    from siss_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def _ac(kw):
    return R.betas_ac(kw["beta_schedule"], kw["beta_start"], kw["beta_end"])


# ---------------------------------------------------------------- timesteps and coefficients
def test_timestep_tables():
    assert _sch().set_timesteps(5) == [999, 799, 599, 400, 200]
    assert _sch(timestep_spacing="leading", steps_offset=1).set_timesteps(5) == [831, 665, 499, 333, 167]
    for spacing, offset in (("linspace", 0), ("leading", 1)):
        s = _sch(timestep_spacing=spacing, steps_offset=offset, **SD)
        ts = s.set_timesteps(50)
        assert ts == R.timesteps(50, 1000, spacing, offset) and len(ts) == 50 and s.timesteps is ts
        assert all(a > b for a, b in zip(ts, ts[1:])) and 0 < ts[-1] and ts[0] < 1000
    assert _sch(**SD).set_timesteps(50)[:3] == [999, 979, 959]
    assert _sch(timestep_spacing="leading", steps_offset=1, **SD).set_timesteps(50)[:3] == [951, 932, 913]     # 19 * 50 + 1
    for bad in (0, 1000):
        with pytest.raises(ValueError):
            _sch().set_timesteps(bad)
    with pytest.raises(ValueError):
        _sch(timestep_spacing="leading", steps_offset=200).set_timesteps(5)       # 830 + 200 >= 1000


@pytest.mark.parametrize("kw,spacing,offset", [(LIN, "linspace", 0), (SD, "leading", 1)])
@pytest.mark.parametrize("order", [1, 2])
def test_coefficients_match_the_f64_restatement(kw, spacing, offset, order):
    s = _sch(solver_order=order, timestep_spacing=spacing, steps_offset=offset, **kw)
    ac, ts = _ac(kw), s.set_timesteps(20)
    for i in range(20):
        for first in ((None,) if i == 0 else (None, True)):
            got, want = s.coeffs(i, first=first), R.coeffs(ac, ts, i, order, first=first)
            assert all(np.float32(g) == g for g in got)                            # rounded once to f32
            np.testing.assert_allclose(got, want, rtol=2.0 ** -23, atol=0)
            assert (got[4] == 0.0) == (order == 1 or i == 0 or bool(first) or i == 19)
    assert s.coeffs(19)[2:] == (0.0, 1.0, 0.0)                                     # the last step: x' = m
    with pytest.raises(ValueError):
        s.coeffs(20)
    with pytest.raises(ValueError):
        _sch().coeffs(0)                                                           # before set_timesteps


def test_order_1_is_ddim():
    from siss_amd.scheduler import DDIMScheduler
    ac, ts = _ac(SD), R.timesteps(10, 1000, "leading", 1)
    rng = np.random.default_rng(0)
    x, e = rng.standard_normal(64), rng.standard_normal(64)
    ddim = DDIMScheduler(steps_offset=1, set_alpha_to_one=False, clip_sample=False, **SD)
    assert ddim.set_timesteps(11)[:10] == ts                  # DDIM's 11-step "leading" grid holds this grid's pairs (stride 90)
    for i in range(9):
        s, t = ts[i], ts[i + 1]
        got, m = R.step(e, x, None, R.coeffs(ac, ts, i, 1))
        want = np.sqrt(ac[t]) * m + np.sqrt(1 - ac[t]) * e
        assert np.abs(got - want).max() <= 1e-12
        # DDIMScheduler.coeffs on the same pair: (sqrt a_s, sqrt(1 - a_s), sqrt a_t, sqrt(1 - a_t)) in f32
        sa, sb, sap, sbp = ddim.coeffs(s)
        a, b, cx, c0, c1 = R.coeffs(ac, ts, i, 1)
        # x' = sap (x - sb e) / sa + sbp e  ==  (sap / sa) x + (sbp - sap sb / sa) e; here: (cx + c0 a) x - c0 b e
        np.testing.assert_allclose(cx + c0 * a, sap / sa, rtol=1e-6)
        np.testing.assert_allclose(-c0 * b, sbp - sap * sb / sa, rtol=1e-6, atol=1e-6 * sbp)
        assert c1 == 0.0


# ---------------------------------------------------------------- exact solutions
@pytest.mark.parametrize("kw,spacing,offset", [(LIN, "linspace", 0), (SD, "leading", 1)])
@pytest.mark.parametrize("order", [1, 2])
def test_point_mass_is_solved_exactly(kw, spacing, offset, order):
    """Data = one point mu: eps(x, s) = (x - a_s mu) / s_s, every x0-prediction is mu and every order is exact."""
    ac, ts = _ac(kw), R.timesteps(20, 1000, spacing, offset)
    rng = np.random.default_rng(1)
    mu, x = rng.standard_normal(32), rng.standard_normal(32)
    eps = lambda v, s: (v - np.sqrt(ac[s]) * mu) / np.sqrt(1 - ac[s])
    states = R.trajectory(ac, ts, x, eps, order)
    prev = x
    for i, got in enumerate(states[:-1]):
        (a_s, s_s, _), (a_t, s_t, _) = R.asl(ac, ts[i]), R.asl(ac, ts[i + 1])
        want = (s_t / s_s) * prev + (a_t - a_s * s_t / s_s) * mu
        assert np.abs(got - want).max() <= 1e-12, (i, np.abs(got - want).max())
        prev = got
    assert np.abs(states[-1] - mu).max() <= 1e-12


def _gaussian_error(kw, spacing, offset, order, K=20, c=0.5, scheduler=None):
    ac, ts = _ac(kw), R.timesteps(K, 1000, spacing, offset)
    var = lambda s: ac[s] * c * c + 1 - ac[s]
    eps = lambda v, s: np.sqrt(1 - ac[s]) * v / var(s)
    x = np.random.default_rng(2).standard_normal(256)
    if scheduler is None:
        got = R.trajectory(ac, ts, x, eps, order)[-2]           # at the last grid time, before the jump to m
    else:                                                       # the same trajectory from the class's own f32 coefficients
        assert scheduler.set_timesteps(K) == ts
        got, m1 = x, None
        for i in range(K - 1):
            got, m1 = R.step(eps(got, ts[i]), got, m1, scheduler.coeffs(i))
    want = x * np.sqrt(var(ts[-1]) / var(ts[0]))
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("kw,spacing,offset,e1,e2", [(LIN, "linspace", 0, 8.6e-2, 1.1e-2), (SD, "leading", 1, 4.8e-2, 3.4e-3)])
def test_gaussian_data_order_2_beats_order_1(kw, spacing, offset, e1, e2):
    """N(0, c^2) data, c = 0.5: the exact solution is known; at K = 20 order 2 has at most 1/4 of order 1's error.  A wrong 1 / (2 r)
    factor or a swapped m / m1 fails this."""
    err1, err2 = (_gaussian_error(kw, spacing, offset, o) for o in (1, 2))
    print(f"\n{kw['beta_schedule']} / {spacing}: order 1 {err1:.3e}, order 2 {err2:.3e}")
    assert err2 <= err1 / 4
    np.testing.assert_allclose([err1, err2], [e1, e2], rtol=0.05)
    for order, want in ((1, err1), (2, err2)):                  # ... and so does the class
        s = _sch(solver_order=order, timestep_spacing=spacing, steps_offset=offset, **kw)
        np.testing.assert_allclose(_gaussian_error(kw, spacing, offset, order, scheduler=s), want, rtol=1e-3)


def test_suffix_starts_at_order_1():
    s = _sch(timestep_spacing="leading", steps_offset=1, **SD)
    ac, ts = _ac(SD), s.set_timesteps(10)
    assert s.coeffs(5, first=True)[4] == 0.0 and s.coeffs(5)[4] != 0.0
    np.testing.assert_allclose(s.coeffs(5, first=True), R.coeffs(ac, ts, 5, 1), rtol=2.0 ** -23)
    eps = lambda v, t: 0.3 * v + 0.1
    x = np.random.default_rng(3).standard_normal(16)
    full = R.trajectory(ac, ts, x, eps, 2, start=5)
    got, m1 = x, None
    for j, i in enumerate(range(5, 10)):
        got, m1 = R.step(eps(got, ts[i]), got, m1, s.coeffs(i, first=(j == 0)))
    assert np.abs(got - full[-1]).max() <= 1e-6 * np.abs(full[-1]).max()


# ---------------------------------------------------------------- refusals and loaders
@pytest.mark.parametrize("key,value", [
    ("algorithm_type", "sde-dpmsolver++"), ("algorithm_type", "dpmsolver"), ("solver_type", "heun"), ("solver_order", 3),
    ("prediction_type", "v_prediction"), ("thresholding", True), ("use_karras_sigmas", True), ("use_lu_lambdas", True),
    ("euler_at_final", True), ("final_sigmas_type", "sigma_min"), ("lower_order_final", False), ("variance_type", "learned"),
    ("trained_betas", [0.1, 0.2]), ("rescale_betas_zero_snr", True), ("timestep_spacing", "trailing")])
def test_refusals_name_the_key(key, value):
    with pytest.raises(NotImplementedError, match=key):
        _sch(**{key: value})


def test_from_pretrained_reads_a_pndm_style_config(tmp_path):
    from siss_amd.scheduler import SD_V1_SCHEDULER, DPMSolverMultistepScheduler as S
    os.makedirs(tmp_path / "scheduler")
    pndm = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
            "beta_start": 0.00085, "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1,
            "trained_betas": None, "clip_sample": False}
    json.dump(pndm, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    s = S.from_pretrained(str(tmp_path))
    assert isinstance(s, S) and s.steps_offset == 1 and s.solver_order == 2 and s.timestep_spacing == "linspace"
    assert torch.equal(s.alphas_cumprod, torch.from_numpy(_ac(SD)).float())
    fallback = S.from_pretrained("/nonexistent")
    assert isinstance(fallback, S) and fallback.steps_offset == SD_V1_SCHEDULER["steps_offset"]
    assert torch.equal(fallback.alphas_cumprod, s.alphas_cumprod)
    assert isinstance(S.from_config(pndm), S)
    json.dump(dict(pndm, prediction_type="v_prediction"), open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    with pytest.raises(NotImplementedError, match="prediction_type"):
        S.from_pretrained(str(tmp_path))


# ---------------------------------------------------------------- the config key
YAMLS = ("delete_celeb", "delete_tshirt", "train_tshirt_mnist", "delete_sd")
NODE = "{name: dpmsolver++, solver_order: 2, timestep_spacing: linspace, steps_offset: 0}"


def _compose(name, overrides=()):
    from siss_amd import hydra_lite as H
    return H.compose(name, os.path.join(ROOT, "config"), list(overrides))


@pytest.mark.parametrize("name", YAMLS)
def test_config_key_is_null_by_default_and_validated(name):
    from siss_amd import hydra_lite as H
    from siss_amd import tasks as T
    from siss_amd.scheduler import DPMSolverMultistepScheduler as S
    cfg = _compose(name)
    assert "sampler" in cfg.pipeline and cfg.pipeline.sampler is None
    assert T._pipeline_sampler(cfg) is None and T._sampler_fields(cfg, None) is None
    on = _compose(name, [f"pipeline.sampler={NODE}", "pipeline.num_inference_steps=20"])
    plain, other = cfg.to_dict(), on.to_dict()
    assert other["pipeline"].pop("sampler") == dict(name="dpmsolver++", solver_order=2, timestep_spacing="linspace", steps_offset=0)
    assert other["pipeline"].pop("num_inference_steps") == 20
    plain["pipeline"].pop("sampler"), plain["pipeline"].pop("num_inference_steps", None)
    assert plain == other                                     # the key touches nothing else of the composed config
    s = T._pipeline_sampler(on)
    assert isinstance(s, S) and s.solver_order == 2 and len(s.timesteps) == 20
    assert T._sampler_fields(on, s) == {"sampler": "dpmsolver++2m", "num_inference_steps": 20}
    # a task refuses another name (and an option the solver does not have) in check_supported: before the first optimizer step
    for bad, exc in (("{name: unipc}", ValueError), ("{name: dpmsolver++, solver_order: 3}", NotImplementedError),
                     ("{name: dpmsolver++, eta: 1.0}", ValueError), ("{solver_order: 2}", ValueError)):
        task = H.instantiate(_compose(name, [f"pipeline.sampler={bad}"]).task, cfg=_compose(name, [f"pipeline.sampler={bad}"]),
                             _recursive_=False)
        with pytest.raises(exc, match="sampler|solver_order"):
            task.check_supported()
    H.instantiate(on.task, cfg=on, _recursive_=False).check_supported()


def test_betas_come_from_the_task():
    from siss_amd import tasks as T
    from siss_amd.scheduler import DDPMScheduler
    on = _compose("delete_tshirt", ["pipeline.sampler={name: dpmsolver++}", "pipeline.num_inference_steps=4"])
    sched = DDPMScheduler(beta_start=2e-4, beta_end=0.03)
    s = T._pipeline_sampler(on, sched)
    assert torch.equal(s.alphas_cumprod, sched.alphas_cumprod) and s.timestep_spacing == "linspace" and s.steps_offset == 0
    # SD: the checkpoint's scheduler_config.json (here: none on disk -> the SD v1 values), "leading" with its steps_offset
    sd = _compose("delete_sd", ["pipeline.sampler={name: dpmsolver++, solver_order: 1}", "pipeline.num_inference_steps=5",
                                "pretrained_model_name_or_path=/nonexistent"])
    s = T.DeleteSD(sd)._sd_solver()
    assert s.timestep_spacing == "leading" and s.steps_offset == 1 and s.solver_order == 1
    assert s.timesteps == [831, 665, 499, 333, 167] and torch.equal(s.alphas_cumprod, torch.from_numpy(_ac(SD)).float())
    assert T.DeleteSD(_compose("delete_sd"))._sd_solver() is None


# ---------------------------------------------------------------- the record fields
def test_records_carry_the_sampler_fields(tmp_path):
    from siss_amd.classifier import TShirtMetrics
    from siss_amd.kmeans import DeletionFraction
    from siss_amd.metric_net import record_mean
    fields = _sch(solver_order=2).record_fields(20)
    assert fields == {"sampler": "dpmsolver++2m", "num_inference_steps": 20}
    assert _sch(solver_order=1).record_fields(15)["sampler"] == "dpmsolver++1m"
    out = str(tmp_path / "m.jsonl")
    assert record_mean(out, "sscd_0", torch.tensor([0.5, 1.0]), 3) == {"global_step": 3, "sscd_0": 0.75}
    assert record_mean(out, "sscd_0", torch.tensor([0.5, 1.0]), 4, fields) == {"global_step": 4, "sscd_0": 0.75, **fields}
    for extra in (None, fields):
        frac = DeletionFraction(None, out)
        frac.extra = extra
        frac.record(0, torch.tensor([0, 1, 1, 1]), 5)
        tm = TShirtMetrics(torch.zeros(1, 4, 4), out, lambda n, b: torch.ones(n, 1, 4, 4), sampling_steps=1, eval_images=2)
        tm.extra = extra
        tm(6)
    lines = [json.loads(l) for l in open(out)]
    assert [set(fields) <= set(r) for r in lines] == [False, True, False, False, True, True]
    assert lines[2] == {"global_step": 5, "deletion_fraction_0": 0.75} and lines[4]["sampler"] == "dpmsolver++2m"
    assert set(lines[3]) == {"global_step", "deletion_class_fraction", "seconds"}

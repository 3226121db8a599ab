"""The likelihood metric's host side (no GPU): the numpy RK45 restatement against scipy, the VP-SDE table / prior / bits-per-dim
formula against f64, and the config surface (target remap, refusals, opt-in)."""
import math
import os

import numpy as np
import pytest
import torch

from likelihood_ref import rk45_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the host RK45 against scipy
def _linear(t, y):
    return np.array([[-0.5, 1.0, 0.0], [-1.0, -0.5, 0.2], [0.0, 0.3, -2.0]]) @ y


def _nonlinear(t, y):
    return np.array([y[1], (1 - y[0] ** 2) * y[1] - y[0], -y[2] * np.cos(3 * t)])      # van der Pol + a forced decay


def _floored(t, y):
    # piecewise constant in t through an f32 floor, as the likelihood ODE's label (t * 999, f32, .long())
    lab = int(np.float32(t) * np.float32(999))
    return -0.5 * (0.1 + 0.0199 * lab) * y + 0.01 * np.sin(lab / 50.0)


@pytest.mark.parametrize("fun, y0, t_span, tol", [
    (_linear, [1.0, -0.5, 2.0], (0.0, 4.0), (1e-5, 1e-5)),
    (_nonlinear, [2.0, 0.0, 1.0], (1e-5, 3.0), (1e-5, 1e-5)),
    (_floored, [1.0, 2.0, -3.0, 0.5], (1e-5, 1.0), (1e-5, 1e-5)),
    (_linear, [1.0, -0.5, 2.0], (0.0, 1.0), (1e-3, 1e-6)),
], ids=["linear", "nonlinear", "floored-label", "linear-loose"])
def test_host_rk45_matches_scipy_solve_ivp(fun, y0, t_span, tol):
    integrate = pytest.importorskip("scipy.integrate")
    ref = integrate.solve_ivp(fun, t_span, np.array(y0), method="RK45", rtol=tol[0], atol=tol[1])
    got = rk45_host(fun, t_span[0], np.array(y0), t_span[1], rtol=tol[0], atol=tol[1])
    assert ref.status == 0
    assert got.nfev == ref.nfev
    assert got.t == list(ref.t)
    np.testing.assert_allclose(got.y, ref.y[:, -1], rtol=1e-13, atol=0)
    assert (got.nfev - 2) % 6 == 0


# ---------------------------------------------------------------- 2. the VP-SDE and the bits/dim formula
def test_vpsde_table_prior_and_bpd_against_f64():
    from siss_amd.likelihood import VPSDE, bits_per_dim
    sde = VPSDE()
    assert (sde.beta_0, sde.beta_1, sde.N, sde.T) == (0.1, 20.0, 1000, 1)
    N = 1000
    ac = np.cumprod(1 - np.linspace(0.1 / N, 20.0 / N, N))
    ref = np.sqrt(1 - ac).astype(np.float32)
    assert sde.sqrt_1m_alphas_cumprod.dtype == torch.float32
    assert np.array_equal(sde.sqrt_1m_alphas_cumprod.numpy(), ref)          # f64, rounded once
    # beta(t), label and std in the reference's f32 arithmetic
    for t in (1e-5, 0.25, 0.5004, 0.999999, 1.0):
        beta, std, label = sde.coefficients(t)
        t32 = torch.ones(1) * t
        assert beta == (0.1 + t32 * (20 - 0.1)).item()
        assert label == int((t32 * 999).long())
        assert std == sde.sqrt_1m_alphas_cumprod[label]
    # prior log-density and bits/dim
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 1, 28, 28, generator=g)
    delta = torch.tensor([3.5, -120.25], dtype=torch.float64)
    D = 784
    prior = -D / 2 * math.log(2 * math.pi) - (z.double() ** 2).sum(dim=(1, 2, 3)) / 2
    assert torch.allclose(sde.prior_logp(z), prior, rtol=1e-15, atol=0)
    bpd = bits_per_dim(z, delta, sde)
    assert torch.allclose(bpd, -(prior + delta) / math.log(2) / D + 7, rtol=1e-15, atol=0)


# ---------------------------------------------------------------- 3. the config surface
def test_target_remap_instantiates_the_reference_config_node():
    from siss_amd import hydra_lite as H
    from siss_amd.likelihood import LikelihoodEvaluator, VPSDE
    assert H.TARGET_REMAP["metrics.likelihood.LikelihoodEvaluator"] == "siss_amd.likelihood.LikelihoodEvaluator"
    assert H.TARGET_REMAP["metrics.song_likelihood.sde_lib.VPSDE"] == "siss_amd.likelihood.VPSDE"
    node = H.Cfg({"_target_": "metrics.likelihood.LikelihoodEvaluator", "sde": {"_target_": "metrics.song_likelihood.sde_lib.VPSDE"}})
    ev = H.instantiate(node)
    assert isinstance(ev, LikelihoodEvaluator) and isinstance(ev.sde, VPSDE)
    assert (ev.hutchinson_type, ev.rtol, ev.atol, ev.method, ev.eps) == ("Rademacher", 1e-5, 1e-5, "RK45", 1e-5)


def test_what_is_not_built_is_refused():
    from siss_amd import hydra_lite as H
    from siss_amd.likelihood import LikelihoodEvaluator, VPSDE
    with pytest.raises(NotImplementedError, match="RK45"):
        LikelihoodEvaluator(VPSDE(), method="RK23")
    with pytest.raises(NotImplementedError, match="VP-SDE"):
        H.instantiate(H.Cfg({"_target_": "metrics.likelihood.LikelihoodEvaluator",
                             "sde": {"_target_": "metrics.song_likelihood.sde_lib.VESDE"}}))
    with pytest.raises(NotImplementedError, match="VP-SDE"):
        LikelihoodEvaluator(object())
    with pytest.raises(NotImplementedError, match="Hutchinson"):
        LikelihoodEvaluator(VPSDE(), hutchinson_type="Uniform")

    from siss_amd.unet_cond import UNetCondEngine              # a conditional (SD) engine is refused before anything runs
    fake = UNetCondEngine.__new__(UNetCondEngine)
    with pytest.raises(NotImplementedError, match="unconditional"):
        LikelihoodEvaluator(VPSDE()).engine_for(type("M", (), {"engine": fake})())


def test_configs_without_the_metric_take_no_new_path(monkeypatch, tmp_path):
    from siss_amd import hydra_lite as H
    from siss_amd import likelihood
    from siss_amd.tasks import DeleteTShirt

    def boom(*a, **k):
        raise AssertionError("the likelihood metric was built for a config without metrics.likelihood")
    monkeypatch.setattr(likelihood.LikelihoodEvaluator, "__init__", boom)
    monkeypatch.setattr(likelihood, "log_likelihood", boom)
    for name in ("delete_tshirt", "delete_celeb"):
        cfg = H.compose(name, os.path.join(ROOT, "config"), [f"output_dir={tmp_path}"])
        assert not (cfg.get("metrics") or {}).get("likelihood")
        assert DeleteTShirt(cfg).likelihood_metric(None, torch.zeros(1, 28, 28), "cpu") is None
    # ... and with it, the reference's node builds (nothing runs until an evaluation)
    monkeypatch.undo()
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    [f"output_dir={tmp_path}", "+metrics.likelihood.step_frequency=30",
                     "+metrics.likelihood.class_cfg._target_=metrics.likelihood.LikelihoodEvaluator",
                     "+metrics.likelihood.class_cfg.sde._target_=metrics.song_likelihood.sde_lib.VPSDE"])
    freq, fn = DeleteTShirt(cfg).likelihood_metric(None, torch.zeros(1, 28, 28), "cpu")
    assert freq == 30 and callable(fn)

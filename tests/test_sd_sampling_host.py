"""CPU tests of the SD validation sampling's host side: the DDIM schedule against a float64 restatement of diffusers 0.27
``DDIMScheduler.set_timesteps`` / ``step`` ("leading" spacing, eta = 0), the scheduler_config.json loader and its refusals,
the empty-prompt token ids, and the make_grid layout of the validation PNGs."""
import json

import numpy as np
import pytest
import torch


def _diffusers_f64(steps, offset, set_alpha_to_one, T=1000, beta_start=0.00085, beta_end=0.012):
    """diffusers 0.27 DDIMScheduler (scaled_linear betas): timesteps and (alpha_prod_t, alpha_prod_t_prev) per step, float64."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float64) ** 2
    ac = np.cumprod(1.0 - betas)
    final = 1.0 if set_alpha_to_one else ac[0]
    ratio = T // steps
    ts = (np.arange(0, steps) * ratio).round()[::-1].astype(np.int64) + offset
    pairs = []
    for t in ts:
        prev = t - T // steps
        pairs.append((ac[t], ac[prev] if prev >= 0 else final))
    return ts.tolist(), pairs


@pytest.mark.parametrize("steps", [1, 10, 50, 1000])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("one", [True, False])
def test_ddim_schedule_matches_diffusers(steps, offset, one):
    from siss_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=offset,
                        set_alpha_to_one=one, clip_sample=False)
    if steps == 1000 and offset == 1:                    # timestep 1000 is past the table (diffusers: an index error)
        with pytest.raises(ValueError):
            sch.set_timesteps(steps)
        return
    ts, pairs = _diffusers_f64(steps, offset, one)
    assert sch.set_timesteps(steps) == ts
    for t, (a, ap) in zip(ts, pairs):
        got_a, got_ap = sch.alphas(t)
        assert abs(float(got_a) - a) <= 2e-6 * a and abs(float(got_ap) - ap) <= 2e-6 * ap, (t, float(got_a), a, float(got_ap), ap)
        sa, sb, sap, sbp = sch.coeffs(t)
        assert abs(sa - a ** 0.5) <= 2e-6 and abs(sb - (1 - a) ** 0.5) <= 2e-6
        assert abs(sap - ap ** 0.5) <= 2e-6 and abs(sbp - (1 - ap) ** 0.5) <= 2e-6


def test_sd_v1_defaults_give_the_reference_schedule():
    from siss_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler.from_pretrained("/nonexistent")
    ts = sch.set_timesteps(50)
    assert ts == list(range(981, 0, -20)) and ts[0] == 981 and ts[-1] == 1
    a, ap = sch.alphas(1)
    assert ap == sch.alphas_cumprod[0]                   # prev_t < 0, set_alpha_to_one = false: alpha_prod_0
    assert not sch.clip_sample


def test_scheduler_config_json_is_read_and_unimplemented_options_refused(tmp_path):
    from siss_amd.scheduler import DDIMScheduler
    (tmp_path / "scheduler").mkdir()
    cfgf = tmp_path / "scheduler" / "scheduler_config.json"
    base = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.7.0.dev0", "beta_end": 0.012,
            "beta_schedule": "scaled_linear", "beta_start": 0.00085, "num_train_timesteps": 1000, "set_alpha_to_one": True,
            "skip_prk_steps": True, "steps_offset": 0, "trained_betas": None, "clip_sample": True, "clip_sample_range": 2.5}
    json.dump(base, open(cfgf, "w"))
    sch = DDIMScheduler.from_pretrained(str(tmp_path))
    assert sch.set_timesteps(10)[0] == 900 and sch.clip_sample and sch.clip_sample_range == 2.5
    assert float(sch.alphas(0)[1]) == 1.0                # set_alpha_to_one
    for bad in ({"timestep_spacing": "trailing"}, {"timestep_spacing": "linspace"}, {"thresholding": True},
                {"prediction_type": "v_prediction"}, {"prediction_type": "sample"}, {"rescale_betas_zero_snr": True}):
        json.dump({**base, **bad}, open(cfgf, "w"))
        with pytest.raises(NotImplementedError):
            DDIMScheduler.from_pretrained(str(tmp_path))


def test_sampler_refuses_eta_and_other_norms():
    from siss_amd.sd_sampler import SDSampler
    pipe = SDSampler(unet=None)
    e = torch.zeros(1, 77, 8)
    with pytest.raises(NotImplementedError):
        pipe(e, eta=0.5)
    with pytest.raises(NotImplementedError):
        pipe(e, lp=1)


def test_unconditional_ids_fallback(tmp_path):
    from siss_amd.sd_sampler import SD_V1_UNCOND_IDS, uncond_ids
    assert SD_V1_UNCOND_IDS == [49406] + [49407] * 76
    for path in (None, str(tmp_path)):                   # no tokenizer/ on disk
        ids = uncond_ids(path)
        assert ids.dtype == torch.long and ids.tolist() == [[49406] + [49407] * 76]


def test_grid_layout_is_make_grids():
    from siss_amd.tasks import _grid
    ims = [np.full((8, 6, 3), 10 * (k + 1), dtype=np.uint8) for k in range(5)]
    g = np.asarray(_grid(ims, 2))
    assert g.shape == (3 * 10 + 2, 2 * 8 + 2, 3)         # ceil(5 / 2) rows of (8 + 2), 2 columns of (6 + 2), + 2
    assert (g[2:10, 2:8] == 10).all() and (g[2:10, 10:16] == 20).all() and (g[22:30, 2:8] == 50).all()
    assert (g[0:2] == 0).all() and (g[22:30, 10:16] == 0).all()      # padding and the empty cell stay black

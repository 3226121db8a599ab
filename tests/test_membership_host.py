"""CPU tests of the membership-loss metric: the f64 restatement against the reference's recorded outputs
(tests/golden/membership_ref.npz, written by tests/make_membership_golden.py), MembershipLoss.sample_images against the recorded
draws, the work-table builder, the config remap and every refusal of check_metrics."""
import os
import random

import numpy as np
import pytest
import torch

from membership_ref import membership_f64, seeded_oracle, state_checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["del1", "del9"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "membership_ref.npz"))


def _case(fx, name):
    pool_all, pool_del = torch.from_numpy(fx["pool_all"]), torch.from_numpy(fx[f"{name}_pool_del"])
    return pool_all, pool_del, fx[f"{name}_idx_all"].tolist(), fx[f"{name}_idx_del"].tolist(), torch.from_numpy(fx[f"{name}_noise"])


@pytest.mark.parametrize("name", CASES)
def test_f64_restatement_matches_the_reference_outputs(fx, name):
    from siss_amd.scheduler import DDPMScheduler
    net = seeded_oracle(int(fx["net_seed"]))
    assert abs(state_checksum(net.state_dict()) - float(fx["checksum"])) <= 1e-9 * abs(float(fx["checksum"])), "the seeded weights differ"
    pool_all, pool_del, ia, idl, noise = _case(fx, name)
    sums, means = membership_f64(net.double(), DDPMScheduler().alphas_cumprod, pool_all[ia], pool_del[idl], noise, fx["timesteps"].tolist())
    ref = fx[f"{name}_ref"].astype(np.float64)
    rel = float((np.abs(means.numpy() - ref) / np.abs(ref)).max())
    print(f"\n{name}: f64 restatement vs the reference's f32 outputs: {rel:.2e} relative")
    assert rel <= 1e-6, rel
    I, J = int(fx["I"]), int(fx["J"])
    assert sums.shape == (len(fx["timesteps"]), 2, I, J)
    if name == "del1":                                   # one forget image: every forget row is the same pair
        assert torch.equal(sums[:, 1], sums[:, 1, :1].expand(-1, I, -1))


@pytest.mark.parametrize("name", CASES)
def test_sample_images_draws_the_recorded_indices(fx, name):
    from siss_amd.membership import MembershipLoss
    pool_all, pool_del, ia, idl, noise = _case(fx, name)
    m = MembershipLoss(list(pool_all), list(pool_del), None, None, int(fx["I"]), int(fx["J"]), int(fx["eval_batch_size"]), "cpu")
    random.seed(int(fx[f"{name}_random_seed"]))
    m.sample_images()
    assert m.all_indices == ia and m.deletion_indices == idl
    assert torch.equal(m.all_sampled_images, pool_all[ia]) and torch.equal(m.deletion_sampled_images, pool_del[idl])
    assert m.all_sampled_images.dtype == torch.float32 and m.all_sampled_images.shape == (int(fx["I"]), 3, 16, 16)
    g = torch.Generator().manual_seed(3)
    m.sample_noises(generator=g)
    assert m.noise.shape == (int(fx["J"]), 3, 16, 16)
    assert torch.equal(m.noise, torch.randn(m.noise.shape, generator=torch.Generator().manual_seed(3)))
    assert m.pairs_per_forward == int(fx["eval_batch_size"])
    assert MembershipLoss(None, None, None, None, 5, 3, 4, "cpu", pairs_per_forward=15).pairs_per_forward == 15


def test_work_table_order_without_dedupe():
    from siss_amd.membership import build_work_table
    items, pair = build_work_table([7, 2], [4, 4], 3, [200, 900], dedupe=False)
    I, J = 2, 3
    want = [(g * I + i, j, t) for t in (200, 900) for g in (0, 1) for i in range(I) for j in range(J)]
    assert items.dtype == np.int64 and items.tolist() == [list(w) for w in want]
    assert pair.shape == (2, 2, I, J) and pair.reshape(-1).tolist() == list(range(len(want)))      # timestep, group, image, noise


def test_work_table_dedupe_shares_a_repeated_forget_image():
    from siss_amd.membership import build_work_table
    I, J, ts = 5, 3, [200, 900]
    items, pair = build_work_table([3, 9, 1, 0, 6], [0] * I, J, ts, dedupe=True)
    assert len(items) == len(ts) * (I * J + J)
    per_t = I * J + J
    for ti, t in enumerate(ts):
        blk = items[ti * per_t:(ti + 1) * per_t]
        assert (blk[:, 2] == t).all()
        assert blk[:I * J, 0].tolist() == [i for i in range(I) for _ in range(J)] and blk[:I * J, 1].tolist() == list(range(J)) * I
        assert blk[I * J:].tolist() == [[I, j, t] for j in range(J)]                      # the forget image once: pool row I
        for i in range(I):
            assert pair[ti, 0, i].tolist() == [ti * per_t + i * J + j for j in range(J)]
            assert pair[ti, 1, i].tolist() == [ti * per_t + I * J + j for j in range(J)]  # every forget row: the same items
    # a partly repeated forget draw: rows 0 and 2 share index 4, row 1 stands alone
    items, pair = build_work_table([0, 1, 2], [4, 8, 4], 2, [10], dedupe=True)
    assert items.tolist() == [[0, 0, 10], [0, 1, 10], [1, 0, 10], [1, 1, 10], [2, 0, 10], [2, 1, 10],
                              [3, 0, 10], [3, 1, 10], [4, 0, 10], [4, 1, 10]]
    assert pair[0, 1].tolist() == [[6, 7], [8, 9], [6, 7]]
    # every pair points at an item of its own timestep, noise and (an image with the same dataset index)
    for (ti, g, i, j), it in np.ndenumerate(pair):
        assert items[it, 1] == j and items[it, 2] == 10


def test_work_table_ragged_tail_and_refusals():
    from siss_amd.membership import build_work_table
    items, _ = build_work_table(list(range(5)), [0] * 5, 3, [200, 900], dedupe=True)
    assert len(items) == 36 and len(items) % 15 == 6 and -(-len(items) // 4) == 9      # forwards at 15 / 4 items each
    items, _ = build_work_table(list(range(5)), [0] * 5, 3, [200, 900], dedupe=False)
    assert len(items) == 60
    with pytest.raises(ValueError):
        build_work_table([0, 1], [0], 3, [1])
    with pytest.raises(ValueError):
        build_work_table([0], [0], 3, [])


def test_target_remap_instantiates_the_reference_class_cfg():
    from siss_amd import hydra_lite as H
    from siss_amd.membership import MembershipLoss
    assert H.TARGET_REMAP["metrics.class_membership.MembershipLoss"] == "siss_amd.membership.MembershipLoss"
    node = H.Cfg({"_target_": "metrics.class_membership.MembershipLoss", "num_image_samples": 32, "num_noise_samples": 32,
                  "eval_batch_size": 4})
    m = H.instantiate(node, dataset_all=[0], dataset_deletion=[0], noise_scheduler=None, unet=None, device="cpu")
    assert type(m) is MembershipLoss and (m.num_image_samples, m.num_noise_samples, m.eval_batch_size) == (32, 32, 4)
    assert m.dedupe and m.use_graph and m.pairs_per_forward == 4


BASE = ["+metrics.membership_loss.class_cfg._target_=metrics.class_membership.MembershipLoss",
        "+metrics.membership_loss.class_cfg.num_image_samples=5", "+metrics.membership_loss.class_cfg.num_noise_samples=3",
        "+metrics.membership_loss.class_cfg.eval_batch_size=4", "+metrics.membership_loss.timesteps=[200, 900]",
        "+metrics.membership_loss.step_frequency=1"]


def _task(config, extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose(config, os.path.join(ROOT, "config"), [*BASE, *extra])
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt"])
def test_check_metrics_refuses_what_cannot_run(config):
    _task(config, []).check_metrics()                                                   # the block as the reference documents it
    _task(config, ["+metrics.membership_loss.plot_params.time_frequency=100"]).check_metrics()
    for bad, exc in (("+metrics.membership_loss.step_frequency=0", ValueError), ("+metrics.membership_loss.step_frequency=-2", ValueError),
                     ("+metrics.membership_loss.step_frequency=null", ValueError), ("+metrics.membership_loss.timesteps=[]", ValueError),
                     ("+metrics.membership_loss.timesteps=[200, 1000]", ValueError), ("+metrics.membership_loss.timesteps=[-1]", ValueError),
                     ("+metrics.membership_loss.timesteps=null", ValueError), ("+metrics.membership_loss.class_cfg=null", ValueError),
                     ("+metrics.membership_loss.class_cfg.num_image_samples=0", ValueError),
                     ("+metrics.membership_loss.plot_params.time_frequency=0", ValueError)):
        with pytest.raises(exc, match="membership_loss"):
            _task(config, [bad]).check_metrics()
    # num_image_samples against the datasets' lengths (known once they are loaded, still before the first step)
    t = _task(config, [])
    assert t.check_membership(5, 1) is not None and t.check_membership(5, 9) is not None   # one forget image is repeated
    with pytest.raises(ValueError, match="dataset_all"):
        t.check_membership(4, 1)
    with pytest.raises(ValueError, match="dataset_deletion"):
        t.check_membership(4096, 3)
    # the key null: nothing to check
    from siss_amd import hydra_lite as H
    cfg = H.compose(config, os.path.join(ROOT, "config"), ["+metrics.membership_loss=null"])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.check_metrics()
    assert task.check_membership(1, 1) is None


def test_the_sd_task_refuses_the_metric():
    with pytest.raises(NotImplementedError, match="membership_loss"):
        _task("delete_sd", []).check_metrics()

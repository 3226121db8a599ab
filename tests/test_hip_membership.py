"""The membership-loss metric on the GPU: the two index-driven kernels (siss_pair_noise bitwise against torch's add_noise,
siss_pair_sqerr against an exact sum), MembershipLoss end to end against the f64 restatement of the reference on the f64 oracle
network (f32 engine: the f32 instrument bound; bf16 engine: against the reference's own bf16 path), graph against eager, the launch
count, the training state, a negative control for the bound, and the two pixel-space tasks."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from membership_ref import CELEB_TINY, f32_bound, membership_f64, seeded_oracle, state_checksum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "membership_ref.npz"))


# ---------------------------------------------------------------- 1. siss_pair_noise
def _table(g, n_items, n_images, n_noises, T=1000):
    """A work table that repeats and permutes its indices (nothing like the builder's regular order)."""
    return torch.stack([torch.randint(0, n_images, (n_items,), generator=g), torch.randint(0, n_noises, (n_items,), generator=g),
                        torch.randint(0, T, (n_items,), generator=g)], dim=1).contiguous()


@pytest.mark.parametrize("chw", [768, 784, 75, 300], ids=lambda c: f"chw{c}")
def test_pair_noise_is_bitwise_torchs_add_noise(dev, chw):
    from siss_amd import lib
    from siss_amd.scheduler import DDPMScheduler
    ac = DDPMScheduler().alphas_cumprod
    # the coefficients by a correctly rounded f32 square root (numpy's), not by torch's CPU one: on an AVX-512 host torch's f32
    # sqrt / pow(x, 0.5) is one ulp off the IEEE value for 177 (sqrt(ac)) and 284 (sqrt(1 - ac)) of the 1000 timesteps (measured on
    # the MI355X host; 6 and 5 on an AVX2 host), while torch on the GPU and the kernel both give the IEEE value for all of them.
    # The products and the sum are torch's CPU f32 ones: IEEE on every host.
    sa, sb = torch.from_numpy(np.sqrt(ac.numpy())), torch.from_numpy(np.sqrt(np.float32(1) - ac.numpy()))
    g = torch.Generator().manual_seed(chw)
    n_images, n_noises, n_items, b = 7, 4, 22, 8                      # 22 = 2 * 8 + 6: the last forward has two rows past the table
    imgs, noise = torch.rand(n_images, chw, generator=g) * 2 - 1, torch.randn(n_noises, chw, generator=g)
    items = _table(g, n_items, n_images, n_noises)
    items[3] = items[11]                                              # a repeated item
    d_imgs, d_noise, d_items, d_ac = imgs.to(dev), noise.to(dev), items.to(dev), ac.to(dev)
    offset = torch.zeros(1, dtype=torch.long, device=dev)
    for off in (0, 8, 16, 5):
        xs = torch.full((b, chw), float("nan"), device=dev)
        ts = torch.full((b,), -7, dtype=torch.long, device=dev)
        offset.fill_(off)
        lib.call("siss_pair_noise", d_imgs, d_noise, d_items, offset, n_items, n_images, n_noises, d_ac, ac.numel(), b, chw, xs, ts)
        torch.cuda.synchronize()
        xs, ts = xs.cpu(), ts.cpu()
        for r in range(b):
            if off + r < n_items:
                i, j, t = items[off + r].tolist()
                want = sa[t] * imgs[i] + sb[t] * noise[j]                                   # DDPMScheduler.add_noise, f32, on the CPU
                assert torch.equal(xs[r].view(torch.int32), want.view(torch.int32)), (off, r)
                assert int(ts[r]) == t
            else:
                assert torch.equal(xs[r], torch.zeros(chw)) and int(ts[r]) == 0, (off, r)     # tail rows: zeros, t = 0
    # the scheduler's own add_noise on the device gives the same bits (what the plain composition computes there)
    want = DDPMScheduler().add_noise(d_imgs[d_items[:b, 0]], d_noise[d_items[:b, 1]], d_items[:b, 2]).cpu()
    offset.fill_(0)
    xs = torch.empty(b, chw, device=dev)
    ts = torch.empty(b, dtype=torch.long, device=dev)
    lib.call("siss_pair_noise", d_imgs, d_noise, d_items, offset, n_items, n_images, n_noises, d_ac, ac.numel(), b, chw, xs, ts)
    assert torch.equal(xs.cpu(), want)


def test_pair_noise_never_follows_an_index_out_of_its_tensor(dev):
    """An item that points outside the images, the noises or the schedule is written as a tail row (zeros), not read."""
    from siss_amd import lib
    chw, b = 64, 4
    imgs, noise, ac = torch.ones(2, chw, device=dev), torch.ones(3, chw, device=dev), torch.full((10,), 0.5, device=dev)
    items = torch.tensor([[0, 0, 1], [2, 0, 1], [0, 3, 1], [0, 0, 10]], device=dev)
    xs, ts = torch.full((b, chw), float("nan"), device=dev), torch.full((b,), -1, dtype=torch.long, device=dev)
    lib.call("siss_pair_noise", imgs, noise, items, torch.zeros(1, dtype=torch.long, device=dev), 4, 2, 3, ac, 10, b, chw, xs, ts)
    assert bool((xs[0] != 0).all()) and bool((xs[1:] == 0).all()) and ts.tolist() == [1, 0, 0, 0]


# ---------------------------------------------------------------- 2. siss_pair_sqerr
@pytest.mark.parametrize("chw", [768, 784, 75, 300], ids=lambda c: f"chw{c}")
def test_pair_sqerr_against_the_exact_sum_of_the_f32_squares(dev, chw):
    from siss_amd import lib
    g = torch.Generator().manual_seed(100 + chw)
    n_noises, n_items, b = 4, 22, 8
    noise, items = torch.randn(n_noises, chw, generator=g), _table(g, n_items, 7, n_noises)
    d_noise, d_items = noise.to(dev), items.to(dev)
    offset = torch.zeros(1, dtype=torch.long, device=dev)
    partials = torch.zeros(int(lib.query("siss_pair_partials_words", b, chw)), dtype=torch.float64, device=dev)
    POISON = -12345.0

    def run():
        sums = torch.full((n_items + b,), POISON, dtype=torch.float64, device=dev)       # b guard entries past the table
        preds = []
        gp = torch.Generator().manual_seed(chw)
        for off in (0, 8, 16):
            pred = torch.randn(b, chw, generator=gp)
            preds.append(pred)
            offset.fill_(off)
            lib.call("siss_pair_sqerr", pred.to(dev), d_noise, d_items, offset, n_items, n_noises, b, chw, sums, partials)
        torch.cuda.synchronize()
        return sums.cpu(), torch.cat(preds)

    sums, preds = run()
    again, _ = run()
    assert torch.equal(sums.view(torch.int64), again.view(torch.int64)), "two runs differ"
    assert bool((sums[n_items:] == POISON).all()), "a row past the end of the table wrote its sum"
    worst = 0.0
    for k in range(n_items):
        d = preds[k] - noise[items[k, 1]]                              # f32 difference, f32 square (torch's (out - noise) ** 2)
        exact = math.fsum((d * d).double().tolist())
        worst = max(worst, abs(float(sums[k]) - exact) / exact)
    print(f"\nchw {chw}: worst relative error of the f64 sum {worst:.2e} (bound {chw * 2.0 ** -53:.2e})")
    assert worst <= chw * 2.0 ** -53
    # a forward in the middle of the table touches its own b entries only
    sums = torch.full((n_items,), POISON, dtype=torch.float64, device=dev)
    offset.fill_(8)
    lib.call("siss_pair_sqerr", preds[:b].to(dev), d_noise, d_items, offset, n_items, n_noises, b, chw, sums, partials)
    s = sums.cpu()
    assert bool((s[:8] == POISON).all()) and bool((s[16:] == POISON).all()) and bool((s[8:16] != POISON).all())


# ---------------------------------------------------------------- 3. end to end
def _engine(dtype, sd, kw=CELEB_TINY):
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    eng = UNetEngine(UNet2DConfig(**kw), "cuda:0", dtype=dtype)
    eng.load_state_dict(sd)
    return eng


def _oracle(fx):
    net = seeded_oracle(int(fx["net_seed"]))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert abs(state_checksum(sd) - float(fx["checksum"])) <= 1e-9 * abs(float(fx["checksum"])), "the seeded weights differ"
    return net, sd


def _case(fx, name):
    pool_all, pool_del = torch.from_numpy(fx["pool_all"]), torch.from_numpy(fx[f"{name}_pool_del"])
    return pool_all, pool_del, fx[f"{name}_idx_all"].tolist(), fx[f"{name}_idx_del"].tolist(), torch.from_numpy(fx[f"{name}_noise"])


def _metric(fx, name, eng, dev, **kw):
    from siss_amd.membership import MembershipLoss
    from siss_amd.scheduler import DDPMScheduler
    pool_all, pool_del, ia, idl, noise = _case(fx, name)
    m = MembershipLoss(list(pool_all), list(pool_del), DDPMScheduler(), eng, int(fx["I"]), int(fx["J"]), int(fx["eval_batch_size"]), dev, **kw)
    random.seed(int(fx[f"{name}_random_seed"]))
    m.sample_images()
    assert m.all_indices == ia and m.deletion_indices == idl
    m.noise = noise.to(dev)
    return m


def _reference(fx, name, net64, roll=0, timesteps=None):
    from siss_amd.scheduler import DDPMScheduler
    pool_all, pool_del, ia, idl, noise = _case(fx, name)
    ts = fx["timesteps"].tolist() if timesteps is None else timesteps
    return membership_f64(net64, DDPMScheduler().alphas_cumprod, torch.roll(pool_all[ia], roll, 0), pool_del[idl], noise, ts, with_pred_max=True)


@pytest.fixture(scope="module")
def world(fx, dev):
    """The oracle network (f32 and f64), the f32 engine with its weights, and the f64 reference of both fixture cases."""
    net, sd = _oracle(fx)
    net64 = seeded_oracle(int(fx["net_seed"])).double()
    ref = {name: _reference(fx, name, net64) for name in ("del1", "del9")}
    return dict(net=net, sd=sd, net64=net64, ref=ref, eng32=_engine(torch.float32, sd))


CHW = 3 * 16 * 16


@pytest.mark.parametrize("name", ["del1", "del9"])
def test_f32_engine_against_the_f64_reference(fx, dev, world, name):
    sums, means, pmax = world["ref"][name]
    m = _metric(fx, name, world["eng32"], dev)
    losses = m.compute_membership_losses(fx["timesteps"].tolist())
    got = m.pair_sums.cpu()
    assert got.dtype == torch.float64 and got.shape == sums.shape
    bound = f32_bound(sums.numpy(), CHW, pmax)
    err = (got - sums).abs().numpy()
    print(f"\n{name}: f32 engine vs f64 reference: worst pair-sum error {err.max():.3e} (bound there {bound.reshape(-1)[err.argmax()]:.3e}); "
          f"worst error / bound {float((err / bound).max()):.3f}; max|pred| {pmax:.3f}")
    assert (err <= bound).all()
    # the group means: the mean of the pairs' bounds
    mean_err = (m.means.cpu() - means).abs().numpy()
    assert (mean_err <= bound.mean(axis=(2, 3))).all()
    # the returned surface: one [all, deletion] pair of 0-d f32 tensors per timestep, the f32 cast of the f64 means
    assert len(losses) == len(fx["timesteps"]) and all(len(p) == 2 and p[0].dim() == 0 and p[0].dtype == torch.float32 for p in losses)
    assert torch.equal(torch.stack([torch.stack(p) for p in losses]).cpu(), m.means.float().cpu())
    # and the reference's recorded f32 outputs, through the same bound
    assert (np.abs(m.means.cpu().numpy() - fx[f"{name}_ref"].astype(np.float64)) <= bound.mean(axis=(2, 3)) + 1e-6 * means.numpy()).all()


def test_negative_control_a_wrong_image_index_breaks_the_bound(fx, dev, world):
    """The bound bites: at t = 200 the reference evaluated with the kept images rolled by one (a wrong image index) is more than 10
    bounds away from the device's f32 pair sums, for every kept pair."""
    name, t = "del9", [int(fx["timesteps"][0])]
    sums, _, pmax = world["ref"][name]
    rolled, _, _ = _reference(fx, name, world["net64"], roll=1, timesteps=t)
    m = _metric(fx, name, world["eng32"], dev)
    m.compute_membership_losses(t)
    got = m.pair_sums.cpu()[0, 0]
    bound = f32_bound(sums[0, 0].numpy(), CHW, pmax)
    shift = (rolled[0, 0] - got).abs().numpy()
    print(f"\nt = {t[0]}: smallest shift under a rolled image index {shift.min():.3g}, largest bound {bound.max():.3g}")
    assert (shift > 10 * bound).all()
    assert ((got - sums[0, 0]).abs().numpy() <= bound).all()            # (the right index is within it)


@pytest.mark.parametrize("name", ["del1", "del9"])
def test_bf16_engine_against_the_references_own_bf16_path(fx, dev, world, name):
    """Yardstick: the oracle network under torch.autocast(bfloat16) on this GPU (the reference's mixed_precision=bf16 path), its worst
    relative pair-sum deviation from the f64 reference = e_ref.  The HIP bf16 engine must stay within 2 * e_ref."""
    from siss_amd.scheduler import DDPMScheduler
    sums, _, _ = world["ref"][name]
    pool_all, pool_del, ia, idl, noise = _case(fx, name)
    sched, net = DDPMScheduler(), seeded_oracle(int(fx["net_seed"])).to(dev)
    I, J = int(fx["I"]), int(fx["J"])
    ref16 = torch.zeros_like(sums)
    with torch.no_grad():
        for ti, t in enumerate(fx["timesteps"].tolist()):
            for g, imgs in enumerate((pool_all[ia], pool_del[idl])):
                x0 = imgs.to(dev)[:, None].expand(-1, J, -1, -1, -1).reshape(I * J, *imgs.shape[1:])
                n = noise.to(dev)[None].expand(I, -1, -1, -1, -1).reshape(I * J, *imgs.shape[1:])
                tt = torch.full((I * J,), t, device=dev)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = net(sched.add_noise(x0, n, tt), tt, return_dict=False)[0]
                ref16[ti, g] = torch.sum((out - n) ** 2, dim=[1, 2, 3]).double().view(I, J).cpu()
    e_ref = float(((ref16 - sums).abs() / sums).max())
    m = _metric(fx, name, _engine(torch.bfloat16, world["sd"]), dev)
    m.compute_membership_losses(fx["timesteps"].tolist())
    e_hip = float(((m.pair_sums.cpu() - sums).abs() / sums).max())
    print(f"\n{name}: worst relative pair-sum deviation from the f64 reference: torch autocast(bf16) oracle e_ref = {e_ref:.3e}, "
          f"HIP bf16 engine {e_hip:.3e} (allowed {2 * e_ref:.3e})")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_graph_and_eager_give_the_same_bits(fx, dev, world, dtype):
    eng = world["eng32"] if dtype == torch.float32 else _engine(dtype, world["sd"])
    ts = fx["timesteps"].tolist()
    a = _metric(fx, "del1", eng, dev, use_graph=True)
    a.compute_membership_losses(ts)
    first = a.pair_sums.clone()
    a.compute_membership_losses(ts)                                   # the captured graph, replayed for a second evaluation
    b = _metric(fx, "del1", eng, dev, use_graph=False)
    b.compute_membership_losses(ts)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), a.pair_sums.view(torch.int64)), "two evaluations on one graph differ"
    assert torch.equal(a.pair_sums.view(torch.int64), b.pair_sums.view(torch.int64)), "graph and eager differ"


def test_grouping_and_dedupe_do_not_move_the_pair_sums(fx, dev, world):
    """pairs_per_forward 4 against 15 and dedupe on against off (one forget image): the same inputs in other batch slots, so the
    same sums within the f32 bound."""
    sums, _, pmax = world["ref"]["del1"]
    bound = f32_bound(sums.numpy(), CHW, pmax)
    ts = fx["timesteps"].tolist()
    got = {}
    for key, kw in (("b4", dict(pairs_per_forward=4)), ("b15", dict(pairs_per_forward=15)), ("b4-all", dict(pairs_per_forward=4, dedupe=False))):
        m = _metric(fx, "del1", world["eng32"], dev, **kw)
        m.compute_membership_losses(ts)
        got[key] = m.pair_sums.cpu()
        assert m.forwards == {"b4": 9, "b15": 3, "b4-all": 15}[key]
    for other in ("b15", "b4-all"):
        d = (got[other] - got["b4"]).abs().numpy()
        print(f"\nb4 vs {other}: worst difference {d.max():.3e} (bound {bound.min():.3e})")
        assert (d <= bound).all()
    assert torch.equal(got["b4"][:, 1], got["b4"][:, 1, :1].expand(-1, int(fx["I"]), -1))      # dedupe: one set of sums, shared


def test_one_launch_of_each_kernel_per_forward(fx, dev, world):
    from siss_amd import lib
    I, J, ts = int(fx["I"]), int(fx["J"]), fx["timesteps"].tolist()
    for kw, items in ((dict(dedupe=True), len(ts) * (I * J + J)), (dict(dedupe=False), len(ts) * 2 * I * J)):
        m = _metric(fx, "del1", world["eng32"], dev, use_graph=False, **kw)
        torch.cuda.synchronize()
        lib.PROF = []
        try:
            m.compute_membership_losses(ts)
            torch.cuda.synchronize()
            names = [r[0] for r in lib.PROF]
        finally:
            lib.PROF = None
        b = m.pairs_per_forward
        assert names.count("siss_pair_noise") == names.count("siss_pair_sqerr") == -(-items // b) == m.forwards, (kw, items)


# ---------------------------------------------------------------- 4. the training state is left alone
MNIST_SMALL = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=(64, 128),
                   down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), layers_per_block=1,
                   attention_head_dim=8, norm_num_groups=32, norm_eps=1e-5, downsample_padding=1, flip_sin_to_cos=True, freq_shift=0)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_an_evaluation_leaves_the_training_state_bitwise(dev):
    from siss_amd import lib
    from siss_amd.config import UNet2DConfig
    from siss_amd.membership import MembershipLoss
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.step import SISSStepper
    from siss_amd.unet import UNetEngine
    eng = UNetEngine(UNet2DConfig(**MNIST_SMALL), "cuda:0", dtype=torch.bfloat16)
    eng.init_random(seed=1)
    B = 2
    sched = DDPMScheduler()
    st = SISSStepper(eng, sched.alphas_cumprod, lr=1e-4, scaling_norm=5.0, train_batch_size=B, mixed_precision="bf16", inf_guard=True)
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (B, 1, 28, 28)
    for _ in range(2):                                   # two steps: AdamW moments, both gradient sets and a sparse-fill plan exist
        x0, a0, noise = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
        st.step(x0, a0, noise, torch.randint(0, 1000, (B,), device=dev, generator=g), torch.rand(B, device=dev, generator=g))
    torch.cuda.synchronize()
    lib.overwrite_log()
    ps = eng.ps
    snap = [ps.flat.clone(), ps.grads.clone(), ps.shadow.clone(), st.opt.m.clone(), st.opt.v.clone()]
    fill = (eng._fill_key, eng._fill_plan, dict(eng._fill_plans), eng.wgrad_overwrite)
    assert fill[2], "the steps recorded no sparse-fill plan"
    gi = torch.Generator().manual_seed(4)
    m = MembershipLoss(list(torch.rand(6, 1, 28, 28, generator=gi) * 2 - 1), [torch.rand(1, 28, 28, generator=gi) * 2 - 1], sched, eng, 3, 2, 4, dev)
    random.seed(0)
    m.sample_images()
    m.sample_noises(generator=torch.Generator(device=dev).manual_seed(1))
    for _ in range(2):                                   # the capture, then a replay
        losses = m.compute_membership_losses([200, 900])
        assert all(math.isfinite(float(v)) and float(v) > 0 for pair in losses for v in pair)
        torch.cuda.synchronize()
        for a, b in zip(snap, [ps.flat, ps.grads, ps.shadow, st.opt.m, st.opt.v]):
            assert torch.equal(_bits(a), _bits(b))
        assert (eng._fill_key, eng._fill_plan, eng.wgrad_overwrite) == (fill[0], fill[1], fill[3])
        assert eng._fill_plans.keys() == fill[2].keys() and all(eng._fill_plans[k] is v for k, v in fill[2].items())
        assert lib.overwrite_log() == []


def test_the_conditional_engine_is_refused_by_name(dev):
    from siss_amd.membership import MembershipLoss
    from siss_amd.scheduler import DDPMScheduler

    class UNetCondEngine:
        pass
    m = MembershipLoss([torch.zeros(1, 4, 4)], [torch.zeros(1, 4, 4)], DDPMScheduler(), UNetCondEngine(), 1, 1, 1, dev)
    m.sample_images()
    m.sample_noises()
    with pytest.raises(NotImplementedError, match="UNetCondEngine"):
        m.compute_membership_losses([5])


# ---------------------------------------------------------------- 5. the tasks
UNETS = {"delete_tshirt": dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
                               down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"],
                               layers_per_block=1),
         "delete_celeb": dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=[64, 128],
                              down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"],
                              layers_per_block=1, attention_head_dim=None, norm_eps=1e-6, downsample_padding=0, flip_sin_to_cos=False,
                              freq_shift=1)}
ML = ["+metrics.membership_loss.class_cfg._target_=metrics.class_membership.MembershipLoss",
      "+metrics.membership_loss.class_cfg.num_image_samples=3", "+metrics.membership_loss.class_cfg.num_noise_samples=2",
      "+metrics.membership_loss.class_cfg.eval_batch_size=4", "+metrics.membership_loss.timesteps=[200, 900]",
      "+metrics.membership_loss.step_frequency=1"]


def _run(config, tmp_path, name, extra, monkeypatch):
    """The task through its config, with every launcher name it calls recorded."""
    from siss_amd import hydra_lite as H
    from siss_amd import lib
    cfg = H.compose(config, os.path.join(ROOT, "config"),
                    ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "save_final=false",
                     "mixed_precision=bf16", "+dataloader_num_workers=1", *extra])
    cfg.unet = UNETS[config]
    called = set()
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda n, *a, **k: (called.add(n), real(n, *a, **k))[1])
    random.seed(5)
    try:
        stepper = H.instantiate(cfg.task, cfg=cfg, _recursive_=False).run()
    finally:
        monkeypatch.setattr(lib, "call", real)
    return stepper, cfg, called


@pytest.mark.parametrize("config", ["delete_tshirt", "delete_celeb"])
def test_task_logs_the_membership_loss_without_changing_the_training(dev, tmp_path, monkeypatch, config):
    plain, cfg0, called = _run(config, tmp_path, "plain", ["+metrics.membership_loss=null"], monkeypatch)
    want = plain.e.ps.flat.clone()
    assert not {"siss_pair_noise", "siss_pair_sqerr"} & called                          # the key null: neither launcher runs,
    assert not [f for f in os.listdir(cfg0.output_dir) if f.startswith("membership")]   # no membership file is written
    st, cfg, called = _run(config, tmp_path, "ml", ML, monkeypatch)
    assert {"siss_pair_noise", "siss_pair_sqerr"} <= called
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "membership_rank0.jsonl"))]
    assert [r["global_step"] for r in lines] == [0, 1, 2]
    for r in lines:
        assert r["seconds"] > 0
        for t in (200, 900):
            a, d, q = (r[f"{k}_t={t}"] for k in ("all_membership_loss", "deletion_membership_loss", "membership_ratio"))
            assert all(math.isfinite(v) and v > 0 for v in (a, d, q)) and q == d / a
    # (two plain runs of a task loop already differ in the last bits of some weights: the bound is 1e-6, as for the likelihood metric)
    assert float((st.e.ps.flat - want).abs().max()) <= 1e-6
    # plot_params: the curve is the whole run
    st, cfg, called = _run(config, tmp_path, "plot", [*ML, "+metrics.membership_loss.plot_params.time_frequency=250"], monkeypatch)
    curve = json.load(open(os.path.join(cfg.output_dir, "membership_curve_rank0.json")))
    assert curve["timesteps"] == [0, 250, 500, 750] and len(curve["all_membership_loss"]) == len(curve["deletion_membership_loss"]) == 4
    assert all(math.isfinite(v) and v > 0 for v in curve["all_membership_loss"] + curve["deletion_membership_loss"])
    assert not os.path.exists(os.path.join(cfg.output_dir, "membership_rank0.jsonl"))
    log = os.path.join(cfg.output_dir, "train_log_rank0.jsonl")
    assert (not os.path.exists(log) or not open(log).read().strip()) and not called & {"siss_mixture_fwd", "siss_recombine_clip_adamw"}

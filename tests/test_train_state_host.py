"""tests/train_state_ref.py against torch's own operators on the CPU, and the f32 restatement ALONE against every bound that
tests/test_hip_train_state.py applies to the kernels, on that test's seeded inputs; the checkpoint format, the epoch sampler, the
configs and the task's refusals.  No GPU."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import optimizer_ref as R
import train_state_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
U = R.U


# ------------------------------------------------------------------ the decay schedule
def test_decay_schedule():
    from siss_amd.ema import get_decay
    e = T.TSHIRT_EMA
    assert T.decay_f64(1, **e) == 0.0                                       # s = 0
    assert T.decay_f64(2, **e) == 1 - 2 ** -0.75
    k = T.first_capped_step(e)
    assert T.decay_f64(k - 1, **e) < 0.9999 and T.decay_f64(k, **e) == 0.9999 and T.decay_f64(10 * k, **e) == 0.9999
    assert k == 215444                                                      # (1 + s)^0.75 > 1e4 from s = 215443 on
    assert T.decay_f64(3, **dict(e, min_decay=0.9)) == 0.9                  # 1 - 3^-0.75 = 0.56 raised to min_decay
    assert T.decay_f64(1, **dict(e, min_decay=0.9)) == 0.0                  # ... but s = 0 returns 0 before any clamp
    assert T.decay_f64(5, **dict(e, update_after=4)) == 0.0 and T.decay_f64(6, **dict(e, update_after=4)) == 1 - 2 ** -0.75
    assert T.decay_f64(2, **dict(e, use_warmup=False)) == 2 / 11 and T.decay_f64(91, **dict(e, use_warmup=False)) == 0.91
    for k in (1, 2, 3, 31, 1000, 215443, 215444, 10 ** 6):                  # the package's own host statement is the same function
        for sch in (e, dict(e, use_warmup=False), dict(e, update_after=7, min_decay=0.5)):
            assert get_decay(k, sch["max_decay"], sch["min_decay"], sch["update_after"], sch["use_warmup"], sch["inv_gamma"],
                             sch["power"]) == T.decay_f64(k, **sch)


def test_f32_one_minus_decay_would_miss_the_bound_and_the_double_keeps_it():
    """at decay = 0.9999 an f32 `1.f - decay` is off by 6e-4 of the EMA's step; the block's value is one rounding of the double"""
    k = T.first_capped_step(T.TSHIRT_EMA)
    blk = T.scalars_f32(1.0, 1.0, 0.95, 0.999, 0, T.TSHIRT_EMA, k - 1)
    assert T.one_rounding_errors(blk, 0.95, 0.999, 1, T.TSHIRT_EMA, k)[2] <= 2.0
    naive = float(f32(1) - f32(0.9999))
    assert abs(naive - 1e-4) / 1e-4 > 1e-4


# ------------------------------------------------------------------ the restatement against torch
def torch_single(g, p0, m, v, ema0, k, hp, dtype, max_norm, omd):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) at step k + the EMA line, on tensors of `dtype`"""
    lr, b1, b2, eps, wd = R.wide(hp)
    p = torch.from_numpy(np.asarray(p0)).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": torch.from_numpy(np.asarray(m)).to(dtype).clone(),
                    "exp_avg_sq": torch.from_numpy(np.asarray(v)).to(dtype).clone()}
    p.grad = torch.from_numpy(np.asarray(g)).to(dtype).clone()
    pre = torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt.step()
    s = torch.from_numpy(np.asarray(ema0)).to(dtype).clone()
    s.sub_(omd * (s - p.detach()))
    st = opt.state[p]
    return (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), s.numpy()), float(pre)


def four_errors(got, ref, p0, ema0):
    e = R.update_errors(got[:3], ref[:3], p0)
    return e + (float(np.abs(np.asarray(got[3], f64) - ref[3]).max() / np.abs(ref[3] - np.asarray(ema0, f64)).max()),)


@pytest.mark.parametrize("name", ["mnist", "lr5e-3"])
@pytest.mark.parametrize("k", [1, 2, 3, 31, 1000])
def test_f64_reference_is_torch_and_the_restatement_keeps_4x_torch_f32(k, name):
    """f64 restatement == torch in f64 to 1e-12 of the update; then, against it: the f32 restatement within 4 x torch's own f32 error
    (the figure tests/test_optimizer_host.py uses for the two-set update), for p, m, v and the EMA (relative to the EMA's own move)."""
    hp = R.hyper(*R.HYPER[name])
    g, p0, m, v = R.precision_case(k, hp, zero_init=False)
    ema0 = (p0 + 0.01 * np.random.default_rng(k).standard_normal(len(p0))).astype(f32)
    ref, sc = T.update_f64(g, p0, m, v, ema0, k, hp, 1.0, T.TSHIRT_EMA, k)
    t64, pre = torch_single(g, p0, m, v, ema0, k, hp, torch.float64, 1.0, sc["one_minus_decay"])
    assert abs(pre - sc["grad_norm"]) <= 1e-12 * pre
    upd = np.abs(t64[0] - p0).max()
    assert np.abs(ref[0] - t64[0]).max() <= 1e-12 * max(upd, np.abs(p0).max() * 1e-3)
    assert np.abs(ref[3] - t64[3]).max() <= 1e-12 * np.abs(t64[3]).max()
    t32, _ = torch_single(g, p0, m, v, ema0, k, hp, torch.float32, 1.0, float(f32(sc["one_minus_decay"])))
    e_ref = four_errors(t32, ref, p0, ema0)
    blk = T.scalars_f32(T.norm_sum_f32(g), 1.0, hp[1], hp[2], k - 1, T.TSHIRT_EMA, k - 1)
    assert blk[T.NAMES["step"]] == k and blk[T.NAMES["ema_step"]] == k
    got = T.update_f32(g, p0, m, v, ema0, blk, hp)
    e = four_errors(got[:4], ref, p0, ema0)
    print(f"[train-state-host] {name} step {k}: error / torch f32's: " + ", ".join(f"{n} {a:.2e} / {b:.2e}" for n, a, b in zip("pmve", e, e_ref)))
    for i in range(4):
        assert e[i] <= 4 * e_ref[i] or e[i] == 0, (k, i, e, e_ref)


# ------------------------------------------------------------------ the restatement alone inside the GPU test's bounds
@pytest.mark.parametrize("n", T.SIZES)
def test_restatement_keeps_the_scalar_bounds(n):
    g = T.gauss(n, n)
    blk = T.scalars_f32(T.norm_sum_f32(g), 1.0, 0.95, 0.999, 0, T.TSHIRT_EMA, 0)
    worst = T.block_errors(blk, g, 1.0)
    print(f"[train-state-host] n {n}: error / allowed {worst}")
    assert max(worst.values()) <= 1.0, worst
    gi = T.ints(n, n)
    xx = int((gi.astype(np.int64) ** 2).sum())
    assert T.norm_sum_f32(gi) == float(xx)
    assert T.scalars_f32(float(xx), 1.0, 0.95, 0.999, 0, T.TSHIRT_EMA, 0)[0] == f32(math.sqrt(xx))


@pytest.mark.parametrize("k", T.STEPS + [T.first_capped_step(T.TSHIRT_EMA)])
def test_restatement_keeps_2u_on_the_one_rounding_fields(k):
    for b1, b2 in R.BETAS:
        blk = T.scalars_f32(1.0, 1.0, b1, b2, k - 1, T.TSHIRT_EMA, k - 1)
        errs = T.one_rounding_errors(blk, b1, b2, k, T.TSHIRT_EMA, k)
        assert max(errs) <= 2.0, (k, errs)


# ------------------------------------------------------------------ save_state / load_state
def host_model(seed):
    """UNet2DModel's checkpoint surface over a small ParamStore on the CPU (every layout kind), a stepper's optimizer state, an EMA"""
    from siss_amd.config import UNet2DConfig
    from siss_amd.ema import EMAModel
    from siss_amd.model import UNet2DModel
    from siss_amd.unet import ParamStore

    class HostUNet(UNet2DModel):
        def __init__(self):
            ps = ParamStore()
            ps.add("conv_in.weight", "conv_in", (8, 1, 3, 3)); ps.add("conv_in.bias", "vec", (8,))
            ps.add("block.conv1.weight", "conv3", (16, 8, 3, 3)); ps.add("block.shortcut.weight", "conv1", (16, 8, 1, 1))
            ps.add("time.linear.weight", "mat", (24, 10))
            ps.relayout(lambda name: name.startswith("time"))
            ps.allocate("cpu", f32=True)
            self.config = UNet2DConfig.mnist_tshirt()
            self.engine = types.SimpleNamespace(ps=ps, f32=True, state_dict=ps.state_dict, refresh_weights=lambda **kw: None,
                                                load_state_dict=lambda sd, strict=True: ps.load_state_dict(sd, strict))
            self._params = {n: torch.nn.Parameter(ps.p(n)) for n in ps.specs}

    g = torch.Generator().manual_seed(seed)
    unet = HostUNet()
    ps = unet.engine.ps
    unet.load_state_dict({n: torch.randn(sp.ref_shape, generator=g) for n, sp in ps.specs.items()})
    ema = EMAModel(unet, decay=0.9999, use_ema_warmup=True, inv_gamma=1.0, power=0.75, model_cls=UNet2DModel, model_config=unet.config)
    blk = torch.zeros(16)
    opt = types.SimpleNamespace(m=torch.zeros(ps.total), v=torch.zeros(ps.total), train_ema_step=0, _train_block=lambda: blk)
    for flat in (opt.m, opt.v, ema.flat):                       # values in every parameter's own stretch (the padding stays zero)
        for n, sp in ps.specs.items():
            flat[sp.off:sp.off + sp.numel] = ps.to_native(sp, torch.randn(sp.ref_shape, generator=g)).reshape(-1)
    blk.copy_(torch.randn(16, generator=g)); blk[5] = 7.0
    ema.optimization_step = 7
    return unet, ema, types.SimpleNamespace(opt=opt)


def bits(t):
    return t.contiguous().view(torch.int32)


def test_save_state_load_state_are_bitwise(tmp_path):
    from siss_amd.checkpoint import load_state, save_state
    unet, ema, st = host_model(1)
    gen = torch.Generator().manual_seed(11)
    torch.rand(3, generator=gen)
    torch.manual_seed(5)
    meta = dict(global_step=4, epoch=1, position=2, lr_position=4, generator=gen)
    path = save_state(str(tmp_path / "checkpoint-4"), unet, ema, st, meta)
    assert sorted(os.listdir(path)) == ["optimizer.safetensors", "state.json", "unet", "unet_ema"]
    cfg = json.load(open(os.path.join(path, "unet_ema", "config.json")))
    assert {k: cfg[k] for k in ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")} == \
        dict(decay=0.9999, min_decay=0.0, optimization_step=7, update_after_step=0, use_ema_warmup=True, inv_gamma=1.0, power=0.75)
    want_cpu, want_gen = torch.get_rng_state(), gen.get_state()
    torch.rand(5); torch.rand(5, generator=gen)
    unet2, ema2, st2 = host_model(2)
    gen2 = torch.Generator()
    state = load_state(path, unet2, ema2, st2, generator=gen2)
    assert (state["global_step"], state["epoch"], state["position"], state["lr_position"], state["format_version"]) == (4, 1, 2, 4, 1)
    for a, b in ((unet.engine.ps.flat, unet2.engine.ps.flat), (ema.flat, ema2.flat), (st.opt.m, st2.opt.m), (st.opt.v, st2.opt.v),
                 (st.opt._train_block(), st2.opt._train_block())):
        assert torch.equal(bits(a), bits(b))
    assert ema2.optimization_step == 7 and st2.opt.train_ema_step == 7
    assert torch.equal(torch.get_rng_state(), want_cpu) and torch.equal(gen2.get_state(), want_gen)
    # the EMA directory is a model directory: the config loader takes it (the seven keys skipped), a misspelt key is still refused
    from siss_amd.config import UNet2DConfig
    assert UNet2DConfig.from_json(os.path.join(path, "unet_ema", "config.json")) == unet.config
    with pytest.raises(ValueError, match="unknown key 'decayy'"):
        UNet2DConfig.from_dict(dict(cfg, decayy=0.5))
    with pytest.raises(ValueError, match="format"):
        json.dump(dict(state, format_version=99), open(os.path.join(path, "state.json"), "w"))
        load_state(path, unet2, ema2, st2)
    for fn in os.listdir(path):                                  # safetensors and JSON only
        assert not fn.endswith((".bin", ".pkl", ".pt"))


@pytest.mark.parametrize("limit,left", [(1, ["checkpoint-10"]), (2, ["checkpoint-8", "checkpoint-10"]),
                                        (None, ["checkpoint-2", "checkpoint-4", "checkpoint-6", "checkpoint-8", "checkpoint-10"])])
def test_rotation(tmp_path, limit, left):
    """before saving, at most limit - 1 remain, oldest first BY STEP NUMBER (checkpoint-10 is newer than checkpoint-8)"""
    from siss_amd.checkpoint import list_checkpoints, save_state
    unet, ema, st = host_model(3)
    (tmp_path / "not-a-checkpoint").mkdir()
    for step in (2, 4, 6, 8, 10):
        save_state(str(tmp_path / f"checkpoint-{step}"), unet, ema, st, dict(global_step=step, epoch=0, position=step, lr_position=step), limit=limit)
    assert list_checkpoints(str(tmp_path)) == left and (tmp_path / "not-a-checkpoint").is_dir()


def test_ema_model_takes_the_parameter_iterable_and_refuses_anything_else():
    from siss_amd.ema import EMAModel, flat_of
    unet, _, _ = host_model(4)
    flat = flat_of(unet.parameters())
    assert flat.data_ptr() == unet.engine.ps.flat.data_ptr() and flat.shape == unet.engine.ps.flat.shape
    ema = EMAModel(unet.parameters(), decay=0.99)
    assert torch.equal(ema.flat, unet.engine.ps.flat) and ema.flat.data_ptr() != flat.data_ptr()
    before = unet.engine.ps.flat.clone()
    ema.flat.add_(1.0)
    ema.store(unet.parameters()); ema.copy_to(unet.parameters())
    assert torch.equal(unet.engine.ps.flat, ema.flat)
    ema.restore(unet.parameters())
    assert torch.equal(unet.engine.ps.flat, before) and not torch.equal(before, ema.flat)
    with pytest.raises(ValueError, match="ONE flat f32 buffer"):
        EMAModel([torch.zeros(4), torch.zeros(4)])
    with pytest.raises(ValueError, match="ONE flat f32 buffer"):
        EMAModel(list(unet.parameters()) + list(unet.parameters())[:1])       # a view twice
    with pytest.raises(ValueError):
        EMAModel(list(unet.parameters())[:-1])
    sd = ema.state_dict()
    assert set(sd) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"}


# ------------------------------------------------------------------ the epoch sampler
def test_epoch_sampler():
    from siss_amd.data import EpochSampler
    s = EpochSampler(10, 4, seed=42, num_epochs=3)
    assert len(s) == 3
    run = list(s)
    assert [len(i) for _, _, i in run] == [4, 4, 2] * 3 and [(e, p) for e, p, _ in run] == [(e, p) for e in range(3) for p in range(3)]
    assert run == T.remaining(10, 4, 42, 3, 0, 0)
    e0, e1 = sum((i for e, _, i in run if e == 0), []), sum((i for e, _, i in run if e == 1), [])
    assert sorted(e0) == sorted(e1) == list(range(10)) and e0 != e1
    for k, (e, p, _) in enumerate(run):                       # resuming at every (epoch, position) yields the rest exactly
        assert list(EpochSampler(10, 4, seed=42, num_epochs=3, epoch=e, position=p)) == run[k:]
    assert list(EpochSampler(10, 4, seed=42, num_epochs=3, epoch=1, position=3)) == run[6:]      # the end of an epoch is the next one's start
    assert list(EpochSampler(10, 4, seed=43, num_epochs=1)) != run[:3]


# ------------------------------------------------------------------ configs, data, refusals
def test_configs_compose():
    import train_unconditional
    from siss_amd import hydra_lite as H
    from siss_amd.tasks import DeleteTShirt, TrainUnconditional
    c = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"))
    assert H.get_object(c.task._target_) is train_unconditional.TrainUnconditional is TrainUnconditional
    assert (c.lr_scheduler, c.lr_warmup_steps, c.checkpointing_steps, c.sampling_steps, c.num_epochs, c.eval_batch_size) == ("cosine", 500, 2500, 50, 250, 64)
    assert c.ema.to_dict() == dict(use_ema=True, ema_inv_gamma=1.0, ema_power=0.75, ema_max_decay=0.9999)
    assert c.subfolders.unet_ema == "unet_ema" and c.checkpoint_path is None and c.checkpoints_total_limit is None
    TrainUnconditional(c).check_supported()
    d = H.compose("delete_tshirt", os.path.join(ROOT, "config"))
    assert (d.lr_scheduler, d.lr_warmup_steps, d.ema.use_ema, d.checkpointing_steps) == ("constant", 0, False, None)
    assert d.get("sampling_steps") is None and d.get("eval_batch_size") is None and d.subfolders.unet == "unet_ema"
    DeleteTShirt(d).check_supported()


def test_hf_dataset_reads_a_directory_and_refuses_a_hub_id(tmp_path):
    from siss_amd import hydra_lite as H
    from siss_amd.tasks import TrainUnconditional
    rng = np.random.default_rng(0)
    img, lab = rng.integers(0, 256, (12, 28, 28), dtype=np.uint8), np.arange(12) % 11
    np.savez(tmp_path / "train.npz", image=img, label=lab)
    c = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [f"dataset.name={tmp_path}"])
    ds = TrainUnconditional(c).dataset((1, 28, 28))
    assert len(ds) == 12 and ds[3].shape == (1, 28, 28) and torch.equal(ds[3], (torch.from_numpy(img[3]).float() / 255 - 0.5)[None] / 0.5)
    node = dict(c.dataset.to_dict(), class_to_remove=10)
    assert len(H.instantiate(dict(node, filter="deletion"))) == 1 and len(H.instantiate(dict(node, filter="nondeletion"))) == 11
    with pytest.raises(ValueError, match="requires removal class"):
        H.instantiate(dict(c.dataset.to_dict(), filter="deletion"))
    with pytest.raises(ValueError, match="Invalid filter"):
        H.instantiate(dict(node, filter="some"))
    hub = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["dataset.name=claserken/mnist-with-tshirt"])
    with pytest.raises(FileNotFoundError, match="allow_synthetic"):
        TrainUnconditional(hub).dataset((1, 28, 28))
    syn = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["dataset.name=claserken/mnist-with-tshirt", "allow_synthetic=true", "+synthetic_images=10"])
    assert len(TrainUnconditional(syn).dataset((1, 28, 28))) == 10


@pytest.mark.parametrize("override,match", [("scheduler.prediction_type=sample", "prediction_type"), ("mixed_precision=fp16", "fp16"),
                                            ("enable_xformers_memory_efficient_attention=true", "xformers")])
def test_refusals_by_name(override, match):
    from siss_amd import hydra_lite as H
    from siss_amd.tasks import TrainUnconditional
    with pytest.raises(NotImplementedError, match=match):
        TrainUnconditional(H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [override])).check_supported()


def test_more_than_one_rank_is_refused(monkeypatch):
    from siss_amd import hydra_lite as H
    from siss_amd.tasks import TrainUnconditional
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        TrainUnconditional(H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"))).check_supported()

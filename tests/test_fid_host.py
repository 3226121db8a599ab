"""CPU tests of the FID metric (siss_amd/fid.py): the state dict and its strict loading against the restatement's modules
(tests/fid_ref.py), compute() / reset() on given statistics against the reference formula, the evaluator's refusals and its
real-statistics file, the config remap, every refusal of DeleteCeleb.check_metrics, and the network's wiring (packed layers, channel
offsets, padded strides, pools) with the launchers emulated by torch on the host."""
import os

import pytest
import torch

import fid_ref
import metric_net_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_has_the_checkpoint_keys_and_shapes():
    from siss_amd.fid import InceptionV3FID, convs
    want = fid_ref.checkpoint_state_dict(fid_ref.FIDInceptionV3())
    got = InceptionV3FID().state_dict()
    assert list(got) == list(want)                              # names AND order
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert all(v.dtype == torch.float32 for v in got.values())
    assert len(convs()) == 94 and len(got) == 94 * 5 + 2 and tuple(got["fc.weight"].shape) == (1008, 2048)


def test_load_state_dict_is_strict():
    from siss_amd.fid import InceptionV3FID
    net = InceptionV3FID()
    ref = fid_ref.make(3)
    assert net.load_state_dict(ref.state_dict()) is None        # torch's own state dict: num_batches_tracked passed over
    sd = net.state_dict()
    assert torch.equal(sd["Mixed_6c.branch7x7dbl_3.conv.weight"], ref.Mixed_6c.branch7x7dbl_3.conv.weight)
    assert torch.equal(sd["Mixed_7c.branch_pool.bn.running_var"], ref.Mixed_7c.branch_pool.bn.running_var)
    good = fid_ref.checkpoint_state_dict(ref)
    missing = {k: v for k, v in good.items() if k != "Mixed_5b.branch5x5_2.bn.running_mean"}
    with pytest.raises(RuntimeError, match="missing keys.*Mixed_5b.branch5x5_2.bn.running_mean"):
        net.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="missing keys.*fc.bias"):        # fc is loaded and checked although it is not run
        net.load_state_dict({k: v for k, v in good.items() if k != "fc.bias"})
    with pytest.raises(RuntimeError, match="unexpected keys.*AuxLogits"):
        net.load_state_dict({**good, "AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1)})
    with pytest.raises(RuntimeError, match="Mixed_6b.branch7x7_2.conv.weight has shape"):
        net.load_state_dict({**good, "Mixed_6b.branch7x7_2.conv.weight": torch.zeros(128, 128, 7, 1)})     # (1, 7) transposed
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.train()
    assert net.train(False) is net and net.eval() is net
    with pytest.raises(RuntimeError, match="cuda"):              # no CPU path
        net(torch.zeros(1, 3, 8, 8))


def _emulated_call(name, *a):
    """What the launchers compute, by torch's f64 operations on host tensors (the arguments as lib.call gets them): the shared
    convolution and max pool in tests/metric_net_emul.py, csrc/inception.hip's own here."""
    import torch.nn.functional as F
    if metric_net_emul.call(name, *a) == 0:
        return 0
    if name == "siss_inc_avgpool":
        x, y = a[:2]
        y.copy_(F.avg_pool2d(x.permute(0, 3, 1, 2).double(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1).float())
    elif name == "siss_inc_global_avg":
        x, y = a[:2]
        y.copy_(x.double().mean(dim=(1, 2)).float())
    else:
        raise KeyError(name)
    return 0


def test_network_wiring_with_emulated_launchers(monkeypatch):
    """siss_amd/fid.py's side of the network -- BN folding, weight packing over padded channel strides, which layer reads what and
    writes at which column, the pools, Mixed_7c's max pool -- against the f64 restatement, no GPU: the launchers are replaced by
    torch's f64 operations (f32 between layers).  The bound is 8 x the f32 restatement's own deviation from f64 (3.13e-7 of max
    |f64| on these two images, the figure tests/test_hip_fid.py records); measured 8.9e-8."""
    from siss_amd import fid, lib, metric_net
    monkeypatch.setattr(lib, "call", _emulated_call)
    net = fid_ref.make(0)
    imgs = torch.randint(0, 256, (2, 3, 64, 64), generator=torch.Generator().manual_seed(1)).float() / 255
    ref = fid_ref.features(net, imgs, torch.float64)
    m = fid.InceptionV3FID()
    m.load_state_dict(net.state_dict())
    m.device = torch.device("cuda")                              # packing is refused on a CPU model; the tensors below stay on the host
    monkeypatch.setattr(metric_net, "pack_conv", lambda w, b, s, p, d, _pack=metric_net.pack_conv: _pack(w, b, s, p, "cpu"))
    m._pack()
    m.device = torch.device("cpu")
    got = m.features(fid_ref.preprocess(imgs).permute(0, 2, 3, 1).contiguous()).double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"\nwiring with emulated launchers: {err:.2e} of max|f64|")
    assert got.shape == (2, 2048) and err <= 8 * 3.13e-7


def _given(D, n1, n2, seed):
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(n1, D, generator=g) * 0.5 + 1.0
    f2 = torch.randn(n2, D, generator=g) * 0.7 + 0.8
    return f1, f2


def _fill(fc, side, f):
    n, s, c = fid_ref.statistics(f)
    getattr(fc, side + "_features_sum").copy_(s)
    getattr(fc, side + "_features_cov_sum").copy_(c)
    setattr(fc, side + "_features_num_samples", n)


def test_compute_from_given_statistics_matches_the_reference_formula():
    from siss_amd.fid import FrechetInceptionDistance
    for D, n1, n2 in ((64, 200, 150), (32, 5, 7)):              # full rank, and fewer samples than dimensions (a singular product)
        f1, f2 = _given(D, n1, n2, D)
        fc = FrechetInceptionDistance(None, D, "cpu")
        _fill(fc, "real", f1)
        _fill(fc, "fake", f2)
        got, want = fc.compute(), fid_ref.fid_from_features(f1, f2)
        assert got.dtype == torch.float32 and got.dim() == 0
        assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)), (float(got), float(want))      # (one f32 rounding of the result)
    with pytest.raises(ValueError, match="multiple of 16"):
        FrechetInceptionDistance(None, 40, "cpu")


def test_compute_needs_two_samples_on_each_side_and_reset_keeps_the_real_side():
    from siss_amd.fid import FrechetInceptionDistance
    f1, f2 = _given(16, 9, 9, 0)
    fc = FrechetInceptionDistance(None, 16, "cpu")
    with pytest.raises(RuntimeError, match="More than one sample"):
        fc.compute()
    _fill(fc, "real", f1)
    with pytest.raises(RuntimeError, match="More than one sample"):
        fc.compute()
    _fill(fc, "fake", f2[:1])
    with pytest.raises(RuntimeError, match="More than one sample"):
        fc.compute()
    _fill(fc, "fake", f2)
    first = float(fc.compute())
    fc.reset()
    assert fc.fake_features_num_samples == 0 and not fc.fake_features_sum.any() and not fc.fake_features_cov_sum.any()
    assert fc.real_features_num_samples == 9 and torch.equal(fc.real_features_sum, f1.double().sum(0))
    assert torch.equal(fc.real_features_cov_sum, f1.double().t().mm(f1.double()))
    with pytest.raises(RuntimeError, match="More than one sample"):
        fc.compute()
    _fill(fc, "fake", f2)
    assert float(fc.compute()) == first
    with pytest.raises(RuntimeError, match="feature extractor"):
        fc.update(torch.zeros(2, 3, 8, 8), real=False)
    with pytest.raises(ValueError, match="features"):
        fc.update_features(torch.zeros(2, 8), real=False)


def test_evaluator_refusals_and_real_statistics_round_trip(tmp_path, capsys):
    from siss_amd.fid import DEFAULT_CKPT, FEATURES, FIDEvaluator
    assert DEFAULT_CKPT == "checkpoints/classifiers/pt_inception-2015-12-05-6726825d.pth"
    with pytest.raises(FileNotFoundError, match="allow_random_init"):
        FIDEvaluator(4, "cpu", inception_ckpt=str(tmp_path / "absent.pth"))
    with pytest.raises(ValueError, match="inception_batch_size"):
        FIDEvaluator(0, "cpu", allow_random_init=True)
    with pytest.raises(TypeError):                                # the additions are keyword-only
        FIDEvaluator(4, "cpu", None, None, True, str(tmp_path / "absent.pth"))
    path = tmp_path / "real_stats.npz"
    ev = FIDEvaluator(4, "cpu", inception_ckpt=str(tmp_path / "absent.pth"), allow_random_init=True, real_stats_path=str(path))
    assert "RANDOM-INIT" in capsys.readouterr().out               # as loud as the UNet stand-in
    assert (ev.batch_size, ev.remove_class, ev.classifier, ev.filter_fake) == (4, None, None, True)
    with pytest.raises(NotImplementedError, match="load_cifar"):
        ev.load_cifar()
    with pytest.raises(FileNotFoundError):                        # no statistics file yet and no image directory
        FIDEvaluator(4, "cpu", allow_random_init=True, data_path=str(tmp_path / "nodir"), real_stats_path=str(path)).load_celeb()
    # a checkpoint on disk is loaded strictly
    ref = fid_ref.make(5)
    torch.save(fid_ref.checkpoint_state_dict(ref), tmp_path / "inc.pth")
    ev2 = FIDEvaluator(4, "cpu", inception_ckpt=str(tmp_path / "inc.pth"))
    assert torch.equal(ev2.fid_computer.inception.state_dict()["Mixed_7a.branch3x3_2.conv.weight"], ref.Mixed_7a.branch3x3_2.conv.weight)
    torch.save({"fc.bias": torch.zeros(1008)}, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="missing keys"):
        FIDEvaluator(4, "cpu", inception_ckpt=str(tmp_path / "bad.pth"))
    # the real side written by one evaluator is what the next one starts from, bit for bit
    g = torch.Generator().manual_seed(1)
    f = torch.rand(5, FEATURES, generator=g)
    n, s, c = fid_ref.statistics(f)
    fc = ev.fid_computer
    fc.real_features_sum.copy_(s)
    fc.real_features_cov_sum.copy_(c)
    fc.real_features_num_samples = n
    ev.save_real_stats(path)
    ev3 = FIDEvaluator(4, "cpu", allow_random_init=True, data_path=str(tmp_path / "nodir"), real_stats_path=str(path))
    ev3.load_celeb()
    fc3 = ev3.fid_computer
    assert fc3.real_features_num_samples == 5 and torch.equal(fc3.real_features_sum, s) and torch.equal(fc3.real_features_cov_sum, c)
    assert fc3.fake_features_num_samples == 0
    import numpy as np
    with open(tmp_path / "short.npz", "wb") as fh:
        np.savez(fh, n=np.int64(3), sum=np.zeros(64), cov_sum=np.zeros((64, 64)))
    with pytest.raises(ValueError, match="real_stats_path"):
        FIDEvaluator(4, "cpu", allow_random_init=True, real_stats_path=str(tmp_path / "short.npz")).load_celeb()


def test_target_remap_instantiates_the_reference_class_cfg():
    from siss_amd import hydra_lite as H
    from siss_amd.fid import FIDEvaluator
    assert H.TARGET_REMAP["metrics.fid.FIDEvaluator"] == "siss_amd.fid.FIDEvaluator"
    node = H.Cfg({"_target_": "metrics.fid.FIDEvaluator", "inception_batch_size": 64, "allow_random_init": True})
    ev = H.instantiate(node, device="cpu")
    assert type(ev) is FIDEvaluator and ev.batch_size == 64 and ev.data_path == "data/examples/celeba_hq_256"


def _task(extra, tmp_path, drop=()):
    from siss_amd import hydra_lite as H
    data = tmp_path / "real"
    data.mkdir(exist_ok=True)
    base = {"class_cfg._target_": "metrics.fid.FIDEvaluator", "class_cfg.inception_batch_size": 8, "class_cfg.allow_random_init": "true",
            "class_cfg.data_path": str(data), "step_frequency": 5, "num_imgs_to_generate": 16, "batch_size": 4}
    over = [f"+metrics.fid.{k}={v}" for k, v in base.items() if k not in drop]
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), [*over, *extra])
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


def test_check_metrics_refuses_a_fid_block_that_cannot_run(tmp_path):
    _task([], tmp_path).check_metrics()                          # the block as the reference documents it (+ the stand-in weights)
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), ["+metrics.fid=null"])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.check_metrics()                                         # the key null, as the reference ships it: nothing to check
    assert task.deletion_metrics(None, None, None, "cpu") is None
    for bad, exc in (("+metrics.fid.step_frequency=0", ValueError), ("+metrics.fid.step_frequency=-5", ValueError),
                     ("+metrics.fid.step_frequency=null", ValueError), ("+metrics.fid.step_frequency=2.5", ValueError),
                     ("+metrics.fid.step_frequency=true", ValueError),
                     ("+metrics.fid.num_imgs_to_generate=1", ValueError), ("+metrics.fid.num_imgs_to_generate=0", ValueError),
                     ("+metrics.fid.num_imgs_to_generate=null", ValueError),
                     ("+metrics.fid.batch_size=0", ValueError), ("+metrics.fid.batch_size=-1", ValueError),
                     ("+metrics.fid.batch_size=null", ValueError),
                     ("unet.in_channels=1", ValueError),
                     ("+metrics.fid.class_cfg.allow_random_init=false", FileNotFoundError),
                     (f"+metrics.fid.class_cfg.inception_ckpt={tmp_path}/absent.pth", None),
                     (f"+metrics.fid.class_cfg.data_path={tmp_path}/nodir", FileNotFoundError)):
        if exc is None:                                          # a missing checkpoint is fine only while random init is asked for
            _task([bad], tmp_path).check_metrics()
            with pytest.raises(FileNotFoundError, match="metrics.fid"):
                _task([bad, "+metrics.fid.class_cfg.allow_random_init=false"], tmp_path).check_metrics()
            continue
        with pytest.raises(exc, match="metrics.fid"):
            _task([bad], tmp_path).check_metrics()
    with pytest.raises(ValueError, match="class_cfg"):
        _task([], tmp_path, drop=[k for k in ("class_cfg._target_", "class_cfg.inception_batch_size", "class_cfg.allow_random_init",
                                              "class_cfg.data_path")]).check_metrics()
    # an existing statistics file stands in for the image directory
    stats = tmp_path / "stats.npz"
    stats.write_bytes(b"")
    _task([f"+metrics.fid.class_cfg.data_path={tmp_path}/nodir", f"+metrics.fid.class_cfg.real_stats_path={stats}"], tmp_path).check_metrics()


def test_the_other_tasks_do_not_read_the_block(tmp_path):
    """delete_tshirt.py and delete_sd.py of the reference never read metrics.fid: the T-shirt and SD tasks stay as they were."""
    from siss_amd.tasks import DeleteCeleb, DeleteSD, DeleteTShirt
    assert "check_metrics" in vars(DeleteCeleb) and "deletion_metrics" in vars(DeleteCeleb)
    assert "deletion_metrics" not in vars(DeleteSD)
    assert DeleteTShirt.deletion_metrics is not DeleteCeleb.deletion_metrics

"""Host side of the SD SSCD copy-detection score (siss_amd/sscd.py, DeleteSD's opt-in metric): the parameter surface against the
restatement tests/sscd_ref.py, strict loading, the checkpoint loader on a TorchScript file / a state dict / the `embeddings.1.*`
spelling / a safetensors file, the network's wiring with the launchers emulated by torch, the tracker's records and the task's
refusals.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import metric_net_emul  # noqa: E402
import sscd_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def net():
    return R.make(0)


def test_restatement_is_scriptable_and_counts_its_parameters(net):
    assert sum(p.numel() for p in net.parameters()) == R.PARAMETERS == 23_508_032 + 1_049_088
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        a, b = net(x), torch.jit.script(net)(x)
    assert a.shape == (2, 512) and torch.equal(a, b)
    assert torch.allclose(a.norm(dim=1), torch.ones(2), atol=1e-6)
    assert R.embed(net, x, torch.float64).dtype == torch.float64 and next(net.parameters()).dtype == torch.float32


def test_keys_order_shapes_and_parameter_count(net):
    from siss_amd.sscd import SSCDModel
    ref = net.state_dict()
    m = SSCDModel()
    sd = m.state_dict()
    assert list(sd) == list(ref)                                  # torch's state-dict order, `backbone.` in front
    assert all(k.startswith("backbone.") for k in sd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ref.values()]
    assert {"backbone.conv1.weight", "backbone.layer3.5.bn2.running_var", "backbone.fc.weight", "backbone.layer1.0.downsample.1.bias",
            "backbone.layer4.2.conv3.weight"} <= set(sd)
    learned = [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert sum(sd[k].numel() for k in learned) == 24_557_120
    assert sum(sd[k].numel() for k in learned if ".fc." in k) == 1_049_088
    assert SSCDModel(dims=128).state_dict()["backbone.fc.weight"].shape == (128, 2048)
    # building the model leaves the global random stream where it was
    torch.manual_seed(5)
    a = torch.rand(3)
    torch.manual_seed(5)
    SSCDModel()
    assert torch.equal(torch.rand(3), a)


def test_strict_load_refusals_and_eval_only(net):
    from siss_amd.sscd import SSCDModel
    good = net.state_dict()
    m = SSCDModel()
    assert m.load_state_dict(good) is None
    assert all(torch.equal(v, good[k]) for k, v in m.state_dict().items())
    m.load_state_dict({k: v for k, v in good.items() if not k.endswith("num_batches_tracked")})      # the one key that may be missing
    with pytest.raises(RuntimeError, match=r"missing keys \['backbone.layer2.0.downsample.0.weight'\]"):
        m.load_state_dict({k: v for k, v in good.items() if k != "backbone.layer2.0.downsample.0.weight"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['backbone.layer1.3.conv1.weight'\]"):
        m.load_state_dict({**good, "backbone.layer1.3.conv1.weight": torch.zeros(64, 256, 1, 1)})
    with pytest.raises(RuntimeError, match="backbone.fc.weight has shape"):
        m.load_state_dict({**good, "backbone.fc.weight": torch.zeros(1000, 2048)})
    with pytest.raises(RuntimeError, match="backbone.layer1.0.conv2.weight has shape"):
        m.load_state_dict({**good, "backbone.layer1.0.conv2.weight": torch.zeros(64, 64, 1, 1)})
    with pytest.raises(NotImplementedError, match="eval mode"):
        m.train()
    assert m.train(False) is m and m.eval() is m
    with pytest.raises(RuntimeError, match="cuda"):                # no CPU path
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="cuda"):
        m.embed_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        m.embed_u8(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        m(torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError, match="positive"):
        SSCDModel(batch_size=0)


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_loader_on_torchscript_state_dict_alias_and_safetensors(net, tmp_path):
    from safetensors.torch import save_file
    from siss_amd.sscd import SSCDModel
    good = net.state_dict()
    want = SSCDModel()
    want.load_state_dict(good)
    want = want.state_dict()
    torch.jit.script(net).save(str(tmp_path / "sscd.torchscript.pt"))
    torch.save(good, str(tmp_path / "state.pt"))
    alias = {("embeddings.1." + k.rsplit(".", 1)[1] if k.startswith("backbone.fc.") else k): v for k, v in good.items()}
    assert "embeddings.1.weight" in alias and "backbone.fc.weight" not in alias
    torch.save(alias, str(tmp_path / "alias.pt"))
    save_file({k: v.contiguous() for k, v in good.items()}, str(tmp_path / "sscd.safetensors"))
    for name in ("sscd.torchscript.pt", "state.pt", "alias.pt", "sscd.safetensors"):
        m = SSCDModel.load(tmp_path / name)
        assert m.dims == 512 and not m.training and _same(m.state_dict(), want), name
    # dims follow the file
    torch.save(R.make(1, dims=64).state_dict(), str(tmp_path / "narrow.pt"))
    assert SSCDModel.load(tmp_path / "narrow.pt").dims == 64
    # a foreign key set: a ClassyVision-style trunk, named in the message with what is missing
    foreign = {"backbone._feature_blocks.conv1.weight" if k == "backbone.conv1.weight" else k: v for k, v in good.items()}
    torch.save(foreign, str(tmp_path / "foreign.pt"))
    with pytest.raises(RuntimeError) as e:
        SSCDModel.load(tmp_path / "foreign.pt")
    assert "missing keys ['backbone.conv1.weight']" in str(e.value) and "unexpected keys ['backbone._feature_blocks.conv1.weight']" in str(e.value)
    torch.save({**good, **{k: v for k, v in alias.items() if k.startswith("embeddings")}}, str(tmp_path / "twice.pt"))
    with pytest.raises(RuntimeError, match="twice"):
        SSCDModel.load(tmp_path / "twice.pt")
    (tmp_path / "junk.bin").write_bytes(b"not a checkpoint at all")
    with pytest.raises(RuntimeError, match="neither"):
        SSCDModel.load(tmp_path / "junk.bin")
    with pytest.raises(FileNotFoundError, match="not a file"):
        SSCDModel.load(tmp_path / "missing.pt")


def _emulated_call(name, *a):
    """What the launchers compute, by torch's f64 operations on host tensors (the arguments as lib.call gets them): the shared
    convolution and max pool in tests/metric_net_emul.py, csrc/sscd.hip's own here."""
    if metric_net_emul.call(name, *a) == 0:
        return 0
    if name == "siss_sscd_gem":
        x, y, N, HW, C, p, eps = a
        assert x.numel() == N * HW * C and tuple(y.shape) == (N, C)
        y.copy_(x.reshape(N, HW, C).clamp(min=eps).double().pow(p).mean(1).pow(1 / p).float())
    elif name == "siss_sscd_normalize_score":
        e, N, D, eps, r, out, score = a
        q = (e.double() / e.double().norm(dim=1, keepdim=True).clamp(min=eps)).float()
        out.copy_(q)
        if r is not None:
            score.copy_((q.double() @ r.double()).float())
    else:
        raise KeyError(name)
    return 0


def test_network_wiring_with_emulated_launchers(net, monkeypatch):
    """siss_amd/sscd.py's side of the network -- BN folding, packing, which layer reads what, where the stride and the shortcut sit,
    GeM, fc as a 1 x 1 convolution, the normalisation and the score -- against the f64 restatement, no GPU: the launchers are replaced
    by torch's f64 operations (f32 between layers).  Bound: 8 x the f32 restatement's own deviation from f64, measured here."""
    from siss_amd import lib, metric_net, sscd
    monkeypatch.setattr(lib, "call", _emulated_call)
    u8 = torch.randint(0, 256, (2, 40, 56, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    x = R.normalise(u8, R.IMAGENET_MEAN, R.IMAGENET_STD)
    ref = R.embed(net, x, torch.float64)
    e32 = float((R.embed(net, x, torch.float32) - ref).abs().max())
    m = sscd.SSCDModel(batch_size=1)                              # two chunks
    m.load_state_dict(net.state_dict())
    m.device = torch.device("cuda")                               # packing is refused on a CPU model; the tensors below stay on the host
    monkeypatch.setattr(metric_net, "pack_conv", lambda w, b, s, p, d, _pack=metric_net.pack_conv: _pack(w, b, s, p, "cpu"))
    m._pack()
    m.device = torch.device("cpu")
    unit = torch.nn.functional.normalize(torch.randn(512, generator=torch.Generator().manual_seed(2)), dim=0)
    got, scores, _ = m._run(x, None, None, None, unit)
    err = float((got.double() - ref).abs().max())
    print(f"\nwiring with emulated launchers: max|d| {err:.2e}, f32 restatement {e32:.2e}")
    assert got.shape == (2, 512) and err <= 8 * e32
    assert float((scores.double() - ref @ unit.double()).abs().max()) <= 2.0 ** -22
    # the controls are far away: the wiring test can tell them apart
    for ctl in (R.variant(net, stride_on_conv1=True), R.variant(net, gem=False), R.reset_bn(net)):
        assert float((R.embed(ctl, x) - got.double()).abs().max()) >= 100 * 8 * e32
    # a chunk whose largest tensor would reach 2^31 elements is refused before anything runs
    assert m.max_elements(1, 512, 512) == 256 * 256 * 64
    with pytest.raises(ValueError, match="2\\^31"):
        m._features(torch.empty(512, 3, 512, 512, device="meta"))


def test_tracker_records(tmp_path):
    from siss_amd.sscd import SSCDScore
    out = tmp_path / "metrics_rank0.jsonl"
    tr = SSCDScore(None, "mem.png", str(out), [0.5], [0.5])
    assert tr.mean == [0.5] * 3 and tr.std == [0.5] * 3
    vals = torch.tensor([0.25, -0.5, 1.0, 0.1], dtype=torch.float32)
    assert tr.record(0, vals, 3) == {"global_step": 3, "sscd_0": float(vals.double().mean())}
    tr.record(1, torch.tensor([1.0]), 3)
    tr.record(0, torch.tensor([float("nan"), 0.5]), 4)
    lines = [json.loads(l) for l in open(out)]
    assert lines == [{"global_step": 3, "sscd_0": float(vals.double().mean())}, {"global_step": 3, "sscd_1": 1.0},
                     {"global_step": 4, "sscd_0": None}]
    with pytest.raises(ValueError, match="one or three"):
        SSCDScore(None, "mem.png", str(out), [0.5, 0.5], [0.5])


NORMALIZE = ("{_target_: torchvision.transforms.Compose, transforms: [{_target_: torchvision.transforms.Normalize, "
             "mean: [0.485, 0.456, 0.406], std: [0.229, 0.224, 0.225]}]}")


def _cfg(tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    return H.compose("delete_sd", os.path.join(ROOT, "config"), [f"base_dir={tmp_path}", f"output_dir={tmp_path}/out", *overrides])


def test_check_sscd_refusals_fire_before_any_step(net, tmp_path, capsys):
    from PIL import Image
    from siss_amd.sscd import SSCDScore
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    (ckpt / "vae").mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "mem.png"))
    torch.save(net.state_dict(), str(tmp_path / "sscd.pt"))
    foreign = {"trunk." + k: v for k, v in net.state_dict().items()}
    torch.save(foreign, str(tmp_path / "foreign.pt"))
    base = [f"pretrained_model_name_or_path={ckpt}", f"data_files.mem_img_path={tmp_path}/mem.png"]
    model = f"metrics.sscd.model_path={tmp_path}/sscd.pt"

    def check(*ov):                                  # what run() does before it loads anything onto the device
        task = DeleteSD(_cfg(tmp_path, *ov))
        task.fill_cfg()
        task.check_supported()
        task.check_metrics()
        return task.sscd

    assert check(*base) is None                                                       # key null (the shipped default)
    assert _cfg(tmp_path, *base).metrics.sscd is None
    cfg = _cfg(tmp_path, *base)
    del cfg["metrics"]
    assert DeleteSD(cfg).check_sscd() is None                                         # no metrics block at all
    tr = check(*base, model, f"metrics.sscd.data_transforms={NORMALIZE}")
    assert isinstance(tr, SSCDScore) and tr.mean == [0.485, 0.456, 0.406] and tr.std == [0.229, 0.224, 0.225]
    assert tr.model.dims == 512 and tr.out_path == f"{tmp_path}/out/metrics_rank0.jsonl" and tr.mem_img_path == f"{tmp_path}/mem.png"
    tr = check(*base, model)                                                          # data_transforms absent: the identity
    assert tr.mean == [0.0] * 3 and tr.std == [1.0] * 3
    one = NORMALIZE.replace("[0.485, 0.456, 0.406]", "[0.5]").replace("[0.229, 0.224, 0.225]", "[0.25]")
    assert check(*base, model, f"metrics.sscd.data_transforms={one}").std == [0.25] * 3
    with pytest.raises(ValueError, match="model_path"):
        check(*base, "metrics.sscd=true")
    with pytest.raises(FileNotFoundError, match="model_path.*not a file"):
        check(*base, f"metrics.sscd.model_path={tmp_path}/missing.pt")
    with pytest.raises(RuntimeError, match="not a torchvision-layout SSCD ResNet-50.*missing keys"):
        check(*base, f"metrics.sscd.model_path={tmp_path}/foreign.pt")
    with pytest.raises(FileNotFoundError, match="vae"):
        check(f"pretrained_model_name_or_path={tmp_path}/nowhere", base[1], model)
    with pytest.raises(FileNotFoundError, match="mem_img_path"):
        check(base[0], model)                                                         # the placeholder left null
    with pytest.raises(FileNotFoundError, match="mem_img_path"):
        check(base[0], f"data_files.mem_img_path={tmp_path}/gone.png", model)
    two = NORMALIZE.replace("[0.485, 0.456, 0.406]", "[0.5, 0.5]")
    with pytest.raises(ValueError, match="one or three"):
        check(*base, model, f"metrics.sscd.data_transforms={two}")
    tot = NORMALIZE.replace("transforms: [", "transforms: [{_target_: torchvision.transforms.ToTensor}, ")
    with pytest.raises(ValueError, match="exactly one Normalize"):
        check(*base, model, f"metrics.sscd.data_transforms={tot}")
    with pytest.raises(ValueError, match="exactly one Normalize"):
        check(*base, model, "metrics.sscd.data_transforms={_target_: torchvision.transforms.Normalize, mean: [0.5], std: [0.5]}")
    # mem_img_path comes from clustering_info.json when deletion.frac_deletion is null (fill_cfg runs first)
    os.makedirs(tmp_path / "images")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "images" / "sylvester_stallone_007.png"))
    json.dump({"frac_deletion": 0.375, "mem_idx": 7}, open(tmp_path / "clustering_info.json", "w"))
    assert check(base[0], model).mem_img_path.endswith("images/sylvester_stallone_007.png")
    # a missing checkpoint with allow_random_init: a random-init network, loudly
    capsys.readouterr()
    tr = check(*base, f"metrics.sscd.model_path={tmp_path}/missing.pt", "allow_random_init=true")
    assert isinstance(tr, SSCDScore) and "RANDOM-INIT" in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "out" / "train_log_rank0.jsonl")


def test_new_entry_points_are_declared_and_bound():
    from siss_amd import lib
    from siss_amd.build import EXACT
    for n in ("siss_sscd_preprocess", "siss_sscd_gem", "siss_sscd_normalize_score"):
        assert n in lib.SIGNATURES and lib.PARAMS[n][-1] == "stream" and n in lib.F32_SAME, n
    assert "sscd.hip" in EXACT                                    # no contraction into an fma: the preprocessing is a bitwise claim
    assert lib.PARAMS["siss_sscd_preprocess"][:5] == ("src", "form", "n", "h", "w")

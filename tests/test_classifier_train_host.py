"""CPU tests of the classifier trainer's host side: the restatements of tests/classifier_train_ref.py (the oracle of
tests/test_hip_classifier_train.py) against f64 autograd on the cases the GPU tests use, the layout of the trainer's flat buffers
against ResNet18Ref's state dict, and tools/train_classifier.py's arguments, dataset filtering and its one refusal."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_train_ref as T
from classifier_ref import ResNet18Ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _tool():
    spec = importlib.util.spec_from_file_location("train_classifier_tool", os.path.join(ROOT, "tools", "train_classifier.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", T.CONV_CASES + [T.STEM_CASE, T.SPLIT_CASE], ids=lambda c: c[0])
def test_gather_forms_agree_with_autograd(case):
    _, cin, cout, k, s, p, N, H, W = case
    x, w, dy = T.conv_inputs(case)
    dx, dw = T.autograd_conv(x, w, dy, s, p)
    got_dx, got_dw = T.dgrad_gather(dy, w, H, W, s, p), T.wgrad_gather(x, dy, k, s, p)
    # f64 against f64 in another summation order: 2^-53 K sum |a b|, with the bound's own sums
    bx = T.dgrad_gather(dy.abs(), w.abs(), H, W, s, p) * (k * k * cout + 4) * 2.0 ** -53
    bw = T.wgrad_gather(x.abs(), dy.abs(), k, s, p) * (dy.numel() // cout + 4) * 2.0 ** -53
    assert bool(((got_dx - dx).abs() <= bx).all()), float((got_dx - dx).abs().max())
    assert bool(((got_dw - dw).abs() <= bw).all()), float((got_dw - dw).abs().max())
    assert float(dx.abs().max()) > 0 and float(dw.abs().max()) > 0


def test_centre_tap_and_padding_cases_are_what_they_claim():
    """512 -> 512 on a 1 x 1 map: only the centre tap has a non-zero weight gradient; 2 x 2 -> 1 x 1 at stride 2: the taps of the
    first row and column fall in the padding."""
    x, w, dy = T.conv_inputs(T.CONV_CASES[4])
    dw = T.wgrad_gather(x, dy, 3, 1, 1)
    mask = torch.zeros(3, 3, dtype=torch.bool)
    mask[1, 1] = True
    assert bool((dw[:, :, ~mask] == 0).all()) and bool((dw[:, :, 1, 1] != 0).any())
    x, w, dy = T.conv_inputs(T.CONV_CASES[3])
    dw = T.wgrad_gather(x, dy, 3, 2, 1)
    assert bool((dw[:, :, 0, :] == 0).all()) and bool((dw[:, :, :, 0] == 0).all()) and bool((dw[:, :, 1:, 1:] != 0).any())


@pytest.mark.parametrize("shape", T.BN_COUNTS, ids=str)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_backward_restatement_agrees_with_autograd(shape, res, relu):
    N, H, W = shape
    g = torch.Generator().manual_seed(N * H)
    x, dy, r = (torch.randn(N, 64, H, W, generator=g, dtype=F64) for _ in range(3))
    gamma, beta = torch.rand(64, generator=g, dtype=F64) + 0.5, torch.randn(64, generator=g, dtype=F64)
    y, dx, dgamma, dbeta, dres = T.autograd_bn(x, gamma, beta, r if res else None, relu, dy, F64)
    y2, _, _ = T.bn_forward(x, gamma, beta)
    y2 = y2 + r if res else y2
    y2 = torch.relu(y2) if relu else y2
    torch.testing.assert_close(y2, y, rtol=1e-10, atol=1e-10)
    got = T.bn_backward(dy, y if relu else None, x, gamma)
    # (count 2: xhat = +-1 / sqrt(1 + 4 eps / d^2) and dx is a small difference of O(1) terms, hence the absolute term)
    for a, b in zip(got[:3], (dx, dgamma, dbeta)):
        torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-9)
    if res:
        torch.testing.assert_close(got[3], dres, rtol=0, atol=0)


def test_pool_tie_rule_is_autograd_s_bit_for_bit():
    x, dy = T.pool_inputs()
    for dtype in (torch.float32, F64):
        xx = x.to(dtype).clone().requires_grad_(True)
        F.max_pool2d(xx, 3, 2, 1).backward(dy.to(dtype))
        got = T.maxpool_backward(x.to(dtype), dy.to(dtype))
        assert torch.equal(got, xx.grad)
    # ties occur and the zero block is hit: a rule that took the LAST maximum would differ
    win = F.unfold(x, 3, 1, 1, 2).view(2, 64, 9, -1)
    assert int(((win == win.max(dim=2, keepdim=True).values).sum(dim=2) > 1).sum()) > 100


def test_state_dict_layout_matches_the_reference_network():
    from siss_amd.classifier import ResNet18, _convs
    from siss_amd import classifier_train as ct
    ref = ResNet18Ref().state_dict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        sd = ResNet18(10, True).state_dict()
    assert list(sd) == list(ref) and [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ref.values()]
    # the packed sizes the trainer lays its flat buffer out with
    for name, cin, cout, k, s, p, bn in _convs(1):
        assert ct.packed_kp(cin, k) % 32 == 0 and ct.packed_kp(cin, k) >= k * k * cin
    assert ct.packed_kp(1, 7) == 64 and ct.packed_kp(64, 3) == 576 and ct.packed_kp(512, 1) == 512
    assert ct.wgrad_splits(1024, 64, 576) == 8 and ct.wgrad_splits(98, 64, 576) == 1 and ct.wgrad_splits(3, 512, 2304) == 1
    with pytest.raises(RuntimeError, match="cuda device"):
        ct.ResNet18Trainer(device="cpu")


def test_tool_arguments_and_defaults():
    tool = _tool()
    a = tool.parse_args(["--data", "d", "--out", "o.pt"])
    assert (a.split, a.test_split, a.remove_class, a.epochs, a.batch_size, a.lr, a.seed, a.allow_synthetic) == \
        ("train", "test", 10, 10, 128, 1e-3, 1, False)
    a = tool.parse_args(["--allow-synthetic", "--out", "o.pt", "--remove-class", "none", "--epochs", "2", "--batch-size", "64"])
    assert a.remove_class is None and a.epochs == 2 and a.batch_size == 64 and a.synthetic_images == 640
    for bad in (["--out", "o.pt"], ["--data", "d"], ["--data", "d", "--out", "o", "--batch-size", "1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_tool_filters_the_removed_class_and_refuses_a_missing_split(tmp_path):
    tool = _tool()
    rng = np.random.default_rng(0)
    labels = np.arange(44) % 11
    np.savez(tmp_path / "train.npz", image=rng.integers(0, 256, (44, 28, 28), dtype=np.uint8), label=labels)
    a = tool.parse_args(["--data", str(tmp_path), "--out", str(tmp_path / "o.pt")])
    ds = tool.load_split(a, "train")
    assert len(ds) == 40 and 10 not in set(ds.labels.tolist())
    a.remove_class = None
    assert len(tool.load_split(a, "train")) == 44
    a.remove_class = 3
    assert 3 not in set(tool.load_split(a, "train").labels.tolist())
    x, y = tool.batch_of(ds, [0, 5, 7])
    from siss_amd.data import ToTensor
    assert x.shape == (3, 1, 28, 28) and y.dtype == torch.int64 and torch.equal(x, torch.stack([ToTensor()(ds.images[i]) for i in (0, 5, 7)]))
    with pytest.raises(FileNotFoundError):
        tool.main(["--data", str(tmp_path), "--split", "absent", "--out", str(tmp_path / "o.pt")])
    assert not os.path.exists(tmp_path / "o.pt")
    s1, s2 = tool.Synthetic(640, 1, "train"), tool.Synthetic(640, 1, "train")
    assert len(s1) == 640 and np.array_equal(s1.images, s2.images) and not np.array_equal(s1.images, tool.Synthetic(640, 1, "test").images)

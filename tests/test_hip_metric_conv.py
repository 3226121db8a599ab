"""The convolution and the 3 x 3 max pool that the four metric networks share (csrc/metric_conv.hip behind siss_amd/metric_net.py),
called directly: the convolution against F.conv2d in f64 at every corner the networks reach -- Inception's (padded channel strides,
1 x 7 / 7 x 1 taps, channel slices), the ResNets' (the NCHW image, the residual through split-K, the strided shortcut without ReLU,
fc as a 1 x 1 convolution on a 1 x 1 map) -- the launcher's refusals, and the max pool bitwise against F.max_pool2d."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CONV_BOUND = 1e-4       # max |d| <= CONV_BOUND * max |ref| (the bound tests/test_hip_classifier.py holds the same arithmetic to)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


# ---------------------------------------------------------------- convolution
def _conv_case(dev, seed, N, H, W, cin, cout, k, stride, pad):
    from siss_amd import metric_net as mn
    g = torch.Generator().manual_seed(seed)
    kh, kw = mn.pair(k)
    w = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
    b = torch.randn(cout, generator=g) * 0.3
    x = torch.randn(N, cin, H, W, generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=mn.pair(pad)))
    L = mn.pack_conv(w, b, stride, pad, dev)
    return mn, L, x.permute(0, 2, 3, 1).contiguous().to(dev), ref


CONV_CASES = {
    # (N, H, W, Cin, Cout, k, stride, pad, whether the call splits K)
    "stem 3->32 k3 s2 at 299": (1, 299, 299, 3, 32, 3, 2, 0, False),
    "80->192 k3 at 9 (Cin off the K step)": (2, 9, 9, 80, 192, 3, 1, 0, True),
    "64->48 k1 at 7 (Cout off the tile)": (2, 7, 7, 64, 48, 1, 1, 0, False),
    "128->128 (1,7) p(0,3) at 17": (1, 17, 17, 128, 128, (1, 7), 1, (0, 3), True),
    "128->128 (7,1) p(3,0) at 17": (1, 17, 17, 128, 128, (7, 1), 1, (3, 0), True),
    "288->384 k3 s2 at 35 (odd map, no padding)": (1, 35, 35, 288, 384, 3, 2, 0, True),
    "448->384 k3 p1 at 8 (split-K)": (2, 8, 8, 448, 384, 3, 1, 1, True),
}


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_convolution_against_conv2d_in_f64(dev, case):
    N, H, W, cin, cout, k, stride, pad, split = CONV_CASES[case]
    mn, L, x, ref = _conv_case(dev, len(case), N, H, W, cin, cout, k, stride, pad)
    y = mn.conv(L, x)
    got = y[..., :cout].permute(0, 3, 1, 2).cpu().double()
    assert got.shape == ref.shape
    scale, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"\n{case}: max|d| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}")
    assert float((ref == 0).double().mean()) > 0.1 and scale > 0.5          # the ReLU cuts, and not everything
    assert err <= CONV_BOUND * scale
    if y.shape[3] != cout:                                       # a padded channel stride: zero beyond Cout
        assert not y[..., cout:].any()
    assert (mn.conv_splits(N * ref.shape[2] * ref.shape[3], cout, L["Kp"]) > 1) == split
    assert torch.equal(y, mn.conv(L, x))                # the same call, the same bits


@pytest.mark.parametrize("N, H, cin, k, pad", [(2, 7, 48, 5, 2), (2, 35, 192, 1, 0)])
def test_convolution_into_a_channel_slice_leaves_the_neighbours_alone(dev, N, H, cin, k, pad):
    """A branch written at column offset 64 of a 288-wide buffer (the 5 x 5 branch of Mixed_5d): once through split-K, once not."""
    mn, L, x, ref = _conv_case(dev, H, N, H, H, cin, 64, k, 1, pad)
    assert (mn.conv_splits(N * H * H, 64, L["Kp"]) > 1) == (H == 7)
    buf = torch.randn(N, H, H, 288, generator=torch.Generator().manual_seed(9)).to(dev)
    before = buf.clone()
    assert mn.conv(L, x, out=buf, col=64) is buf
    assert torch.equal(buf[..., :64], before[..., :64]) and torch.equal(buf[..., 128:], before[..., 128:])
    got = buf[..., 64:128].permute(0, 3, 1, 2).cpu().double()
    assert float((got - ref).abs().max()) <= CONV_BOUND * float(ref.abs().max())
    with pytest.raises(ValueError, match="column"):
        mn.conv(L, x, out=buf, col=256)                           # 256 + 64 > 288: refused on the host
    from siss_amd import lib
    with pytest.raises(RuntimeError, match="bad argument"):      # and by the launcher
        lib.call("siss_metric_conv", x.contiguous() if cin % 32 == 0 else F.pad(x, (0, 16)), 0, L["w"], L["b"], None, buf, None, 0,
                 N, H, H, L["cin_p"], H, H, 64, k, k, 1, pad, pad, L["Kp"], 288, 256, 1, 1)
    assert torch.equal(buf[..., 128:], before[..., 128:])


# ---------------------------------------------------------------- the ResNets' forms
RESNET_CASES = {
    # (N, Cin, H, W, Cout, k, stride, pad, ReLU, residual, NCHW image, the split-K factor)
    "NCHW stem 1->64 k7 s2 p3 at 28 (K 49 padded to 64)": (2, 1, 28, 28, 64, 7, 2, 3, True, False, True, 1),
    "NCHW stem 3->64 k7 s2 p3 at 17x23 (odd, non-square)": (1, 3, 17, 23, 64, 7, 2, 3, True, False, True, 1),
    "64->64 k3 p1 at 7, residual + ReLU through split-K (M 98)": (2, 64, 7, 7, 64, 3, 1, 1, True, True, False, 4),
    "64->128 k1 s2 at 8, the shortcut: no ReLU": (2, 64, 8, 8, 128, 1, 2, 0, False, False, False, 1),
    "fc 512->10 on a 1x1 map, no ReLU (M 3, Cout 10)": (3, 512, 1, 1, 10, 1, 1, 0, False, False, False, 4),
}


@pytest.mark.parametrize("case", list(RESNET_CASES))
def test_resnet_forms_against_conv2d_in_f64(dev, case):
    from siss_amd import metric_net as mn
    N, cin, H, W, cout, k, stride, pad, relu, residual, nchw, splits = RESNET_CASES[case]
    g = torch.Generator().manual_seed(len(case))
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.3
    x = torch.randn(N, cin, H, W, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    res = torch.randn(ref.shape, generator=g) if residual else None
    if residual:
        ref = ref + res.double()
    if relu:
        ref = F.relu(ref)
    L = mn.pack_conv(w, b, stride, pad, dev)
    assert mn.conv_splits(N * ref.shape[2] * ref.shape[3], cout, L["Kp"]) == splits
    xd = (x if nchw else x.permute(0, 2, 3, 1)).contiguous().to(dev)
    rd = res.permute(0, 2, 3, 1).contiguous().to(dev) if residual else None
    if (H, W) == (1, 1):
        run = lambda: mn.linear(L, xd.view(N, cin)).view(N, 1, 1, cout)              # the form fc and the projections take
    else:
        run = lambda: mn.conv(L, xd, relu=relu, res=rd, nchw_in=nchw)
    y = run()
    assert tuple(y.shape) == (N, ref.shape[2], ref.shape[3], cout)
    got = y.permute(0, 3, 1, 2).cpu().double()
    scale, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"\n{case}: max|d| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}")
    assert scale > 0.5
    if relu:
        assert float((ref == 0).double().mean()) > 0.1              # the ReLU cuts, and not everything
    else:
        assert float((ref < 0).double().mean()) > 0.1 and bool((got < 0).any())      # negative outputs survive
    assert err <= CONV_BOUND * scale
    assert torch.equal(y, run())                                     # the same call, the same bits


def test_launcher_refuses_a_residual_into_a_slice_and_a_wide_nchw_input(dev):
    """Both are refused before any launch: the buffers stay as they were."""
    from siss_amd import lib, metric_net as mn
    g = torch.Generator().manual_seed(11)
    N, H, C = 2, 7, 64
    L = mn.pack_conv(torch.randn(C, C, 3, 3, generator=g), torch.randn(C, generator=g), 1, 1, dev)
    x = torch.randn(N, H, H, C, generator=g).to(dev)
    res = torch.randn(N, H, H, C, generator=g).to(dev)
    buf = torch.randn(N, H, H, 2 * C, generator=g).to(dev)
    before = buf.clone()
    ws = torch.empty(4 * N * H * H * C, device=dev)
    args = (N, H, H, C, H, H, C, 3, 3, 1, 1, 1, L["Kp"])
    with pytest.raises(RuntimeError, match="bad argument"):          # res with coff != 0 (and ldy != Cout)
        lib.call("siss_metric_conv", x, 0, L["w"], L["b"], res, buf, ws, ws.numel(), *args, 2 * C, C, 1, 4)
    assert torch.equal(buf, before)
    lib.call("siss_metric_conv", x, 0, L["w"], L["b"], None, buf, ws, ws.numel(), *args, 2 * C, C, 1, 4)      # without res: taken
    assert torch.equal(buf[..., :C], before[..., :C]) and not torch.equal(buf[..., C:], before[..., C:])
    L = mn.pack_conv(torch.randn(C, 32, 1, 1, generator=g), torch.randn(C, generator=g), 1, 0, dev)
    x = torch.randn(N, 32, H, H, generator=g).to(dev)
    y = torch.randn(N, H, H, C, generator=g).to(dev)
    before = y.clone()
    with pytest.raises(RuntimeError, match="bad argument"):          # nchw_in with Cin = 32
        lib.call("siss_metric_conv", x, 1, L["w"], L["b"], None, y, None, 0, N, H, H, 32, H, H, C, 1, 1, 1, 0, 0, L["Kp"], C, 0, 1, 1)
    assert torch.equal(y, before)


# ---------------------------------------------------------------- max pool
def _nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw(y):
    return y.permute(0, 3, 1, 2).cpu()


def test_max_pool_against_torch(dev):
    from siss_amd import metric_net as mn
    g = torch.Generator().manual_seed(4)
    # max pools match bitwise; all-negative maps: a padded position, were it ever chosen, would win with its zero
    for N, C, H, stride, pad in ((2, 64, 7, 2, 0), (1, 288, 35, 2, 0), (2, 2048, 8, 1, 1)):
        x = -torch.rand(N, C, H, H, generator=g) - 0.5
        x[:, ::3] = torch.randn(N, len(range(0, C, 3)), H, H, generator=g)
        ref = F.max_pool2d(x, 3, stride, pad)
        assert ref.shape[2] == {7: 3, 35: 17, 8: 8}[H]
        assert torch.equal(_nchw(mn.max_pool3(_nhwc(x, dev), stride, pad)), ref)
        # into a channel slice of a wider buffer: the neighbours stay
        buf = torch.randn(N, ref.shape[2], ref.shape[3], C + 40, generator=g).to(dev)
        before = buf.clone()
        mn.max_pool3(_nhwc(x, dev), stride, pad, buf, 8)
        assert torch.equal(_nchw(buf[..., 8:8 + C]), ref)
        assert torch.equal(buf[..., :8], before[..., :8]) and torch.equal(buf[..., 8 + C:], before[..., 8 + C:])
    # the ResNets' nn.MaxPool2d(3, 2, 1) on an odd, non-square map: the padded border is never chosen
    x = -torch.rand(2, 64, 7, 9, generator=g) - 0.5
    x[:, ::3] = torch.randn(2, 22, 7, 9, generator=g)
    ref = F.max_pool2d(x, 3, 2, 1)
    assert tuple(ref.shape) == (2, 64, 4, 5)
    assert torch.equal(_nchw(mn.max_pool3(_nhwc(x, dev), 2, 1)), ref)

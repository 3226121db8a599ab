"""Plain-torch CPU restatement of what metrics/fid.py of the reference computes (torchmetrics 1.3.1 FrechetInceptionDistance(feature=2048,
normalize=True) over torch-fidelity 0.3.0's FeatureExtractorInceptionV3), written from their description and independently of
siss_amd/fid.py: nn.Conv2d / nn.BatchNorm2d modules under the checkpoint's key names, the TF1 bilinear resize from its formula, the
statistics and the Frechet distance in f64.  A helper for tests/test_fid_host.py and tests/test_hip_fid.py, not a test."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        d = self.branch7x7dbl_1(x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            d = m(d)
        return torch.cat([self.branch1x1(x), self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x))), d, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool                    # "avg" (Mixed_7b) or "max" (Mixed_7c: the FID variant)
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        a = self.branch3x3_1(x)
        d = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        p = _avg(x) if self.pool == "avg" else F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(a), self.branch3x3_2b(a), self.branch3x3dbl_3a(d),
                          self.branch3x3dbl_3b(d), self.branch_pool(p)], 1)


class FIDInceptionV3(nn.Module):
    """[N, 3, 299, 299] in [-1, 1) -> [N, 2048]."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, "avg")
        self.Mixed_7c = InceptionE(2048, "max")
        self.fc = nn.Linear(2048, 1008)

    def forward(self, x):
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
                     "Mixed_7b", "Mixed_7c"):
            x = getattr(self, name)(x)
        return x.mean(dim=(2, 3))


def checkpoint_state_dict(net):
    """The state dict as the checkpoint has it: without the BatchNorms' num_batches_tracked."""
    return {k: v.detach().clone() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}


def make(seed):
    """A network in eval mode with He-normal convolutions and randomised BatchNorm statistics (gamma, var in [0.8, 1.25], beta, mean
    ~ 0.1 N(0, 1)): activations stay O(1) through all 94 convolutions."""
    g = torch.Generator().manual_seed(seed)
    net = FIDInceptionV3()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.8 + 0.45 * torch.rand(c, generator=g))
                m.running_var.copy_(0.8 + 0.45 * torch.rand(c, generator=g))
                m.bias.copy_(0.1 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(c, generator=g))
    return net.eval()


def reset_bn(net):
    """(negative control) the running statistics back to mean 0 / var 1."""
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.reset_running_stats()
    return net


def resize_tf1(x, size=299):
    """Bilinear resize of [N, C, H, W] f32 the TF1 way (no half-pixel centres): src = dst * in / out, i0 = floor(src),
    i1 = min(i0 + 1, in - 1), top = tl + (tr - tl) fx, bottom likewise, out = top + (bottom - top) fy."""
    def axis(n_in):
        scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(size), dtype=torch.float32)
        src = torch.arange(size, dtype=torch.float32, device=x.device) * scale.to(x.device)
        i0f = src.floor()
        i0 = i0f.long().clamp(max=n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0f
    y0, y1, fy = axis(x.shape[2])
    x0, x1, fx = axis(x.shape[3])
    fy, fx = fy.view(1, 1, -1, 1), fx.view(1, 1, 1, -1)
    rows0, rows1 = x[:, :, y0], x[:, :, y1]
    tl, tr, bl, br = rows0[..., x0], rows0[..., x1], rows1[..., x0], rows1[..., x1]
    top = tl + (tr - tl) * fx
    bot = bl + (br - bl) * fx
    return top + (bot - top) * fy


def preprocess(imgs):
    """[N, 3, H, W] floats in [0, 1] -> [N, 3, 299, 299] f32 in [-1, 1): torchmetrics' (imgs * 255).byte(), torch-fidelity's float
    conversion, TF1 resize and (x - 128) / 128."""
    x = (imgs.float() * 255).byte().float()
    return (resize_tf1(x) - 128) / 128


@torch.no_grad()
def features(net, imgs, dtype=torch.float64):
    """The [N, 2048] features of `imgs` with the network's arithmetic in `dtype` (the network is left in f32)."""
    net = net.to(dtype)
    try:
        return net(preprocess(imgs).to(dtype))
    finally:
        net.to(torch.float32)


def statistics(f):
    """(n, sum, cov_sum) in f64 of features [N, D]."""
    f = f.double()
    return f.shape[0], f.sum(0), f.t().mm(f)


def fid_from_statistics(n1, sum1, cov_sum1, n2, sum2, cov_sum2):
    """torchmetrics' compute(): means, unbiased covariances and |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eigvals(S1 S2)).real, f64."""
    mu1, mu2 = (sum1 / n1).unsqueeze(0), (sum2 / n2).unsqueeze(0)
    s1 = (cov_sum1 - n1 * mu1.t().mm(mu1)) / (n1 - 1)
    s2 = (cov_sum2 - n2 * mu2.t().mm(mu2)) / (n2 - 1)
    a = (mu1.squeeze(0) - mu2.squeeze(0)).square().sum()
    c = torch.linalg.eigvals(s1 @ s2).sqrt().real.sum()
    return a + s1.trace() + s2.trace() - 2 * c


def fid_from_features(f_real, f_fake):
    return fid_from_statistics(*statistics(f_real), *statistics(f_fake))

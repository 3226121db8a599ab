"""Host restatements (test infrastructure only) of what csrc/metric_train.hip computes, in f64 and in the kernels' own form -- the
gather-form data gradient, the weight gradient over gathered pixels, the BatchNorm backward, the max pool's first-maximum rule -- with
the sums of absolute products that the per-element bounds need, and the cases the GPU tests and the CPU tests share.
tests/test_classifier_train_host.py holds these against f64 autograd before the GPU sees them."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                                             # f32 unit roundoff
F64 = torch.float64

# (name, Cin, Cout, k, stride, pad, N, H, W) of the data- and weight-gradient cases
CONV_CASES = [
    ("3x3s1_64_7x7", 64, 64, 3, 1, 1, 2, 7, 7),
    ("3x3s2_64_128_7x7_odd", 64, 128, 3, 2, 1, 2, 7, 7),
    ("3x3s2_128_256_4x4_even", 128, 256, 3, 2, 1, 2, 4, 4),
    ("3x3s2_256_512_2x2_padding", 256, 512, 3, 2, 1, 3, 2, 2),
    ("3x3s1_512_1x1_centre", 512, 512, 3, 1, 1, 2, 1, 1),
    ("1x1s2_64_128_7x7", 64, 128, 1, 2, 0, 2, 7, 7),
    ("3x3s1_64_5x5_m75", 64, 64, 3, 1, 1, 3, 5, 5),
    ("fc_512_10", 512, 10, 1, 1, 0, 5, 1, 1),
]
STEM_CASE = ("stem_7x7s2", 1, 64, 7, 2, 3, 2, 28, 28)
SPLIT_CASE = ("3x3s1_64_16x16_split", 64, 64, 3, 1, 1, 4, 16, 16)      # N Ho Wo = 1024 pixels = 32 steps: wgrad_splits gives 8
BN_COUNTS = [(2, 1, 1), (3, 5, 5), (2, 7, 7), (8, 32, 32)]             # (N, H, W): 2, 75, 98, 8192 values per channel


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def conv_inputs(case, seed=0):
    """(x [N, Cin, H, W], w [Cout, Cin, k, k], dy [N, Cout, Ho, Wo]) as f32 normals."""
    _, cin, cout, k, s, p, N, H, W = case
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, k, s, p)
    return (torch.randn(N, cin, H, W, generator=g), torch.randn(cout, cin, k, k, generator=g) * 0.1, torch.randn(N, cout, Ho, Wo, generator=g))


def autograd_conv(x, w, dy, s, p):
    """(dx, dw) of F.conv2d in f64 under autograd."""
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(x, w, None, s, p).backward(dy.double())
    return x.grad, w.grad


def dgrad_gather(dy, w, H, W, s, p):
    """dx[n, ci, h, w] = sum over (kh, kw, co) of dy[n, co, (h + p - kh) / s, (w + p - kw) / s] w[co, ci, kh, kw], over the taps
    where the division is exact and the output position is in range -- f64, NCHW."""
    dy, w = dy.double(), w.double()
    N, cout, Ho, Wo = dy.shape
    k = w.shape[2]
    dx = torch.zeros(N, w.shape[1], H, W, dtype=F64)
    for kh in range(k):
        hs = [(h, (h + p - kh) // s) for h in range(H) if h + p - kh >= 0 and (h + p - kh) % s == 0 and (h + p - kh) // s < Ho]
        for kw in range(k):
            ws = [(x, (x + p - kw) // s) for x in range(W) if x + p - kw >= 0 and (x + p - kw) % s == 0 and (x + p - kw) // s < Wo]
            if not hs or not ws:
                continue
            hi, oy = (torch.tensor(v) for v in zip(*hs))
            wi, ox = (torch.tensor(v) for v in zip(*ws))
            part = torch.einsum("nohw,oc->nchw", dy[:, :, oy][:, :, :, ox], w[:, :, kh, kw])
            dx[:, :, hi[:, None], wi[None, :]] += part
    return dx


def wgrad_gather(x, dy, k, s, p):
    """dw[co, ci, kh, kw] = sum over the output pixels of dy[n, co, oy, ox] x[n, ci, oy s - p + kh, ox s - p + kw] (zero outside) --
    f64, NCHW."""
    x, dy = x.double(), dy.double()
    N, cout, Ho, Wo = dy.shape
    xp = F.pad(x, (p, p, p, p))
    dw = torch.zeros(cout, x.shape[1], k, k, dtype=F64)
    for kh in range(k):
        for kw in range(k):
            win = xp[:, :, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            dw[:, :, kh, kw] = torch.einsum("nohw,nchw->oc", dy, win)
    return dw


def product_bound(K, abs_sum):
    """The issue's per-element bound of a product of reduction length K: (K + 4) 2^-24 sum |a_i b_i|, in f64."""
    return (K + 4) * U * abs_sum.double()


def bn_forward(x, gamma, beta, eps=1e-5):
    """(xhat-based y, mean, biased var) of training-mode BN over NCHW x, in x's dtype."""
    mean = x.mean(dim=(0, 2, 3))
    var = x.var(dim=(0, 2, 3), unbiased=False)
    xh = (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps)
    return xh * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1), mean, var


def bn_backward(dy, y, x, gamma, eps=1e-5):
    """(dx, dgamma, dbeta, g) of y = relu?(gamma xhat + beta + res): g = dy where the saved output y > 0 (all of dy when y is None),
    dx = gamma invstd (g - mean g - xhat mean(g xhat)) -- in the inputs' dtype, NCHW."""
    g = dy if y is None else dy * (y > 0).to(dy.dtype)
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    invstd = 1 / torch.sqrt(x.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + eps)
    xh = (x - mean) * invstd
    dbeta = g.sum(dim=(0, 2, 3))
    dgamma = (g * xh).sum(dim=(0, 2, 3))
    m = x.numel() // x.shape[1]
    dx = gamma.view(1, -1, 1, 1) * invstd * (g - dbeta.view(1, -1, 1, 1) / m - xh * dgamma.view(1, -1, 1, 1) / m)
    return dx, dgamma, dbeta, g


def autograd_bn(x, gamma, beta, res, relu, dy, dtype):
    """(y, dx, dgamma, dbeta, dres or None) of F.batch_norm(training) (+ res) (ReLU) under autograd in `dtype`."""
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    res = None if res is None else res.to(dtype).clone().requires_grad_(True)
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, 1e-5)
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, gamma.grad, beta.grad, None if res is None else res.grad


def maxpool_backward(x, dy):
    """dx of the 3 x 3 / 2 pad 1 max pool in gather form's terms: per window the FIRST maximum in (kh, kw) ascending scan order (a
    later tap wins only when strictly larger), windows visited in (oy, ox) order -- x, dy NCHW, any dtype, exact additions order."""
    N, C, H, W = x.shape
    Ho, Wo = dy.shape[2:]
    xn, dyn = x.numpy(), dy.numpy()
    dx = np.zeros_like(xn)
    ni, ci = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    for oy in range(Ho):
        for ox in range(Wo):
            best = np.full((N, C), -np.inf, xn.dtype)
            by, bx = np.full((N, C), -1), np.full((N, C), -1)
            for kh in range(3):
                iy = oy * 2 - 1 + kh
                if iy < 0 or iy >= H:
                    continue
                for kw in range(3):
                    ix = ox * 2 - 1 + kw
                    if ix < 0 or ix >= W:
                        continue
                    v = xn[:, :, iy, ix]
                    take = (by < 0) | (v > best)
                    best, by, bx = np.where(take, v, best), np.where(take, iy, by), np.where(take, ix, bx)
            np.add.at(dx, (ni, ci, by, bx), dyn[:, :, oy, ox])
    return torch.from_numpy(dx)


def pool_inputs(seed=0):
    """x [2, 64, 14, 14] quantised to 1 / 4 (ties occur) with a block of exact zeros, dy [2, 64, 7, 7]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(2, 64, 14, 14, generator=g) * 4) / 4
    x[:, :, 3:9, 4:10] = 0.0
    return x, torch.randn(2, 64, 7, 7, generator=g)


def rel_l2(a, b):
    """|a - b| / |b| in f64 (|a - b| when b is zero)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def ref_steps(sd, batches, dtype, lr=1e-3):
    """ResNet18Ref in train mode from the state dict `sd` over `batches` [(images, labels)] with F.cross_entropy and
    torch.optim.Adam(lr), on the CPU in `dtype`: per step (loss, {name: gradient}, state dict after the update)."""
    from classifier_ref import ResNet18Ref
    net = ResNet18Ref().to(dtype)
    net.load_state_dict({k: (v if v.dtype == torch.int64 else v.to(dtype)) for k, v in sd.items()})
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    out = []
    for x, y in batches:
        opt.zero_grad()
        loss = F.cross_entropy(net(x.to(dtype)), y)
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        opt.step()
        out.append((float(loss.detach()), grads, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    return out

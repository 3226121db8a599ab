"""Training of the MNIST ResNet-18 that the quality metrics of the T-shirt experiment read (`checkpoints/classifiers/mnist.pt`):
the reference's notebooks/cnn-resnet18-mnist.ipynb -- train-mode BatchNorm, F.cross_entropy, torch.optim.Adam -- on the f32 HIP
kernels of csrc/metric_train.hip, with the forward convolutions and the max pool of csrc/metric_conv.hip (BN is NOT folded here).

`ResNet18Trainer` is a class of its own beside the eval-only `classifier.ResNet18` (whose `.train(True)` keeps refusing); its
`save()` writes the state dict that `Classifier(classifier_ckpt=...)` loads unchanged.  There is no CPU path: a missing kernel
library raises.  The functions below are the launches, one per kernel group; the tests call them directly.
"""
from collections import OrderedDict

import torch

from . import lib
from . import metric_net as mn
from .classifier import ResNet18, _convs
from .optim import FlatAdamW

LD_LOGITS = 32                  # the channel stride dlogits is carried with (fc's Cout = num_classes <= 32 carried as 32)


def layer(w, cin, cout, k, stride, pad):
    """The packed-layer dict of metric_net.conv around packed weights `w` [Cout][Kp] (a view of the flat parameter buffer)."""
    return dict(w=w, b=None, cin=cin, cin_p=mn.padded(cin), cout=cout, cout_p=mn.padded(cout), kh=k, kw=k, stride=stride, ph=pad,
                pw=pad, Kp=w.shape[1])


def packed_kp(cin, k):
    return -(-(k * k * mn.padded(cin)) // mn.BK) * mn.BK


def wgrad_splits(M, cout, Kp):
    """How many parts the weight gradient's reduction over the M output pixels is cut into: 1 when the 64 x 64 tiles of dW number
    at least 128, else enough parts for up to 256 blocks with at least 4 steps of 32 pixels each (metric_net.conv_splits's rule on
    the other axis; no sweep has been run)."""
    tiles = -(-cout // 64) * -(-Kp // 64)
    steps = -(-M // 32)
    return 1 if tiles >= 128 else max(1, min(steps // 4, -(-256 // tiles)))


def dgrad_splits(M, cin, steps):
    """Split-K factor of one data gradient (M input pixels, `steps` K steps of 32 output channels of a tap): metric_net.conv_splits's
    rule -- 1 when the 64 x 64 tiles number at least 128, else enough splits for up to 256 blocks with at least 4 K steps each.  At
    B = 128 the unsplit kernel took 44 % of the step's kernel time (layer4: 16 blocks over 144 steps)."""
    blocks = -(-M // 64) * -(-cin // 64)
    return 1 if blocks >= 128 else max(1, min(steps // 4, -(-256 // blocks)))


def conv_dgrad(L, dy, in_shape, add=None, splits=None, out=None):
    """dx [N, H, W, Cin] of the packed layer L from dy [N, Ho, Wo, ldy] (+ add), into out when given."""
    N, H, W, C = in_shape
    _, Ho, Wo, ldy = dy.shape
    dx = torch.empty(N, H, W, C, device=dy.device, dtype=torch.float32) if out is None else out
    if splits is None:
        splits = dgrad_splits(N * H * W, C, L["kh"] * L["kw"] * (ldy // mn.BK))
    ws = torch.empty(splits * N * H * W * C, device=dy.device, dtype=torch.float32) if splits > 1 else None
    lib.call("siss_cls_conv_dgrad", dy, L["w"], add, dx, ws, 0 if ws is None else ws.numel(), N, H, W, C, Ho, Wo, L["cout"], ldy, L["kh"],
             L["kw"], L["stride"], L["ph"], L["pw"], L["Kp"], splits)
    return dx


def conv_wgrad(L, x, dy, dw, nchw_in=False, splits=None):
    """dw [Cout][Kp] (packed, pad slots zero) of the packed layer L from its input x (NHWC, or the NCHW image) and dy."""
    if nchw_in:
        N, C, H, W = x.shape
    else:
        N, H, W, C = x.shape
    _, Ho, Wo, ldy = dy.shape
    if splits is None:
        splits = wgrad_splits(N * Ho * Wo, L["cout"], L["Kp"])
    ws = torch.empty(splits * L["cout"] * L["Kp"], device=dy.device, dtype=torch.float32) if splits > 1 else None
    lib.call("siss_cls_conv_wgrad", x, nchw_in, dy, dw, ws, 0 if ws is None else ws.numel(), N, H, W, C, Ho, Wo, L["cout"], ldy,
             L["kh"], L["kw"], L["stride"], L["ph"], L["pw"], L["Kp"], splits)
    return dw


def bn_partials(C, device):
    return torch.empty(lib.query("siss_cls_bn_partials_words", C), device=device, dtype=torch.float64)


def bn_forward(x, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, partials, res=None, relu=False,
               training=True):
    """y of BatchNorm2d over the rows of NHWC x (+ res) (ReLU); training: batch statistics, the running ones updated in place."""
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x)
    lib.call("siss_cls_bn_fwd", x, gamma, beta, res, y, running_mean, running_var, num_batches_tracked, save_mean, save_invstd,
             partials, 0 if partials is None else partials.numel(), M, C, relu, training)
    return y


def bn_backward(dy, y, x, gamma, save_mean, save_invstd, dgamma, dbeta, partials, dres=None):
    """dx of the training-mode BatchNorm (ReLU mask from the saved output y when given); dgamma / dbeta written; dres = masked dy."""
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    lib.call("siss_cls_bn_bwd", dy, y, x, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, partials, partials.numel(), M, C)
    return dx


def max_pool3_backward(x, dy):
    """dx of the 3 x 3 / 2 pad 1 max pool from its NHWC input x and dy."""
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    lib.call("siss_cls_maxpool3_bwd", x, dy, dx, N, H, W, C, dy.shape[1], dy.shape[2])
    return dx


def softmax_ce(logits, labels, ldd=LD_LOGITS):
    """(mean cross-entropy as a device scalar, dlogits [B, ldd]) of logits [B, C] and int64 labels [B]."""
    B, C = logits.shape
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty(B, ldd, device=logits.device, dtype=torch.float32)
    lib.call("siss_cls_softmax_ce", logits, labels, loss, dlogits, B, C, logits.stride(0), ldd)
    return loss, dlogits


class ResNet18Trainer:
    """metrics/mnist_resnet.py's resnet18(num_classes, grayscale) in training: `step(images, labels)` is one iteration of the
    reference notebook's loop (forward with batch-statistics BN, F.cross_entropy, backward, Adam), enqueued without a host sync.

    All trainable parameters live in ONE flat f32 buffer `flat` in the kernels' packed layout (per convolution [Cout][Kp] then its
    BN's gamma and beta, in `classifier._convs` order; then fc.weight [classes][512] and fc.bias), the gradients in `grad` beside it,
    the BN running statistics in `stats` and the batch counters in `tracked`.  The pad slots of a packed weight are zero, their
    gradients are written as zero, and Adam leaves a zero parameter with zero moments where it is.

    The update is `FlatAdamW(flat, lr, betas, eps, weight_decay=0.0, max_grad_norm=inf).launch_single(grad)`: with no weight decay the
    decay factor 1 - lr * 0 is exactly 1, and with an infinite norm bound the clip coefficient min(1, inf / (|g| + 1e-6)) is exactly 1,
    so g * 1 and p * 1 change no bit and what remains -- m.lerp(g, 1 - b1), v * b2 + g g (1 - b2), p -= lr / bc1 * m / (sqrt(v) /
    sqrt(bc2) + eps) -- is torch.optim.Adam's single-tensor arithmetic.
    """

    def __init__(self, num_classes=10, grayscale=True, device="cuda", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=1):
        self.num_classes, self.in_ch = int(num_classes), (1 if grayscale else 3)
        if not 0 < self.num_classes <= LD_LOGITS:
            raise ValueError(f"ResNet18Trainer: 1 .. {LD_LOGITS} classes, got {num_classes}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ResNet18Trainer: a cuda device is needed -- the network trains on the HIP kernels only")
        lib.load()
        self.convs = _convs(self.in_ch)
        # the layout of the flat buffers
        self.slots, self.stat_slots, off, soff = OrderedDict(), OrderedDict(), 0, 0
        for name, cin, cout, k, _, _, bn in self.convs:
            for key, n in ((name + ".weight", cout * packed_kp(cin, k)), (bn + ".weight", cout), (bn + ".bias", cout)):
                self.slots[key] = (off, n)
                off += n
            for key in (bn + ".running_mean", bn + ".running_var"):
                self.stat_slots[key] = (soff, cout)
                soff += cout
        for key, n in (("fc.weight", self.num_classes * 512), ("fc.bias", self.num_classes)):
            self.slots[key] = (off, n)
            off += n
        dev = self.device
        self.flat = torch.zeros(off, device=dev)
        self.grad = torch.zeros(off, device=dev)
        self.stats = torch.zeros(soff, device=dev)
        self.saved = torch.zeros(soff, device=dev, dtype=torch.float64)   # per BN: the batch mean, then 1 / sqrt(var + eps), of the last forward (f64)
        self.tracked = torch.zeros(len(self.convs), device=dev, dtype=torch.int64)
        self.P = {k: self.flat[o:o + n] for k, (o, n) in self.slots.items()}
        self.G = {k: self.grad[o:o + n] for k, (o, n) in self.slots.items()}
        self.S = {k: self.stats[o:o + n] for k, (o, n) in self.stat_slots.items()}
        self.V = {k: self.saved[o:o + n] for k, (o, n) in self.stat_slots.items()}
        self.bn_index = {bn: i for i, (*_, bn) in enumerate(self.convs)}
        zero_bias = torch.zeros(512, device=dev)
        self.L = {}
        for name, cin, cout, k, s, p, _ in self.convs:
            self.L[name] = layer(self.P[name + ".weight"].view(cout, -1), cin, cout, k, s, p)
            self.L[name]["b"] = zero_bias[:cout]                  # (the convolution's identity bias: BN follows unfolded)
        self.L["fc"] = layer(self.P["fc.weight"].view(self.num_classes, 512), 512, self.num_classes, 1, 1, 0)
        self.L["fc"]["b"] = self.P["fc.bias"]
        self.partials = bn_partials(512, dev)
        # the reference constructor's scheme (ResNet18._init), drawn from a forked generator seeded by `seed`
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            sd = ResNet18(self.num_classes, grayscale).state_dict()
        self.load_state_dict(sd)
        self.opt = FlatAdamW(self.flat, lr, betas=betas, eps=eps, weight_decay=0.0, max_grad_norm=float("inf"))

    # ------------------------------------------------------------------ state
    def _unpacked(self, flat):
        """The trainable tensors of a flat buffer in `flat`'s layout (host copy) under torch's names and shapes."""
        get = lambda k: flat[self.slots[k][0]:self.slots[k][0] + self.slots[k][1]]
        out = OrderedDict()
        for name, cin, cout, k, _, _, bn in self.convs:
            cp = mn.padded(cin)
            w = get(name + ".weight").view(cout, -1)[:, :k * k * cp].reshape(cout, k, k, cp)[..., :cin]
            out[name + ".weight"] = w.permute(0, 3, 1, 2).contiguous()
            out[bn + ".weight"], out[bn + ".bias"] = get(bn + ".weight").clone(), get(bn + ".bias").clone()
        out["fc.weight"] = get("fc.weight").view(self.num_classes, 512).clone()
        out["fc.bias"] = get("fc.bias").clone()
        return out

    def gradients(self):
        """The gradients of the last step under torch's parameter names and shapes, on the host."""
        return self._unpacked(self.grad.cpu())

    def state_dict(self):
        """torch's key names and shapes, in `ResNet18._ordered`'s order, on the host."""
        params, stats, tracked = self._unpacked(self.flat.cpu()), self.stats.cpu(), self.tracked.cpu()
        sd = OrderedDict()
        for i, (name, *_, bn) in enumerate(self.convs):
            for key in (name + ".weight", bn + ".weight", bn + ".bias"):
                sd[key] = params[key]
            for key in (bn + ".running_mean", bn + ".running_var"):
                o, n = self.stat_slots[key]
                sd[key] = stats[o:o + n].clone()
            sd[bn + ".num_batches_tracked"] = tracked[i].clone()
        sd["fc.weight"], sd["fc.bias"] = params["fc.weight"], params["fc.bias"]
        return sd

    def load_state_dict(self, sd):
        """The inverse of state_dict(): strict over the key names and shapes.  The optimizer's moments are left as they are."""
        want = {}
        for name, cin, cout, k, _, _, bn in self.convs:
            want[name + ".weight"] = (cout, cin, k, k)
            for s in (".weight", ".bias", ".running_mean", ".running_var"):
                want[bn + s] = (cout,)
            want[bn + ".num_batches_tracked"] = ()
        want["fc.weight"], want["fc.bias"] = (self.num_classes, 512), (self.num_classes,)
        missing, unexpected = [k for k in want if k not in sd], [k for k in sd if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"ResNet18Trainer.load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, shape in want.items():
            if tuple(sd[k].shape) != shape:
                raise RuntimeError(f"ResNet18Trainer.load_state_dict: {k} has shape {tuple(sd[k].shape)}, the model {shape}")
        flat, stats = torch.zeros(self.flat.numel()), torch.zeros(self.stats.numel())
        tracked = torch.zeros(len(self.convs), dtype=torch.int64)

        def put(buf, slot, v):
            buf[slot[0]:slot[0] + slot[1]] = v.detach().to("cpu", torch.float32).reshape(-1)
        for i, (name, cin, cout, k, s, p, bn) in enumerate(self.convs):
            put(flat, self.slots[name + ".weight"], mn.pack_conv(sd[name + ".weight"].detach().cpu().float(), torch.zeros(cout), s, p, "cpu")["w"])
            for sfx in (".weight", ".bias"):
                put(flat, self.slots[bn + sfx], sd[bn + sfx])
            for sfx in (".running_mean", ".running_var"):
                put(stats, self.stat_slots[bn + sfx], sd[bn + sfx])
            tracked[i] = int(sd[bn + ".num_batches_tracked"])
        put(flat, self.slots["fc.weight"], sd["fc.weight"])
        put(flat, self.slots["fc.bias"], sd["fc.bias"])
        self.flat.copy_(flat)
        self.stats.copy_(stats)
        self.tracked.copy_(tracked)

    def save(self, path):
        """torch.save of the state dict: the file `Classifier(classifier_ckpt=path)` reads."""
        torch.save(self.state_dict(), str(path))

    # ------------------------------------------------------------------ forward
    def _images(self, x):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.in_ch:
            raise ValueError(f"ResNet18Trainer expects [N, {self.in_ch}, H, W] images, got {tuple(getattr(x, 'shape', ()))}")
        if x.shape[2] > 32 or x.shape[3] > 32 or min(x.shape[2:]) < 1:
            raise ValueError(f"ResNet18Trainer: {x.shape[2]} x {x.shape[3]} images: fc reads a 512 x 1 x 1 map, 1 <= H, W <= 32")
        return x.to(self.device, torch.float32).contiguous()

    def _bn(self, bn, x, res, relu, training):
        return bn_forward(x, self.P[bn + ".weight"], self.P[bn + ".bias"], self.S[bn + ".running_mean"], self.S[bn + ".running_var"],
                          self.tracked[self.bn_index[bn]:], self.V[bn + ".running_mean"], self.V[bn + ".running_var"], self.partials,
                          res=res, relu=relu, training=training)

    def _forward(self, x, training):
        """(logits [N, classes], the saved activations of the backward)."""
        L, conv = self.L, mn.conv
        c0 = conv(L["conv1"], x, relu=False, nchw_in=True)
        r0 = self._bn("bn1", c0, None, True, training)
        h = mn.max_pool3(r0, 2, 1)
        saved = [(x, c0, r0)]
        for i in range(1, 5):
            for j in range(2):
                pre = f"layer{i}.{j}."
                c1 = conv(L[pre + "conv1"], h, relu=False)
                a = self._bn(pre + "bn1", c1, None, True, training)
                c2 = conv(L[pre + "conv2"], a, relu=False)
                cd, sc = None, h
                if pre + "downsample.0" in L:
                    cd = conv(L[pre + "downsample.0"], h, relu=False)
                    sc = self._bn(pre + "downsample.1", cd, None, False, training)
                out = self._bn(pre + "bn2", c2, sc, True, training)
                saved.append((pre, h, c1, a, c2, out, cd))
                h = out
        assert h.shape[1] == 1 and h.shape[2] == 1
        return mn.linear(L["fc"], h.view(h.shape[0], 512)), saved

    @torch.no_grad()
    def eval_logits(self, images):
        """[N, classes] logits with the running statistics (eval-mode BN), through the same kernels; nothing is updated."""
        x = self._images(images)
        if x.shape[0] == 0:
            return torch.empty(0, self.num_classes, device=self.device)
        return self._forward(x, False)[0]

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, bn, dy, y, x, dres=None):
        return bn_backward(dy, y, x, self.P[bn + ".weight"], self.V[bn + ".running_mean"], self.V[bn + ".running_var"],
                           self.G[bn + ".weight"], self.G[bn + ".bias"], self.partials, dres=dres)

    def _wgrad(self, name, x, dy, nchw_in=False):
        conv_wgrad(self.L[name], x, dy, self.G[name + ".weight"].view(self.L[name]["cout"], -1), nchw_in=nchw_in)

    def _backward(self, saved, dlogits):
        """Every gradient into `grad` from dlogits [N, LD_LOGITS]."""
        L, N = self.L, dlogits.shape[0]
        feat = saved[-1][5]
        dl = dlogits.view(N, 1, 1, LD_LOGITS)
        self._wgrad("fc", feat, dl)
        lib.call("siss_cls_bias_grad", dlogits, self.G["fc.bias"], N, self.num_classes, LD_LOGITS)
        d = conv_dgrad(L["fc"], dl, feat.shape)
        for pre, h, c1, a, c2, out, cd in reversed(saved[1:]):
            dc2 = self._bn_bwd(pre + "bn2", d, out, c2, dres=d)              # d becomes the masked gradient: the shortcut's
            self._wgrad(pre + "conv2", a, dc2)
            da = conv_dgrad(L[pre + "conv2"], dc2, a.shape)
            dc1 = self._bn_bwd(pre + "bn1", da, a, c1)
            self._wgrad(pre + "conv1", h, dc1)
            if cd is not None:
                dcd = self._bn_bwd(pre + "downsample.1", d, None, cd)
                self._wgrad(pre + "downsample.0", h, dcd)
                d = conv_dgrad(L[pre + "downsample.0"], dcd, h.shape)
            d = conv_dgrad(L[pre + "conv1"], dc1, h.shape, add=d)
        x, c0, r0 = saved[0]
        dc0 = self._bn_bwd("bn1", max_pool3_backward(r0, d), r0, c0)
        self._wgrad("conv1", x, dc0, nchw_in=True)

    @torch.no_grad()
    def step(self, images, labels):
        """One training iteration on images [N, C, H, W] in [0, 1] and labels [N] (N >= 2: layer4's BatchNorm sees N values per
        channel); returns the mean cross-entropy as a device scalar.  Nothing here waits for the device."""
        x = self._images(images)
        N = x.shape[0]
        labels = torch.as_tensor(labels)
        if N < 2 or tuple(labels.shape) != (N,):
            raise ValueError(f"ResNet18Trainer.step: at least 2 images and one label each, got {tuple(x.shape)} / {tuple(labels.shape)}")
        labels = labels.to(self.device, torch.int64).contiguous()
        logits, saved = self._forward(x, True)
        loss, dlogits = softmax_ce(logits, labels)
        self._backward(saved, dlogits)
        self.opt.launch_single(self.grad)
        return loss

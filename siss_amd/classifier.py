"""Quality metrics of the MNIST T-shirt experiment: the reference's MNIST ResNet-18 (metrics/mnist_resnet.py) on the HIP implicit-GEMM
convolution of csrc/metric_conv.hip (behind siss_amd/metric_net.py), and the class surface around it -- `Classifier`
(metrics/classifier.py), `InceptionScore` (metrics/inception_score.py), `TShirtClassifier` (metrics/tshirt.py) -- plus `TShirtMetrics`, the tracker of delete_tshirt.py's
log_metrics (fraction -> deletion_steps -> Inception Score trigger) that the task loop drives.

The network runs in f32, in eval mode (BatchNorm with its running statistics, folded into the convolutions at load time in f64);
there is no CPU path: a missing kernel library raises.
"""
import math
import os
import time
from collections import OrderedDict

import torch

from . import metric_net as mn
from .records import append_jsonl, finite_or_none
from .metric_net import conv_splits  # noqa: F401  (tests/test_hip_sscd.py reads the split-K choice from here)

BN_EPS = 1e-5
_WIDTHS = (64, 128, 256, 512)


def _convs(in_ch):
    """(prefix, Cin, Cout, k, stride, pad, bn prefix) of every convolution, in torch's state-dict order."""
    out = [("conv1", in_ch, 64, 7, 2, 3, "bn1")]
    inp = 64
    for i, w in enumerate(_WIDTHS, 1):
        for j in range(2):
            s = 2 if (i > 1 and j == 0) else 1
            p = f"layer{i}.{j}."
            out.append((p + "conv1", inp, w, 3, s, 1, p + "bn1"))
            out.append((p + "conv2", w, w, 3, 1, 1, p + "bn2"))
            if j == 0 and (s != 1 or inp != w):
                out.append((p + "downsample.0", inp, w, 1, s, 0, p + "downsample.1"))
            inp = w
    return out


class ResNet18(mn.MetricNet):
    """metrics/mnist_resnet.py's resnet18(num_classes, grayscale) on the HIP kernels: `[N, C, H, W]` f32 images -> `[N, num_classes]`
    logits (the reference disables avgpool, so fc reads the flattened 512 x 1 x 1 map: H, W <= 32).  The parameters live on the host
    under torch's key names; `.to(device)` / the first call packs them (BN folded) onto the device."""

    def __init__(self, num_classes, grayscale):
        self.num_classes, self.in_ch = int(num_classes), (1 if grayscale else 3)
        sd = OrderedDict()
        # the reference's constructor: conv N(0, sqrt(2 / (k^2 Cout))), BN weight 1 / bias 0 (stats 0 / 1), nn.Linear's default for fc;
        # drawn from a fork of the global generator, so that building the metric leaves the global stream where it was
        with torch.random.fork_rng(devices=[]):
            self._init(sd)
        super().__init__(self._ordered(sd))

    def _init(self, sd):
        for name, cin, cout, k, _, _, bn in _convs(self.in_ch):
            sd[name + ".weight"] = torch.empty(cout, cin, k, k).normal_(0, math.sqrt(2.0 / (k * k * cout)))
            sd[bn + ".weight"], sd[bn + ".bias"] = torch.ones(cout), torch.zeros(cout)
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.zeros(cout), torch.ones(cout)
            sd[bn + ".num_batches_tracked"] = torch.tensor(0)
        bound = 1.0 / math.sqrt(512)
        sd["fc.weight"] = torch.empty(self.num_classes, 512).uniform_(-bound, bound)
        sd["fc.bias"] = torch.empty(self.num_classes).uniform_(-bound, bound)

    def _ordered(self, sd):
        # torch's order: conv1, bn1, layer*, fc (the BN of a layer right after its conv)
        keys = []
        for name, *_, bn in _convs(self.in_ch):
            keys += [name + ".weight"] + [bn + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]
        keys += ["fc.weight", "fc.bias"]
        return OrderedDict((k, sd[k]) for k in keys)

    def _pack(self):
        """Per convolution the folded BN in f64, rounded once to f32 (metric_net.pack_conv); fc is a 1 x 1 convolution with its bias."""
        self._need_device()
        sd = self._sd
        layers = {}
        for name, cin, cout, k, s, p, bn in _convs(self.in_ch):
            layers[name] = mn.pack_conv(*mn.fold_bn(sd, name, bn, BN_EPS), s, p, self.device)
        layers["fc"] = mn.pack_conv(sd["fc.weight"].double().view(self.num_classes, 512, 1, 1), sd["fc.bias"].double(), 1, 0,
                                            self.device)
        self._packed = layers

    @torch.no_grad()
    def __call__(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_ch:
            raise ValueError(f"ResNet18 expects [N, {self.in_ch}, H, W] images, got {tuple(x.shape)}")
        N, _, H, W = x.shape
        if H > 32 or W > 32:
            raise ValueError(f"ResNet18: {H} x {W} images leave layer4 larger than 1 x 1, and the reference's fc (512 inputs, avgpool "
                             "disabled) does not take them: H, W <= 32")
        if self._packed is None:
            self._pack()
        x = x.to(self.device, torch.float32).contiguous()
        if N == 0:
            return torch.empty(0, self.num_classes, device=self.device)
        P, conv = self._packed, mn.conv
        h = mn.max_pool3(conv(P["conv1"], x, nchw_in=True), 2, 1)
        for i in range(1, 5):
            for j in range(2):
                pre = f"layer{i}.{j}."
                a = conv(P[pre + "conv1"], h)
                sc = conv(P[pre + "downsample.0"], h, relu=False) if pre + "downsample.0" in P else h
                h = conv(P[pre + "conv2"], a, res=sc)
        assert h.shape[1] == 1 and h.shape[2] == 1
        return mn.linear(P["fc"], h.view(N, 512))

    forward = __call__


def resnet18(num_classes, grayscale):
    """metrics/mnist_resnet.py::resnet18 (BasicBlock, [2, 2, 2, 2])."""
    return ResNet18(num_classes, grayscale)


class Classifier:
    """metrics/classifier.py::Classifier: `classifier(**classifier_args)` on `device`, the checkpoint (a state dict) loaded with
    torch.load(..., map_location="cpu"), eval mode."""

    def __init__(self, classifier, classifier_ckpt, classifier_args, transform, device):
        self.classifier = classifier(**dict(classifier_args or {})).to(device)
        if classifier_ckpt is not None:
            if not os.path.isfile(str(classifier_ckpt)):
                raise FileNotFoundError(f"classifier_ckpt {classifier_ckpt!r} is not a file on disk")
            self.classifier.load_state_dict(torch.load(str(classifier_ckpt), map_location="cpu"))
        self.classifier.eval()
        self.transform = transform

    def compute_logits(self, imgs, batch_size=2048):
        """[N, C, H, W] in [0, 1] -> [N, num_classes] logits, in batches of batch_size."""
        n = imgs.size(0)
        if self.transform is not None:
            imgs = self.transform(imgs)
        out = [self.classifier(imgs[s:s + batch_size]) for s in range(0, n, batch_size)]
        return torch.cat(out, dim=0)

    def compute_class_frequency(self, imgs, img_class):
        """Fraction of the images whose argmax is img_class (one forward over all of them, as the reference)."""
        if self.transform is not None:
            imgs = self.transform(imgs)
        preds = self.classifier(imgs).argmax(-1)
        return (preds == img_class).sum().item() / imgs.size(0)


class InceptionScore:
    """metrics/inception_score.py::InceptionScore (torchmetrics' formula on the classifier's logits): per torch.chunk split,
    exp(mean_i KL(p_i || mean p)); (mean, unbiased std) over the splits.  With remove_class: rows whose argmax is that class and
    that column are dropped, and splits - 1 splits are used."""

    def __init__(self, classifier, splits=10, remove_class=None):
        self.splits = splits if remove_class is None else splits - 1
        self.remove_class = remove_class
        self.classifier = classifier
        self.logits = []

    def update(self, imgs):
        logits = self.classifier.compute_logits(imgs)
        if self.remove_class is not None:
            logits = logits[logits.argmax(-1) != self.remove_class]
            logits = logits[:, torch.arange(logits.size(-1), device=logits.device) != self.remove_class]
        self.logits.append(logits)

    def compute(self, generator=None):
        """(mean, std) as 0-d tensors; the row permutation is torch.randperm with `generator` (the global CPU generator if None)."""
        if not self.logits:
            raise ValueError("No samples to concatenate")
        logits = torch.cat(self.logits, dim=0)
        idx = torch.randperm(logits.shape[0], generator=generator, device=generator.device if generator is not None else "cpu")
        logits = logits[idx.to(logits.device)]
        prob = logits.softmax(dim=1).chunk(self.splits, dim=0)
        log_prob = logits.log_softmax(dim=1).chunk(self.splits, dim=0)
        mean_prob = [p.mean(dim=0, keepdim=True) for p in prob]
        kl = torch.stack([(p * (lp - mp.log())).sum(dim=1).mean().exp() for p, lp, mp in zip(prob, log_prob, mean_prob)])
        return kl.mean(), kl.std()


class TShirtClassifier:
    """metrics/tshirt.py::TShirtClassifier."""

    @staticmethod
    def get_tshirt_frequency(imgs, tshirt_img, threshold=10):
        """(share of images whose flattened L2 distance to tshirt_img is strictly below threshold, the [N] bool matches)."""
        d = torch.norm(imgs.reshape(imgs.size(0), -1) - tshirt_img.reshape(-1), dim=1)
        matches = d < threshold
        return matches.float().mean().item(), matches


class TShirtMetrics:
    """The metric half of delete_tshirt.py's log_metrics (:438-482) for one rank: at a global step that is a multiple of
    `sampling_steps` the T-shirt fraction of `eval_images` samples (the first step where it is 0 becomes `deletion_steps`); at a
    multiple of `is_every` and at `deletion_steps` the Inception Score of `is_images` samples that do not match the T-shirt.
    `sample(n, batch_size)` returns [n, C, H, W] images in [0, 1]; `inception()` a fresh InceptionScore.  One JSON line per step at
    which a metric ran: {global_step, deletion_class_fraction, is_mean, is_std, is_images, seconds} (a key only when its metric ran,
    non-finite values as null, "deletion_steps" on the first line whose fraction is 0)."""

    def __init__(self, tshirt_img, out_path, sample, sampling_steps=None, eval_images=128, eval_batch_size=None,
                 inception=None, is_every=None, is_images=1024, is_batch_size=None, generator=None):
        self.tshirt, self.out_path, self.sample = tshirt_img, out_path, sample
        self.sampling_steps = int(sampling_steps) if sampling_steps else 0
        self.eval_images, self.eval_batch_size = int(eval_images), int(eval_batch_size or eval_images)
        self.inception, self.is_every = inception, int(is_every or 0)
        self.is_images, self.is_batch_size = int(is_images), int(is_batch_size or is_images)
        self.generator = generator
        self.deletion_steps = None
        self.extra = None                                # fields added to every record (pipeline.sampler: name and step count)

    def __call__(self, global_step):
        t0 = time.perf_counter()
        rec = {"global_step": int(global_step)}
        if self.sampling_steps and global_step % self.sampling_steps == 0:
            frac, _ = TShirtClassifier.get_tshirt_frequency(self.sample(self.eval_images, self.eval_batch_size), self.tshirt)
            rec["deletion_class_fraction"] = finite_or_none(frac)
            if frac == 0 and self.deletion_steps is None:
                self.deletion_steps = rec["deletion_steps"] = int(global_step)
        if self.inception is not None and ((self.is_every and global_step % self.is_every == 0) or self.deletion_steps == global_step):
            imgs = self.sample(self.is_images, self.is_batch_size)
            _, matches = TShirtClassifier.get_tshirt_frequency(imgs, self.tshirt)
            kept = imgs[~matches]
            mean = std = float("nan")
            if kept.shape[0] > 0:
                calc = self.inception()
                calc.update(kept)
                mean, std = calc.compute(generator=self.generator)
            rec.update(is_mean=finite_or_none(mean), is_std=finite_or_none(std), is_images=int(kept.shape[0]))
        if len(rec) == 1:
            return None
        rec["seconds"] = time.perf_counter() - t0
        rec.update(self.extra or {})
        return append_jsonl(self.out_path, rec)

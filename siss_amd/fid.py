"""The FID metric of the CelebA-HQ experiment (metrics/fid.py of the reference: `FIDEvaluator` around torchmetrics'
`FrechetInceptionDistance(normalize=True, reset_real_features=False)`, feature dimension 2048) on the HIP kernels of
csrc/metric_conv.hip (behind siss_amd/metric_net.py) and csrc/inception.hip:
`InceptionV3FID` (the FID Inception-v3 of torch-fidelity, pt_inception-2015-12-05, up to the global average pool),
`FrechetInceptionDistance` (the six statistics on the device in f64, the eigenvalue step on the host) and `FIDEvaluator`, plus
`FIDTracker`, what the task loop drives.

The network runs in f32, in eval mode (BatchNorm with its running statistics, folded into the convolutions at pack time in f64); there
is no CPU path: a missing kernel library raises.  Images handed to the metric on the device reach the statistics without leaving it;
what `compute()` moves to the host is the D x D product of the two covariances, once per evaluation.  (In the task loop the samples
themselves make one round trip before that: `Evaluator.sample_images` returns host arrays, as the reference's pipeline does.)
"""
import math
import os
import time
from collections import OrderedDict

import torch

from . import lib
from . import metric_net as mn
from .records import append_jsonl, finite_or_none

BN_EPS = 1e-3
FEATURES = 2048
SIZE = 299
DEFAULT_CKPT = "checkpoints/classifiers/pt_inception-2015-12-05-6726825d.pth"


def _block_a(name, cin, pf):
    return [(f"{name}.branch1x1", cin, 64, 1, 1, 0), (f"{name}.branch5x5_1", cin, 48, 1, 1, 0), (f"{name}.branch5x5_2", 48, 64, 5, 1, 2),
            (f"{name}.branch3x3dbl_1", cin, 64, 1, 1, 0), (f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1),
            (f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1), (f"{name}.branch_pool", cin, pf, 1, 1, 0)]


def _block_c(name, c7):
    p = f"{name}.branch7x7"
    return [(f"{name}.branch1x1", 768, 192, 1, 1, 0),
            (p + "_1", 768, c7, 1, 1, 0), (p + "_2", c7, c7, (1, 7), 1, (0, 3)), (p + "_3", c7, 192, (7, 1), 1, (3, 0)),
            (p + "dbl_1", 768, c7, 1, 1, 0), (p + "dbl_2", c7, c7, (7, 1), 1, (3, 0)), (p + "dbl_3", c7, c7, (1, 7), 1, (0, 3)),
            (p + "dbl_4", c7, c7, (7, 1), 1, (3, 0)), (p + "dbl_5", c7, 192, (1, 7), 1, (0, 3)),
            (f"{name}.branch_pool", 768, 192, 1, 1, 0)]


def _block_e(name, cin):
    return [(f"{name}.branch1x1", cin, 320, 1, 1, 0), (f"{name}.branch3x3_1", cin, 384, 1, 1, 0),
            (f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), (f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{name}.branch3x3dbl_1", cin, 448, 1, 1, 0), (f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1),
            (f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), (f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{name}.branch_pool", cin, 192, 1, 1, 0)]


def convs():
    """(name, Cin, Cout, (KH, KW), stride, (pad_h, pad_w)) of the 94 BasicConv2d layers, in the state dict's order."""
    out = [("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
           ("Conv2d_3b_1x1", 64, 80, 1, 1, 0), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0)]
    out += _block_a("Mixed_5b", 192, 32) + _block_a("Mixed_5c", 256, 64) + _block_a("Mixed_5d", 288, 64)
    out += [("Mixed_6a.branch3x3", 288, 384, 3, 2, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 0),
            ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1), ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2, 0)]
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        out += _block_c(name, c7)
    p = "Mixed_7a.branch7x7x3"
    out += [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 2, 0),
            (p + "_1", 768, 192, 1, 1, 0), (p + "_2", 192, 192, (1, 7), 1, (0, 3)), (p + "_3", 192, 192, (7, 1), 1, (3, 0)),
            (p + "_4", 192, 192, 3, 2, 0)]
    out += _block_e("Mixed_7b", 1280) + _block_e("Mixed_7c", 2048)
    return [(n, ci, co, mn.pair(k), s, mn.pair(p)) for n, ci, co, k, s, p in out]


def avg_pool3(x):
    """F.avg_pool2d(3, stride 1, padding 1, count_include_pad=False) of NHWC f32 x."""
    N, H, W, C = x.shape
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    lib.call("siss_inc_avgpool", x.contiguous(), out, N, H, W, C)
    return out


def global_avg(x):
    """[N, H, W, C] -> [N, C]: the mean over the pixels."""
    N, H, W, C = x.shape
    out = torch.empty(N, C, device=x.device, dtype=torch.float32)
    lib.call("siss_inc_global_avg", x.contiguous(), out, N, H * W, C)
    return out


def preprocess(imgs):
    """[N, 3, H, W] f32 in [0, 1] -> NHWC [N, 299, 299, 3] in [-1, 1): (imgs * 255).byte(), the TF1 bilinear resize, (x - 128) / 128."""
    N, C, H, W = imgs.shape
    if C != 3:
        raise ValueError(f"the FID Inception-v3 takes 3-channel images, got {tuple(imgs.shape)}")
    out = torch.empty(N, SIZE, SIZE, 3, device=imgs.device, dtype=torch.float32)
    lib.call("siss_inc_preprocess", imgs.to(torch.float32).contiguous(), out, N, H, W)
    return out


class InceptionV3FID(mn.MetricNet):
    """torch-fidelity's FeatureExtractorInceptionV3 (the network torchmetrics' FrechetInceptionDistance(feature=2048) runs) on the HIP
    kernels: `[N, 3, H, W]` f32 images in [0, 1] -> `[N, 2048]` pool features.  The parameters live on the host under the key names of
    pt_inception-2015-12-05-6726825d.pth (`<block>.<branch>.conv.weight`, `<block>.<branch>.bn.*`, `fc.*`; fc is loaded and checked
    but not run); `.to(device)` / the first call packs them (BN folded) onto the device."""

    ignored = (".num_batches_tracked",)         # a BatchNorm's counter, which eval mode never reads, is passed over

    def __init__(self):
        sd = OrderedDict()
        # He-normal convolutions under identity BatchNorms (activations stay O(1) through the 94 layers), drawn from a fork of the
        # global generator, so that building the metric leaves the global stream where it was
        with torch.random.fork_rng(devices=[]):
            for name, cin, cout, (kh, kw), _, _ in convs():
                sd[name + ".conv.weight"] = torch.empty(cout, cin, kh, kw).normal_(0, math.sqrt(2.0 / (kh * kw * cin)))
                sd[name + ".bn.weight"], sd[name + ".bn.bias"] = torch.ones(cout), torch.zeros(cout)
                sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = torch.zeros(cout), torch.ones(cout)
            bound = 1.0 / math.sqrt(FEATURES)
            sd["fc.weight"] = torch.empty(1008, FEATURES).uniform_(-bound, bound)
            sd["fc.bias"] = torch.empty(1008).uniform_(-bound, bound)
        super().__init__(sd)

    def _pack(self):
        """Per convolution the folded BN in f64, rounded once to f32 (metric_net.pack_conv)."""
        self._need_device()
        self._packed = {name: mn.pack_conv(*mn.fold_bn(self._sd, name + ".conv", name + ".bn", BN_EPS), stride, pad, self.device)
                        for name, _, _, _, stride, pad in convs()}

    # -- forward ---------------------------------------------------------------------------------
    def _out(self, x, c, stride=1):
        N, H, W, _ = x.shape
        Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if stride == 2 else (H, W)
        return torch.empty(N, Ho, Wo, c, device=self.device, dtype=torch.float32)

    def _chain(self, x, names, out=None, col=0):
        P = self._packed
        for n in names[:-1]:
            x = mn.conv(P[n], x)
        return mn.conv(P[names[-1]], x, out=out, col=col)

    def _a(self, name, x, pf):
        y, b = self._out(x, 224 + pf), name + ".branch"
        self._chain(x, [b + "1x1"], y, 0)
        self._chain(x, [b + "5x5_1", b + "5x5_2"], y, 64)
        self._chain(x, [b + "3x3dbl_1", b + "3x3dbl_2", b + "3x3dbl_3"], y, 128)
        self._chain(avg_pool3(x), [b + "_pool"], y, 224)
        return y

    def _b(self, name, x):
        y, b = self._out(x, 768, stride=2), name + ".branch"
        self._chain(x, [b + "3x3"], y, 0)
        self._chain(x, [b + "3x3dbl_1", b + "3x3dbl_2", b + "3x3dbl_3"], y, 384)
        mn.max_pool3(x, 2, 0, y, 480)
        return y

    def _c(self, name, x):
        y, b = self._out(x, 768), name + ".branch"
        self._chain(x, [b + "1x1"], y, 0)
        self._chain(x, [b + f"7x7_{i}" for i in (1, 2, 3)], y, 192)
        self._chain(x, [b + f"7x7dbl_{i}" for i in (1, 2, 3, 4, 5)], y, 384)
        self._chain(avg_pool3(x), [b + "_pool"], y, 576)
        return y

    def _d(self, name, x):
        y, b = self._out(x, 1280, stride=2), name + ".branch"
        self._chain(x, [b + "3x3_1", b + "3x3_2"], y, 0)
        self._chain(x, [b + f"7x7x3_{i}" for i in (1, 2, 3, 4)], y, 320)
        mn.max_pool3(x, 2, 0, y, 512)
        return y

    def _e(self, name, x, pooled):
        y, b, P = self._out(x, 2048), name + ".branch", self._packed
        self._chain(x, [b + "1x1"], y, 0)
        t = mn.conv(P[b + "3x3_1"], x)
        mn.conv(P[b + "3x3_2a"], t, out=y, col=320)
        mn.conv(P[b + "3x3_2b"], t, out=y, col=704)
        t = self._chain(x, [b + "3x3dbl_1", b + "3x3dbl_2"])
        mn.conv(P[b + "3x3dbl_3a"], t, out=y, col=1088)
        mn.conv(P[b + "3x3dbl_3b"], t, out=y, col=1472)
        self._chain(pooled, [b + "_pool"], y, 1856)
        return y

    def features(self, x):
        """The network proper: NHWC [N, 299, 299, 3] in [-1, 1) -> [N, 2048]."""
        if self._packed is None:
            self._pack()
        x = self._chain(x, ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"])
        x = mn.max_pool3(x, 2, 0)
        x = self._chain(x, ["Conv2d_3b_1x1", "Conv2d_4a_3x3"])
        x = mn.max_pool3(x, 2, 0)
        x = self._a("Mixed_5b", x, 32)
        x = self._a("Mixed_5c", x, 64)
        x = self._a("Mixed_5d", x, 64)
        x = self._b("Mixed_6a", x)
        for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._c(name, x)
        x = self._d("Mixed_7a", x)
        x = self._e("Mixed_7b", x, avg_pool3(x))
        x = self._e("Mixed_7c", x, mn.max_pool3(x, 1, 1))          # the FID variant: a MAX pool in the last block's pool branch
        return global_avg(x)

    @torch.no_grad()
    def __call__(self, imgs):
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"InceptionV3FID expects [N, 3, H, W] images in [0, 1], got {tuple(imgs.shape)}")
        self._need_device()
        if imgs.shape[0] == 0:
            return torch.empty(0, FEATURES, device=self.device)
        return self.features(preprocess(imgs.to(self.device, torch.float32)))

    forward = __call__


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """torchmetrics' _compute_fid: |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 sum(sqrt(eigvals(S1 S2)).real), f64; the eigenvalues on the
    host CPU (a general D x D matrix, a few seconds at D = 2048, once per evaluation)."""
    a = (mu1 - mu2).square().sum(dim=-1)
    b = sigma1.trace() + sigma2.trace()
    c = torch.linalg.eigvals((sigma1 @ sigma2).cpu()).sqrt().real.sum(dim=-1)
    return a.cpu() + b.cpu() - 2 * c


class FrechetInceptionDistance:
    """torchmetrics.image.fid.FrechetInceptionDistance(feature=2048, normalize=True, reset_real_features=False): per side the count,
    the f64 feature sum [D] and the f64 sum of outer products [D, D], held on `device` and updated there by one launcher call per
    batch.  `inception` maps [N, 3, H, W] images in [0, 1] to [N, D] features (None: update_features only).  `sink` (None: nothing
    changes) is called as sink(f, real) with every batch of features the statistics take (feature_sets.FeatureSets keeps them)."""

    def __init__(self, inception=None, num_features=FEATURES, device="cpu", sink=None):
        if num_features % 16:
            raise ValueError(f"num_features={num_features}: a multiple of 16 is needed")
        self.inception, self.num_features, self.device = inception, int(num_features), torch.device(device)
        self.sink = sink
        D = self.num_features
        for side in ("real", "fake"):
            setattr(self, side + "_features_sum", torch.zeros(D, dtype=torch.float64, device=self.device))
            setattr(self, side + "_features_cov_sum", torch.zeros(D, D, dtype=torch.float64, device=self.device))
            setattr(self, side + "_features_num_samples", 0)

    def update(self, imgs, real):
        """imgs: [N, 3, H, W] floats in [0, 1] (normalize=True)."""
        if self.inception is None:
            raise RuntimeError("FrechetInceptionDistance.update needs the feature extractor; update_features takes features")
        self.update_features(self.inception(imgs), real)

    def update_features(self, f, real):
        """f: [N, D] f32 features on the device: sum += f.sum(0), cov_sum += f^T f in f64, n += N."""
        if f.dim() != 2 or f.shape[1] != self.num_features:
            raise ValueError(f"expected [N, {self.num_features}] features, got {tuple(f.shape)}")
        if f.shape[0] == 0:
            return
        side = "real" if real else "fake"
        f = f.to(self.device, torch.float32).contiguous()
        lib.call("siss_fid_stats_update", f, f.shape[0], self.num_features, getattr(self, side + "_features_sum"),
                 getattr(self, side + "_features_cov_sum"))
        setattr(self, side + "_features_num_samples", getattr(self, side + "_features_num_samples") + int(f.shape[0]))
        if self.sink is not None:
            self.sink(f, real)

    def compute(self):
        n1, n2 = int(self.real_features_num_samples), int(self.fake_features_num_samples)
        if n1 < 2 or n2 < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        mean_real = (self.real_features_sum / n1).unsqueeze(0)
        mean_fake = (self.fake_features_sum / n2).unsqueeze(0)
        cov_real = (self.real_features_cov_sum - n1 * mean_real.t().mm(mean_real)) / (n1 - 1)
        cov_fake = (self.fake_features_cov_sum - n2 * mean_fake.t().mm(mean_fake)) / (n2 - 1)
        return frechet_distance(mean_real.squeeze(0), cov_real, mean_fake.squeeze(0), cov_fake).to(torch.float32)

    def reset(self):
        """reset_real_features=False: the fake side only."""
        self.fake_features_sum.zero_()
        self.fake_features_cov_sum.zero_()
        self.fake_features_num_samples = 0


class FIDEvaluator:
    """metrics/fid.py::FIDEvaluator.  Beyond the reference's arguments (keyword-only): inception_ckpt (None: DEFAULT_CKPT, the
    state dict torch-fidelity downloads), allow_random_init (a missing checkpoint is an error unless this is set), data_path (the
    directory load_celeb walks), real_stats_path (an .npz the real side's statistics are read from when it exists, written to
    after the pass otherwise) and feature_sets (a feature_sets.FeatureSets that receives the features the statistics take; None:
    nothing changes)."""

    def __init__(self, inception_batch_size, device, classifier=None, remove_class=None, filter_fake=True, *, inception_ckpt=None,
                 allow_random_init=False, data_path="data/examples/celeba_hq_256", real_stats_path=None, feature_sets=None):
        self.batch_size = int(inception_batch_size)
        if self.batch_size <= 0:
            raise ValueError(f"inception_batch_size={inception_batch_size!r}: a positive batch size is needed")
        self.device = torch.device(device)
        self.remove_class, self.classifier, self.filter_fake = remove_class, classifier, filter_fake
        self.data_path, self.real_stats_path = data_path, real_stats_path
        net = InceptionV3FID()
        ckpt = str(inception_ckpt or DEFAULT_CKPT)
        if os.path.isfile(ckpt):
            net.load_state_dict(torch.load(ckpt, map_location="cpu"))
        elif not allow_random_init:
            raise FileNotFoundError(f"inception_ckpt {ckpt!r} is not a file on disk (no network: torch-fidelity's weights cannot be "
                                    "fetched); pass allow_random_init=true for random-init weights of the same architecture instead")
        else:
            print(f"[siss_amd] allow_random_init: inception checkpoint {ckpt!r} not on disk, RANDOM-INIT Inception-v3: the FID "
                  "figures are NOT comparable with published ones")
        self.fid_computer = FrechetInceptionDistance(net.to(self.device).eval(), FEATURES, self.device, sink=feature_sets)
        self.feature_sets = feature_sets

    def load_cifar(self, limit=None):
        raise NotImplementedError("FIDEvaluator.load_cifar downloads CIFAR-10 (torchvision.datasets.CIFAR10(download=True)); there is "
                                  "no network here and the CIFAR experiment is not built: load_celeb is the real side")

    def load_real_stats(self, path):
        """The real side's (n, sum, cov_sum) from the .npz save_real_stats wrote."""
        import numpy as np
        fc = self.fid_computer
        with np.load(str(path)) as z:
            s, c = torch.from_numpy(z["sum"]), torch.from_numpy(z["cov_sum"])
            D = fc.num_features
            if s.dtype != torch.float64 or c.dtype != torch.float64 or tuple(s.shape) != (D,) or tuple(c.shape) != (D, D):
                raise ValueError(f"real_stats_path {path!r}: expected f64 sum [{D}] and cov_sum [{D}, {D}]")
            fc.real_features_sum.copy_(s)
            fc.real_features_cov_sum.copy_(c)
            fc.real_features_num_samples = int(z["n"])

    def save_real_stats(self, path):
        import numpy as np
        fc = self.fid_computer
        with open(str(path), "wb") as f:                 # (a handle: np.savez would append .npz to a name without it)
            np.savez(f, n=np.int64(fc.real_features_num_samples), sum=fc.real_features_sum.cpu().numpy(),
                     cov_sum=fc.real_features_cov_sum.cpu().numpy())

    def load_celeb(self):
        if self.feature_sets is not None:
            return self._load_celeb_with_sets()
        fc, path = self.fid_computer, self.real_stats_path
        if path and os.path.isfile(str(path)):
            self.load_real_stats(path)
            print(f"Loaded the FID real statistics of {fc.real_features_num_samples} images from {path}")
            return
        from .data import CelebAHQ, ToTensor
        print("Loading CelebAHQ as FID real examples...")
        ds = CelebAHQ("all", str(self.data_path), [], ToTensor())
        for s in range(0, len(ds), self.batch_size):
            batch = torch.stack([ds[i] for i in range(s, min(s + self.batch_size, len(ds)))])
            fc.update(batch.to(self.device), real=True)
        if path:
            self.save_real_stats(path)

    def _load_celeb_with_sets(self):
        """load_celeb with `feature_sets`: the real FEATURES come from its real_features_path when that file was written under this
        network's weights and these image files (names, sizes, mtimes); otherwise the pass over the images runs and writes it -- also
        when real_stats_path already supplies the FID's sums, which hold no features (the sums are then left as loaded)."""
        from .data import CelebAHQ, ToTensor
        from .feature_sets import FeatureBank, real_fingerprint
        fc, sets, path = self.fid_computer, self.feature_sets, self.real_stats_path
        have_stats = bool(path and os.path.isfile(str(path)))
        if have_stats:
            self.load_real_stats(path)
            print(f"Loaded the FID real statistics of {fc.real_features_num_samples} images from {path}")
        ds = CelebAHQ("all", str(self.data_path), [], ToTensor())
        fp = real_fingerprint(fc.inception, ds.paths)
        fpath = sets.real_features_path
        if fpath and FeatureBank.exists(fpath) and FeatureBank.matches(fpath, fp):
            sets.adopt_real(FeatureBank.load(fpath, fp, self.device))
            print(f"[siss_amd] metrics.fid.sets: {len(sets.real)} real feature rows loaded from {fpath}")
            if have_stats:
                return
            fc.sink = None                                   # the pass below feeds the statistics alone
        else:
            if fpath and FeatureBank.exists(fpath):
                print(f"[siss_amd] metrics.fid.sets: the features under {fpath} describe other weights or files: computed again")
            sets.open_real(len(ds))
        print("Loading CelebAHQ as FID real examples...")
        try:
            for s in range(0, len(ds), self.batch_size):
                batch = torch.stack([ds[i] for i in range(s, min(s + self.batch_size, len(ds)))]).to(self.device)
                if have_stats:
                    sets(fc.inception(batch), True)          # the sums are on file: the features alone
                else:
                    fc.update(batch, real=True)
        finally:
            loaded, fc.sink = fc.sink is None, sets
        if path and not have_stats:
            self.save_real_stats(path)
        if fpath and not loaded:
            sets.real.save(fpath, fp)

    def add_fake_images(self, fake_imgs):
        if self.remove_class is not None and self.filter_fake:
            preds = self.classifier.compute_logits(fake_imgs).argmax(-1)
            fake_imgs = fake_imgs[(preds != self.remove_class).to(fake_imgs.device)]
        for i in range(0, len(fake_imgs), self.batch_size):
            self.fid_computer.update(fake_imgs[i:i + self.batch_size], real=False)

    def compute(self, reset=True, verbose=False):
        t0 = time.time()
        fid_score = self.fid_computer.compute()
        if verbose:
            print(f"FID score: {fid_score}")
            print(f"Time taken for computing FID score: {time.time() - t0}")
        if reset:
            self.fid_computer.reset()
        return fid_score


class FIDTracker:
    """The FID part of delete_celeb.py's log_metrics (:532-542) for rank 0: at step 0 and every `step_frequency` steps, `num_images`
    samples in batches of `batch_size` -- `sample(n)` returns [n, 3, H, W] images in [0, 1] on the device -- each batch handed to
    add_fake_images as it is produced (the statistics are additive: the result is the reference's all-at-once one, without holding
    the images); `begin()` / `end()` bracket an evaluation's batches.  One JSON line per evaluation: {global_step, fid, fake_images, real_images, seconds}.
    `sets` (a feature_sets.FeatureSets; None: the record is exactly the one above) adds the KID and precision / recall / density /
    coverage of the same features: NOT the reference's protocol, which reports FID only."""

    def __init__(self, evaluator, out_path, sample, step_frequency, num_images, batch_size, begin=None, end=None, sets=None):
        self.sets = sets
        self.evaluator, self.out_path, self.sample, self.begin, self.end = evaluator, out_path, sample, begin, end
        self.step_frequency, self.num_images, self.batch_size = int(step_frequency), int(num_images), int(batch_size)
        self.extra = None                                # fields added to every record (pipeline.sampler: name and step count)

    def __call__(self, global_step):
        if global_step % self.step_frequency:
            return None
        t0 = time.perf_counter()
        fc = self.evaluator.fid_computer
        fc.reset()
        if self.sets is not None:
            self.sets.begin()
        if self.begin is not None:
            self.begin()                                 # (`begin()` runs before an evaluation's first batch)
        try:
            for s in range(0, self.num_images, self.batch_size):
                self.evaluator.add_fake_images(self.sample(min(self.batch_size, self.num_images - s)))
        finally:
            if self.end is not None:
                self.end()                               # (`end()` after the last batch: the sampler's buffers go before training resumes)
        fake, real = int(fc.fake_features_num_samples), int(fc.real_features_num_samples)
        fid = float(self.evaluator.compute(reset=True))
        rec = {"global_step": int(global_step), "fid": finite_or_none(fid), "fake_images": fake, "real_images": real,
               "seconds": time.perf_counter() - t0, **(self.extra or {})}
        if self.sets is not None:
            rec.update(self.sets.evaluate())
        print(f"FID: {fid}")
        return append_jsonl(self.out_path, rec)

"""The SD experiment's copy-detection score (delete_sd.py:226-228,:277-283): the SSCD network -- `sscd_disc_mixup.torchscript.pt`, a
torchvision-layout ResNet-50 (Bottleneck [3, 4, 6, 3], the stride on the 3 x 3 conv2, BN eps 1e-5) whose average pool is GeM pooling
(p = 3, eps 1e-6), whose fc is a 2048 -> dims linear layer, followed by F.normalize -- on the HIP kernels: the trunk and fc on
metric_conv.hip's implicit-GEMM convolution (fc as a 1 x 1 convolution on a 1 x 1 map), the preprocessing, GeM pooling and the
normalisation with the score on csrc/sscd.hip.  `SSCDScore` is the tracker the task loop drives.

The network runs in f32, in eval mode (BatchNorm folded into the convolutions at pack time in f64); the reference runs it under
torch.autocast (fp16) -- a deliberate deviation, as for every metric network here.  There is no CPU path: a missing kernel library
raises.  Neither the checkpoint nor torchvision was available when this was written: the architecture is restated from its public
description (tests/sscd_ref.py is the same restatement in torch.nn); tools/check_sscd.py is the check for whoever has the file.
"""
import math
from collections import OrderedDict

import torch

from . import lib
from . import metric_net as mn
from .records import append_jsonl, finite_or_none

BN_EPS = 1e-5
BLOCKS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
FEATURES = 2048
GEM_EPS = 1e-6              # GlobalGeMPool2d's clamp
NORM_EPS = 1e-12            # F.normalize's default
_ALIASES = {"embeddings.1.weight": "backbone.fc.weight", "embeddings.1.bias": "backbone.fc.bias"}


def _convs():
    """(prefix, Cin, Cout, k, stride, pad, bn prefix) of every convolution, in torch's state-dict order (without `backbone.`)."""
    out = [("conv1", 3, 64, 7, 2, 3, "bn1")]
    inp = 64
    for i, (w, n) in enumerate(zip(WIDTHS, BLOCKS), 1):
        for j in range(n):
            s = 2 if (i > 1 and j == 0) else 1
            p = f"layer{i}.{j}."
            out.append((p + "conv1", inp, w, 1, 1, 0, p + "bn1"))
            out.append((p + "conv2", w, w, 3, s, 1, p + "bn2"))            # the stride sits on the 3 x 3 (torchvision's ResNet v1.5)
            out.append((p + "conv3", w, 4 * w, 1, 1, 0, p + "bn3"))
            if j == 0:
                out.append((p + "downsample.0", inp, 4 * w, 1, s, 0, p + "downsample.1"))
            inp = 4 * w
    return out


def _three(v, what):
    v = [float(x) for x in (v if isinstance(v, (list, tuple)) else [v])]
    if len(v) == 1:
        v = v * 3
    if len(v) != 3:
        raise ValueError(f"{what}: one or three values are needed, got {len(v)}")
    return v


class SSCDModel(mn.ChunkedImageNet):
    """The SSCD ResNet-50: `[N, 3, H, W]` f32 images, already normalised -> `[N, dims]` unit rows on the device.  The parameters live
    on the host under torchvision's key names with the prefix `backbone.`; `.to(device)` / the first call packs them (BN folded)
    onto the device.  Images are embedded in chunks of `batch_size`."""

    def __init__(self, dims=512, pool_param=3.0, batch_size=16):
        self.dims, self.pool_param, self.batch_size = int(dims), float(pool_param), int(batch_size)
        if self.dims <= 0 or self.pool_param <= 0 or self.batch_size <= 0:
            raise ValueError(f"SSCDModel(dims={dims!r}, pool_param={pool_param!r}, batch_size={batch_size!r}): positive values are needed")
        sd = OrderedDict()
        # torchvision's constructor: conv kaiming_normal_(fan_out, relu), BN weight 1 / bias 0 (stats 0 / 1), nn.Linear's default for
        # fc; drawn from a fork of the global generator, so that building the metric leaves the global stream where it was
        with torch.random.fork_rng(devices=[]):
            for name, cin, cout, k, _, _, bn in _convs():
                sd["backbone." + name + ".weight"] = torch.empty(cout, cin, k, k).normal_(0, math.sqrt(2.0 / (k * k * cout)))
                b = "backbone." + bn
                sd[b + ".weight"], sd[b + ".bias"] = torch.ones(cout), torch.zeros(cout)
                sd[b + ".running_mean"], sd[b + ".running_var"] = torch.zeros(cout), torch.ones(cout)
                sd[b + ".num_batches_tracked"] = torch.tensor(0)
            bound = 1.0 / math.sqrt(FEATURES)
            sd["backbone.fc.weight"] = torch.empty(self.dims, FEATURES).uniform_(-bound, bound)
            sd["backbone.fc.bias"] = torch.empty(self.dims).uniform_(-bound, bound)
        super().__init__(sd)    # (filled in torch's order: a convolution, then its BN; fc last)

    @classmethod
    def load(cls, path, pool_param=3.0, batch_size=16):
        """The network of a checkpoint file: a TorchScript archive (`torch.jit.load(path).state_dict()`, the form SSCD is published
        in), else a `torch.load` state dict, else -- when the file is not a zip archive -- a `.safetensors` file.  The linear layer
        is taken as `backbone.fc.{weight,bias}` or as `embeddings.1.{weight,bias}`; its rows give `dims`.  Any other key set (a
        ClassyVision-style trunk among them) raises RuntimeError with the missing and unexpected keys."""
        sd = mn.read_state_dict(path, "SSCD")
        clash = [a for a, k in _ALIASES.items() if a in sd and k in sd]
        if clash:
            raise RuntimeError(f"{path}: the linear layer is there twice ({clash} beside backbone.fc.*)")
        sd = OrderedDict((_ALIASES.get(k, k), v) for k, v in sd.items())
        fc = sd.get("backbone.fc.weight")
        dims = int(fc.shape[0]) if fc is not None and fc.dim() == 2 else 512
        net = cls(dims=dims, pool_param=pool_param, batch_size=batch_size)
        try:
            net.load_state_dict(sd)
        except RuntimeError as e:
            raise RuntimeError(f"{path} is not a torchvision-layout SSCD ResNet-50: {e}") from e
        return net.eval()

    # -- packing ---------------------------------------------------------------------------------
    def _pack(self):
        self._need_device()
        sd = self._sd
        layers = {}
        for name, _, _, _, s, p, bn in _convs():
            layers[name] = mn.pack_conv(*mn.fold_bn(sd, "backbone." + name, "backbone." + bn, BN_EPS), s, p, self.device)
        layers["fc"] = mn.pack_conv(sd["backbone.fc.weight"].double().view(self.dims, FEATURES, 1, 1), sd["backbone.fc.bias"].double(),
                                    1, 0, self.device)
        self._packed = layers

    def max_elements(self, N, H, W):
        """The largest tensor (input, activation or split-K slab, in elements) a chunk of N images of H x W touches."""
        if self._packed is None:
            self._pack()
        P = self._packed
        big = N * 3 * H * W

        def after(L, H, W):
            nonlocal big
            Ho, Wo = mn.conv_out(L, H, W)
            M = N * Ho * Wo
            big = max(big, M * L["cout"] * mn.conv_splits(M, L["cout"], L["Kp"]))
            return Ho, Wo
        H, W = after(P["conv1"], H, W)
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for i, n in enumerate(BLOCKS, 1):
            for j in range(n):
                pre = f"layer{i}.{j}."
                if j == 0:
                    after(P[pre + "downsample.0"], H, W)
                Ha, Wa = after(P[pre + "conv1"], H, W)
                H, W = after(P[pre + "conv2"], Ha, Wa)
                after(P[pre + "conv3"], H, W)
        return big

    # -- forward ---------------------------------------------------------------------------------
    def _features(self, x):
        """One chunk: the normalised NCHW images -> the raw (not yet normalised) fc rows [n, dims]."""
        N, H, W = self._chunk_shape(x)
        P = self._packed
        h = mn.max_pool3(mn.conv(P["conv1"], x, nchw_in=True), 2, 1)
        for i, n in enumerate(BLOCKS, 1):
            for j in range(n):
                pre = f"layer{i}.{j}."
                sc = mn.conv(P[pre + "downsample.0"], h, relu=False) if j == 0 else h
                a = mn.conv(P[pre + "conv2"], mn.conv(P[pre + "conv1"], h))
                h = mn.conv(P[pre + "conv3"], a, res=sc)
        pooled = torch.empty(N, FEATURES, device=self.device, dtype=torch.float32)
        lib.call("siss_sscd_gem", h, pooled, N, h.shape[1] * h.shape[2], FEATURES, self.pool_param, GEM_EPS)
        return mn.linear(P["fc"], pooled)

    def _finish(self, rows, ref):
        """(unit rows, scores against the unit row `ref` or None) of raw fc rows."""
        n = rows.shape[0]
        score = None
        if ref is not None:
            ref = ref.to(self.device, torch.float32).reshape(-1).contiguous()
            if ref.numel() != self.dims:
                raise ValueError(f"a reference row of {ref.numel()} values, embeddings of {self.dims}")
            score = torch.empty(n, device=self.device, dtype=torch.float32)
        lib.call("siss_sscd_normalize_score", rows, n, self.dims, NORM_EPS, ref, rows, score)
        return rows, score

    def _run(self, src, form, mean, std, ref):
        """Chunks of batch_size through (preprocess ->) trunk -> GeM -> fc -> normalise: (embeddings, scores or None, uint8 or None)."""
        return self._chunks(src, form, mean, std, lambda rows: self._finish(rows, ref))

    def __call__(self, x, ref=None):
        """`[N, 3, H, W]` f32, already normalised (the reference's call form) -> `[N, dims]` unit rows; with `ref` (a unit row)
        -> (rows, their cosines with it [N])."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"SSCDModel expects [N, 3, H, W] images, got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        emb, scores, _ = self._run(x.to(self.device, torch.float32), None, None, None, ref)
        return emb if ref is None else (emb, scores)

    forward = __call__

    def embed_u8(self, u8, mean=(0.0,), std=(1.0,), ref=None):
        """uint8 images `[n, H, W, 3]` -> unit rows of Normalize(mean, std)(ToTensor(image)), the preprocessing fused into one launch
        (bitwise torch's f32 chain); with `ref` -> (rows, scores)."""
        emb, scores, _ = self._run(self._check_u8(u8), 0, _three(mean, "mean"), _three(std, "std"), ref)
        return emb if ref is None else (emb, scores)

    def embed_decoded(self, img, mean=(0.0,), std=(1.0,), ref=None):
        """The VAE decoder's output `[n, 3, H, W]` (f32 or bf16, on the device) -> (unit rows, the uint8 images `[n, H, W, 3]`
        -- bitwise `kmeans.from_decoded`'s -- ) in one preprocessing launch per chunk; with `ref` -> (rows, uint8, scores)."""
        emb, scores, u8 = self._run(img, self._check_decoded(img), _three(mean, "mean"), _three(std, "std"), ref)
        return (emb, u8) if ref is None else (emb, u8, scores)


class SSCDScore:
    """delete_sd.py:277-283 for one rank: the cosine of the memorized image's embedding with each validation image's.  The memorized
    image's embedding is computed once (the metric network never changes).  `record(prompt, scores, step)` appends {global_step,
    sscd_<i>} to `out_path`, the value the mean of the scores in f64 on the host (the reference's `sscd_scores.mean().item()`)."""

    def __init__(self, model, mem_img_path, out_path, mean=(0.0,), std=(1.0,)):
        self.model, self.mem_img_path, self.out_path = model, str(mem_img_path), out_path
        self.mean, self.std = _three(mean, "mean"), _three(std, "std")
        self._ref = None

    def reference(self, device):
        """The unit embedding [dims] of `Normalize(ToTensor(Image.open(mem_img_path).convert('RGB')))`, on the device."""
        if self._ref is None or self._ref.device != torch.device(device):
            import numpy as np
            from PIL import Image
            u8 = torch.from_numpy(np.asarray(Image.open(self.mem_img_path).convert("RGB"), dtype=np.uint8).copy())[None]
            self._ref = self.model.to(device).eval().embed_u8(u8, self.mean, self.std)[0].clone()
        return self._ref

    def score_u8(self, u8):
        """Scores [n] (device) of uint8 images [n, H, W, 3]."""
        ref = self.reference(u8.device if torch.is_tensor(u8) and u8.is_cuda else self.model.device)
        return self.model.embed_u8(u8, self.mean, self.std, ref=ref)[1]

    def score_decoded(self, img):
        """(scores [n], uint8 images [n, H, W, 3]), both on the device, of the decoder's output."""
        _, u8, scores = self.model.embed_decoded(img, self.mean, self.std, ref=self.reference(img.device))
        return scores, u8

    extra = None                # fields added to every record (pipeline.sampler: the sampler's name and step count)

    def record(self, prompt, scores, step):
        return mn.record_mean(self.out_path, f"sscd_{prompt}", scores, step, self.extra)


class InjectionScore(SSCDScore):
    """The inject-then-denoise check of the pixel-space tasks as numbers (the paper's SSCD similarity for CelebA-HQ; the reference
    only logs the image grid, delete_celeb.py:404-436,:500-503, and scores offline): the cosine of the forget image's embedding with
    each denoised injection's, both taken from uint8 bytes -- the PNG grid's own -- as an offline scorer would read them.
    `record(scores, step, timestep)` appends {global_step, timestep, sscd_mean, sscd_max, sscd} to `out_path`, the mean in f64 on
    the host."""

    def record(self, scores, step, timestep):
        s = torch.as_tensor(scores).detach().cpu().double().reshape(-1)
        return append_jsonl(self.out_path, {"global_step": int(step), "timestep": int(timestep), "sscd_mean": finite_or_none(s.mean()),
                                            "sscd_max": finite_or_none(s.max()), "sscd": [finite_or_none(v) for v in s.tolist()]})

"""The SD experiment's copy-detection score (delete_sd.py:226-228,:277-283): the SSCD network -- `sscd_disc_mixup.torchscript.pt`, a
torchvision-layout ResNet-50 (Bottleneck [3, 4, 6, 3], the stride on the 3 x 3 conv2, BN eps 1e-5) whose average pool is GeM pooling
(p = 3, eps 1e-6), whose fc is a 2048 -> dims linear layer, followed by F.normalize -- on the HIP kernels: the trunk and fc on
classifier.hip's implicit-GEMM convolution (fc as a 1 x 1 convolution on a 1 x 1 map), the preprocessing, GeM pooling and the
normalisation with the score on csrc/sscd.hip.  `SSCDScore` is the tracker the task loop drives.

The network runs in f32, in eval mode (BatchNorm folded into the convolutions at pack time in f64); the reference runs it under
torch.autocast (fp16) -- a deliberate deviation, as for every metric network here.  There is no CPU path: a missing kernel library
raises.  Neither the checkpoint nor torchvision was available when this was written: the architecture is restated from its public
description (tests/sscd_ref.py is the same restatement in torch.nn); tools/check_sscd.py is the check for whoever has the file.
"""
import json
import math
import os
import zipfile
from collections import OrderedDict

import torch

from . import lib
from .classifier import conv_out, conv_splits, fold_bn, max_pool, pack_conv, run_conv

BLOCKS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
FEATURES = 2048
GEM_EPS = 1e-6              # GlobalGeMPool2d's clamp
NORM_EPS = 1e-12            # F.normalize's default
MAX_ELEMENTS = 1 << 31      # an activation (or split-K slab) of a chunk stays below this many elements
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


class SSCDModel:
    """The SSCD ResNet-50: `[N, 3, H, W]` f32 images, already normalised -> `[N, dims]` unit rows on the device.  The parameters live
    on the host under torchvision's key names with the prefix `backbone.`; `.to(device)` / the first call packs them (BN folded)
    onto the device.  Images are embedded in chunks of `batch_size`."""

    def __init__(self, dims=512, pool_param=3.0, batch_size=16):
        self.dims, self.pool_param, self.batch_size = int(dims), float(pool_param), int(batch_size)
        if self.dims <= 0 or self.pool_param <= 0 or self.batch_size <= 0:
            raise ValueError(f"SSCDModel(dims={dims!r}, pool_param={pool_param!r}, batch_size={batch_size!r}): positive values are needed")
        self.device = torch.device("cpu")
        self.training = False
        self._packed = None
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
        self._sd = sd           # (filled in torch's order: a convolution, then its BN; fc last)

    # -- the nn.Module surface -------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device, self._packed = device, None
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("SSCDModel runs in eval mode only (BatchNorm folded into the convolutions); the reference "
                                      "loads a TorchScript archive exported in eval mode")
        return self.eval()

    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def load_state_dict(self, sd, strict=True):
        """Strict over the key names; only `num_batches_tracked` may be missing.  Missing / unexpected keys or a wrong shape raise."""
        want = self._sd
        got = {k: v for k, v in sd.items()}
        missing = [k for k in want if k not in got and not k.endswith("num_batches_tracked")]
        unexpected = [k for k in got if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"SSCDModel.load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in got.items():
            if tuple(v.shape) != tuple(want[k].shape):
                raise RuntimeError(f"SSCDModel.load_state_dict: {k} has shape {tuple(v.shape)}, the model {tuple(want[k].shape)}")
        new = OrderedDict()
        for k, v in want.items():
            src = got.get(k, v)
            new[k] = src.detach().to("cpu", torch.long if k.endswith("num_batches_tracked") else torch.float32).clone()
        self._sd = new
        self._packed = None
        return None

    @classmethod
    def load(cls, path, pool_param=3.0, batch_size=16):
        """The network of a checkpoint file: a TorchScript archive (`torch.jit.load(path).state_dict()`, the form SSCD is published
        in), else a `torch.load` state dict, else -- when the file is not a zip archive -- a `.safetensors` file.  The linear layer
        is taken as `backbone.fc.{weight,bias}` or as `embeddings.1.{weight,bias}`; its rows give `dims`.  Any other key set (a
        ClassyVision-style trunk among them) raises RuntimeError with the missing and unexpected keys."""
        path = str(path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"SSCD checkpoint {path!r} is not a file on disk")
        if zipfile.is_zipfile(path):
            try:
                sd = torch.jit.load(path, map_location="cpu").state_dict()
            except RuntimeError:                        # a zip archive without TorchScript code: torch.save's format
                sd = torch.load(path, map_location="cpu")
        else:
            try:
                from safetensors.torch import load_file
                sd = load_file(path, device="cpu")
            except Exception as e:
                raise RuntimeError(f"{path}: neither a TorchScript / torch.save archive nor a .safetensors file ({e})") from e
        if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
            raise RuntimeError(f"{path}: a state dict of tensors is needed, got {type(sd).__name__}")
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
        if self.device.type != "cuda":
            raise RuntimeError("SSCDModel: call .to(<cuda device>) first -- the network runs on the HIP kernels only")
        sd = self._sd
        layers = {}
        for name, _, _, _, s, p, bn in _convs():
            layers[name] = pack_conv(*fold_bn(sd, "backbone." + name, "backbone." + bn), s, p, self.device)
        layers["fc"] = pack_conv(sd["backbone.fc.weight"].double().view(self.dims, FEATURES, 1, 1), sd["backbone.fc.bias"].double(),
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
            Ho, Wo = conv_out(L, H, W)
            M = N * Ho * Wo
            big = max(big, M * L["cout"] * conv_splits(M, L["cout"], L["Kp"]))
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
        N, _, H, W = x.shape
        if H < 1 or W < 1:
            raise ValueError(f"SSCDModel: empty images {tuple(x.shape)}")
        big = self.max_elements(N, H, W)
        if big >= MAX_ELEMENTS:
            raise ValueError(f"SSCDModel: a chunk of {N} images of {H} x {W} holds a tensor of {big} elements, 2^31 or more: lower "
                             f"batch_size (now {self.batch_size})")
        P = self._packed
        h, H, W = run_conv(P["conv1"], x, N, H, W, relu=True, nchw_in=True)
        h, H, W = max_pool(h, N, H, W, 64)
        for i, n in enumerate(BLOCKS, 1):
            for j in range(n):
                pre = f"layer{i}.{j}."
                sc = run_conv(P[pre + "downsample.0"], h, N, H, W, relu=False)[0] if j == 0 else h
                a, Ha, Wa = run_conv(P[pre + "conv1"], h, N, H, W, relu=True)
                a, H, W = run_conv(P[pre + "conv2"], a, N, Ha, Wa, relu=True)
                h, H, W = run_conv(P[pre + "conv3"], a, N, H, W, relu=True, res=sc)
        pooled = torch.empty(N, FEATURES, device=self.device, dtype=torch.float32)
        lib.call("siss_sscd_gem", h, pooled, N, H * W, FEATURES, self.pool_param, GEM_EPS)
        return run_conv(P["fc"], pooled.view(N, 1, 1, FEATURES), N, 1, 1, relu=False)[0].view(N, self.dims)

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

    def _preprocess(self, src, form, mean, std, want_u8):
        n = src.shape[0]
        h, w = (src.shape[1], src.shape[2]) if form == 0 else (src.shape[2], src.shape[3])
        x = torch.empty(n, 3, h, w, device=self.device, dtype=torch.float32)
        u8 = torch.empty(n, h, w, 3, device=self.device, dtype=torch.uint8) if want_u8 else None
        lib.call("siss_sscd_preprocess", src, form, n, h, w, *mean, *std, u8, x)
        return x, u8

    @torch.no_grad()
    def _run(self, src, form, mean, std, ref):
        """Chunks of batch_size through (preprocess ->) trunk -> GeM -> fc -> normalise: (embeddings, scores or None, uint8 or None)."""
        if self._packed is None:
            self._pack()
        n = src.shape[0]
        if n == 0:
            raise ValueError("SSCDModel: no images")
        emb, scores, u8s = [], [], []
        for s in range(0, n, self.batch_size):
            part = src[s:s + self.batch_size].contiguous()
            u8 = None
            if form is not None:
                part, u8 = self._preprocess(part, form, mean, std, want_u8=form != 0)
            e, sc = self._finish(self._features(part), ref)
            emb.append(e)
            scores.append(sc)
            u8s.append(u8)
        cat = lambda xs: None if xs[0] is None else (xs[0] if len(xs) == 1 else torch.cat(xs))
        return cat(emb), cat(scores), cat(u8s)

    def __call__(self, x, ref=None):
        """`[N, 3, H, W]` f32, already normalised (the reference's call form) -> `[N, dims]` unit rows; with `ref` (a unit row)
        -> (rows, their cosines with it [N])."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"SSCDModel expects [N, 3, H, W] images, got {tuple(getattr(x, 'shape', ()))}")
        if self.device.type != "cuda":
            raise RuntimeError("SSCDModel: call .to(<cuda device>) first -- the network runs on the HIP kernels only")
        emb, scores, _ = self._run(x.to(self.device, torch.float32), None, None, None, ref)
        return emb if ref is None else (emb, scores)

    forward = __call__

    def embed_u8(self, u8, mean=(0.0,), std=(1.0,), ref=None):
        """uint8 images `[n, H, W, 3]` -> unit rows of Normalize(mean, std)(ToTensor(image)), the preprocessing fused into one launch
        (bitwise torch's f32 chain); with `ref` -> (rows, scores)."""
        u8 = torch.as_tensor(u8)
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError(f"uint8 images [n, H, W, 3] are needed, got {u8.dtype} {tuple(u8.shape)}")
        if self.device.type != "cuda":
            raise RuntimeError("SSCDModel: call .to(<cuda device>) first -- the network runs on the HIP kernels only")
        emb, scores, _ = self._run(u8.to(self.device), 0, _three(mean, "mean"), _three(std, "std"), ref)
        return emb if ref is None else (emb, scores)

    def embed_decoded(self, img, mean=(0.0,), std=(1.0,), ref=None):
        """The VAE decoder's output `[n, 3, H, W]` (f32 or bf16, on the device) -> (unit rows, the uint8 images `[n, H, W, 3]`
        -- bitwise `kmeans.from_decoded`'s -- ) in one preprocessing launch per chunk; with `ref` -> (rows, uint8, scores)."""
        if not (torch.is_tensor(img) and img.is_cuda and img.dim() == 4 and img.shape[1] == 3):
            raise ValueError("the decoder's output [n, 3, H, W] on the device is needed")
        if img.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"decoder output of dtype {img.dtype}: float32 or bfloat16")
        if img.device != self.device:
            raise ValueError(f"decoder output on {img.device}, the network on {self.device}")
        emb, scores, u8 = self._run(img, 2 if img.dtype == torch.bfloat16 else 1, _three(mean, "mean"), _three(std, "std"), ref)
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

    def record(self, prompt, scores, step):
        value = float(torch.as_tensor(scores).detach().cpu().double().mean())
        rec = {"global_step": int(step), f"sscd_{prompt}": value if math.isfinite(value) else None}
        with open(self.out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        return rec

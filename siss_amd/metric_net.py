"""The host side that the four f32, eval-only, BN-folded metric networks share -- the MNIST ResNet-18 (classifier.py), the FID
Inception-v3 (fid.py), the SSCD ResNet-50 (sscd.py) and the CLIP RN50 (clip_iqa.py) -- over the convolution and max pool of
csrc/metric_conv.hip: the BN fold and the weight packing, the split-K choice, the two launches, the checkpoint-file reader, the
nn.Module surface with its strict state dict (`MetricNet`) and the chunked run over images (`ChunkedImageNet`).  What is a network's
own -- layer tables, init, forward wiring, its own kernels -- stays in its module.  There is no CPU path: a missing kernel library raises.
"""
import os
import zipfile
from collections import OrderedDict

import torch

from . import lib
from .records import append_jsonl, finite_or_none

BK = 32                     # K step of metric_conv_kernel: input channel strides and packed weight rows are multiples of it


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def padded(c):
    """The channel stride a C-channel activation is carried with: C itself for an image, else the next multiple of the K step."""
    return c if c <= 4 else -(-c // BK) * BK


def fold_bn(sd, conv, bn, eps):
    """(w', b') in f64 of the convolution `conv` followed by the eval-mode BatchNorm `bn` of the state dict `sd`:
    w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps)."""
    w = sd[conv + ".weight"].double()
    scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + eps)
    b = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale
    return w * scale.view(-1, 1, 1, 1), b


def pack_conv(w, b, stride, pad, device):
    """A packed layer from f64 / f32 conv weights [Cout, Cin, KH, KW] and bias [Cout] (BN already folded), each rounded once to f32:
    the weights as [Cout][Kp] in (kh, kw, ci) order over the padded channel stride (zero weights on the padding), Kp % 32 == 0."""
    cout, cin, kh, kw = w.shape
    cp = padded(cin)
    K = kh * kw * cp
    Kp = -(-K // BK) * BK
    wp = torch.zeros(cout, kh, kw, cp, dtype=torch.float32)
    wp[..., :cin] = w.permute(0, 2, 3, 1).float()
    wk = torch.zeros(cout, Kp, dtype=torch.float32)
    wk[:, :K] = wp.reshape(cout, K)
    ph, pw = pair(pad)
    return dict(w=wk.to(device), b=b.float().to(device), cin=cin, cin_p=cp, cout=cout, cout_p=padded(cout), kh=kh, kw=kw,
                stride=int(stride), ph=ph, pw=pw, Kp=Kp)


def conv_out(L, H, W):
    return (H + 2 * L["ph"] - L["kh"]) // L["stride"] + 1, (W + 2 * L["pw"] - L["kw"]) // L["stride"] + 1


def conv_splits(M, cout, Kp):
    """Split-K factor of one convolution: 1 when the 64 x 64 tiles number at least 128, else enough splits for up to 256 blocks -- one
    per CU of an MI355X -- with at least 4 K steps per split (the late layers / fc at small N, Inception's 17 x 17 and 8 x 8 maps).
    128 and 256 rest on the CU count alone: no sweep has been run for these shapes."""
    steps = Kp // BK
    blocks = -(-M // 64) * -(-cout // 64)
    return 1 if blocks >= 128 else max(1, min(steps // 4, -(-256 // blocks)))


def conv(L, x, relu=True, res=None, out=None, col=0, nchw_in=False):
    """conv(x) + bias (+ res) (ReLU when relu) of a packed layer, written into out[..., col:col + Cout] (a fresh [N, Ho, Wo, padded
    Cout] buffer of x's dtype, zero beyond Cout, when out is None).  x: NHWC [N, H, W, C] (C the layer's Cin or its padded stride), or
    the NCHW image when nchw_in; res: NHWC [N, Ho, Wo, Cout], only into a buffer of that width.  Returns the buffer."""
    if nchw_in:
        N, C, H, W = x.shape
    else:
        N, H, W, C = x.shape
    cin_p, cout, stride, kh, kw, ph, pw = L["cin_p"], L["cout"], L["stride"], L["kh"], L["kw"], L["ph"], L["pw"]
    if C != cin_p:
        if C != L["cin"] or nchw_in:
            raise ValueError(f"conv: the input has {C} channels, the layer {L['cin']} (carried as {cin_p})")
        x = torch.nn.functional.pad(x, (0, cin_p - C))
    if not x.is_contiguous():
        x = x.contiguous()
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    if out is None:
        ldy = L["cout_p"]
        out = (torch.empty if ldy == cout else torch.zeros)(N, Ho, Wo, ldy, device=x.device, dtype=x.dtype)
    else:
        ldy = out.shape[3]
        if tuple(out.shape[:3]) != (N, Ho, Wo) or not out.is_contiguous() or col < 0 or col + cout > ldy:
            raise ValueError(f"conv: output {tuple(out.shape)} does not take {(N, Ho, Wo, cout)} at column {col}")
    M = N * Ho * Wo
    splits = conv_splits(M, cout, L["Kp"])
    ws = torch.empty(splits * M * cout, device=x.device, dtype=x.dtype) if splits > 1 else None
    lib.call("siss_metric_conv", x, nchw_in, L["w"], L["b"], res, out, ws, 0 if ws is None else ws.numel(), N, H, W, cin_p,
             Ho, Wo, cout, kh, kw, stride, ph, pw, L["Kp"], ldy, col, relu, splits)
    return out


def linear(L, rows):
    """A packed 1 x 1 layer as the linear layer it is: rows [n, Cin] -> [n, Cout] (a convolution on a 1 x 1 map, no ReLU)."""
    n = rows.shape[0]
    out = torch.empty(n, 1, 1, L["cout"], device=rows.device, dtype=rows.dtype)
    return conv(L, rows.view(n, 1, 1, -1), relu=False, out=out).view(n, L["cout"])


def max_pool3(x, stride, pad, out=None, col=0):
    """3 x 3 max pool of NHWC f32 x into out[..., col:col + C] (a fresh buffer when None)."""
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    if out is None:
        out = torch.empty(N, Ho, Wo, C, device=x.device, dtype=x.dtype)
    if tuple(out.shape[:3]) != (N, Ho, Wo) or not out.is_contiguous() or col < 0 or col + C > out.shape[3]:
        raise ValueError(f"max_pool3: output {tuple(out.shape)} does not take {(N, Ho, Wo, C)} at column {col}")
    lib.call("siss_metric_maxpool3", x.contiguous(), out, N, H, W, C, Ho, Wo, stride, pad, out.shape[3], col)
    return out


def read_state_dict(path, what):
    """The state dict of a checkpoint file of the `what` network: a TorchScript archive (`torch.jit.load(path).state_dict()`), else a
    `torch.load` state dict, else -- when the file is not a zip archive -- a `.safetensors` file."""
    path = str(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{what} checkpoint {path!r} is not a file on disk")
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
    return sd


def record_mean(out_path, key, scores, step, extra=None):
    """Append {global_step, key: the mean of the scores in f64 on the host (null when not finite)} to `out_path`; returns the record.
    extra: fields added to it (the sampler's name and step count when the images came from the opt-in pipeline.sampler)."""
    value = torch.as_tensor(scores).detach().cpu().double().mean()
    return append_jsonl(out_path, {"global_step": int(step), key: finite_or_none(value), **(extra or {})})


def score_chain(scorers, img):
    """The scorers that share one set of uint8 bytes, in their order, on one decoder output: the first makes the bytes with its fused
    `score_decoded(img) -> (result, u8)`, every later one takes them through `score_u8(u8) -> result` (one fused entry, the `_u8`
    entry for the rest).  Returns ([result per scorer], u8).  The methods are looked up now, at the call."""
    first, u8 = scorers[0].score_decoded(img)
    return [first] + [s.score_u8(u8) for s in scorers[1:]], u8


def _named(k, names):
    """Whether the key `k` is one of `names`: an entry that starts with a dot is a suffix, any other the whole key."""
    return any(k.endswith(n) if n.startswith(".") else k == n for n in names)


class MetricNet:
    """The nn.Module surface of an eval-only network on the HIP kernels: the parameters live on the host in `_sd` under the
    checkpoint's key names; `.to(device)` / the first call packs them (BN folded) onto the device (`_pack()`, the subclass's).
    `optional_missing`: keys load_state_dict accepts the absence of; `ignored`: keys it drops from its input unless the model has them."""

    optional_missing = (".num_batches_tracked",)
    ignored = ()

    def __init__(self, sd):
        self.device = torch.device("cpu")
        self.training = False
        self._sd = sd
        self._dropped()

    def _dropped(self):
        """The packed layers no longer match the state dict or the device (a subclass drops what else it derived from them)."""
        self._packed = None

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device = device
            self._dropped()
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} runs in eval mode only (BatchNorm folded into the convolutions)")
        return self.eval()

    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def load_state_dict(self, sd, strict=True):
        """Strict over the key names, but for `optional_missing` and `ignored`.  Missing / unexpected keys or a wrong shape raise."""
        want, name = self._sd, type(self).__name__
        got = {k: v for k, v in sd.items() if k in want or not _named(k, self.ignored)}
        missing = [k for k in want if k not in got and not _named(k, self.optional_missing)]
        unexpected = [k for k in got if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"{name}.load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in got.items():
            if tuple(v.shape) != tuple(want[k].shape):
                raise RuntimeError(f"{name}.load_state_dict: {k} has shape {tuple(v.shape)}, the model {tuple(want[k].shape)}")
        new = OrderedDict()
        for k, v in want.items():
            new[k] = got.get(k, v).detach().to("cpu", torch.long if k.endswith("num_batches_tracked") else torch.float32).clone()
        self._sd = new
        self._dropped()
        return None

    def _need_device(self):
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: call .to(<cuda device>) first -- the network runs on the HIP kernels only")


class ChunkedImageNet(MetricNet):
    """A network that embeds images in chunks of `batch_size`, from normalised NCHW f32, from uint8 NHWC or from the VAE decoder's
    output (csrc/sscd.hip's preprocessing).  The subclass supplies `_features(x)` (one chunk's rows) and `max_elements(N, H, W)`."""

    MAX_ELEMENTS = 1 << 31      # an activation (or split-K slab) of a chunk stays below this many elements

    def _chunk_shape(self, x):
        """(N, H, W) of one chunk of NCHW images; ValueError for empty images and for a chunk that holds a tensor of 2^31 elements."""
        N, _, H, W = x.shape
        name = type(self).__name__
        if H < 1 or W < 1:
            raise ValueError(f"{name}: empty images {tuple(x.shape)}")
        big = self.max_elements(N, H, W)
        if big >= self.MAX_ELEMENTS:
            raise ValueError(f"{name}: a chunk of {N} images of {H} x {W} holds a tensor of {big} elements, 2^31 or more: lower "
                             f"batch_size (now {self.batch_size})")
        return N, H, W

    def _preprocess(self, src, form, mean, std, want_u8):
        n = src.shape[0]
        h, w = (src.shape[1], src.shape[2]) if form == 0 else (src.shape[2], src.shape[3])
        x = torch.empty(n, 3, h, w, device=self.device, dtype=torch.float32)
        u8 = torch.empty(n, h, w, 3, device=self.device, dtype=torch.uint8) if want_u8 else None
        lib.call("siss_sscd_preprocess", src, form, n, h, w, *mean, *std, u8, x)
        return x, u8

    @torch.no_grad()
    def _chunks(self, src, form, mean, std, finish):
        """Chunks of batch_size through (preprocess ->) `_features` -> `finish(rows)` = (rows, scores or None): (rows, scores or
        None, uint8 or None) of all of them.  form: None (src is normalised NCHW f32), 0 (uint8 NHWC), 1 / 2 (decoder f32 / bf16)."""
        if self._packed is None:
            self._pack()
        n = src.shape[0]
        if n == 0:
            raise ValueError(f"{type(self).__name__}: no images")
        rows, scores, u8s = [], [], []
        for s in range(0, n, self.batch_size):
            part = src[s:s + self.batch_size].contiguous()
            u8 = None
            if form is not None:
                part, u8 = self._preprocess(part, form, mean, std, want_u8=form != 0)
            r, sc = finish(self._features(part))
            rows.append(r)
            scores.append(sc)
            u8s.append(u8)
        cat = lambda xs: None if xs[0] is None else (xs[0] if len(xs) == 1 else torch.cat(xs))
        return cat(rows), cat(scores), cat(u8s)

    def _check_u8(self, u8):
        u8 = torch.as_tensor(u8)
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError(f"uint8 images [n, H, W, 3] are needed, got {u8.dtype} {tuple(u8.shape)}")
        self._need_device()
        return u8.to(self.device)

    def _check_decoded(self, img):
        """The preprocessing form (1: f32, 2: bf16) of the decoder's output."""
        if not (torch.is_tensor(img) and img.is_cuda and img.dim() == 4 and img.shape[1] == 3):
            raise ValueError("the decoder's output [n, 3, H, W] on the device is needed")
        if img.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"decoder output of dtype {img.dtype}: float32 or bfloat16")
        if img.device != self.device:
            raise ValueError(f"decoder output on {img.device}, the network on {self.device}")
        return 2 if img.dtype == torch.bfloat16 else 1

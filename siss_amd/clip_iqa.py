"""The SD experiment's image-quality score (delete_sd.py:222-223,:264-267): torchmetrics' `CLIPImageQualityAssessment()` with its
defaults (`model_name_or_path="clip_iqa"`, `data_range=1.0`, `prompts=("quality",)`) -- the OpenAI CLIP RN50: its "ModifiedResNet"
image tower (a three-convolution stem, Bottlenecks [3, 4, 6, 3] whose stride is an AvgPool2d after the 3 x 3 conv2 and in front of the
shortcut's 1 x 1, BN eps 1e-5, attention pooling called WITHOUT its positional embedding, at the image's own size: no resize, no crop)
and the text tower that embeds the anchor prompts "Good photo." / "Bad photo."; the score is the positive anchor's share of
softmax(100 cos(image, anchors)) -- on the HIP kernels: every convolution and the q / c_proj / text_projection products on
metric_conv.hip's implicit-GEMM convolution, the preprocessing on sscd.hip's, the average pools, the attention pool and the score on
csrc/clip_iqa.hip, the text tower on `CLIPTextEncoder(dtype=torch.float32)`.  `CLIPIQAScore` is the tracker the task loop drives.

The attention pool has one query (the mean token) per head, so the key and value projections of the T = HW + 1 tokens are never
taken: with q_h = (W_q m + b_q)_h / sqrt(D),  s[h, t] = (W_{k,h}^T q_h) . x_t + q_h . b_{k,h}  and
out_h = W_{v,h} (sum_t softmax_t(s)[h, t] x_t) + b_{v,h}  (the softmax's weights sum to one, so b_v comes through unchanged).

The networks run in f32, in eval mode (BatchNorm folded into the convolutions at pack time in f64); the reference runs them under
torch.autocast (fp16) -- a deliberate deviation, as for every metric network here.  There is no CPU path: a missing kernel library
raises.  Neither the checkpoint nor torchmetrics / piq was available when this was written: everything is restated from the public
description (tests/clip_iqa_ref.py is the same restatement in torch.nn); tools/check_clip_iqa.py is the check for whoever has them.
"""
import math
import os
from collections import OrderedDict

import torch

from . import lib
from . import metric_net as mn

BN_EPS = 1e-5
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
ACT = torch.float32         # of every activation and result (the host test of the wiring runs this module on f64 emulations)
NORM_EPS = 1e-12            # of the anchors' normalisation (F.normalize's default; the rows are far from it)
OPTIONAL_KEYS = ("input_resolution", "context_length", "vocab_size", "logit_scale")    # may be absent from / extra in a checkpoint
# torchmetrics' built-in prompt pairs (functional/multimodal/clip_iqa.py _PROMPTS): name -> (positive, negative)
PROMPTS = OrderedDict([
    ("quality", ("Good photo.", "Bad photo.")), ("brightness", ("Bright photo.", "Dark photo.")),
    ("noisiness", ("Clean photo.", "Noisy photo.")), ("colorfullness", ("Colorful photo.", "Dull photo.")),
    ("sharpness", ("Sharp photo.", "Blurry photo.")), ("contrast", ("High contrast photo.", "Low contrast photo.")),
    ("complexity", ("Complex photo.", "Simple photo.")), ("natural", ("Natural photo.", "Synthetic photo.")),
    ("happy", ("Happy photo.", "Sad photo.")), ("scary", ("Scary photo.", "Peaceful photo.")),
    ("new", ("New photo.", "Old photo.")), ("warm", ("Warm photo.", "Cold photo.")),
    ("real", ("Real photo.", "Abstract photo.")), ("beautiful", ("Beautiful photo.", "Ugly photo.")),
    ("lonely", ("Lonely photo.", "Sociable photo.")), ("relaxing", ("Relaxing photo.", "Stressful photo."))])


def visual_convs(layers, width):
    """(prefix, Cin, Cout, k, conv stride, pad, bn prefix, pool) of every convolution of the image tower, in the state dict's order
    (without `visual.`).  `pool` is the AvgPool2d in FRONT of a shortcut's convolution or BEHIND conv2 / the stem's conv3 (1: none);
    the only strided convolution is the stem's conv1."""
    out = [("conv1", 3, width // 2, 3, 2, 1, "bn1", 1), ("conv2", width // 2, width // 2, 3, 1, 1, "bn2", 1),
           ("conv3", width // 2, width, 3, 1, 1, "bn3", 2)]
    inp = width
    for i, n in enumerate(layers, 1):
        planes = width * 2 ** (i - 1)
        for j in range(n):
            s = 2 if (i > 1 and j == 0) else 1
            p = f"layer{i}.{j}."
            out.append((p + "conv1", inp, planes, 1, 1, 0, p + "bn1", 1))
            out.append((p + "conv2", planes, planes, 3, 1, 1, p + "bn2", s))
            out.append((p + "conv3", planes, 4 * planes, 1, 1, 0, p + "bn3", 1))
            if s > 1 or inp != 4 * planes:
                out.append((p + "downsample.0", inp, 4 * planes, 1, 1, 0, p + "downsample.1", s))
            inp = 4 * planes
    return out


def format_prompts(prompts):
    """torchmetrics' _clip_iqa_format_prompts: (the prompt strings [2 P], positive then negative of each pair; the names [P]) of a
    tuple of built-in names and / or (positive, negative) string pairs (named user_defined_0, user_defined_1, ...)."""
    if not isinstance(prompts, tuple):
        raise ValueError("Argument `prompts` must be a tuple containing strings or tuples of strings")
    texts, names, count = [], [], 0
    for p in prompts:
        if not isinstance(p, (str, tuple)):
            raise ValueError("Argument `prompts` must be a tuple containing strings or tuples of strings")
        if isinstance(p, str):
            if p not in PROMPTS:
                raise ValueError(f"All elements of `prompts` must be one of {list(PROMPTS)} if not custom tuple prompts, got {p}.")
            texts.extend(PROMPTS[p])
            names.append(p)
        else:
            if len(p) != 2 or not all(isinstance(t, str) for t in p):
                raise ValueError("If a tuple is provided in argument `prompts`, it must be of length 2 (two strings)")
            texts.extend(p)
            names.append(f"user_defined_{count}")
            count += 1
    if not names:
        raise ValueError("Argument `prompts`: at least one prompt is needed")
    return texts, names


def eot_positions(ids):
    """The pooling position of each row of token ids: the FIRST occurrence of the row's largest id (the end-of-text token has the
    vocabulary's last id).  A CLIP tokenizer pads with that id, torchmetrics' processor with zeros; under the causal mask the row at
    the first occurrence sees the same tokens either way."""
    ids = torch.as_tensor(ids).cpu()
    return [int((row == row.max()).nonzero()[0]) for row in ids]


def text_encoder_state(sd, layers):
    """The OpenAI text-tower keys of `sd` under CLIPTextEncoder's (transformers') names: in_proj_* split into q / k / v."""
    out = {"embeddings.token_embedding.weight": sd["token_embedding.weight"], "embeddings.position_embedding.weight": sd["positional_embedding"],
           "final_layer_norm.weight": sd["ln_final.weight"], "final_layer_norm.bias": sd["ln_final.bias"]}
    for i in range(layers):
        src, dst = f"transformer.resblocks.{i}.", f"encoder.layers.{i}."
        w, b = sd[src + "attn.in_proj_weight"], sd[src + "attn.in_proj_bias"]
        C = w.shape[1]
        for k, name in enumerate(("q_proj", "k_proj", "v_proj")):
            out[dst + f"self_attn.{name}.weight"], out[dst + f"self_attn.{name}.bias"] = w[k * C:(k + 1) * C], b[k * C:(k + 1) * C]
        for a, b_ in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                      ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[dst + b_ + ".weight"], out[dst + b_ + ".bias"] = sd[src + a + ".weight"], sd[src + a + ".bias"]
    return out


def pack_linear(w, b, device):
    """(weight [out][in], bias) of a projection the attention pool's own kernels read, f32 on the device."""
    return w.to(device, torch.float32).contiguous(), b.to(device, torch.float32).contiguous()


class CLIPIQAModel(mn.ChunkedImageNet):
    """OpenAI CLIP RN50 as clip_iqa uses it: `[N, 3, H, W]` f32 images, already normalised -> the raw `[N, output_dim]` rows of the
    image tower on the device; `anchors(ids)` the unit rows of the text tower; `scores_*` the probabilities `[N, P]`.  The parameters
    live on the host under the OpenAI state dict's key names; `.to(device)` / the first call packs them (BN folded) onto the device.
    Images go through in chunks of `batch_size`.  The architecture's sizes are arguments so that small networks can be built."""

    # Strict over the key names: only `num_batches_tracked` and `logit_scale` may be missing, only `input_resolution`, `context_length`
    # and `vocab_size` (the scalars an OpenAI archive carries) may be extra.
    optional_missing = (".num_batches_tracked",) + OPTIONAL_KEYS
    ignored = OPTIONAL_KEYS

    def __init__(self, layers=(3, 4, 6, 3), width=64, heads=None, output_dim=1024, input_resolution=224, text_width=512, text_heads=8,
                 text_layers=12, vocab_size=49408, context_length=77, batch_size=16):
        self.layers, self.width = tuple(int(n) for n in layers), int(width)
        self.embed = self.width * 32
        self.heads = int(heads) if heads is not None else self.embed // 64
        self.output_dim, self.input_resolution, self.batch_size = int(output_dim), int(input_resolution), int(batch_size)
        self.text_width, self.text_heads, self.text_layers = int(text_width), int(text_heads), int(text_layers)
        self.vocab_size, self.context_length = int(vocab_size), int(context_length)
        if len(self.layers) != 4 or min(self.layers) < 1:
            raise ValueError(f"CLIPIQAModel(layers={layers!r}): four positive block counts are needed")
        if self.width <= 0 or self.width % 64 != 0:
            raise ValueError(f"CLIPIQAModel(width={width!r}): width % 64 == 0 is needed (the stem's width / 2 channels feed an NHWC "
                             "convolution that takes Cin % 32 == 0)")
        if self.heads <= 0 or self.embed % self.heads != 0 or self.heads > 256:
            raise ValueError(f"CLIPIQAModel(heads={heads!r}): the attention pool's {self.embed} channels split into 1 .. 256 heads")
        if self.text_width % 64 != 0 or self.text_heads <= 0 or self.text_width % self.text_heads != 0 or (self.text_width // self.text_heads) % 8 != 0:
            raise ValueError(f"CLIPIQAModel(text_width={text_width!r}, text_heads={text_heads!r}): text_width % 64 == 0 and a head "
                             "width that is a multiple of 8 are needed")
        if min(self.output_dim, self.batch_size, self.text_layers, self.vocab_size, self.context_length) <= 0 or self.input_resolution < 32:
            raise ValueError("CLIPIQAModel: positive sizes (and input_resolution >= 32) are needed")
        E, C, sd = self.embed, self.text_width, OrderedDict()
        with torch.random.fork_rng(devices=[]):      # building the metric leaves the global random stream where it was
            sd["positional_embedding"] = torch.empty(self.context_length, C).normal_(0, 0.01)
            sd["text_projection"] = torch.empty(C, self.output_dim).normal_(0, C ** -0.5)
            sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
            for name, cin, cout, k, _, _, bn, _ in visual_convs(self.layers, self.width):
                sd["visual." + name + ".weight"] = torch.empty(cout, cin, k, k).normal_(0, math.sqrt(2.0 / (k * k * cout)))
                b = "visual." + bn
                sd[b + ".weight"], sd[b + ".bias"] = torch.ones(cout), torch.zeros(cout)
                sd[b + ".running_mean"], sd[b + ".running_var"] = torch.zeros(cout), torch.ones(cout)
                sd[b + ".num_batches_tracked"] = torch.tensor(0)
            sd["visual.attnpool.positional_embedding"] = torch.empty((self.input_resolution // 32) ** 2 + 1, E).normal_(0, E ** -0.5)
            for name in ("k_proj", "q_proj", "v_proj", "c_proj"):
                out = self.output_dim if name == "c_proj" else E
                sd[f"visual.attnpool.{name}.weight"] = torch.empty(out, E).normal_(0, E ** -0.5)
                sd[f"visual.attnpool.{name}.bias"] = torch.zeros(out)
            attn, proj, fc = C ** -0.5, C ** -0.5 * (2 * self.text_layers) ** -0.5, (2 * C) ** -0.5
            for i in range(self.text_layers):
                p = f"transformer.resblocks.{i}."
                sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = torch.empty(3 * C, C).normal_(0, attn), torch.zeros(3 * C)
                sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = torch.empty(C, C).normal_(0, proj), torch.zeros(C)
                sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = torch.ones(C), torch.zeros(C)
                sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = torch.empty(4 * C, C).normal_(0, fc), torch.zeros(4 * C)
                sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = torch.empty(C, 4 * C).normal_(0, proj), torch.zeros(C)
                sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = torch.ones(C), torch.zeros(C)
            sd["token_embedding.weight"] = torch.empty(self.vocab_size, C).normal_(0, 0.02)
            sd["ln_final.weight"], sd["ln_final.bias"] = torch.ones(C), torch.zeros(C)
        super().__init__(sd)    # (filled in the OpenAI module's order: its own parameters, visual, transformer, token_embedding, ln_final)

    def _dropped(self):
        self._packed, self._text, self._anchors = None, None, {}

    @classmethod
    def load(cls, path, batch_size=16):
        """The network of a checkpoint file: a TorchScript archive (`torch.jit.load(path).state_dict()`, the form OpenAI publishes
        RN50.pt in), else a `torch.load` state dict, else -- when the file is not a zip archive -- a `.safetensors` file.  The sizes
        are read from the tensors' shapes, as OpenAI's build_model reads them.  Any other key set raises RuntimeError with the
        missing and unexpected keys."""
        sd = mn.read_state_dict(path, "CLIP")
        kw = {}
        try:
            blocks = lambda i: len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{i}.")})
            kw["layers"] = tuple(blocks(i) for i in range(1, 5))
            kw["width"] = int(sd["visual.layer1.0.conv1.weight"].shape[0])
            kw["output_dim"] = int(sd["text_projection"].shape[1])
            kw["input_resolution"] = 32 * int(round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5))
            kw["text_width"] = int(sd["ln_final.weight"].shape[0])
            kw["text_heads"] = max(1, kw["text_width"] // 64)
            kw["text_layers"] = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
            kw["vocab_size"], kw["context_length"] = int(sd["token_embedding.weight"].shape[0]), int(sd["positional_embedding"].shape[0])
            net = cls(batch_size=batch_size, **kw)
        except (KeyError, ValueError, IndexError, AttributeError):
            net = cls(batch_size=batch_size)            # not readable as an OpenAI CLIP ResNet: the strict load below says what is missing
        try:
            net.load_state_dict(sd)
        except RuntimeError as e:
            raise RuntimeError(f"{path} is not an OpenAI-format CLIP ResNet state dict: {e}") from e
        return net.eval()

    # -- packing ---------------------------------------------------------------------------------
    def _pack(self):
        self._need_device()
        sd, E = self._sd, self.embed
        P = {}
        for name, _, _, _, s, p, bn, _ in visual_convs(self.layers, self.width):
            P[name] = mn.pack_conv(*mn.fold_bn(sd, "visual." + name, "visual." + bn, BN_EPS), s, p, self.device)
        for name in ("q_proj", "c_proj"):
            w = sd[f"visual.attnpool.{name}.weight"].double()
            P[name] = mn.pack_conv(w.view(w.shape[0], E, 1, 1), sd[f"visual.attnpool.{name}.bias"].double(), 1, 0, self.device)
        for name in ("k_proj", "v_proj"):                # (visual.attnpool.positional_embedding is loaded and not used)
            P[name + ".w"], P[name + ".b"] = pack_linear(sd[f"visual.attnpool.{name}.weight"], sd[f"visual.attnpool.{name}.bias"], self.device)
        self._packed = P

    def _shapes(self, N, H, W):
        """(final map (H, W), the largest tensor in elements) of a chunk of N images of H x W; ValueError when a map vanishes."""
        if self._packed is None:
            self._pack()
        P = self._packed
        big = N * 3 * H * W

        def after(name, H, W):
            nonlocal big
            if min(H, W) < 1:
                raise ValueError(f"CLIPIQAModel: the map in front of {name} is empty: the images are too small")
            L = P[name]
            Ho, Wo = mn.conv_out(L, H, W)
            M = N * Ho * Wo
            big = max(big, M * L["cout"] * mn.conv_splits(M, L["cout"], L["Kp"]))
            return Ho, Wo
        for name in ("conv1", "conv2", "conv3"):
            H, W = after(name, H, W)
        H, W = H // 2, W // 2
        for i, n in enumerate(self.layers, 1):
            for j in range(n):
                pre = f"layer{i}.{j}."
                s = 2 if (i > 1 and j == 0) else 1
                after(pre + "conv1", H, W)
                after(pre + "conv2", H, W)
                if pre + "downsample.0" in P:
                    after(pre + "downsample.0", H // s, W // s)
                H, W = after(pre + "conv3", H // s, W // s)
        return (H, W), max(big, N * self.heads * self.embed, N * self.heads * (H * W + 1))

    def max_elements(self, N, H, W):
        """The largest tensor (input, activation or split-K slab, in elements) a chunk of N images of H x W touches."""
        return self._shapes(N, H, W)[1]

    # -- forward ---------------------------------------------------------------------------------
    def _avg_pool(self, x, k=2):
        N, H, W, C = x.shape
        if H < k or W < k:
            raise ValueError(f"CLIPIQAModel: a {H} x {W} map in front of AvgPool2d({k}): the images are too small")
        y = torch.empty(N, H // k, W // k, C, device=x.device, dtype=ACT)
        lib.call("siss_clipiqa_avgpool", x, y, N, H, W, C, k)
        return y

    def attention_pool(self, h, N, HW, return_logits=False):
        """The NHWC layer4 map `h` ([N, HW, embed] as rows) -> [N, output_dim]: mean token, q, the folded query, the logits over the
        mean token and the HW rows, softmax and pooling, the value projection, c_proj.  return_logits: (rows, logits [N, heads,
        HW + 1]) -- the q . b_k term is the same for every token of a head, so only the logits show it."""
        P, E, Hh = self._packed, self.embed, self.heads
        f32 = dict(device=h.device, dtype=ACT)
        m = torch.empty(N, E, **f32)
        lib.call("siss_clipiqa_token_mean", h, m, N, HW, E)
        q = mn.linear(P["q_proj"], m)
        qt, c = torch.empty(N, Hh, E, **f32), torch.empty(N, Hh, **f32)
        lib.call("siss_clipiqa_fold_query", q, P["k_proj.w"], P["k_proj.b"], qt, c, N, E, Hh, float((E // Hh) ** -0.5))
        s = torch.empty(N, Hh, HW + 1, **f32)
        lib.call("siss_clipiqa_scores", h, m, qt, c, s, N, HW, E, Hh)
        xbar = torch.empty(N, Hh, E, **f32)
        lib.call("siss_clipiqa_pool", h, m, s, xbar, N, HW, E, Hh)
        o = torch.empty(N, E, **f32)
        lib.call("siss_clipiqa_head_value", xbar, P["v_proj.w"], P["v_proj.b"], o, N, E, Hh)
        out = mn.linear(P["c_proj"], o)
        return (out, s) if return_logits else out

    def _features(self, x):
        """One chunk: the normalised NCHW images -> the image tower's raw rows [n, output_dim]."""
        N, H, W = self._chunk_shape(x)
        P = self._packed
        h = mn.conv(P["conv3"], mn.conv(P["conv2"], mn.conv(P["conv1"], x, nchw_in=True)))
        h = self._avg_pool(h)
        for i, n in enumerate(self.layers, 1):
            for j in range(n):
                pre = f"layer{i}.{j}."
                s = 2 if (i > 1 and j == 0) else 1
                a = mn.conv(P[pre + "conv2"], mn.conv(P[pre + "conv1"], h))      # stride 1: the stride is the pool behind it
                sc = h
                if s > 1:
                    a = self._avg_pool(a)
                if pre + "downsample.0" in P:
                    if s > 1:
                        sc = self._avg_pool(h)
                    sc = mn.conv(P[pre + "downsample.0"], sc, relu=False)
                h = mn.conv(P[pre + "conv3"], a, res=sc)
        return self.attention_pool(h, N, h.shape[1] * h.shape[2])

    def _score(self, rows, anchors):
        n, P = rows.shape[0], anchors.shape[0] // 2
        out = torch.empty(n, P, device=self.device, dtype=ACT)
        lib.call("siss_clipiqa_score", rows, anchors, n, self.output_dim, P, out)
        return out

    def _run(self, src, form, anchors):
        """Chunks of batch_size through (preprocess ->) the image tower (-> the score): (rows, scores or None, uint8 or None)."""
        if anchors is not None:
            anchors = anchors.to(self.device, ACT).contiguous()
            if anchors.dim() != 2 or anchors.shape[0] < 2 or anchors.shape[0] % 2 or anchors.shape[1] != self.output_dim:
                raise ValueError(f"anchor rows [2 P, {self.output_dim}] are needed, got {tuple(anchors.shape)}")
        return self._chunks(src, form, CLIP_MEAN, CLIP_STD, lambda r: (r, None if anchors is None else self._score(r, anchors)))

    def __call__(self, x, anchors=None):
        """`[N, 3, H, W]` f32, already normalised with CLIP's mean / std -> the image tower's raw rows `[N, output_dim]`; with
        `anchors` (unit rows [2 P, output_dim]) -> (rows, probabilities [N, P])."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"CLIPIQAModel expects [N, 3, H, W] images, got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        rows, scores, _ = self._run(x.to(self.device, torch.float32), None, anchors)
        return rows if anchors is None else (rows, scores)

    forward = __call__

    def embed_u8(self, u8):
        """uint8 images `[n, H, W, 3]` -> the raw rows of Normalize(CLIP mean, std)(ToTensor(image)), the preprocessing fused into one
        launch (bitwise torch's f32 chain)."""
        return self._run(self._check_u8(u8), 0, None)[0]

    def embed_decoded(self, img):
        """The VAE decoder's output `[n, 3, H, W]` (f32 or bf16, on the device) -> (raw rows, the uint8 images `[n, H, W, 3]` --
        bitwise `kmeans.from_decoded`'s --) in one preprocessing launch per chunk."""
        rows, _, u8 = self._run(img, self._check_decoded(img), None)
        return rows, u8

    def scores_u8(self, u8, anchors):
        """Probabilities `[n, P]` (device) of uint8 images `[n, H, W, 3]` against the unit anchor rows `[2 P, output_dim]`."""
        return self._run(self._check_u8(u8), 0, anchors)[1]

    def scores_decoded(self, img, anchors):
        """(probabilities `[n, P]`, the uint8 images `[n, H, W, 3]`), both on the device, of the decoder's output."""
        _, scores, u8 = self._run(img, self._check_decoded(img), anchors)
        return scores, u8

    # -- the anchors -----------------------------------------------------------------------------
    def text_encoder(self):
        """The text tower as a CLIPTextEncoder in f32 (built once per device)."""
        self._need_device()
        if self._text is None:
            from .text_encoder import CLIPTextEncoder
            self._text = CLIPTextEncoder(text_encoder_state(self._sd, self.text_layers), self.text_heads, 1e-5, self.device,
                                         dtype=torch.float32)
        return self._text

    @torch.no_grad()
    def anchors(self, ids):
        """Token ids `[2 P, L]` (a positive and a negative prompt per pair) -> the unit rows `[2 P, output_dim]` on the device: the
        text tower's row at the first occurrence of each prompt's largest id, through ln_final (inside the encoder), times
        text_projection, normalised.  Computed once per set of ids and kept."""
        ids = torch.as_tensor(ids).detach().cpu()
        if ids.is_floating_point() or ids.dim() != 2 or ids.shape[0] < 2 or ids.shape[0] % 2:
            raise ValueError(f"token ids [2 P, L] (integers) are needed, got {ids.dtype} {tuple(ids.shape)}")
        ids = ids.long()
        if ids.shape[1] > self.context_length:
            raise ValueError(f"prompts of {ids.shape[1]} tokens, the text tower has {self.context_length} positions")
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab_size:    # (checked here: a bad id would fault the gather on the device)
            raise ValueError(f"token ids reach {int(ids.max())} (smallest {int(ids.min())}), beyond the text tower's vocabulary of "
                             f"{self.vocab_size}")
        key = (tuple(ids.shape), tuple(ids.reshape(-1).tolist()))
        if key not in self._anchors:
            hidden = self.text_encoder()(ids.to(self.device))[0]                     # [2 P, L, C], ln_final applied
            n, C = ids.shape[0], self.text_width
            rows = hidden[torch.arange(n, device=self.device), torch.tensor(eot_positions(ids), device=self.device)].contiguous()
            if "text_projection" not in (self._packed or {}):
                if self._packed is None:
                    self._pack()
                wp = self._sd["text_projection"].double().t().contiguous().view(self.output_dim, C, 1, 1)
                self._packed["text_projection"] = mn.pack_conv(wp, torch.zeros(self.output_dim, dtype=torch.float64), 1, 0, self.device)
            a = mn.linear(self._packed["text_projection"], rows)
            lib.call("siss_sscd_normalize_score", a, n, self.output_dim, NORM_EPS, None, a, None)
            self._anchors[key] = a
        return self._anchors[key]


def tokenize(prompts, tokenizer, context_length=77):
    """Token ids [len(prompts), context_length] of prompt strings through a CLIP tokenizer: a `transformers.CLIPTokenizer`, or the
    directory of one."""
    if isinstance(tokenizer, (str, os.PathLike)):
        if not os.path.isdir(str(tokenizer)):
            raise FileNotFoundError(f"CLIP tokenizer directory {str(tokenizer)!r} is not on disk")
        from transformers import CLIPTokenizer
        tokenizer = CLIPTokenizer.from_pretrained(str(tokenizer))
    return tokenizer(list(prompts), max_length=context_length, padding="max_length", truncation=True, return_tensors="pt").input_ids


class CLIPImageQualityAssessment:
    """torchmetrics.multimodal.CLIPImageQualityAssessment's call surface on the HIP network: `update(images)` / `compute()` /
    `reset()` / `__call__(images)` on `[N, 3, H, W]` floats in `[0, data_range]`.  `model`: a CLIPIQAModel (there is nothing to
    download here: None is refused).  `prompts`: built-in names and / or (positive, negative) pairs; their token ids come from
    `prompt_ids` `[2 P, L]`, or from `tokenizer` (a CLIP tokenizer or its directory).  One prompt gives `[N]`, several a dict by name."""

    def __init__(self, model=None, prompts=("quality",), data_range=1.0, prompt_ids=None, tokenizer=None, model_name_or_path="clip_iqa"):
        if model_name_or_path != "clip_iqa":
            raise ValueError(f"model_name_or_path={model_name_or_path!r}: only 'clip_iqa' (OpenAI CLIP RN50 without the positional "
                             "embedding) is built here")
        if not isinstance(model, CLIPIQAModel):
            raise ValueError("CLIPImageQualityAssessment(model=...): a CLIPIQAModel is needed (CLIPIQAModel.load(<RN50 checkpoint>)); "
                             "nothing is downloaded here")
        if not (isinstance(data_range, (int, float)) and data_range > 0):
            raise ValueError("Argument `data_range` should be a positive number.")
        self.model, self.data_range = model, float(data_range)
        self.prompts_list, self.prompts_names = format_prompts(prompts)
        if prompt_ids is not None:
            ids = torch.as_tensor(prompt_ids)
            if ids.dim() != 2 or ids.shape[0] != len(self.prompts_list):
                raise ValueError(f"prompt_ids of shape {tuple(ids.shape)}: [{len(self.prompts_list)}, L] is needed -- a positive and a "
                                 f"negative row per prompt ({self.prompts_names})")
        elif tokenizer is not None:
            ids = tokenize(self.prompts_list, tokenizer, model.context_length)
        else:
            raise ValueError("the prompts' token ids are needed: pass prompt_ids [2 P, L], or tokenizer (a CLIP tokenizer or its directory)")
        self.prompt_ids = ids.long().cpu()
        self.probs_list = []

    def _probs(self, images):
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or not images.is_floating_point():
            raise ValueError(f"float images [N, 3, H, W] in [0, {self.data_range}] are needed")
        m = self.model
        m._need_device()
        x = images.to(m.device, torch.float32)
        col = lambda v: torch.tensor(v, device=m.device, dtype=torch.float32).view(1, -1, 1, 1)
        x = (x / col([self.data_range]) - col(CLIP_MEAN)) / col(CLIP_STD)         # tensor operands: true IEEE divisions on the device
        return m(x, anchors=m.anchors(self.prompt_ids))[1]

    def _format(self, probs):
        if len(self.prompts_names) == 1:
            return probs[:, 0]
        return {name: probs[:, i] for i, name in enumerate(self.prompts_names)}

    def update(self, images):
        self.probs_list.append(self._probs(images))

    def compute(self):
        if not self.probs_list:
            raise ValueError("No samples to concatenate")
        return self._format(torch.cat(self.probs_list))

    def reset(self):
        self.probs_list = []

    def __call__(self, images):
        """torchmetrics' forward: the value of this batch alone; the batch is added to the state as well."""
        probs = self._probs(images)
        self.probs_list.append(probs)
        return self._format(probs)

    forward = __call__


class CLIPIQAScore:
    """delete_sd.py:264-267 for one rank: the CLIP-IQA probabilities of the validation images.  `record(prompt, scores, step)` appends
    {global_step, clip_iqa_<i>} to `out_path`, the value the mean of the scores in f64 on the host (the reference's
    `clip_scores.mean().item()`)."""

    def __init__(self, model, prompt_ids, out_path):
        self.model, self.out_path = model, out_path
        self.prompt_ids = torch.as_tensor(prompt_ids).long().cpu()
        if self.prompt_ids.dim() != 2 or self.prompt_ids.shape[0] < 2 or self.prompt_ids.shape[0] % 2:
            raise ValueError(f"prompt ids [2 P, L] are needed, got {tuple(self.prompt_ids.shape)}")

    def _anchors(self, device):
        return self.model.to(device).eval().anchors(self.prompt_ids)

    def score_u8(self, u8):
        """Probabilities [n, P] (device) of uint8 images [n, H, W, 3]."""
        device = u8.device if torch.is_tensor(u8) and u8.is_cuda else self.model.device
        return self.model.scores_u8(u8, self._anchors(device))

    def score_decoded(self, img):
        """(probabilities [n, P], uint8 images [n, H, W, 3]), both on the device, of the decoder's output."""
        return self.model.scores_decoded(img, self._anchors(img.device))

    extra = None                # fields added to every record (pipeline.sampler: the sampler's name and step count)

    def record(self, prompt, scores, step):
        return mn.record_mean(self.out_path, f"clip_iqa_{prompt}", scores, step, self.extra)

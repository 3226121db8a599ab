"""A plain torch.nn restatement of what torchmetrics' CLIPImageQualityAssessment("clip_iqa") computes: the OpenAI CLIP RN50 -- the
"ModifiedResNet" image tower with its attention pooling called without the positional embedding, the text tower, the anchors and
the score -- written from the public description of that network (module and parameter names as in the OpenAI state dict), generic
over the dtype: the f64 run is the reference of the tests, the f32 run measures what f32 arithmetic alone costs.

The attention pool calls F.multi_head_attention_forward directly, with the key and value projections taken for every token: the
UNFOLDED form, so that the folded form of siss_amd/clip_iqa.py is checked against something independent of it.
"""
import copy
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        # every convolution has stride 1: an average pool behind conv2 (and in front of the shortcut's convolution) is the stride
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu2 = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu3 = nn.ReLU(inplace=True)
        self.downsample = None
        self.stride = stride
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(OrderedDict([("-1", nn.AvgPool2d(stride)), ("0", nn.Conv2d(inplanes, planes * 4, 1, bias=False)),
                                                         ("1", nn.BatchNorm2d(planes * 4))]))

    def forward(self, x):
        identity = x
        out = self.relu1(self.bn1(self.conv1(x)))
        out = self.relu2(self.bn2(self.conv2(out)))
        out = self.avgpool(out)
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu3(out + identity)


class AttentionPool2d(nn.Module):
    def __init__(self, spacial_dim, embed_dim, num_heads, output_dim):
        super().__init__()
        self.positional_embedding = nn.Parameter(torch.randn(spacial_dim ** 2 + 1, embed_dim) / embed_dim ** 0.5)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.c_proj = nn.Linear(embed_dim, output_dim)
        self.num_heads = num_heads
        self.pos_embedding, self.query_token = False, 0         # clip_iqa: no positional embedding, the mean token is the query

    def forward(self, x):
        x = x.flatten(start_dim=2).permute(2, 0, 1)             # N C H W -> (HW) N C
        x = torch.cat([x.mean(dim=0, keepdim=True), x], dim=0)  # (HW + 1) N C
        if self.pos_embedding:
            x = x + self.positional_embedding[:x.shape[0], None, :].to(x.dtype)
        q = self.query_token
        x, _ = F.multi_head_attention_forward(
            query=x[q:q + 1], key=x, value=x, embed_dim_to_check=x.shape[-1], num_heads=self.num_heads,
            q_proj_weight=self.q_proj.weight, k_proj_weight=self.k_proj.weight, v_proj_weight=self.v_proj.weight, in_proj_weight=None,
            in_proj_bias=torch.cat([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]), bias_k=None, bias_v=None,
            add_zero_attn=False, dropout_p=0.0, out_proj_weight=self.c_proj.weight, out_proj_bias=self.c_proj.bias,
            use_separate_proj_weight=True, training=False, need_weights=False)
        return x.squeeze(0)


class ModifiedResNet(nn.Module):
    def __init__(self, layers, output_dim, heads, input_resolution=224, width=64):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width // 2, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(width // 2, width // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(width // 2, width, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.relu3 = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(2)
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.attnpool = AttentionPool2d(input_resolution // 32, width * 32, heads, output_dim)

    def _make_layer(self, planes, blocks, stride=1):
        layers = [Bottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(self._inplanes, planes))
        return nn.Sequential(*layers)

    def trunk(self, x):
        x = self.relu1(self.bn1(self.conv1(x)))
        x = self.relu2(self.bn2(self.conv2(x)))
        x = self.relu3(self.bn3(self.conv3(x)))
        x = self.avgpool(x)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def forward(self, x):
        return self.attnpool(self.trunk(x))


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)

    def forward(self, x):
        L = x.shape[0]
        mask = torch.full((L, L), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)       # causal
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False, attn_mask=mask)[0]
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class CLIP(nn.Module):
    def __init__(self, embed_dim=1024, image_resolution=224, vision_layers=(3, 4, 6, 3), vision_width=64, context_length=77,
                 vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12):
        super().__init__()
        self.context_length = context_length
        self.visual = ModifiedResNet(vision_layers, embed_dim, vision_width * 32 // 64, image_resolution, vision_width)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads)
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592)

    def encode_image(self, x):
        return self.visual(x)

    def encode_text(self, ids):
        x = self.token_embedding(ids) + self.positional_embedding[:ids.shape[1]]
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)
        x = self.ln_final(x)
        return x[torch.arange(x.shape[0]), first_largest(ids)] @ self.text_projection


def first_largest(ids):
    """Per row the position of the FIRST occurrence of the largest id, by a loop (independent of argmax's tie rule)."""
    out = []
    for row in ids.tolist():
        best = 0
        for k, v in enumerate(row):
            if v > row[best]:
                best = k
        out.append(best)
    return torch.tensor(out)


# (the text tower's heads are width // 64, the rule by which OpenAI's loader -- and CLIPIQAModel.load -- reads them off a file)
SMALL = dict(embed_dim=64, vision_layers=(1, 1, 1, 1), vision_width=64, context_length=16, vocab_size=96, transformer_width=128,
             transformer_heads=2, transformer_layers=2)


def make(seed, **kw):
    """A seeded random network in eval mode with NON-TRIVIAL BatchNorm statistics and affine parameters, non-zero biases and
    LayerNorm parameters, scaled so that the activations stay of order one through the 16 blocks."""
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = CLIP(**kw)
    rnd = lambda t, std: t.copy_(torch.randn(t.shape, generator=g) * std)
    uni = lambda t, lo, hi: t.copy_(torch.rand(t.shape, generator=g) * (hi - lo) + lo)
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                rnd(m.weight, (2.0 / (m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3])) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                last = name.endswith("bn3") and "layer" in name
                uni(m.weight, *((0.3, 0.6) if last else (0.7, 1.3)))
                rnd(m.bias, 0.1)
                rnd(m.running_mean, 0.2)
                uni(m.running_var, 0.6, 1.6)
            elif isinstance(m, nn.LayerNorm):
                uni(m.weight, 0.7, 1.3)
                rnd(m.bias, 0.1)
            elif isinstance(m, nn.Linear):
                rnd(m.weight, m.weight.shape[1] ** -0.5)
                rnd(m.bias, 0.1)
            elif isinstance(m, nn.MultiheadAttention):
                rnd(m.in_proj_weight, m.in_proj_weight.shape[1] ** -0.5)
                rnd(m.in_proj_bias, 0.1)
            elif isinstance(m, nn.Embedding):
                rnd(m.weight, 0.5)
        rnd(net.positional_embedding, 0.1)
        rnd(net.text_projection, net.text_projection.shape[0] ** -0.5)
        rnd(net.visual.attnpool.positional_embedding, 0.5)
    return net.eval()


def variant(net, maxpool=False, stride_on_conv2=False, pos_embedding=False, query_token=0):
    """A copy of `net` with one thing wrong (the negative controls): max pools for the average pools; the stride on a block's conv2
    instead of the pool behind it; the positional embedding added in the attention pool; token `query_token` as its query."""
    net = copy.deepcopy(net)
    if maxpool:
        for m in list(net.modules()):
            for name, child in list(m.named_children()):
                if isinstance(child, nn.AvgPool2d):
                    setattr(m, name, nn.MaxPool2d(child.kernel_size))
    if stride_on_conv2:
        for m in net.modules():
            if isinstance(m, Bottleneck) and m.stride > 1:
                m.conv2.stride = (m.stride, m.stride)
                m.avgpool = nn.Identity()
    net.visual.attnpool.pos_embedding, net.visual.attnpool.query_token = pos_embedding, query_token
    return net


def reset_bn(net):
    net = copy.deepcopy(net)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.reset_running_stats()
    return net


def normalise(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """Normalize(mean, std)(ToTensor(image)) of uint8 [n, H, W, 3] as the host code rounds it in f32: [n, 3, H, W]."""
    x = u8.permute(0, 3, 1, 2).float() / 255
    return (x - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)


def _as(net, dtype, device):
    return copy.deepcopy(net).to(device=device, dtype=dtype)


@torch.no_grad()
def embed(net, x, dtype=torch.float64, device="cpu"):
    """The image tower's raw rows [N, embed_dim] in `dtype`."""
    return _as(net, dtype, device).encode_image(x.to(device=device, dtype=dtype))


@torch.no_grad()
def anchors(net, ids, dtype=torch.float64, device="cpu"):
    """The unit anchor rows [2 P, embed_dim] of token ids [2 P, L]."""
    a = _as(net, dtype, device).encode_text(ids.to(device))
    return a / a.norm(dim=-1, keepdim=True)


def score(rows, anchor_rows):
    """The probabilities [N, P]: the positive anchor's share of softmax(100 cos) over each (positive, negative) pair."""
    f = rows / rows.norm(dim=-1, keepdim=True)
    logits = 100 * f @ anchor_rows.to(f.dtype).t()
    return logits.reshape(logits.shape[0], -1, 2).softmax(-1)[:, :, 0]


@torch.no_grad()
def attention_pool(pool, x, dtype=torch.float64, device="cpu"):
    """An AttentionPool2d alone on an NCHW map, in `dtype`."""
    return _as(pool, dtype, device)(x.to(device=device, dtype=dtype))

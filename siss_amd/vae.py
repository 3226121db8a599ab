"""VAE encoder (diffusers ``AutoencoderKL.encode``, SD v1.x) forward on HIP -- the frozen front end that maps both
image batches to latents before the SISS step (delete_sd.py:464-468 load, :879-888
``vae.encode(x).latent_dist.sample() * vae.config.scaling_factor``) -- and the decoder half
(``AutoencoderKL.decode``) that turns the validation pipeline's latents into images (delete_sd.py:170-340,
data/src/local_sd_pipeline.py:203-206).

Forward only (the VAE is frozen, delete_sd.py:476).  It is the UNet engine's own machinery on a different graph:
padded-NHWC bf16 activations, GroupNorm+SiLU kernels, 3x3 / 1x1 / stride-2 convolutions, nearest-2x upsampling
convolutions and the single-head attention as MFMA GEMMs.  ``quant_conv`` (1x1, 8 -> 8) is folded into ``conv_out``
when the weights are loaded (both are linear: W' = W_q W_out, b' = W_q b_out + b_q), so the moments come out of one
3x3 GEMM.  ``post_quant_conv`` (1x1, 4 -> 4) is folded into the decoder's ``conv_in`` the same way, except for its
bias: ``conv_in`` zero-pads its input, so a constant added before it is NOT a constant after it on the border pixels.
The bias rides in a fifth input channel of ones instead (zero-padded like the rest, weights W_in . b_pq): exact.
Parameter names are the diffusers state-dict keys (``encoder.*``, ``quant_conv.*``, ``decoder.*``, ``post_quant_conv.*``).
"""
from dataclasses import dataclass
from typing import Tuple

import torch

from . import lib, ops
from .unet import ParamStore, UNetEngine


@dataclass
class VAEEncoderConfig:
    in_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    scaling_factor: float = 0.18215
    downsample_padding: int = 0          # Downsample2D(padding=0): F.pad (0,1,0,1) then stride 2

    @classmethod
    def from_dict(cls, d):
        names = set(cls.__dataclass_fields__)
        return cls(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items() if k in names})

    def head_dim(self, channels):
        return channels                  # mid-block attention: one head as wide as the block


@dataclass
class VAEDecoderConfig(VAEEncoderConfig):
    out_channels: int = 3


class _VAEHalf(UNetEngine):
    """What the two halves share: a forward-only bf16 engine over (part of) a diffusers AutoencoderKL state dict."""
    forward_only = True
    config_class = VAEEncoderConfig

    def __init__(self, cfg=None, device="cuda"):
        lib.load()
        self.cfg = cfg or self.config_class()
        self.device = torch.device(device)
        lib.ensure_workspace(self.device)
        self.ps = ParamStore()
        self._declare_params()
        self.ps.allocate(self.device, nsets=1)
        self.adt, self.f32 = torch.bfloat16, False         # (forward-only front end: the bf16 path)
        self._init_runtime_state()

    def _declare_enc_resnet(self, pre, cin, cout):
        a = self.ps.add
        a(f"{pre}.norm1.weight", "vec", (cin,)); a(f"{pre}.norm1.bias", "vec", (cin,))
        a(f"{pre}.conv1.weight", "conv3", (cout, cin, 3, 3)); a(f"{pre}.conv1.bias", "vec", (cout,))
        a(f"{pre}.norm2.weight", "vec", (cout,)); a(f"{pre}.norm2.bias", "vec", (cout,))
        a(f"{pre}.conv2.weight", "conv3", (cout, cout, 3, 3)); a(f"{pre}.conv2.bias", "vec", (cout,))
        if cin != cout:
            a(f"{pre}.conv_shortcut.weight", "conv1", (cout, cin, 1, 1)); a(f"{pre}.conv_shortcut.bias", "vec", (cout,))

    def refresh_weights(self, cast_shadow=False):
        ps = self.ps
        lib.call("siss_cast_f32_bf16", ps.flat, ps.shadow, ps.total)       # frozen: no dgrad copies needed
        for n, (wf, wd) in self._up_w.items():          # sub-pixel upsample sites (decoder): phase weights from the f32 master
            lib.call("siss_upsample_phase_weights", ps.p(n), wf, wd, wf.shape[2], wf.shape[3])

    @classmethod
    def from_pretrained(cls, path, subfolder="vae", device="cuda"):
        import json
        import os
        from safetensors.torch import load_file
        d = os.path.join(path, subfolder) if subfolder else path
        m = cls(cls.config_class.from_dict(json.load(open(os.path.join(d, "config.json")))), device)
        m.load_state_dict(load_file(os.path.join(d, "diffusion_pytorch_model.safetensors")))
        return m

    def _enc_resnet(self, x, pre):
        a1, _ = self.gn(x, pre + ".norm1", True)
        h, _ = self.conv(a1, pre + ".conv1")
        a2, _ = self.gn(h, pre + ".norm2", True)
        if (pre + ".conv_shortcut.weight") in self.ps.specs:
            res, _ = self.conv(x, pre + ".conv_shortcut", ksize=1)
        else:
            res = x
        out, _ = self.conv(a2, pre + ".conv2", residual=res)
        return out


class VAEEncoder(_VAEHalf):
    # ------------------------------------------------------------------ parameters
    def _declare_params(self):
        cfg, a = self.cfg, self.ps.add
        ch = cfg.block_out_channels
        a("conv_in.weight", "conv_in", (ch[0], cfg.in_channels, 3, 3)); a("conv_in.bias", "vec", (ch[0],))
        self.plan = []
        out = ch[0]
        for i, c in enumerate(ch):
            cin, out = out, c
            down = i != len(ch) - 1
            for j in range(cfg.layers_per_block):
                self._declare_enc_resnet(f"down_blocks.{i}.resnets.{j}", cin if j == 0 else out, out)
            if down:
                a(f"down_blocks.{i}.downsamplers.0.conv.weight", "conv3", (out, out, 3, 3))
                a(f"down_blocks.{i}.downsamplers.0.conv.bias", "vec", (out,))
            self.plan.append((i, down))
        c = ch[-1]
        self._declare_enc_resnet("mid_block.resnets.0", c, c)
        self._declare_attn("mid_block.attentions.0", c)
        self._declare_enc_resnet("mid_block.resnets.1", c, c)
        a("conv_norm_out.weight", "vec", (c,)); a("conv_norm_out.bias", "vec", (c,))
        # conv_out with quant_conv folded in (see load_state_dict)
        a("conv_out.weight", "conv3", (2 * cfg.latent_channels, c, 3, 3)); a("conv_out.bias", "vec", (2 * cfg.latent_channels,))

    def load_state_dict(self, sd, strict=True):
        """diffusers AutoencoderKL state dict (decoder / post_quant_conv entries are ignored)."""
        enc = {k[len("encoder."):]: v.float() for k, v in sd.items() if k.startswith("encoder.")}
        wq = sd["quant_conv.weight"].float()[:, :, 0, 0]
        enc["conv_out.bias"] = wq @ enc["conv_out.bias"] + sd["quant_conv.bias"].float()
        enc["conv_out.weight"] = torch.einsum("om,mckl->ockl", wq, enc["conv_out.weight"])
        self.ps.load_state_dict(enc, strict)
        self.refresh_weights(cast_shadow=True)

    # ------------------------------------------------------------------ graph
    @torch.no_grad()
    def moments(self, x):
        """x [N, 3, H, W] images in [-1, 1] (f32 / bf16, device).  Returns (mean, logvar) [N, 4, H/8, W/8] f32."""
        mean, logvar = self.raw_moments(x).chunk(2, dim=1)
        return mean.contiguous(), logvar.clamp(-30.0, 20.0).contiguous()

    @torch.no_grad()
    def raw_moments(self, x):
        """The posterior moments as conv_out (with quant_conv folded in) leaves them: [N, 8, H/8, W/8] f32, the mean in channels
        0..3, the UNCLAMPED log-variance in 4..7 -- what siss_latent_inject (siss_amd/sd_sampler.py) samples from in one launch."""
        cfg = self.cfg
        assert x.is_cuda and x.dim() == 4 and x.shape[1] == cfg.in_channels
        self.tape, self.gmap, self._uid = [], {}, 0
        self.nf = x.shape[0]
        h = self._conv_in(x.contiguous())
        for i, down in self.plan:
            for j in range(cfg.layers_per_block):
                h = self._enc_resnet(h, f"down_blocks.{i}.resnets.{j}")
            if down:
                h = self.downsample(h, f"down_blocks.{i}.downsamplers.0")
        h = self._enc_resnet(h, "mid_block.resnets.0")
        h = self.attention(h, "mid_block.attentions.0")
        h = self._enc_resnet(h, "mid_block.resnets.1")
        a, _ = self.gn(h, "conv_norm_out", True)
        m, _ = self.conv(a, "conv_out")
        self.tape = []                                   # forward only: drop the backward closures
        return m.to_nchw()

    @torch.no_grad()
    def encode(self, x, eps=None, generator=None):
        """``vae.encode(x).latent_dist.sample() * scaling_factor`` (delete_sd.py:879-888)."""
        mean, logvar = self.moments(x)
        if eps is None:
            eps = torch.randn(mean.shape, device=mean.device, generator=generator)
        return (mean + torch.exp(0.5 * logvar) * eps.to(mean.device)) * self.cfg.scaling_factor


class VAEDecoder(_VAEHalf):
    """``AutoencoderKL.decode(z).sample`` of diffusers 0.27 (SD v1.x): post_quant_conv -> conv_in -> mid block (resnet,
    single-head attention, resnet) -> up blocks over the reversed block_out_channels (layers_per_block + 1 resnets each,
    all but the last ending in nearest-2x + 3x3 conv) -> GroupNorm + SiLU -> conv_out.  49,490,179 + 20 parameters at the
    SD v1 sizes."""
    config_class = VAEDecoderConfig

    # ------------------------------------------------------------------ parameters
    def _declare_params(self):
        cfg, a = self.cfg, self.ps.add
        ch = cfg.block_out_channels
        c = ch[-1]
        # conv_in with post_quant_conv folded in, plus the ones channel that carries post_quant_conv's bias (module docstring)
        a("conv_in.weight", "conv_in", (c, cfg.latent_channels + 1, 3, 3)); a("conv_in.bias", "vec", (c,))
        self._declare_enc_resnet("mid_block.resnets.0", c, c)
        self._declare_attn("mid_block.attentions.0", c)
        self._declare_enc_resnet("mid_block.resnets.1", c, c)
        rev = list(reversed(ch))
        self.plan = []
        out = rev[0]
        for i, co in enumerate(rev):
            prev, out = out, co
            up = i != len(ch) - 1
            for j in range(cfg.layers_per_block + 1):
                self._declare_enc_resnet(f"up_blocks.{i}.resnets.{j}", prev if j == 0 else out, out)
            if up:
                a(f"up_blocks.{i}.upsamplers.0.conv.weight", "conv3", (out, out, 3, 3))
                a(f"up_blocks.{i}.upsamplers.0.conv.bias", "vec", (out,))
            self.plan.append((i, up))
        a("conv_norm_out.weight", "vec", (ch[0],)); a("conv_norm_out.bias", "vec", (ch[0],))
        a("conv_out.weight", "conv3", (cfg.out_channels, ch[0], 3, 3)); a("conv_out.bias", "vec", (cfg.out_channels,))

    def diffusers_shapes(self):
        """{diffusers state-dict key: shape} of what load_state_dict consumes (the decoder.* and post_quant_conv.* entries)."""
        lc = self.cfg.latent_channels
        out = {}
        for n, sp in self.ps.specs.items():
            shape = sp.ref_shape
            if n == "conv_in.weight":
                shape = (shape[0], lc, 3, 3)
            out["decoder." + n] = tuple(shape)
        out["post_quant_conv.weight"], out["post_quant_conv.bias"] = (lc, lc, 1, 1), (lc,)
        return out

    def load_state_dict(self, sd, strict=True):
        """diffusers AutoencoderKL state dict (encoder / quant_conv entries are ignored)."""
        dec = {k[len("decoder."):]: v.float() for k, v in sd.items() if k.startswith("decoder.")}
        if strict:
            want = self.diffusers_shapes()
            have = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(("decoder.", "post_quant_conv."))}
            if have != want:
                missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
                bad = sorted(k for k in set(want) & set(have) if want[k] != have[k])
                raise KeyError(f"VAEDecoder.load_state_dict: missing {missing[:8]}, unexpected {extra[:8]}, wrong shape {bad[:8]}")
        wp = sd["post_quant_conv.weight"].float()[:, :, 0, 0]              # [m, c]
        bp = sd["post_quant_conv.bias"].float()
        w_in = dec["conv_in.weight"]                                         # [o, m, 3, 3]
        dec["conv_in.weight"] = torch.cat([torch.einsum("omkl,mc->ockl", w_in, wp),
                                           torch.einsum("omkl,m->okl", w_in, bp)[:, None]], dim=1)
        self.ps.load_state_dict(dec, strict)
        self.refresh_weights(cast_shadow=True)

    # ------------------------------------------------------------------ graph
    def _dec_conv_in(self, x):
        """conv_in over [z, 1] (NCHW f32): im2col rows (K = 9 * 5 padded to 64) then a one-panel GEMM."""
        ps = self.ps
        N, cin, H, W = x.shape
        kp = ps.specs["conv_in.weight"].native_shape[1]
        c = self.cfg.block_out_channels[-1]
        col = self._act("conv_in.col", N, H, W, kp)
        lib.call("siss_im2col3x3", x, 0, col.data, N, cin, H, W, kp, 0)
        h = self._act("conv_in.out", N, H, W, c)
        ops.gemm_nt(lib.ptr(col.data), kp, ps.sh("conv_in.weight"), lib.ptr(h.data), c, col.rows, c, kp, [0], [0],
                    bias=ps.p("conv_in.bias"), rows_per_image=col.rows_per_image, hp=col.hp, wp=col.wp)
        return h

    @torch.no_grad()
    def decode(self, z):
        """z [N, 4, h, w] = latents / scaling_factor (as diffusers' pipelines call it).  Returns [N, 3, 8h, 8w] f32 images,
        about [-1, 1]."""
        cfg, ps = self.cfg, self.ps
        assert z.is_cuda and z.dim() == 4 and z.shape[1] == cfg.latent_channels
        self.tape, self.gmap, self._uid = [], {}, 0
        N, _, h0, w0 = z.shape
        self.nf = N
        ones = torch.ones(N, 1, h0, w0, dtype=torch.float32, device=z.device)
        h = self._dec_conv_in(torch.cat([z.float(), ones], dim=1))
        h = self._enc_resnet(h, "mid_block.resnets.0")
        h = self.attention(h, "mid_block.attentions.0")
        h = self._enc_resnet(h, "mid_block.resnets.1")
        for i, up in self.plan:
            for j in range(cfg.layers_per_block + 1):
                h = self._enc_resnet(h, f"up_blocks.{i}.resnets.{j}")
            if up:
                h = self.upsample(h, f"up_blocks.{i}.upsamplers.0")
        a, _ = self.gn(h, "conv_norm_out", True)
        c0, co = cfg.block_out_channels[0], cfg.out_channels
        img = self._buf("img", (N, co, h.h, h.w))
        lib.call("siss_conv_out_fprop", a.data, ps.p("conv_out.weight"), ps.p("conv_out.bias"), img, N, h.h, h.w, c0, co)
        self.tape = []                                   # forward only: drop the backward closures
        return img.clone()

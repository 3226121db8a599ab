"""Torch-only restatement of the DECODER half of diffusers==0.27.2 ``AutoencoderKL`` (SD v1.x VAE) for the GPU tests of
siss_amd.vae.VAEDecoder: ``decode(z) = decoder(post_quant_conv(z))``.  Test infrastructure only (nothing in siss_amd
imports it).  Pinned, like oracle/vae.py's encoder, by the published parameter count of the SD v1 ``vae`` decoder +
post_quant_conv (49,490,179 + 20) and its state-dict key names.
"""
import torch.nn as nn
import torch.nn.functional as F

from oracle.unet import Attention, Upsample2D
from oracle.vae import EncResnet, VAEConfig


class DecUpBlock(nn.Module):
    """UpDecoderBlock2D: layers_per_block + 1 resnets, then Upsample2D (nearest 2x + 3x3 conv) unless last."""

    def __init__(self, cin, cout, cfg, add_up):
        super().__init__()
        self.resnets = nn.ModuleList([EncResnet(cin if i == 0 else cout, cout, cfg.norm_num_groups, cfg.norm_eps)
                                      for i in range(cfg.layers_per_block + 1)])
        self.add_up = add_up
        if add_up:
            self.upsamplers = nn.ModuleList([Upsample2D(cout)])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if self.add_up else x


class DecMidBlock(nn.Module):
    def __init__(self, ch, cfg):
        super().__init__()
        self.resnets = nn.ModuleList([EncResnet(ch, ch, cfg.norm_num_groups, cfg.norm_eps) for _ in range(2)])
        self.attentions = nn.ModuleList([Attention(ch, ch, cfg.norm_num_groups, cfg.norm_eps)])   # one head of `ch`

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class Decoder(nn.Module):
    def __init__(self, cfg, out_channels=3):
        super().__init__()
        ch = cfg.block_out_channels
        rev = list(reversed(ch))
        self.conv_in = nn.Conv2d(cfg.latent_channels, rev[0], 3, padding=1)
        self.mid_block = DecMidBlock(rev[0], cfg)
        self.up_blocks = nn.ModuleList()
        out = rev[0]
        for i, c in enumerate(rev):
            prev, out = out, c
            self.up_blocks.append(DecUpBlock(prev, out, cfg, i != len(ch) - 1))
        self.conv_norm_out = nn.GroupNorm(cfg.norm_num_groups, ch[0], eps=cfg.norm_eps)
        self.conv_out = nn.Conv2d(ch[0], out_channels, 3, padding=1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class RefVAEDecoder(nn.Module):
    """``vae.decode(z).sample`` with z = latents / scaling_factor."""

    def __init__(self, cfg: VAEConfig):
        super().__init__()
        self.cfg = cfg
        self.decoder = Decoder(cfg)
        self.post_quant_conv = nn.Conv2d(cfg.latent_channels, cfg.latent_channels, 1)

    def forward(self, z):
        return self.decoder(self.post_quant_conv(z))

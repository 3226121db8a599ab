"""Stable Diffusion validation sampling on the HIP forward kernels: the reference's ``LocalStableDiffusionPipeline.__call__``
(data/src/local_sd_pipeline.py:60-215) with ``DDIMScheduler.from_config`` (delete_sd.py:204), as ``log_validation``
(delete_sd.py:170-340) runs it after every optimizer step.

Per denoising step: ONE replay of the captured text-conditioned UNet forward over the 2n batch (``cat([x, x])``,
``cat([uncond, text])``) and ONE fused launch (csrc/siss_loss.hip ``siss_cfg_ddim_step``) that applies classifier-free
guidance and the DDIM update and leaves the step's per-block partial sums of ||eps_uncond||^2 and ||eps_text - eps_uncond||^2
in a [steps, 2, n, blocks] slab.  The host reads that slab ONCE, after the last step (the reference pays 2n ``.item()``
syncs per step for the same norms), and sums each sample's partials in f64.  Then the VAE decoder (siss_amd/vae.py) and
diffusers' postprocess.

The img2img half of that class (``get_timesteps``, ``prepare_latents_img2img``, :241-323) enters the same loop part of the way
down: ``denoise_injection`` noises an image's latents to the first remaining timestep -- ONE launch from the VAE encoder's posterior
moments (csrc/injection.hip ``siss_latent_inject``) -- and denoises them back under the prompt.

OPT-IN (``pipeline.sampler``; not the reference's protocol): ``SDSampler(scheduler=DPMSolverMultistepScheduler(...))`` runs the same loop
with DPM-Solver++ multistep updates (csrc/dpm_solver.hip ``siss_cfg_dpmpp_step``: one launch per step, the same noise norms, one extra
buffer for the previous x0-prediction) in place of the DDIM step; a suffix of the grid (img2img) starts at order 1.
"""
import contextlib
import os

import torch

from . import lib
from .sampler import Evaluator
from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler

# CLIPTokenizer("") of the SD v1 checkpoints padded to 77: <|startoftext|>, then <|endoftext|> as the pad token
SD_V1_UNCOND_IDS = [49406] + [49407] * 76


def uncond_ids(path=None):
    """[1, 77] token ids of the empty prompt (diffusers' default negative prompt): the checkpoint's own tokenizer/ when it is
    on disk, else SD_V1_UNCOND_IDS."""
    if path and os.path.isdir(os.path.join(str(path), "tokenizer")):
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(str(path), subfolder="tokenizer")
        return tok([""], max_length=tok.model_max_length, padding="max_length", truncation=True, return_tensors="pt").input_ids
    return torch.tensor([SD_V1_UNCOND_IDS], dtype=torch.long)


def ddim_blocks(n, chw):
    """Blocks per sample of siss_cfg_ddim_step: one per 1024 elements (one f32x4 sweep of 256 lanes), the grid capped at
    2048 blocks (a streaming kernel: cdna_hip_programming.md Guideline 11); the rest is grid-strided."""
    return max(1, min(-(-chw // 1024), 2048 // n, 1024))


def cfg_ddim_step(eps, x, out, coeffs, guidance, clip=0.0, norms=None):
    """out = DDIM step (eta = 0) of x under eps_uncond + g (eps_text - eps_uncond); eps [2n, ...] when guidance > 1 (the
    partial sums of the two norms go to `norms`, [2, n, ddim_blocks(n, chw)] f32), else [n, ...].  coeffs:
    DDIMScheduler.coeffs(t).  out may be x."""
    n, chw = x.shape[0], x[0].numel()
    cfg = guidance > 1.0
    assert x.dtype == eps.dtype == out.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous() and out.is_contiguous()
    assert eps.numel() == (2 if cfg else 1) * n * chw and out.shape == x.shape
    nblk = ddim_blocks(n, chw)
    if cfg:
        assert norms is not None and norms.dtype == torch.float32 and norms.is_contiguous() and norms.numel() == 2 * n * nblk
    lib.call("siss_cfg_ddim_step", eps, x, out, n, chw, float(guidance), *coeffs, float(clip), norms if cfg else None, nblk)
    return out


def cfg_dpmpp_step(eps, x, m_prev, x_out, m_out, coeffs, guidance, norms=None, nblk=None):
    """(x_out, m_out) = one DPM-Solver++ multistep update of x under eps_uncond + g (eps_text - eps_uncond): m_out the step's
    x0-prediction, m_prev the previous step's (None exactly when coeffs[4] == 0: an order-1 or final step).  eps [2n, ...] when
    guidance > 1 (the partial sums of the two norms go to `norms`, [2, n, ddim_blocks(n, chw)] f32: the bits siss_cfg_ddim_step
    leaves), else [n, ...].  coeffs: DPMSolverMultistepScheduler.coeffs(i).  x_out may be x, m_out may be m_prev."""
    n, chw = x.shape[0], x[0].numel()
    cfg = guidance > 1.0
    for t in (eps, x, x_out, m_out) + (() if m_prev is None else (m_prev,)):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert eps.numel() == (2 if cfg else 1) * n * chw and x_out.shape == m_out.shape == x.shape
    assert m_prev is None or m_prev.shape == x.shape
    nblk = ddim_blocks(n, chw) if nblk is None else int(nblk)
    if cfg and norms is not None:
        assert norms.dtype == torch.float32 and norms.is_contiguous() and norms.numel() == 2 * n * nblk
    lib.call("siss_cfg_dpmpp_step", eps, x, m_prev, x_out, m_out, n, chw, float(guidance), *coeffs, norms if cfg else None, nblk)
    return x_out, m_out


def latent_inject(moments, eps_z, eps_t, scaling, a, b, out=None, nblk=None):
    """x[i] = a * ((mean[j] + exp(0.5 * clamp(logvar[j], -30, 20)) * eps_z[j]) * scaling) + b * eps_t[i], j = i mod m: the n
    starting latents of an img2img DDIM loop from the posterior moments [m, 2C, h, w] (f32 or bf16; mean first) of m images,
    eps_z [m, C, h, w] and eps_t [n, C, h, w] (f32).  a, b: sqrt(alphas_cumprod[t]), sqrt(1 - alphas_cumprod[t]).  nblk: blocks per
    sample (default ddim_blocks: the same capped grid as the DDIM step)."""
    m, n = moments.shape[0], eps_t.shape[0]
    chw = eps_t[0].numel()
    if moments.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"moments of dtype {moments.dtype}: f32 or bf16 are taken")
    assert eps_z.dtype == eps_t.dtype == torch.float32 and moments.is_contiguous() and eps_z.is_contiguous() and eps_t.is_contiguous()
    assert moments[0].numel() == 2 * chw and eps_z.shape[0] == m and eps_z[0].numel() == chw
    out = torch.empty_like(eps_t) if out is None else out
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == eps_t.shape
    lib.call("siss_latent_inject", moments, int(moments.dtype == torch.bfloat16), eps_z, eps_t, out, m, n, chw, float(scaling),
             float(a), float(b), ddim_blocks(n, chw) if nblk is None else int(nblk))
    return out


class SDSampler:
    """Text-to-image pipeline over the HIP ``UNet2DConditionModel``, ``VAEDecoder`` and ``CLIPTextEncoder``; the call surface of
    the reference's LocalStableDiffusionPipeline.  ``unconditional_ids``: token ids of the negative (empty) prompt; or pass
    ``negative_prompt_embeds`` to every call (then no text encoder is needed).  ``vae_encoder``: the VAEEncoder that
    ``denoise_injection`` / ``prepare_latents_img2img`` turn an image into latents with (not needed for 4-channel latents)."""

    def __init__(self, unet, vae=None, text_encoder=None, scheduler=None, unconditional_ids=None, use_graph=True,
                 vae_encoder=None):
        self.unet, self.vae, self.text_encoder, self.vae_encoder = unet, vae, text_encoder, vae_encoder
        self.scheduler = scheduler or DDIMScheduler.from_pretrained(None)
        self.unconditional_ids = torch.tensor([SD_V1_UNCOND_IDS]) if unconditional_ids is None else unconditional_ids
        self.use_graph = use_graph
        self._ev, self._hold = None, False
        self.vae_scale_factor = 2 ** (len(vae.cfg.block_out_channels) - 1) if vae is not None else 8

    @contextlib.contextmanager
    def holding_graphs(self):
        """Calls inside the block share their captured forwards (one capture per batch shape for a whole validation pass);
        they are dropped when it ends.  Outside such a block every call drops its own."""
        self._hold = True
        try:
            yield self
        finally:
            self._hold, self._ev = False, None

    def _negative(self, n_prompts):
        if self.text_encoder is None:
            raise ValueError("classifier-free guidance needs negative_prompt_embeds or a text encoder for the empty prompt")
        e = self.text_encoder(self.unconditional_ids.reshape(1, -1))[0].float()
        return e.expand(n_prompts, *e.shape[1:])

    def _ddim_only(self, what):
        if isinstance(self.scheduler, DPMSolverMultistepScheduler):
            raise NotImplementedError(f"{what} is defined on the DDIM step: build the SDSampler with a DDIMScheduler, not with "
                                      f"{self.scheduler.label}")

    def _check_call(self, output_type, eta, lp):
        if eta != 0.0:
            raise NotImplementedError(f"eta={eta}: only the deterministic DDIM step (eta = 0) is implemented")
        if lp != 2:
            raise NotImplementedError(f"lp={lp}: only the L2 noise norm is implemented")
        if output_type not in ("pil", "np", "latent", "decoded"):
            raise ValueError(f"output_type={output_type!r}: one of 'pil', 'np', 'latent', 'decoded'")
        if output_type != "latent" and self.vae is None:
            raise ValueError(f"output_type={output_type!r} needs a VAE decoder")

    def _embeddings(self, prompt_embeds, negative_prompt_embeds, num_images_per_prompt, cfg):
        """(the UNet's encoder_hidden_states -- uncond rows first under guidance, as diffusers orders them --, images n)."""
        dev = self.unet.device
        text = prompt_embeds.to(dev).float().repeat_interleave(num_images_per_prompt, dim=0)
        if not cfg:
            return text.contiguous(), text.shape[0]
        neg = self._negative(prompt_embeds.shape[0]) if negative_prompt_embeds is None else negative_prompt_embeds
        neg = neg.to(dev).float().repeat_interleave(num_images_per_prompt, dim=0)
        return torch.cat([neg, text]).contiguous(), text.shape[0]

    def _denoise(self, x, steps, emb, guidance_scale, output_type, track_noise_norm):
        """The per-step loop over the timesteps `steps` (a suffix of the scheduler's current set_timesteps) from the start latents
        x [n, C, h, w] (f32, contiguous, overwritten), then the noise norms and the output of `output_type`."""
        unet, sch = self.unet, self.scheduler
        dev = unet.device
        cfg = guidance_scale > 1.0
        n = x.shape[0]
        solver = isinstance(sch, DPMSolverMultistepScheduler)       # opt-in: DPM-Solver++ (2M) instead of the DDIM step
        clip = 0.0 if solver else (sch.clip_sample_range if sch.clip_sample else 0.0)
        first = sch.timesteps.index(steps[0]) if solver else 0      # a suffix (img2img) starts at order 1: there is no earlier m
        m = torch.empty_like(x) if solver else None                 # the one extra buffer: the previous step's x0-prediction
        chw = x[0].numel()
        slab = torch.zeros(len(steps), 2, n, ddim_blocks(n, chw), dtype=torch.float32, device=dev) if cfg else None
        unet.engine.refresh_weights(cast_shadow=True)
        if self._ev is None:
            self._ev = Evaluator(use_graph=self.use_graph)
            self._ev.load_model(unet, None)
        try:
            for i, t in enumerate(steps):
                eps = self._ev._eps(torch.cat([x, x]) if cfg else x, t, emb)
                if solver:
                    co = sch.coeffs(first + i, first=(i == 0))
                    cfg_dpmpp_step(eps, x, m if co[4] != 0.0 else None, x, m, co, guidance_scale, slab[i] if cfg else None)
                else:
                    cfg_ddim_step(eps, x, x, sch.coeffs(t), guidance_scale, clip, slab[i] if cfg else None)
        finally:
            if not self._hold:
                self._ev = None                          # the captured graphs and their static buffers live for this call only
        stats = {"uncond_noise_norm": [], "text_noise_norm": []}
        if cfg:
            nrm = slab.cpu().double().sum(-1).sqrt()     # [steps, 2, n]: the one device -> host read of the loop
            stats["uncond_noise_norm"] = nrm[:, 0].t().tolist()
            stats["text_noise_norm"] = nrm[:, 1].t().tolist()
        if not track_noise_norm:
            stats = {"uncond_noise_norm": None, "text_noise_norm": None}
        if output_type == "latent":
            return x, stats
        img = self.vae.decode(x / self.vae.cfg.scaling_factor)
        if output_type == "decoded":
            return img, stats
        u8 = ((img / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        if output_type == "np":
            return u8, stats
        from PIL import Image
        return [Image.fromarray(a) for a in u8], stats

    @torch.no_grad()
    def __call__(self, prompt_embeds, negative_prompt_embeds=None, num_inference_steps=50, guidance_scale=7.5,
                 num_images_per_prompt=1, generator=None, latents=None, output_type="pil", track_noise_norm=True,
                 height=None, width=None, eta=0.0, lp=2):
        """prompt_embeds [B, L, X].  Returns (images, {"uncond_noise_norm", "text_noise_norm"}): images a list of PIL images
        ("pil"), a uint8 [n, H, W, 3] array ("np"), the final latents ("latent") or the VAE decoder's raw output [n, 3, H, W] on the
        device ("decoded": what KMeansClassifier.from_decoded turns into the uint8 images and their labels without leaving it); the
        norms per image and denoising step, in step order (empty without guidance)."""
        self._check_call(output_type, eta, lp)
        unet = self.unet
        dev = unet.device
        cfg = guidance_scale > 1.0                       # do_classifier_free_guidance (local_sd_pipeline.py:109)
        emb, n = self._embeddings(prompt_embeds, negative_prompt_embeds, num_images_per_prompt, cfg)
        C, s = unet.config.in_channels, unet.config.sample_size
        h = (height or s * self.vae_scale_factor) // self.vae_scale_factor
        w = (width or s * self.vae_scale_factor) // self.vae_scale_factor
        if latents is None:
            gdev = generator.device if generator is not None else dev
            latents = torch.randn((n, C, h, w), generator=generator, device=gdev)
        x = latents.to(dev).float().contiguous().clone()       # (DDIM: init_noise_sigma = 1)
        steps = self.scheduler.set_timesteps(num_inference_steps)
        return self._denoise(x, steps, emb, guidance_scale, output_type, track_noise_norm)

    def get_timesteps(self, num_inference_steps, strength, device=None):
        """The reference's get_timesteps (data/src/local_sd_pipeline.py:241-248): (the last init_timestep = min(int(steps *
        strength), steps) timesteps of set_timesteps(steps), their count).  The scheduler's order is 1; `device` is accepted for the
        reference's signature (the timesteps are host integers).  No step left (strength * steps < 1) raises."""
        n = int(num_inference_steps)
        init_timestep = min(int(n * strength), n)
        t_start = max(n - init_timestep, 0)
        timesteps = self.scheduler.set_timesteps(n)[t_start:]
        if not timesteps:
            raise ValueError(f"strength={strength!r} of num_inference_steps={n} leaves no denoising step (int({n} * {strength!r}) "
                             "< 1)")
        return timesteps, n - t_start

    @torch.no_grad()
    def prepare_latents_img2img(self, image, timestep, batch_size, num_images_per_prompt, dtype=None, device=None, generator=None):
        """The reference's prepare_latents_img2img (:250-323): `image` [m, 4, h, w] is taken as latents; any other image [m, 3, H, W]
        in [-1, 1] goes through the VAE encoder and its posterior is sampled (normals drawn first) and scaled.  The m latents are
        tiled to batch_size * num_images_per_prompt (a multiple of m, else ValueError) as torch.cat([latents] * k) orders them and
        noised to `timestep` with normals drawn second -- sample, scale, tile and add_noise in ONE launch (siss_latent_inject; latents
        go in as moments of zero variance: mean + std * 0 = mean exactly).  Returns [n, C, h, w] f32."""
        if isinstance(generator, (list, tuple)):
            raise NotImplementedError("a list of generators (one per image) is not implemented: pass one generator")
        if dtype not in (None, torch.float32):
            raise NotImplementedError(f"dtype={dtype}: the starting latents of the loop are f32")
        dev = torch.device(device) if device is not None else self.unet.device
        gdev = generator.device if generator is not None else dev
        image = image.to(dev)
        if image.dim() != 4:
            raise ValueError(f"image of shape {tuple(image.shape)}: [m, C, H, W] is needed")
        want = batch_size * num_images_per_prompt
        if image.shape[1] == 4:
            z = image.float()
            moments = torch.cat([z, torch.zeros_like(z)], dim=1).contiguous()
            eps_z, scaling = torch.zeros_like(z).contiguous(), 1.0
        else:
            if self.vae_encoder is None:
                raise ValueError(f"an image with {image.shape[1]} channels has to be encoded: SDSampler(vae_encoder=...) is needed")
            moments = self.vae_encoder.raw_moments(image)
            m, c2, h, w = moments.shape
            eps_z = torch.randn((m, c2 // 2, h, w), generator=generator, device=gdev).to(dev)   # latent_dist.sample(generator)
            scaling = self.vae_encoder.cfg.scaling_factor
        m = moments.shape[0]
        if want > m and want % m != 0:
            raise ValueError(f"Cannot duplicate `image` of batch size {m} to {want} text prompts.")
        n = want if want > m else m
        eps_t = torch.randn((n, *eps_z.shape[1:]), generator=generator, device=gdev).to(dev)
        ac = self.scheduler.alphas_cumprod[int(timestep)]                  # add_noise's f32 coefficients
        return latent_inject(moments, eps_z, eps_t, scaling, float(ac ** 0.5), float((1 - ac) ** 0.5))

    @torch.no_grad()
    def denoise_injection(self, image, prompt_embeds, strength=0.5, negative_prompt_embeds=None, num_inference_steps=50,
                          guidance_scale=7.5, num_images_per_prompt=1, generator=None, output_type="pil", track_noise_norm=True,
                          eta=0.0, lp=2):
        """Inject-then-denoise: `image` (latents [m, 4, h, w], or images [m, 3, H, W] in [-1, 1] through the VAE encoder) noised to
        the first of the last int(num_inference_steps * strength) timesteps, then denoised under the prompt over those timesteps --
        the reference pipeline's img2img entry (get_timesteps, prepare_latents_img2img) into the loop of __call__.  Returns what
        __call__ returns for `output_type`; the noise norms have one entry per executed step."""
        self._check_call(output_type, eta, lp)
        cfg = guidance_scale > 1.0
        emb, _ = self._embeddings(prompt_embeds, negative_prompt_embeds, num_images_per_prompt, cfg)
        steps, _ = self.get_timesteps(num_inference_steps, strength)
        x = self.prepare_latents_img2img(image, steps[0], prompt_embeds.shape[0], num_images_per_prompt, generator=generator)
        if x.shape[0] != emb.shape[0] // (2 if cfg else 1):
            raise ValueError(f"{x.shape[0]} starting latents for {emb.shape[0] // (2 if cfg else 1)} prompt rows: pass at most as "
                             "many images as prompts x num_images_per_prompt")
        return self._denoise(x, steps, emb, guidance_scale, output_type, track_noise_norm)

    def aug_prompt(self, prompt=None, height=None, width=None, num_inference_steps=50, guidance_scale=7.5, negative_prompt=None,
                   num_images_per_prompt=1, eta=0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                   target_steps=(0,), lr=0.1, optim_iters=10, target_loss=None, print_optim=False, optim_epsilon=None, alpha=0.5,
                   return_trace=False):
        """The reference's LocalStableDiffusionPipeline.aug_prompt (data/src/local_sd_pipeline.py:474-663), its argument names and
        defaults: the prompt embedding [1, L, X] optimised (AdamW, row 0's gradient masked) so that the text-conditional noise norm
        at the first target step goes down -- what validation_prompts[0] takes under using_augmented_prompt.  siss_amd/prompt_aug.py."""
        from . import prompt_aug
        self._ddim_only("aug_prompt")
        return prompt_aug.aug_prompt(self, prompt, height, width, num_inference_steps, guidance_scale, negative_prompt,
                                     num_images_per_prompt, eta, generator, latents, prompt_embeds, negative_prompt_embeds,
                                     target_steps, lr, optim_iters, target_loss, print_optim, optim_epsilon, alpha, return_trace)

    def get_text_cond_grad(self, prompt=None, height=None, width=None, num_inference_steps=50, guidance_scale=7.5,
                           negative_prompt=None, num_images_per_prompt=1, eta=0.0, generator=None, latents=None, prompt_embeds=None,
                           negative_prompt_embeds=None, target_steps=(0,), return_trace=False):
        """The reference's get_text_cond_grad (:325-445): per-token L2 norms [L] of the noise norm's gradient with respect to the TEXT
        embedding, averaged over the target steps.  siss_amd/prompt_aug.py."""
        from . import prompt_aug
        self._ddim_only("get_text_cond_grad")
        return prompt_aug.get_text_cond_grad(self, prompt, height, width, num_inference_steps, guidance_scale, negative_prompt,
                                             num_images_per_prompt, eta, generator, latents, prompt_embeds, negative_prompt_embeds,
                                             target_steps, return_trace)

"""Prompt-embedding gradients of the SD UNet and the augmented prompt built on them: the reference's
``LocalStableDiffusionPipeline.get_text_cond_grad`` (data/src/local_sd_pipeline.py:325-445) and ``aug_prompt`` (:474-663), whose
result ``delete_sd.py`` reads back as ``validation_prompts[0]`` under ``using_augmented_prompt`` (:175-177, :235-241, :938).

Both differentiate the text-conditional noise norm  ||eps(z, t, e) - eps(z, t, empty)||_2  with respect to the prompt embedding e.
The reference runs a 2n-image forward and a full autograd backward per iteration; here

* the unconditional prediction u = eps(z, t, empty) depends neither on e nor on the iteration: ONE forward per target step;
* an iteration is one forward of the n text samples, one launch pair for the loss and its cotangent (csrc/prompt_grad.hip
  ``siss_noise_norm_cot``: the scalar stays on the device), ``UNetCondEngine.context_vjp`` -- a data-gradient-only backward over
  the n text samples, summed over them in f32 in a fixed order -- and one launch for the masked / penalised AdamW step
  (``siss_prompt_embed_update``);
* the host reads the loss only where the loop needs it (``target_loss``, ``print_optim``); otherwise once, after the last iteration.

So one ``aug_prompt`` call is 1 + optim_iters forwards of n images and optim_iters data-only backwards of n images.  The text forward
is the last forward before ``context_vjp`` (the engine keeps one set of saved activations).

Deliberate deviation: the reference's ``get_text_cond_grad`` cannot run as written -- it differentiates with
respect to a tensor that is not in the graph and swaps the text and dummy rows relative to ``aug_prompt``; here it is the gradient with
respect to the TEXT embedding with the empty prompt as the dummy, consistent with ``aug_prompt``.
"""
import json
import math
import os

import torch

from . import lib
from .sd_sampler import cfg_ddim_step, ddim_blocks

ADAMW_BETAS, ADAMW_EPS, ADAMW_WEIGHT_DECAY = (0.9, 0.999), 1e-8, 1e-2      # torch.optim.AdamW([e], lr=lr): its defaults


def noise_norm_cot(p, u, cot, loss, partials=None):
    """loss[0] = ||p - u||_2 over ALL elements, cot = (p - u) / loss (zeros when the norm is zero).  p, u, cot: [n, ...] f32 on the
    device; loss: a 1-element f32 view; partials: f64 scratch (allocated when None)."""
    n, chw = p.shape[0], p[0].numel()
    for t in (p, u, cot):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n * chw
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1
    words = int(lib.query("siss_noise_norm_partials_words", n, chw))
    if partials is None:
        partials = torch.empty(words, dtype=torch.float64, device=p.device)
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= words
    lib.call("siss_noise_norm_cot", p, u, n, chw, cot, loss, partials)
    return cot


def bias_corrections(step, betas=ADAMW_BETAS):
    """(1 - beta1^t, sqrt(1 - beta2^t)) in f64, as the flat-buffer AdamW's callers form them."""
    return 1.0 - betas[0] ** step, math.sqrt(1.0 - betas[1] ** step)


def embed_update(e, e0, g, m, v, dist, step, lr, alpha=0.5, optim_epsilon=None, betas=ADAMW_BETAS, eps=ADAMW_EPS,
                 weight_decay=ADAMW_WEIGHT_DECAY):
    """One step on the embedding e [L, X] f32 in place: row 0's gradient is zero (it still takes the decoupled decay); with
    optim_epsilon set and the mean row distance to e0 above it, rows 1.. take alpha g + (1 - alpha) d(mean distance) / de."""
    L, X = e.shape
    for t in (e, g, m, v):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (L, X)
    assert dist.dtype == torch.float64 and dist.numel() >= L
    pen = optim_epsilon is not None
    if pen:
        assert e0 is not None and e0.dtype == torch.float32 and e0.is_contiguous() and tuple(e0.shape) == (L, X)
    bc1, bc2s = bias_corrections(step, betas)
    lib.call("siss_prompt_embed_update", e, e0 if pen else None, g, m, v, dist, L, X, float(lr), float(betas[0]), float(betas[1]),
             float(eps), float(weight_decay), float(bc1), float(bc2s), float(alpha), float(optim_epsilon or 0.0), int(pen))


def _refuse(eta, prompt, negative_prompt, guidance_scale, prompt_embeds):
    if eta != 0.0:
        raise NotImplementedError(f"eta={eta}: only the deterministic DDIM step (eta = 0) is implemented")
    if prompt is not None or negative_prompt is not None:
        raise NotImplementedError("prompt / negative_prompt strings: pass prompt_embeds (and negative_prompt_embeds), as to __call__")
    if not guidance_scale > 1.0:
        raise ValueError(f"guidance_scale={guidance_scale}: the text-conditional noise norm needs classifier-free guidance (> 1)")
    if prompt_embeds is None or prompt_embeds.dim() != 3 or prompt_embeds.shape[0] != 1:
        raise ValueError("prompt_embeds: one prompt's embedding [1, L, X]")


class _Setup:
    """What both methods share: the two embeddings, the initial latents, the timesteps and the guided DDIM advance."""

    def __init__(self, sampler, prompt_embeds, negative_prompt_embeds, num_inference_steps, guidance_scale, n, generator, latents,
                 height, width):
        unet = sampler.unet
        self.sampler, self.eng, self.dev, self.n, self.guidance = sampler, unet.engine, unet.device, int(n), float(guidance_scale)
        dev = self.dev
        self.e = prompt_embeds.to(dev).float().contiguous()                               # [1, L, X]
        neg = sampler._negative(1) if negative_prompt_embeds is None else negative_prompt_embeds
        self.e_neg = neg.to(dev).float().contiguous()
        if self.e_neg.shape != self.e.shape:
            raise ValueError(f"negative_prompt_embeds {tuple(self.e_neg.shape)} against prompt_embeds {tuple(self.e.shape)}")
        C, s = unet.config.in_channels, unet.config.sample_size
        h = (height or s * sampler.vae_scale_factor) // sampler.vae_scale_factor
        w = (width or s * sampler.vae_scale_factor) // sampler.vae_scale_factor
        if latents is None:
            gdev = generator.device if generator is not None else dev
            latents = torch.randn((self.n, C, h, w), generator=generator, device=gdev)
        self.z = latents.to(dev).float().contiguous().clone()
        if self.z.shape[0] != self.n:
            raise ValueError(f"latents: {self.z.shape[0]} samples, num_images_per_prompt = {self.n}")
        self.sch = sampler.scheduler
        self.steps = self.sch.set_timesteps(num_inference_steps)
        self.clip = self.sch.clip_sample_range if self.sch.clip_sample else 0.0
        self.neg_n = self.e_neg.repeat(self.n, 1, 1)
        self._norms, self._cfg_emb = None, None             # built by the first DDIM step / guided advance: target step 0 needs neither
        unet.engine.refresh_weights(cast_shadow=True)

    def t_of(self, i):
        return torch.full((self.n,), int(self.steps[i]), dtype=torch.long, device=self.dev)

    def ddim(self, eps, i):
        """z <- one DDIM step (eta = 0) under eps_uncond + g (eps_text - eps_uncond), eps [2n, ...]."""
        if self._norms is None:
            self._norms = torch.zeros(2, self.n, ddim_blocks(self.n, self.z[0].numel()), dtype=torch.float32, device=self.dev)
        cfg_ddim_step(eps, self.z, self.z, self.sch.coeffs(self.steps[i]), self.guidance, self.clip, self._norms)

    def advance(self, i):
        """Step i of the sampler's own loop: one forward over the 2n batch (captured, as in __call__) and the fused DDIM step."""
        from .sampler import Evaluator
        s = self.sampler
        if s._ev is None:
            s._ev = Evaluator(use_graph=s.use_graph)
            s._ev.load_model(s.unet, None)
        if self._cfg_emb is None:                           # uncond rows first, as __call__ orders them: the ORIGINAL embedding
            self._cfg_emb = torch.cat([self.neg_n, self.e.repeat(self.n, 1, 1)]).contiguous()
        self.ddim(s._ev._eps(torch.cat([self.z, self.z]), self.steps[i], self._cfg_emb), i)

    def done(self):
        if not self.sampler._hold:
            self.sampler._ev = None

    def uncond(self, i):
        """u = eps(z, t_i, empty prompt), kept: the engine's output buffer is the next forward's."""
        return self.eng.forward(self.z, self.t_of(i), self.neg_n).clone()

    def text(self, i, e_n):
        """p = eps(z, t_i, e): the forward context_vjp differentiates (the engine's own output buffer, valid until the next forward)."""
        return self.eng.forward(self.z, self.t_of(i), e_n)


def _target(target_steps, nsteps):
    ts = sorted({int(t) for t in target_steps})
    if not ts or ts[0] < 0 or ts[-1] >= nsteps:
        raise ValueError(f"target_steps={list(target_steps)}: indices into the {nsteps} inference steps")
    return ts


@torch.no_grad()
def aug_prompt(sampler, prompt=None, height=None, width=None, num_inference_steps=50, guidance_scale=7.5, negative_prompt=None,
               num_images_per_prompt=1, eta=0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
               target_steps=(0,), lr=0.1, optim_iters=10, target_loss=None, print_optim=False, optim_epsilon=None, alpha=0.5,
               return_trace=False):
    """The prompt embedding optimised so that the text-conditional noise norm at the first target step goes down: [1, L, X] f32.
    return_trace: also {"noise_norm": [per iteration], "iterations": updates done, "stopped_early": bool, "step": i, "timestep": t}."""
    _refuse(eta, prompt, negative_prompt, guidance_scale, prompt_embeds)
    st = _Setup(sampler, prompt_embeds, negative_prompt_embeds, num_inference_steps, guidance_scale, num_images_per_prompt,
                generator, latents, height, width)
    i = _target(target_steps, len(st.steps))[0]               # the loop returns at the first target step it reaches
    try:
        for k in range(i):
            st.advance(k)
    finally:
        st.done()
    dev, n, eng = st.dev, st.n, st.eng
    L, X = st.e.shape[1:]
    e = st.e[0].clone()                                        # [L, X]: the optimised tensor
    e0 = st.e[0].clone() if optim_epsilon is not None else None
    m, v, g = torch.zeros_like(e), torch.zeros_like(e), torch.empty_like(e)
    dist = torch.zeros(L, dtype=torch.float64, device=dev)
    iters = int(optim_iters)
    losses = torch.zeros(max(iters, 1), dtype=torch.float32, device=dev)
    cot = torch.empty_like(st.z)
    partials = torch.empty(int(lib.query("siss_noise_norm_partials_words", n, st.z[0].numel())), dtype=torch.float64, device=dev)
    e_n = torch.empty(n, L, X, dtype=torch.float32, device=dev)
    u = st.uncond(i)                                           # once: it depends neither on e nor on the iteration
    done, early = 0, False
    for j in range(iters):
        e_n.copy_(e.unsqueeze(0).expand(n, L, X))
        p = st.text(i, e_n)
        noise_norm_cot(p, u, cot, losses[j:j + 1], partials)
        if target_loss is not None and float(losses[j]) <= target_loss:     # (the one host read the loop needs) stop BEFORE the update
            early = True
            if print_optim:
                print(f"step: {j}, curr loss: {float(losses[j])}")
            done = j + 1
            break
        eng.context_vjp(cot, out=g, reduce=True)
        embed_update(e, e0, g, m, v, dist, j + 1, lr, alpha, optim_epsilon)
        done = j + 1
        if print_optim:
            print(f"step: {j}, curr loss: {float(losses[j])}")
    out = e.unsqueeze(0).clone()
    if not return_trace:
        return out
    trace = {"noise_norm": losses[:done].cpu().tolist(), "iterations": done - int(early), "stopped_early": early, "step": i,
             "timestep": int(st.steps[i])}
    return out, trace


@torch.no_grad()
def get_text_cond_grad(sampler, prompt=None, height=None, width=None, num_inference_steps=50, guidance_scale=7.5,
                       negative_prompt=None, num_images_per_prompt=1, eta=0.0, generator=None, latents=None, prompt_embeds=None,
                       negative_prompt_embeds=None, target_steps=(0,), return_trace=False):
    """Per-token L2 norms [L] of d ||eps(z, t, e) - eps(z, t, empty)||_2 / de, averaged over the target steps; between the steps the
    latents advance under guidance.  return_trace: also {"per_step": [L] per target step, "latents": z at each target step,
    "noise_norm": per target step}."""
    _refuse(eta, prompt, negative_prompt, guidance_scale, prompt_embeds)
    st = _Setup(sampler, prompt_embeds, negative_prompt_embeds, num_inference_steps, guidance_scale, num_images_per_prompt,
                generator, latents, height, width)
    ts = _target(target_steps, len(st.steps))
    dev, n = st.dev, st.n
    L, X = st.e.shape[1:]
    e_n = st.e.repeat(n, 1, 1).contiguous()
    g = torch.empty(L, X, dtype=torch.float32, device=dev)
    cot = torch.empty_like(st.z)
    losses = torch.zeros(len(ts), dtype=torch.float32, device=dev)
    vecs, lat = [], []
    try:
        for i in range(ts[-1] + 1):
            if i not in ts:
                st.advance(i)
                continue
            lat.append(st.z.clone())
            u = st.uncond(i)
            p = st.text(i, e_n)
            noise_norm_cot(p, u, cot, losses[len(vecs):len(vecs) + 1])
            st.eng.context_vjp(cot, out=g, reduce=True)
            vecs.append(g.norm(p=2, dim=-1))
            if i != ts[-1]:
                st.ddim(torch.cat([u, p]), i)                  # the step's two predictions are at hand: no third forward
    finally:
        st.done()
    out = torch.stack(vecs).mean(0)
    if not return_trace:
        return out
    return out, {"per_step": vecs, "latents": lat, "noise_norm": losses.cpu().tolist(), "steps": ts}


def save_aug_prompt(path, embeds, trace=None, token_grads=None):
    """Write the [1, L, X] f32 embedding as the .pt that validation_prompts[0] consumes and, beside it (<path minus .pt>.json), the
    per-iteration noise norms and (when given) the per-token gradient norms."""
    e = embeds.detach().float().cpu().reshape(1, embeds.shape[-2], embeds.shape[-1]).contiguous()
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    torch.save(e, path)
    side = os.path.splitext(path)[0] + ".json"
    rec = dict(trace or {})
    rec["shape"] = list(e.shape)
    if token_grads is not None:
        rec["token_grad_norms"] = [float(x) for x in token_grads.detach().cpu().reshape(-1)]
    with open(side, "w") as f:
        json.dump(rec, f, indent=1)
    return path, side

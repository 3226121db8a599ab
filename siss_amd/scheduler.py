"""DDPM noise schedule (the part of diffusers' DDPMScheduler the unlearning loop uses:
delete_celeb.py:229 load, :367-371 alphas_cumprod -> gamma/sigma, :602-603 add_noise;
config/train_tshirt_mnist.yaml:43-50 for the initialise-from-config form)."""
import json
import os

import torch


class DDPMScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear",
                 prediction_type="epsilon", **unused):
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise ValueError(f"unsupported beta_schedule {beta_schedule!r}")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.config = type("Cfg", (), dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                           beta_end=beta_end, beta_schedule=beta_schedule,
                                           prediction_type=prediction_type))()

    @classmethod
    def from_pretrained(cls, path, subfolder="scheduler"):
        fn = os.path.join(path, subfolder, "scheduler_config.json")
        with open(fn) as f:
            d = json.load(f)
        return cls(**{k: v for k, v in d.items() if not k.startswith("_")})

    def add_noise(self, original_samples, noise, timesteps):
        """alphas_cumprod is cast to the sample dtype first (bf16 mode rounds it) -- SURVEY Appendix A1.
        The fused HIP kernel (csrc/siss_loss.hip) reproduces this bit-for-bit; this torch form exists
        for the class-surface path where callers ask for noisy latents explicitly."""
        ac = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        a = (ac[timesteps] ** 0.5).flatten()
        b = ((1 - ac[timesteps]) ** 0.5).flatten()
        while a.dim() < original_samples.dim():
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        return a * original_samples + b * noise


def lr_multiplier(name, step, num_warmup_steps=0, num_training_steps=0):
    """LR multiplier at scheduler step `step` of diffusers.optimization.get_scheduler(name, ...) (0.27.2, as published):
    what delete_celeb.py:296-301 builds from cfg.lr_scheduler / cfg.warmup_steps / cfg.training_steps and steps after
    every optimizer update (:770).  Schedules outside this table raise instead of silently training at a constant rate."""
    import math
    w, total = int(num_warmup_steps), int(num_training_steps)
    if name == "constant":
        return 1.0
    if name == "constant_with_warmup":
        return step / max(1.0, w) if step < w else 1.0
    if name == "linear":
        if step < w:
            return step / max(1, w)
        return max(0.0, (total - step) / max(1, total - w))
    if name == "cosine":
        if step < w:
            return step / max(1, w)
        progress = (step - w) / max(1, total - w)
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
    raise NotImplementedError(f"lr_scheduler={name!r}: implemented: constant, constant_with_warmup, linear, cosine "
                              "(diffusers.optimization.get_scheduler)")


# The scheduler_config.json of the SD v1 checkpoints (CompVis/stable-diffusion-v1-4, runwayml/stable-diffusion-v1-5): what
# DDIMScheduler.from_config(pipeline.scheduler.config) (delete_sd.py:204) starts from when no checkpoint directory is on disk.
SD_V1_SCHEDULER = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                       set_alpha_to_one=False, steps_offset=1, clip_sample=False)


class DDIMScheduler:
    """diffusers 0.27 DDIMScheduler as the validation pipeline uses it (delete_sd.py:204): "leading" timestep spacing and the
    deterministic (eta = 0) epsilon-prediction step.  The update itself runs on the device (csrc/siss_loss.hip
    siss_cfg_ddim_step); this class holds the schedule and hands out each step's coefficients, computed in f32 the way
    DDIMScheduler.step computes them.  Options it does not implement are refused, not ignored."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                 clip_sample_range=1.0, timestep_spacing="leading", rescale_betas_zero_snr=False, **unused):
        if timestep_spacing != "leading":
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r}: only 'leading' (the diffusers 0.27 default) is implemented")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"prediction_type={prediction_type!r}: only epsilon prediction is implemented")
        if thresholding:
            raise NotImplementedError("thresholding=true: dynamic thresholding is not implemented")
        if rescale_betas_zero_snr:
            raise NotImplementedError("rescale_betas_zero_snr=true is not implemented")
        if trained_betas is not None:
            raise NotImplementedError("trained_betas: only the linear / scaled_linear beta schedules are implemented")
        self.alphas_cumprod = DDPMScheduler(num_train_timesteps, beta_start, beta_end, beta_schedule).alphas_cumprod
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_train_timesteps = int(num_train_timesteps)
        self.steps_offset = int(steps_offset)
        self.clip_sample, self.clip_sample_range = bool(clip_sample), float(clip_sample_range)
        self.num_inference_steps, self.timesteps = None, None

    @classmethod
    def from_config(cls, d):
        return cls(**{k: v for k, v in d.items() if not k.startswith("_")})

    @classmethod
    def from_pretrained(cls, path=None, subfolder="scheduler"):
        """<path>/scheduler/scheduler_config.json when it is on disk, else the SD v1 values (SD_V1_SCHEDULER)."""
        fn = os.path.join(str(path), subfolder, "scheduler_config.json") if path else None
        if fn and os.path.isfile(fn):
            with open(fn) as f:
                return cls.from_config(json.load(f))
        return cls(**SD_V1_SCHEDULER)

    def set_timesteps(self, num_inference_steps):
        """DDIMScheduler.set_timesteps, "leading": arange(steps) * (T // steps), reversed, + steps_offset."""
        n, T = int(num_inference_steps), self.num_train_timesteps
        if not 1 <= n <= T:
            raise ValueError(f"num_inference_steps={n}: must lie in [1, num_train_timesteps={T}]")
        ratio = T // n
        ts = [i * ratio + self.steps_offset for i in range(n)][::-1]
        if ts[0] >= T:                                   # diffusers fails here with an index error on alphas_cumprod
            raise ValueError(f"num_inference_steps={n} with steps_offset={self.steps_offset} reaches timestep {ts[0]} >= {T}")
        self.num_inference_steps, self.timesteps = n, ts
        return ts

    def alphas(self, t):
        """(alpha_prod_t, alpha_prod_t_prev) of DDIMScheduler.step at timestep t (f32 tensors)."""
        prev_t = int(t) - self.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[int(t)], (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod)

    def coeffs(self, t):
        """(sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)) as DDIMScheduler.step forms them (f32, eta = 0)."""
        a_t, a_prev = self.alphas(t)
        return tuple(float(v) for v in (a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5))

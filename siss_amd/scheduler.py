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


SAMPLER_NAME = "dpmsolver++"      # the one value of pipeline.sampler.name


class DPMSolverMultistepScheduler:
    """DPM-Solver++ multistep of order 1 or 2 ("2M"; Lu et al. 2022), the subset of diffusers' DPMSolverMultistepScheduler an
    epsilon-prediction VP model is sampled with in 15-25 steps: algorithm_type "dpmsolver++", solver_type "midpoint", the last step
    to sigma = 0.  OPT-IN (pipeline.sampler) and not the reference's protocol: its samplers are DDPM / DDIM at 50 steps.  The update
    runs on the device (csrc/dpm_solver.hip siss_cfg_dpmpp_step); this class holds the grid and hands out each step's five
    coefficients, formed in f64 from alphas_cumprod and rounded once to f32.  Options it does not implement are refused, not ignored.

    With a_s = sqrt(ac[s]), s_s = sqrt(1 - ac[s]), l_s = ln a_s - ln s_s, a step from the grid time s to the next one t has the
    x0-prediction m = (x - s_s e) / a_s, h = l_t - l_s, E = a_t (1 - exp(-h)), c_x = s_t / s_s, and
        order 1:  x' = c_x x + E m                                         (DDIM with eta = 0)
        order 2:  x' = c_x x + E (1 + 1 / (2 r)) m - (E / (2 r)) m1,       r = (l_s - l_s1) / h, m1 the prediction at the previous time s1
    The last step is x' = m."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False,
                 final_sigmas_type="zero", variance_type=None, timestep_spacing="linspace", steps_offset=0,
                 rescale_betas_zero_snr=False, **unused):
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: only 'dpmsolver++' (the deterministic data-prediction solver) is implemented")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type={solver_type!r}: only 'midpoint' is implemented")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order!r}: orders 1 and 2 are implemented")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"prediction_type={prediction_type!r}: only epsilon prediction is implemented")
        if thresholding:
            raise NotImplementedError("thresholding=true: dynamic thresholding is not implemented")
        if use_karras_sigmas:
            raise NotImplementedError("use_karras_sigmas=true is not implemented")
        if use_lu_lambdas:
            raise NotImplementedError("use_lu_lambdas=true is not implemented")
        if euler_at_final:
            raise NotImplementedError("euler_at_final=true is not implemented")
        if final_sigmas_type != "zero":
            raise NotImplementedError(f"final_sigmas_type={final_sigmas_type!r}: only 'zero' (the last step lands on the x0-prediction) is implemented")
        if not lower_order_final:
            raise NotImplementedError("lower_order_final=false: the last step to sigma = 0 is of order 1")
        if variance_type is not None:
            raise NotImplementedError(f"variance_type={variance_type!r}: learned variances are not implemented")
        if trained_betas is not None:
            raise NotImplementedError("trained_betas: only the linear / scaled_linear beta schedules are implemented")
        if rescale_betas_zero_snr:
            raise NotImplementedError("rescale_betas_zero_snr=true is not implemented")
        if timestep_spacing not in ("linspace", "leading"):
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r}: 'linspace' and 'leading' are implemented")
        self.alphas_cumprod = DDPMScheduler(num_train_timesteps, beta_start, beta_end, beta_schedule).alphas_cumprod
        self.num_train_timesteps = int(num_train_timesteps)
        self.solver_order, self.timestep_spacing, self.steps_offset = int(solver_order), timestep_spacing, int(steps_offset)
        self.num_inference_steps, self.timesteps = None, None

    from_config = classmethod(DDIMScheduler.from_config.__func__)             # (keys of other schedulers fall into **unused)
    from_pretrained = classmethod(DDIMScheduler.from_pretrained.__func__)     # scheduler_config.json on disk, else SD_V1_SCHEDULER

    @classmethod
    def from_sampler_config(cls, node, base=None, **defaults):
        """The scheduler a `pipeline.sampler` node asks for, or None for a null node.  `base`: the scheduler_config.json-style dict the
        betas come from (SD: the checkpoint's), or a DDPMScheduler (the pixel tasks' own noise scheduler); `defaults`: the values
        of solver_order / timestep_spacing / steps_offset where the node leaves them out.  Any name but 'dpmsolver++' is a
        ValueError."""
        if node is None:
            return None
        node = dict(node)
        name = node.pop("name", None)
        if name != SAMPLER_NAME:
            raise ValueError(f"pipeline.sampler.name={name!r}: the one sampler that can be asked for is {SAMPLER_NAME!r} (null: the "
                             "task's own DDPM / DDIM sampling)")
        extra = set(node) - {"solver_order", "timestep_spacing", "steps_offset"}
        if extra:
            raise ValueError(f"pipeline.sampler: unknown keys {sorted(extra)} (name, solver_order, timestep_spacing, steps_offset)")
        if isinstance(base, DDPMScheduler):
            c = base.config
            base = dict(num_train_timesteps=c.num_train_timesteps, beta_start=c.beta_start, beta_end=c.beta_end,
                        beta_schedule=c.beta_schedule, prediction_type=c.prediction_type)
        betas = {k: v for k, v in (base or {}).items() if k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule",
                                                                "trained_betas", "prediction_type", "rescale_betas_zero_snr")}
        return cls(**{**betas, **defaults, **node})

    @property
    def label(self):
        """What a record written from this sampler's images carries as "sampler": 'dpmsolver++2m' (order 2), 'dpmsolver++1m'."""
        return f"{SAMPLER_NAME}{self.solver_order}m"

    def record_fields(self, num_inference_steps):
        return {"sampler": self.label, "num_inference_steps": int(num_inference_steps)}

    def set_timesteps(self, num_inference_steps):
        """The K grid times, largest first.  linspace: linspace(0, T - 1, K + 1).round() reversed, without the 0; leading:
        arange(K + 1) * (T // (K + 1)) reversed, without the 0, + steps_offset (diffusers' DPMSolverMultistepScheduler)."""
        import numpy as np
        K, T = int(num_inference_steps), self.num_train_timesteps
        if not 1 <= K < T:
            raise ValueError(f"num_inference_steps={K}: must lie in [1, num_train_timesteps={T})")
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, K + 1).round()[::-1][:-1]
        else:
            ts = (np.arange(0, K + 1) * (T // (K + 1)))[::-1][:-1] + self.steps_offset
        ts = [int(t) for t in ts]
        if ts[0] >= T or any(a <= b for a, b in zip(ts, ts[1:])):
            raise ValueError(f"num_inference_steps={K} with steps_offset={self.steps_offset}: the grid {ts[:3]}... leaves [0, {T}) or "
                             "repeats a timestep")
        self.num_inference_steps, self.timesteps = K, ts
        return ts

    def _asl(self, t):
        """(a_t, s_t, l_t) in f64 from alphas_cumprod[t] widened to f64."""
        import math
        ac = float(self.alphas_cumprod[int(t)].double())
        a, s = math.sqrt(ac), math.sqrt(1.0 - ac)
        return a, s, math.log(a) - math.log(s)

    def coeffs(self, i, first=None):
        """The five f32 coefficients (1 / a_s, s_s / a_s, c_x, c_0, c_1) of step i of the current grid (s = timesteps[i]), as
        siss_cfg_dpmpp_step takes them: m = (1 / a_s) x - (s_s / a_s) e, x' = c_x x + c_0 m + c_1 m1.  first: this is the first step
        the caller runs (default: i == 0) -- there is no earlier prediction, so it is of order 1, as is every step of solver_order 1;
        the last step of the grid is x' = m.  c_1 == 0 exactly when m1 is not needed."""
        import math
        import struct
        ts = self.timesteps
        if ts is None or not 0 <= i < len(ts):
            raise ValueError(f"step {i}: set_timesteps first; steps run from 0 to {len(ts or []) - 1}")
        first = (i == 0) if first is None else bool(first)
        a_s, s_s, l_s = self._asl(ts[i])
        if i == len(ts) - 1:
            cx, c0, c1 = 0.0, 1.0, 0.0
        else:
            a_t, s_t, l_t = self._asl(ts[i + 1])
            h = l_t - l_s
            E = -a_t * math.expm1(-h)
            cx, c0, c1 = s_t / s_s, E, 0.0
            if self.solver_order == 2 and not first:
                r = (l_s - self._asl(ts[i - 1])[2]) / h
                c0, c1 = E * (1.0 + 0.5 / r), -0.5 * E / r
        f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
        return tuple(f32(v) for v in (1.0 / a_s, s_s / a_s, cx, c0, c1))

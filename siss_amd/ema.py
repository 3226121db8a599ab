"""Exponential moving average of the UNet's weights: the surface of diffusers 0.27.2 `training_utils.EMAModel` (what the reference's
train_unconditional.py:186-194, :421, :431-452 and its save / load hooks :134-155 call) over ONE flat f32 buffer in the engine's native
layout, stepped by csrc/train_state.hip -- fused into the optimizer's pass (FlatAdamW.launch_single) or on its own (`step`).

The decay schedule (EMAModel.get_decay), with k = optimization_step AFTER the increment of this step and s = max(0, k -
update_after_step - 1):  s == 0 -> 0;  else 1 - (1 + s / inv_gamma)^-power (use_ema_warmup) or (1 + s) / (10 + s);  then clamped to
[min_decay, decay].  The device forms it in double and keeps 1 - decay, rounded once.
"""
import contextlib
import json
import os

import torch

from . import lib
from .config import EMA_KEYS
from .optim import EMA_STEP
from .unet import ALIGN, ParamStore


def _layout(ps):
    """The name -> (offset, shape, layout kind) table of a ParamStore without its buffers (all save_pretrained needs)."""
    out = ParamStore()
    out.specs, out.total = ps.specs, ps.total
    return out


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """EMAModel.get_decay in Python doubles (the host's statement of what siss_grad_norm_single / siss_ema_advance compute)."""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    cur = 1 - (1 + step / inv_gamma) ** -power if use_ema_warmup else (1 + step) / (10 + step)
    return max(min(cur, decay), min_decay)


def flat_of(parameters):
    """The ONE flat f32 buffer behind `parameters`: a siss_amd UNet2DModel, or the iterable unet.parameters() -- views that tile one
    storage (taken by offset, each start within the layout's alignment padding of the previous end, none twice).  Anything else
    raises: there is no per-tensor path."""
    if hasattr(parameters, "engine"):
        return parameters.engine.ps.flat
    ps = list(parameters)
    if not ps or not all(torch.is_tensor(p) for p in ps):
        raise TypeError("EMAModel: parameters must be a siss_amd UNet2DModel or its .parameters()")
    st = ps[0].untyped_storage()
    end = 0
    for p in sorted(ps, key=lambda p: p.storage_offset()):
        if (p.dtype != torch.float32 or not p.is_contiguous() or p.untyped_storage().data_ptr() != st.data_ptr()
                or not end <= p.storage_offset() < end + ALIGN):
            raise ValueError("EMAModel: the parameters are not views that tile ONE flat f32 buffer (the layout of "
                             "siss_amd.model.UNet2DModel.parameters()); per-tensor EMA is not provided")
        end = p.storage_offset() + p.numel()
    total = st.nbytes() // 4
    if not end <= total < end + ALIGN:
        raise ValueError("EMAModel: the parameters do not cover their flat buffer")
    return torch.empty(0, dtype=torch.float32, device=ps[0].device).set_(st, 0, (total,))


class EMAModel:
    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
                 power=2 / 3, model_cls=None, model_config=None):
        self.flat = flat_of(parameters).detach().clone()            # shadow_params, as one buffer
        self._ps = _layout(parameters.engine.ps) if hasattr(parameters, "engine") else None
        self.decay, self.min_decay, self.update_after_step = float(decay), float(min_decay), int(update_after_step)
        self.use_ema_warmup, self.inv_gamma, self.power = bool(use_ema_warmup), float(inv_gamma), float(power)
        self.optimization_step = 0
        self.model_cls, self.model_config = model_cls, model_config
        self.temp_stored = None
        self.scalars = None                 # the block of step() on its own (the fused update keeps the optimizer's)
        self._dev_step = 0

    # ---- the schedule -----------------------------------------------------------
    def schedule_args(self):
        """(max_decay, min_decay, inv_gamma, power, use_warmup, update_after) as siss_grad_norm_single / siss_ema_advance take them"""
        return (self.decay, self.min_decay, self.inv_gamma, self.power, int(self.use_ema_warmup), self.update_after_step)

    def get_decay(self, optimization_step):
        return get_decay(optimization_step, self.decay, self.min_decay, self.update_after_step, self.use_ema_warmup,
                         self.inv_gamma, self.power)

    @property
    def cur_decay_value(self):
        """The decay of the LAST step, from the host's step count (the device holds the same in its scalar block)."""
        return self.get_decay(self.optimization_step) if self.optimization_step else 0.0

    # ---- EMAModel.step on its own -----------------------------------------------
    @torch.no_grad()
    def step(self, parameters):
        p = flat_of(parameters)
        if self.scalars is None:
            self.scalars = torch.zeros(lib.query("siss_train_scalars_words"), dtype=torch.float32, device=self.flat.device)
        if self._dev_step != self.optimization_step:                # stepped by the fused update since, or loaded
            self.scalars[EMA_STEP:EMA_STEP + 1].fill_(float(self.optimization_step))
        lib.call("siss_ema_advance", *self.schedule_args(), self.scalars)
        lib.call("siss_ema_step", p, self.flat, p.numel(), self.scalars)
        self.optimization_step += 1
        self._dev_step = self.optimization_step

    # ---- store / copy_to / restore (diffusers' meaning) and the swap ------------
    def copy_to(self, parameters):
        flat_of(parameters).copy_(self.flat)
        if hasattr(parameters, "engine"):
            parameters.engine.refresh_weights(cast_shadow=True)

    def store(self, parameters):
        self.temp_stored = flat_of(parameters).detach().clone()

    def restore(self, parameters):
        if self.temp_stored is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        flat_of(parameters).copy_(self.temp_stored)
        self.temp_stored = None
        if hasattr(parameters, "engine"):
            parameters.engine.refresh_weights(cast_shadow=True)

    @contextlib.contextmanager
    def applied(self, unet):
        """`with ema.applied(unet):` -- the EMA weights under the engine (master, operand shadow, dgrad copies) for an evaluation,
        the training weights back afterwards bit for bit: one siss_swap_f32 each way instead of store + copy_to + restore."""
        eng = unet.engine
        ps = eng.ps

        def swap():
            lib.call("siss_swap_f32", ps.flat, self.flat, None if eng.f32 else ps.shadow, ps.total)
            eng.refresh_weights()
        swap()
        try:
            yield unet
        finally:
            swap()

    def to(self, *a, **k):
        return self

    # ---- state ------------------------------------------------------------------
    def state_dict(self):
        d = {k: getattr(self, k) for k in EMA_KEYS}
        d["shadow_params"] = [self.flat]
        return d

    def load_state_dict(self, sd):
        for k in EMA_KEYS:
            if k in sd:
                cur = getattr(self, k)
                setattr(self, k, type(cur)(sd[k]))
        sp = sd.get("shadow_params")
        if sp is not None:
            if len(sp) != 1 or sp[0].shape != self.flat.shape:
                raise ValueError("shadow_params must be the one flat buffer of this EMAModel")
            self.flat.copy_(sp[0])

    def _store(self):
        if self._ps is None:
            if self.model_cls is None or self.model_config is None:
                raise ValueError("`save_pretrained` can only be used if `model_cls` and `model_config` were defined at __init__ "
                                 "(or the EMAModel was built from the model itself)")
            self._ps = _layout(self.model_cls(self.model_config, device=self.flat.device).engine.ps)
            if self._ps.total != self.flat.numel():
                raise ValueError("model_config does not describe the network these parameters belong to")
        return self._ps

    def save_pretrained(self, path):
        """The model's config.json + the seven EMA keys, and the EMA weights as diffusion_pytorch_model.safetensors (reference layout)."""
        from safetensors.torch import save_file
        ps = self._store()
        os.makedirs(path, exist_ok=True)
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(self.model_config).items()} if self.model_config is not None else {}
        cfg["_class_name"] = getattr(self.model_cls, "class_name", "UNet2DModel")
        cfg.update({k: getattr(self, k) for k in EMA_KEYS})
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f, indent=2)
        save_file({k: v.contiguous() for k, v in ps.flat_to_ref(self.flat).items()},
                  os.path.join(path, "diffusion_pytorch_model.safetensors"))

    @classmethod
    def from_pretrained(cls, path, model_cls, **model_kw):
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        model = model_cls.from_pretrained(path, **model_kw)
        ema = cls(model, model_cls=model_cls, model_config=model.config)
        ema.load_state_dict({k: cfg[k] for k in EMA_KEYS if k in cfg})
        return ema

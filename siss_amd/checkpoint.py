"""Resumable training state: `checkpoint-<global_step>/` as the reference's train_unconditional.py writes it through
accelerator.save_state and its hooks (:134-171, :480-519), in safetensors and JSON only:

    unet/, unet_ema/          diffusers layout (config.json + diffusion_pytorch_model.safetensors; unet_ema's config carries the
                              seven EMA keys)
    optimizer.safetensors     exp_avg.<name>, exp_avg_sq.<name> per parameter in reference layout, and `scalars`: the update's
                              device block (step counts, bias corrections, 1 - decay)
    state.json                global step, epoch, position in the epoch, LR-schedule position, the CPU and device generator states
                              as lists of bytes, format versions

accelerate's optimizer.bin / random_states_0.pkl are pickles; this format is a stated deviation.
"""
import json
import os
import re
import shutil

import torch

FORMAT_VERSION = 1
_CKPT = re.compile(r"checkpoint-(\d+)$")


def list_checkpoints(output_dir):
    """The checkpoint directories of `output_dir`, oldest first by step number."""
    if not os.path.isdir(output_dir):
        return []
    found = [d for d in os.listdir(output_dir) if _CKPT.match(d) and os.path.isdir(os.path.join(output_dir, d))]
    return sorted(found, key=lambda d: int(d.split("-")[1]))


def rotate(output_dir, limit):
    """train_unconditional.py:484-513: BEFORE saving, at most limit - 1 checkpoints remain (oldest removed first); null keeps all."""
    if limit is None:
        return []
    have = list_checkpoints(output_dir)
    gone = have[:max(len(have) - int(limit) + 1, 0)] if len(have) >= int(limit) else []
    for d in gone:
        shutil.rmtree(os.path.join(output_dir, d))
    return gone


def step_of(path):
    """global_step from the directory name (train_unconditional.py:339)"""
    m = _CKPT.search(os.path.normpath(str(path)))
    if not m:
        raise ValueError(f"checkpoint_path {path!r}: a directory named checkpoint-<global_step> is needed")
    return int(m.group(1))


def _moments(ps, stepper):
    out = {}
    for prefix, flat in (("exp_avg.", stepper.opt.m), ("exp_avg_sq.", stepper.opt.v)):
        out.update({prefix + n: t.contiguous() for n, t in ps.flat_to_ref(flat).items()})
    return out


def save_state(path, unet, ema, stepper, meta, limit=None):
    """Write checkpoint directory `path` (rotating its siblings first when `limit` is given).  meta: dict with global_step, epoch,
    position, lr_position; generator: the device generator the loop draws noise and timesteps from (optional)."""
    from safetensors.torch import save_file
    rotate(os.path.dirname(os.path.normpath(path)), limit)
    os.makedirs(path, exist_ok=True)
    unet.save_pretrained(os.path.join(path, "unet"))
    if ema is not None:
        ema.save_pretrained(os.path.join(path, "unet_ema"))
    opt = _moments(unet.engine.ps, stepper)
    opt["scalars"] = stepper.opt._train_block().detach().cpu().clone()
    save_file(opt, os.path.join(path, "optimizer.safetensors"))
    meta = dict(meta)
    gen = meta.pop("generator", None)
    state = {"format_version": FORMAT_VERSION, "torch_version": torch.__version__,
             **{k: meta[k] for k in ("global_step", "epoch", "position", "lr_position")},
             "extra": {k: v for k, v in meta.items() if k not in ("global_step", "epoch", "position", "lr_position")},
             "cpu_rng_state": torch.get_rng_state().tolist(),
             "device_rng_state": None if gen is None else gen.get_state().tolist()}
    with open(os.path.join(path, "state.json"), "w") as f:
        json.dump(state, f)
    return path


def load_state(path, unet, ema, stepper, generator=None):
    """The inverse: parameters (+ operand copies), EMA buffer and counters, AdamW moments and scalar block, generator states.
    Returns state.json as a dict."""
    from safetensors.torch import load_file
    with open(os.path.join(path, "state.json")) as f:
        state = json.load(f)
    if state.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{path}: checkpoint format {state.get('format_version')!r}, this build reads {FORMAT_VERSION}")
    ps = unet.engine.ps
    unet.load_state_dict(load_file(os.path.join(path, "unet", "diffusion_pytorch_model.safetensors")))
    if ema is not None:
        d = os.path.join(path, "unet_ema")
        with open(os.path.join(d, "config.json")) as f:
            ema.load_state_dict(json.load(f))
        sd = load_file(os.path.join(d, "diffusion_pytorch_model.safetensors"))
        for n, sp in ps.specs.items():
            ema.flat[sp.off:sp.off + sp.numel] = ps.to_native(sp, sd[n].to(ema.flat.device)).reshape(-1)
    opt = load_file(os.path.join(path, "optimizer.safetensors"))
    for prefix, flat in (("exp_avg.", stepper.opt.m), ("exp_avg_sq.", stepper.opt.v)):
        for n, sp in ps.specs.items():
            flat[sp.off:sp.off + sp.numel] = ps.to_native(sp, opt[prefix + n].to(flat.device)).reshape(-1)
    blk = stepper.opt._train_block()
    blk.copy_(opt["scalars"])
    from .optim import EMA_STEP
    stepper.opt.train_ema_step = int(opt["scalars"][EMA_STEP])
    torch.set_rng_state(torch.tensor(state["cpu_rng_state"], dtype=torch.uint8))
    if generator is not None and state.get("device_rng_state") is not None:
        generator.set_state(torch.tensor(state["device_rng_state"], dtype=torch.uint8))
    return state

"""The opt-in variants of the unlearning update -- `deletion.trainable`, `deletion.lora`, `deletion.saliency`, `deletion.ewc`,
`deletion.surgery` -- and
what they share: ONE table of their static facts (which gradient exchanges a variant may use and why not the others, why it runs
alone), the one exclusivity check every entry point calls, the field checks of the parsed keys, and the flat-buffer helpers of what
is built from backward passes at the pretrained weights -- the saliency mask, the Fisher anchor and the importances of siss_amd/ssd.py
(fingerprint, the real-parameter mask, the tensor file beside its JSON, quiet_backward / backward_batch / fisher_of_batches).  At most one variant is active in a run; `full` is the reference's protocol.
Host code only until a tensor is touched.
"""
import json
import os
from collections import namedtuple

# what: how messages name the variant.  alone: why it combines with no other variant.  overlap / sharded: None where the variant may
# use the overlapped early-tail exchange / the sharded update, else the one-line reason it may not.
Variant = namedtuple("Variant", "what alone overlap sharded")
_WHOLE = "the sharded exchange splits the whole buffer over the ranks"
VARIANTS = {
    "full": Variant("the full update", None, None, None),
    "trainable": Variant("trainable subset", "a subset update runs its passes over its own stretches of the buffer",
                         "one grouped all-reduce of the trainable pieces after the backward pass", _WHOLE),
    "lora": Variant("lora", "a LoRA run trains the adapters of its targets and nothing else",
                    "one all-reduce of the adapter gradients after the backward pass", _WHOLE),
    "saliency": Variant("saliency mask", "the saliency mask selects single weights of every tensor", None,
                        "there is no masked sharded update"),
    "ewc": Variant("Fisher anchor", "the Fisher anchor is folded into the whole-buffer update", None, "there is no sharded fold"),
    # (the overlapped early-tail exchange is allowed: the gram pass reads the whole summed buffer after it)
    "surgery": Variant("gradient surgery", "the surgery projects the whole-buffer gradient pair group by group", None,
                       "there is no sharded surgery update"),
}
ALIASES = {"ranges": "trainable", "mask": "saliency"}          # FlatAdamW.launch's keywords
SHARD = "a parameter shard"                                    # launch_sharded's own side of `exclusive`


def variant_of(key):
    """The table row a key names: `deletion.ewc`, `ewc=`, `ewc`; `ranges=` and `mask=` are FlatAdamW's words for trainable / saliency."""
    name = key.rsplit(".", 1)[-1].rstrip("=")
    return ALIASES.get(name, name)


def exclusive(where, present, exc=ValueError):
    """present: {key: value}, in the order the message should name them.  Raises `exc` when two values are set (not None), naming
    both keys and the first one's reason from the table."""
    on = [k for k, v in present.items() if v is not None]
    if len(on) < 2:
        return
    a, b = on[:2]
    v = VARIANTS[variant_of(a)]
    raise exc(f"{where}: {a} and {b} do not combine -- {f'{v.what}: {v.sharded}' if b == SHARD else v.alone} (leave one of the two out)")


def exchange_refusal(variant, overlap, exchange):
    """None, or why `variant` cannot run this gradient exchange (overlap: the early-tail all-reduce from inside the backward pass;
    exchange: 'allreduce' | 'sharded')."""
    v = VARIANTS[variant]
    if overlap and v.overlap is not None:
        return f"{v.what}: the overlapped early-tail gradient exchange is off ({v.overlap})"
    if exchange == "sharded" and v.sharded is not None:
        return f"{v.what}: {v.sharded}"
    return None


# ---------------------------------------------------------------------------------------------------------------- the parsed keys
def is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def need_int(key, x, positive=False, what="an integer"):
    if not is_int(x) or (positive and x < 1):
        raise ValueError(f"{key}={x!r}: {what} is needed")
    return x


def need_bool(key, x):
    if not isinstance(x, bool):
        raise ValueError(f"{key}={x!r}: true or false is needed")
    return x


def need_opt_str(key, x, what):
    if x is not None and not isinstance(x, str):
        raise ValueError(f"{key}={x!r}: null or {what}")
    return x


def need_fields(key, value, fields, example):
    """The mapping of a key as a dict; anything but a mapping and an unknown field are refused by name."""
    if not hasattr(value, "keys"):
        raise ValueError(f"{key}={value!r}: a mapping {{{', '.join(fields)}}} is needed (e.g. +{key}={example})")
    unknown = sorted(set(value) - set(fields))
    if unknown:
        raise ValueError(f"{key}: unknown field(s) {unknown} ({', '.join(fields)})")
    return dict(value)


# ---------------------------------------------------------------------------------------------------------------- the flat buffer
def fingerprint(engine):
    """What a per-float tensor over an engine's flat buffer indexes: the buffer's length, the tensor count and the number of real
    (non-padding) parameters."""
    ps = engine.ps
    return dict(total=int(ps.total), tensors=len(ps.specs), real_params=sum(int(sp.numel) for sp in ps.specs.values()))


def same_layout(obj, engine):
    """Whether obj (.total, .tensors, .params) was built over this engine's parameter layout."""
    fp = fingerprint(engine)
    return (obj.total, obj.tensors, obj.params) == (fp["total"], fp["tensors"], fp["real_params"])


def real_mask(specs, total, device=None):
    """[total] bool: True on the real parameters of a flat buffer, False on its alignment padding."""
    import torch
    real = torch.zeros(int(total), dtype=torch.bool, device=device)
    for sp in specs.values():
        real[sp.off:sp.off + sp.numel] = True
    return real


def files_present(directory, *files):
    return bool(directory) and all(os.path.isfile(os.path.join(str(directory), f)) for f in files)


def save_tensors(directory, tensor_file, tensors, config_file, config):
    """`tensors` ({key: tensor}) in one safetensors file beside its JSON config (safetensors and JSON only)."""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    save_file({k: t.cpu().contiguous() for k, t in tensors.items()}, os.path.join(directory, tensor_file))
    save_config(directory, config_file, config)


def save_config(directory, config_file, config):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, config_file), "w") as f:
        json.dump(config, f, indent=1)


def save_tensor(directory, tensor_file, key, tensor, config_file, config):
    """`tensor` under `key` in a safetensors file beside its JSON config."""
    save_tensors(directory, tensor_file, {key: tensor}, config_file, config)


def load_tensors(directory, tensor_file, config_file, engine, what):
    """({key: tensor}, config) saved by save_tensors, for `engine`: refused, naming the file and the key, when it was taken over another
    buffer (ps.total, the tensor count or the real parameter count differ)."""
    from safetensors.torch import load_file
    path = os.path.join(directory, config_file)
    with open(path) as f:
        c = json.load(f)
    fp = fingerprint(engine)
    for k in ("total", "tensors", "real_params"):
        if int(c.get(k, -1)) != fp[k]:
            raise ValueError(f"{path}: {k} = {c.get(k)!r}, this UNet has {fp[k]} -- the {what} was computed for another architecture "
                             "or parameter layout")
    return load_file(os.path.join(directory, tensor_file)), c


def load_tensor(directory, tensor_file, key, config_file, engine, what):
    """(tensor, config): load_tensors for a file of one key."""
    tensors, c = load_tensors(directory, tensor_file, config_file, engine, what)
    return tensors[key], c


# ---------------------------------------------------------------------------------------------------------------- backward passes outside a step
class quiet_backward:
    """`with quiet_backward(stepper, what):` -- backward passes at the stepper's current weights that are no part of a step (the
    saliency mask's forget gradient, the Fisher estimate of siss_amd/ewc.py): refused in the middle of an accumulation or with
    collectives in flight; the data-parallel overlap hook (SISSStepper._early_allreduce) is off inside -- it would start an all-reduce
    of the gradient tails from inside every backward pass, and the gradient is this rank's own; on exit the hook is back, the gradient
    buffers are zero and no collective is pending."""

    def __init__(self, stepper, what):
        self.stepper, self.what = stepper, what

    def __enter__(self):
        st = self.stepper
        if st._micro != 0:
            raise RuntimeError(f"{self.what} in the middle of an accumulation: the gradient buffers hold a step's micro-batches")
        if st._pending:
            raise RuntimeError(f"{self.what} with gradient collectives of a step still in flight")
        self.hook, st.e.on_early_grads_final = st.e.on_early_grads_final, None
        return self

    def __exit__(self, *exc):
        e = self.stepper.e
        e.wgrad_overwrite = False
        e.on_early_grads_final = self.hook
        e.ps.grads.zero_()
        if exc[0] is None:
            assert not self.stepper._pending, f"{self.what} started a gradient collective"
        return False


def backward_batch(stepper, batch, scale_batches, *, first, prepare=None, sample_noise=None, conditioning=None, timestep_low=0,
                   generator=None):
    """One micro-batch of the eps-MSE at the stepper's current weights into gradient set 0: the forward and the nsets = 1 backward
    that loss_fn = simple_neg_del drives, scale 1 / (B * scale_batches).  first: the buffers are zeroed and one-split weight gradients
    overwrite their tiles; else the micro-batch accumulates (a plain full fill, no sparse key).  Inside quiet_backward."""
    import torch
    from .loss import mixture_fwd, mse_bwd_seed
    e = stepper.e
    dev = e.device
    T = int(stepper.ac.numel())
    e.wgrad_overwrite = first and stepper.wgrad_overwrite
    if first:
        e.zero_grad()
    a0 = batch.to(dev, non_blocking=True)              # (a tensor, or the IndexBatch of an image store / latent cache)
    if prepare is not None:
        a0 = prepare(a0, generator)
    a0 = a0.to(device=dev, dtype=stepper.io_dtype).contiguous()
    B = a0.shape[0]
    noise = (sample_noise(a0.shape, dev, generator) if sample_noise is not None
             else torch.randn(a0.shape, device=dev, generator=generator)).to(stepper.io_dtype).contiguous()
    t = torch.randint(int(timestep_low), T, (B,), device=dev, generator=generator)
    m = mixture_fwd(a0, a0, noise, t, torch.zeros(B, device=dev), stepper.ac, stepper.gamma_tab, stepper.sigma_tab, 0.5)
    pred = e.forward(m.x_mix, t, **dict(conditioning or {}))
    cot, _, _ = mse_bwd_seed(pred, noise, 1.0 / (B * scale_batches))
    e.backward(cot, nsets=1)


def fisher_of_batches(stepper, batches_iter, n_batches, what, **draw):
    """The empirical Fisher of the eps-MSE at the stepper's current weights at MICRO-BATCH granularity, [ps.total] f32 on the engine's
    device: zero, then per micro-batch of batches_iter one backward_batch(first=True) at scale 1 / B (`draw`: its prepare /
    sample_noise / conditioning / timestep_low / generator) and F += g^2 / n_batches (siss_fisher_accumulate on gradient set 0).  The
    one loop under the Fisher anchor (siss_amd/ewc.py) and the two importances of siss_amd/ssd.py; quiet_backward's guarantees hold."""
    import torch
    from . import lib
    ps = stepper.e.ps
    F = torch.zeros_like(ps.flat)
    with quiet_backward(stepper, what):
        for _ in range(n_batches):
            # every micro-batch is a gradient of its own: zeroed buffers, one-split weight gradients overwrite their tiles
            backward_batch(stepper, next(batches_iter), 1, first=True, **draw)
            lib.call("siss_fisher_accumulate", ps.grads[0], F, ps.total, 1.0 / n_batches)
    return F

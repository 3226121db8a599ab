"""Saliency-masked unlearning (OPT-IN, not the reference's protocol): `deletion.saliency`, `SISSStepper(saliency=...)`.

The weight-saliency mask of SalUn (Fan et al., ICLR 2024): take the gradient of the forget loss at the pretrained weights, keep the top
fraction of ALL parameters by |g| under one global threshold, and let the unlearning update touch only those elements.  Here the
mask is one bit per float of the engine's flat parameter buffer (a 32-bit word per 32 floats) and drives the masked forms of the two
flat optimizer passes (csrc/saliency.hip: siss_grad_norms_scale_masked / siss_recombine_clip_adamw_masked); the threshold is the exact
k-th largest magnitude, found on the device by an integer radix select (siss_absf_select), ties included.

The mask files: `saliency_mask.safetensors` (the packed words, key `bits`) beside `saliency.json` (fraction, k, count, threshold,
batches, seed and the fingerprint of the buffer the bits index: ps.total, the tensor count, real_params).
"""
import struct

from .variants import (backward_batch, exclusive, files_present, fingerprint, load_tensor, need_fields, need_int, need_opt_str,
                       quiet_backward, real_mask, save_tensor)

KEY = "deletion.saliency"
MASK_FILE, CONFIG_FILE = "saliency_mask.safetensors", "saliency.json"
FIELDS = ("fraction", "batches", "seed", "path")
DEFAULTS = dict(fraction=0.5, batches=8, seed=0, path=None)
ENTRY_POINTS = ("siss_absf_select", "siss_saliency_mask", "siss_grad_norms_scale_masked", "siss_recombine_clip_adamw_masked")


class SaliencyConfig:
    def __init__(self, fraction, batches, seed, path):
        self.fraction, self.batches, self.seed, self.path = fraction, batches, seed, path


def check_fraction(fraction, key=KEY + ".fraction"):
    """The fraction of the parameters a mask keeps: a number strictly between 0 and 1."""
    if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0.0 < float(fraction) < 1.0:
        raise ValueError(f"{key}={fraction!r}: a number in (0, 1) is needed -- the fraction of all parameters the update may touch "
                         "(leave the key out for the full update)")
    return float(fraction)


def mask_k(fraction, real_params):
    """k = round(fraction * real_params): how many parameters the threshold is set to keep (ties at the threshold add to it)."""
    k = int(round(check_fraction(fraction, "fraction") * int(real_params)))
    if not 1 <= k <= real_params:
        raise ValueError(f"fraction={fraction!r} of {real_params} parameters keeps k = {k}: no parameter would be selected")
    return k


def parse_saliency(value, trainable=None, lora=None):
    """`deletion.saliency`: None (absent / null: the full update, today's run) or a SaliencyConfig.  Refused, naming the entry: anything
    but a mapping, an unknown field, a fraction outside (0, 1), batches < 1, a non-integer seed, a path that is no string, and the key
    together with deletion.trainable or deletion.lora (`trainable`, `lora`: those keys' values)."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{fraction:0.5,batches:8}")
    exclusive("config", {KEY: value, "deletion.lora": lora, "deletion.trainable": trainable})
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    return SaliencyConfig(check_fraction(v["fraction"]),
                          need_int(KEY + ".batches", v["batches"], True, "a positive number of forget micro-batches"),
                          need_int(KEY + ".seed", v["seed"]),
                          need_opt_str(KEY + ".path", v["path"], f"the directory that holds {MASK_FILE} and {CONFIG_FILE}"))


def bits_to_float(bits):
    return struct.unpack("<f", struct.pack("<I", int(bits) & 0xffffffff))[0]


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: a saliency mask needs the kernels of csrc/saliency.hip (there is no "
                               "fall-back to the full update)")


def select_magnitude(g, k):
    """The exact k-th largest |g| of a flat f32 device tensor: {threshold_bits, count_gt, count_ge, nonfinite} (siss_absf_select; one
    small D2H copy)."""
    import torch
    from . import lib
    require_kernels()
    assert g.dtype == torch.float32 and g.is_cuda and g.dim() == 1 and g.is_contiguous()
    work = torch.empty(lib.query("siss_absf_select_work_bytes"), dtype=torch.uint8, device=g.device)
    result = torch.zeros(lib.query("siss_absf_select_result_words"), dtype=torch.int64, device=g.device)
    lib.call("siss_absf_select", g, g.numel(), int(k), work, result)
    r = result.cpu().tolist()
    return dict(threshold_bits=int(r[0]), count_gt=int(r[1]), count_ge=int(r[2]), nonfinite=int(r[3]))


def pack_threshold(g, threshold_bits):
    """The packed mask of |g| >= threshold (bitwise, as integers): int32 words on g's device (siss_saliency_mask)."""
    import torch
    from . import lib
    require_kernels()
    bits = torch.zeros((g.numel() + 31) // 32, dtype=torch.int32, device=g.device)
    lib.call("siss_saliency_mask", g, g.numel(), int(threshold_bits), bits)
    return bits


def pack_bool(flags):
    """A flat bool tensor -> int32 words, bit (i & 31) of word (i >> 5) = flags[i], the tail bits zero."""
    import torch
    n = flags.numel()
    nwords = (n + 31) // 32
    b = torch.zeros(nwords * 32, dtype=torch.int64, device=flags.device)
    b[:n] = flags.reshape(-1).to(torch.int64)
    w = (b.view(nwords, 32) << torch.arange(32, dtype=torch.int64, device=flags.device)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bool(bits, n):
    """The inverse of pack_bool: the first n flags of the words."""
    import torch
    w = bits.to(torch.int64) & 0xffffffff
    return ((w.view(-1, 1) >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1).reshape(-1)[:n].bool()


def count_bits(bits):
    """The number of set bits of the words (a popcount per word: no per-bit temporaries)."""
    import torch
    w = bits.to(torch.int64) & 0xffffffff
    w = w - ((w >> 1) & 0x55555555)
    w = (w & 0x33333333) + ((w >> 2) & 0x33333333)
    w = (w + (w >> 4)) & 0x0f0f0f0f
    return int((((w * 0x01010101) & 0xffffffff) >> 24).sum())


class SaliencyMask:
    """One bit per float of an engine's flat parameter buffer.  bits: int32 words on the engine's device (they live as long as the
    mask: a captured step holds their address); count: the selected parameters (count_ge of the select: more than k on ties); k, the
    threshold (float) and the fraction that were asked for; params: the engine's real parameter count."""

    def __init__(self, engine, bits, count, k=None, threshold=None, fraction=None, batches=None, seed=None):
        import torch
        fp = fingerprint(engine)
        assert bits.dtype == torch.int32 and bits.dim() == 1 and bits.numel() == (fp["total"] + 31) // 32, "mask words do not cover the buffer"
        self.bits = bits.to(engine.device).contiguous()
        self.count, self.k, self.threshold = int(count), (None if k is None else int(k)), threshold
        self.fraction, self.batches, self.seed = fraction, batches, seed
        self.total, self.tensors, self.params = fp["total"], fp["tensors"], fp["real_params"]

    # ---------------------------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_gradient(cls, engine, g, fraction, batches=None, seed=None):
        """g: a flat f32 view of the engine's gradient set, alignment padding included.  The select runs over the whole buffer: padding
        gradients are exactly zero (siss_amd/trainable.py), so they can only tie at the bottom and the k-th largest over the buffer is
        the k-th largest over the real parameters -- unless the threshold itself is zero, which is refused."""
        fp = fingerprint(engine)
        k = mask_k(fraction, fp["real_params"])
        assert g.numel() == fp["total"], "the gradient does not cover the engine's flat buffer"
        r = select_magnitude(g, k)
        if r["nonfinite"] > 0:
            raise ValueError(f"saliency mask: the forget gradient holds {r['nonfinite']} non-finite value(s) (inf / NaN): no threshold "
                             "is taken from it")
        if r["threshold_bits"] == 0:
            raise ValueError(f"saliency mask: the forget gradient has fewer than k = {k} non-zero entries ({r['count_gt']} of "
                             f"{fp['real_params']} parameters): a threshold of zero would select the alignment padding -- use a smaller fraction")
        bits = pack_threshold(g, r["threshold_bits"])
        return cls(engine, bits, r["count_ge"], k=k, threshold=bits_to_float(r["threshold_bits"]), fraction=float(fraction),
                   batches=batches, seed=seed)

    @classmethod
    def ones(cls, engine):
        """Every bit set (the alignment padding included: the masked passes then ARE the whole-buffer passes)."""
        import torch
        fp = fingerprint(engine)
        bits = torch.full(((fp["total"] + 31) // 32,), -1, dtype=torch.int32, device=engine.device)
        tail = fp["total"] % 32
        if tail:
            bits[-1] = (1 << tail) - 1
        return cls(engine, bits, fp["real_params"])

    @classmethod
    def from_bool(cls, engine, tensor):
        """tensor: ps.total flags (bool, or anything whose non-zeros are set), in the flat buffer's order.  count: the set flags that fall
        on real parameters."""
        import torch
        ps = engine.ps
        flags = torch.as_tensor(tensor).reshape(-1).to(engine.device) != 0
        if flags.numel() != ps.total:
            raise ValueError(f"SaliencyMask.from_bool: {flags.numel()} flags for a flat buffer of {ps.total} floats")
        real = real_mask(ps.specs, ps.total, engine.device)
        return cls(engine, pack_bool(flags), int((flags & real).sum()))

    def to_bool(self):
        return unpack_bool(self.bits, self.total)

    # ---------------------------------------------------------------------------------------------------------------- files
    def config(self):
        return dict(fraction=self.fraction, k=self.k, count=self.count, threshold=self.threshold, batches=self.batches, seed=self.seed,
                    total=self.total, tensors=self.tensors, real_params=self.params)

    def save(self, directory):
        """saliency_mask.safetensors + saliency.json under `directory` (safetensors and JSON only)."""
        save_tensor(directory, MASK_FILE, "bits", self.bits, CONFIG_FILE, self.config())

    @staticmethod
    def present(directory):
        return files_present(directory, MASK_FILE, CONFIG_FILE)

    @classmethod
    def load(cls, directory, engine):
        """The mask saved under `directory`, for `engine`: refused when it was taken over another buffer (ps.total, the tensor count
        or the real parameter count differ)."""
        bits, c = load_tensor(directory, MASK_FILE, "bits", CONFIG_FILE, engine, "mask")
        return cls(engine, bits, c["count"], k=c.get("k"), threshold=c.get("threshold"), fraction=c.get("fraction"),
                   batches=c.get("batches"), seed=c.get("seed"))

    def log_fields(self):
        """What every log line of a masked run carries."""
        return dict(saliency_params=self.count, saliency_fraction=self.count / self.params, saliency_threshold=self.threshold)


def forget_gradient(stepper, batches_iter, n_batches, *, prepare=None, sample_noise=None, conditioning=None, timestep_low=0,
                    generator=None):
    """The gradient of the forget eps-MSE loss at the stepper's current weights, averaged over n_batches micro-batches drawn from
    batches_iter: the forward and the nsets = 1 backward that loss_fn = simple_neg_del drives (the sign does not matter for a
    magnitude), scale 1 / (B * n_batches), accumulated in gradient set 0 and RETURNED as a copy [ps.total] f32.  prepare(batch,
    generator) -> images / latents, sample_noise(shape, device, generator), conditioning: the task's own (defaults: identity, randn,
    none); timesteps uniform in [timestep_low, T).  No optimizer launch and no gradient exchange (the overlap hook of a data-parallel
    stepper is off for the duration): on return the gradient buffers are zero and the parameters,
    m, v, the step counters and the sparse-fill records are what they were."""
    if n_batches < 1:
        raise ValueError(f"forget_gradient: n_batches={n_batches!r}")
    with quiet_backward(stepper, "forget_gradient"):
        for k in range(n_batches):
            # first micro-batch: one-split weight gradients overwrite their tiles; the others accumulate
            backward_batch(stepper, next(batches_iter), n_batches, first=k == 0, prepare=prepare, sample_noise=sample_noise,
                           conditioning=conditioning, timestep_low=timestep_low, generator=generator)
        g = stepper.e.ps.grads[0].clone()
    return g

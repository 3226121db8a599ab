"""Fisher-weighted anchor of the unlearning update (OPT-IN, not the reference's protocol): `deletion.ewc`, `SISSStepper(ewc=...)`.

Elastic weight consolidation as Selective Amnesia uses it for diffusion models (Heng & Soh, NeurIPS 2023), and its uniform case L2-SP:
with strength lambda, the weights theta* the run starts from and one value F_i >= 0 per parameter, the penalty (lambda / 2) sum_i F_i
(theta_i - theta*_i)^2 holds the model near the pretrained one where the kept data depend on it.  Its gradient lambda F (theta - theta*)
is folded into the KEEP-side gradient set once per optimizer step, inside pass 1 of the flat update (csrc/ewc.hip:
siss_grad_norms_scale_ewc), so that the three norms, the scaling factor, the clip and AdamW all see g_x + lambda F (theta - theta*); pass 2
is the whole-buffer siss_recombine_clip_adamw.  The single-set objectives keep their gradient in set 0: one rule for all six losses.

F here is the EMPIRICAL Fisher at MICRO-BATCH granularity of the keep eps-MSE: the mean over `batches` keep micro-batches of the squared
gradient of the batch-mean loss (batch_size 1 gives the per-sample Fisher).  It is not Selective Amnesia's generative-replay pipeline.

The files: `fisher.safetensors` (key `fisher`, the flat buffer's layout) beside `fisher.json` (strength, batches, batch_size, seed,
normalize, mean / max before the normalisation, the zero count, whether it was computed or loaded, and the fingerprint of the buffer).
"""
from .variants import (exclusive, files_present, fingerprint, fisher_of_batches, load_tensor, need_bool, need_fields, need_int,
                       need_opt_str, real_mask, save_tensor)

KEY = "deletion.ewc"
FISHER_FILE, CONFIG_FILE = "fisher.safetensors", "fisher.json"
FIELDS = ("strength", "batches", "batch_size", "seed", "normalize", "path")
DEFAULTS = dict(strength=None, batches=8, batch_size=None, seed=0, normalize=True, path=None)
ENTRY_POINTS = ("siss_fisher_accumulate", "siss_grad_norms_scale_ewc", "siss_ewc_partials_words")
PENALTY_SLOT, GRAD_NORM_SLOT = 12, 13          # of the optimizer's 16-float scalar block (csrc/ewc.hip)


class EWCConfig:
    def __init__(self, strength, batches, batch_size, seed, normalize, path):
        self.strength, self.batches, self.batch_size, self.seed, self.normalize, self.path = (strength, batches, batch_size, seed,
                                                                                              normalize, path)

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS}


def check_strength(strength, key=KEY + ".strength"):
    import math
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not math.isfinite(strength) or not strength > 0:
        raise ValueError(f"{key}={strength!r}: a number > 0 is needed -- the weight lambda of the penalty (lambda / 2) sum F (theta - "
                         "theta*)^2 (leave the key out for no anchor)")
    return float(strength)


def parse_ewc(value, trainable=None, lora=None, saliency=None):
    """`deletion.ewc`: None (absent / null: no anchor, today's run) or an EWCConfig.  Refused, naming the entry: anything but a mapping,
    an unknown field, a missing or non-positive strength, batches < 1, batch_size < 1, a non-integer seed, a normalize that is no bool,
    a path that is no string, and the key together with deletion.trainable, deletion.lora or deletion.saliency (those keys' values)."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{strength:10,batches:8}")
    exclusive("config", {KEY: value, "deletion.saliency": saliency, "deletion.lora": lora, "deletion.trainable": trainable})
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    if v["strength"] is None:
        raise ValueError(f"{KEY}.strength is required: a number > 0")
    batch_size = v["batch_size"]
    if batch_size is not None:
        need_int(KEY + ".batch_size", batch_size, True, "null (train_batch_size) or a positive micro-batch size (1: the per-sample Fisher)")
    return EWCConfig(check_strength(v["strength"]),
                     need_int(KEY + ".batches", v["batches"], True, "a positive number of keep micro-batches"), batch_size,
                     need_int(KEY + ".seed", v["seed"]), need_bool(KEY + ".normalize", v["normalize"]),
                     need_opt_str(KEY + ".path", v["path"], f"the directory that holds {FISHER_FILE} and {CONFIG_FILE}"))


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: a Fisher anchor needs the kernels of csrc/ewc.hip (there is no "
                               "fall-back to the plain update)")


def normalize_fisher(F, real):
    """Divide F (any float dtype, in place) by its f64 mean over the real parameters, once, so that the strength reads like a
    per-weight L2 strength.  Returns (mean, max, zeros) of the real parameters BEFORE the division.  Refused: a non-finite entry, an
    all-zero F."""
    stats = fisher_stats(F, real)
    if stats[0] == 0.0:
        raise ValueError("Fisher anchor: F is zero on every parameter (no keep gradient reached the weights): nothing to normalise, "
                         "and the penalty would vanish")
    F.div_(stats[0])
    return stats


def fisher_stats(F, real):
    """(f64 mean, max, number of zeros) of F over the real parameters; a non-finite entry is refused."""
    import torch
    bad = int((~torch.isfinite(F)).sum())
    if bad:
        raise ValueError(f"Fisher anchor: F holds {bad} non-finite value(s) (inf / NaN): no anchor is built from it")
    r = F[real]
    return float(r.double().mean()), float(r.max()), int((r == 0).sum())


class FisherAnchor:
    """F (one value >= 0 per float of an engine's flat parameter buffer, zero on the alignment padding), the anchor point pstar (a
    clone of the flat buffer taken when the anchor is built) and the strength.  Both tensors live as long as the anchor: a captured
    step holds their addresses."""

    def __init__(self, engine, fisher, pstar, strength, *, batches=None, batch_size=None, seed=None, normalize=None, mean=None,
                 max=None, zeros=None, source="given"):
        import torch
        fp = fingerprint(engine)
        ps = engine.ps
        for name, t in (("fisher", fisher), ("pstar", pstar)):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == fp["total"]):
                raise ValueError(f"FisherAnchor: {name} must be {fp['total']} f32 values in the flat buffer's layout")
        self.engine = engine
        self.fisher = fisher.to(ps.flat.device).contiguous()
        self.pstar = pstar.to(ps.flat.device).contiguous()
        self.strength = check_strength(strength, "strength")
        self.batches, self.batch_size, self.seed, self.normalize = batches, batch_size, seed, normalize
        self.mean, self.max, self.zeros, self.source = mean, max, zeros, source
        self.total, self.tensors, self.params = fp["total"], fp["tensors"], fp["real_params"]

    # ---------------------------------------------------------------------------------------------------------------- construction
    @classmethod
    def uniform(cls, engine, strength):
        """F = 1 on the real parameters and 0 on the alignment padding: L2-SP."""
        ps = engine.ps
        F = real_mask(ps.specs, ps.total, ps.flat.device).float()
        return cls(engine, F, ps.flat.detach().clone(), strength, normalize=False, mean=1.0, max=1.0, zeros=0, source="uniform")

    @classmethod
    def from_batches(cls, stepper, batches_iter, n_batches, *, strength, prepare=None, sample_noise=None, conditioning=None,
                     timestep_low=0, generator=None, normalize=True, batch_size=None, seed=None):
        """The empirical Fisher of the keep eps-MSE at the stepper's current weights: for each of n_batches micro-batches drawn from
        batches_iter one forward and one nsets = 1 backward at scale 1 / B (timesteps uniform in [timestep_low, T), noise from
        sample_noise), then F += g^2 / n_batches (siss_fisher_accumulate on gradient set 0).  forget_gradient's guarantees hold: no
        optimizer launch, the overlap hook off, no collective pending; on return the gradient buffers are zero and parameters, moments,
        step counters and sparse-fill records are what they were.  normalize: F is divided by its f64 mean over the real parameters."""
        require_kernels()
        if n_batches < 1:
            raise ValueError(f"FisherAnchor.from_batches: n_batches={n_batches!r}")
        e = stepper.e
        ps = e.ps
        F = fisher_of_batches(stepper, batches_iter, n_batches, "FisherAnchor.from_batches", prepare=prepare, sample_noise=sample_noise,
                              conditioning=conditioning, timestep_low=timestep_low, generator=generator)
        real = real_mask(ps.specs, ps.total, F.device)
        mean, mx, zeros = normalize_fisher(F, real) if normalize else fisher_stats(F, real)
        return cls(e, F, ps.flat.detach().clone(), strength, batches=int(n_batches), batch_size=batch_size, seed=seed,
                   normalize=bool(normalize), mean=mean, max=mx, zeros=zeros, source="computed")

    # ---------------------------------------------------------------------------------------------------------------- files
    def config(self):
        return dict(strength=self.strength, batches=self.batches, batch_size=self.batch_size, seed=self.seed, normalize=self.normalize,
                    mean=self.mean, max=self.max, zeros=self.zeros, source=self.source, total=self.total, tensors=self.tensors,
                    real_params=self.params)

    def save(self, directory):
        """fisher.safetensors + fisher.json under `directory` (safetensors and JSON only)."""
        save_tensor(directory, FISHER_FILE, "fisher", self.fisher, CONFIG_FILE, self.config())

    @staticmethod
    def present(directory):
        return files_present(directory, FISHER_FILE, CONFIG_FILE)

    @classmethod
    def load(cls, directory, engine, strength):
        """The F saved under `directory`, anchored at `engine`'s CURRENT weights with `strength`: refused when it was taken over another
        buffer (ps.total, the tensor count or the real parameter count differ)."""
        F, c = load_tensor(directory, FISHER_FILE, "fisher", CONFIG_FILE, engine, "Fisher")
        return cls(engine, F, engine.ps.flat.detach().clone(), strength, batches=c.get("batches"), batch_size=c.get("batch_size"),
                   seed=c.get("seed"), normalize=c.get("normalize"), mean=c.get("mean"), max=c.get("max"), zeros=c.get("zeros"),
                   source="loaded")

    def log_fields(self):
        """What the anchor itself adds to every log line (ewc_penalty and ewc_grad_norm come out of the step's scalar block)."""
        return dict(ewc_strength=self.strength)

    def stats_from(self, s):
        """The three logged fields from a host copy of the optimizer's scalar block."""
        return dict(ewc_penalty=float(s[PENALTY_SLOT]), ewc_grad_norm=float(s[GRAD_NORM_SLOT]), ewc_strength=self.strength)

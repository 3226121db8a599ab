"""Selective Synaptic Dampening (OPT-IN, not the reference's protocol): `deletion.ssd`.

SSD (Foster, Schoepf & Brintrup, AAAI 2024) unlearns WITHOUT gradient steps: take the diagonal empirical Fisher of the forget set and
of the training data at the pretrained weights, and scale down, once, the weights that matter far more to the forget set than to the
rest.  Per float i of the engine's flat parameter buffer (alignment padding included; both importances are exactly 0 there):

    r[i]    = 0 if F_forget[i] == 0 else F_forget[i] / F_keep[i]        (f32; 0/0 -> 0, x/0 -> +inf, never a NaN)
    selected: r[i] > alpha (the paper's rule), or r[i] >= tau with tau the exact k-th largest r (`fraction`; ties included)
    beta    = lambda / r[i] if r[i] > lambda else 1                      (= min(lambda / r, 1); r = +inf gives 0)
    p[i]   <- p[i] * beta on the selected; every other float keeps its bits

DEVIATION from the paper, which writes F_forget > alpha * F_keep and beta = min(lambda * F_keep / F_forget, 1): the selection and
the dampening here work on the MATERIALISED f32 ratio.  That differs by rounding only, gives the two entry modes (`alpha`,
`fraction`) one definition, and the radix select of the fraction mode needs the buffer anyway.

Both importances are the empirical Fisher of the eps-MSE at MICRO-BATCH granularity (variants.fisher_of_batches; batch_size 1, the
default, is the per-sample Fisher SSD is defined on).  The ratio and the select / dampen / report pass are csrc/ssd.hip; the threshold
of the fraction mode is siss_absf_select (csrc/saliency.hip) on r.  SSD is no update variant: it runs once, before the loop, and
combines with `deletion.saliency` and `deletion.ewc` (which then see the dampened model), not with `deletion.lora` /
`deletion.trainable`.

The files: `ssd_importance.safetensors` (keys `keep`, `forget`, the flat buffer's layout) beside `ssd.json` (the parsed key, the
batch counts, whether the importances were computed or loaded, the fingerprint of the buffer and -- once the run has dampened -- the
threshold as a value and as bits, the statistics of the pass and the selected count per parameter name).
"""
import math
import struct

from .variants import (files_present, fingerprint, fisher_of_batches, load_tensors, need_fields, need_int, need_opt_str, same_layout,
                       save_config, save_tensors)

KEY = "deletion.ssd"
IMPORTANCE_FILE, CONFIG_FILE = "ssd_importance.safetensors", "ssd.json"
FIELDS = ("alpha", "fraction", "lambda", "keep_batches", "forget_batches", "batch_size", "seed", "targets", "path")
DEFAULTS = {"alpha": None, "fraction": None, "lambda": 1.0, "keep_batches": 64, "forget_batches": 64, "batch_size": 1, "seed": 0,
            "targets": None, "path": None}
ENTRY_POINTS = ("siss_ssd_partials_words", "siss_ssd_ratio", "siss_ssd_dampen")
STATS = ("selected", "dampened", "zeroed", "sum_beta", "sum_delta2", "sum_p2_selected", "sum_p2")      # stats[0..6] of siss_ssd_dampen
_FROZEN = ("sets a trainable subset on the engine, which drops the frozen weight-gradient products both Fishers need{extra} -- to "
           "dampen only some tensors use deletion.ssd.targets (leave one of the two keys out)")


class SSDConfig:
    def __init__(self, alpha, fraction, lam, keep_batches, forget_batches, batch_size, seed, targets, path):
        self.alpha, self.fraction, self.lam = alpha, fraction, lam
        self.keep_batches, self.forget_batches, self.batch_size, self.seed = keep_batches, forget_batches, batch_size, seed
        self.targets, self.path = targets, path                 # targets: compiled expressions, or None (every parameter)

    def as_dict(self):
        d = {k: getattr(self, k) for k in FIELDS if k not in ("lambda", "targets")}
        d["lambda"] = self.lam
        d["targets"] = None if self.targets is None else [p.pattern for p in self.targets]
        return d


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def check_alpha(alpha, key=KEY + ".alpha"):
    if not _number(alpha) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError(f"{key}={alpha!r}: a finite number >= 0 is needed -- a weight is selected when F_forget / F_keep > alpha")
    return float(alpha)


def check_fraction(fraction, key=KEY + ".fraction"):
    if not _number(fraction) or not 0.0 < float(fraction) < 1.0:
        raise ValueError(f"{key}={fraction!r}: a number in (0, 1) is needed -- the fraction of all parameters to dampen, by the largest "
                         "F_forget / F_keep")
    return float(fraction)


def check_lambda(lam, key=KEY + ".lambda"):
    if not _number(lam) or not math.isfinite(lam) or not lam > 0:
        raise ValueError(f"{key}={lam!r}: a finite number > 0 is needed -- a selected weight is scaled by min(lambda / ratio, 1)")
    return float(lam)


def parse_ssd(value, trainable=None, lora=None):
    """`deletion.ssd`: None (absent / null: no dampening, today's run) or an SSDConfig.  Refused, naming the entry: anything but a
    mapping, an unknown field, both or neither of alpha / fraction, alpha < 0 or not finite, a fraction outside (0, 1), lambda <= 0, a
    batch count or batch_size < 1, a non-integer seed, a malformed targets, a path that is no string, and the key together with
    deletion.lora or deletion.trainable (`lora`, `trainable`: those keys' values)."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{fraction:0.01,lambda:1}")
    if lora is not None:
        raise ValueError(f"config: {KEY} and deletion.lora do not combine -- lora "
                         + _FROZEN.format(extra=", and its merge rewrites its targets from a base copy taken before the dampening"))
    if trainable is not None:
        raise ValueError(f"config: {KEY} and deletion.trainable do not combine -- a trainable subset " + _FROZEN.format(extra=""))
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    if (v["alpha"] is None) == (v["fraction"] is None):
        raise ValueError(f"{KEY}: exactly one of alpha and fraction is needed (alpha={v['alpha']!r}, fraction={v['fraction']!r}): alpha "
                         "selects by ratio > alpha, fraction the top fraction of all parameters by ratio")
    from .trainable import parse_patterns
    return SSDConfig(None if v["alpha"] is None else check_alpha(v["alpha"]),
                     None if v["fraction"] is None else check_fraction(v["fraction"]), check_lambda(v["lambda"]),
                     need_int(KEY + ".keep_batches", v["keep_batches"], True, "a positive number of keep micro-batches"),
                     need_int(KEY + ".forget_batches", v["forget_batches"], True, "a positive number of forget micro-batches"),
                     need_int(KEY + ".batch_size", v["batch_size"], True, "a positive micro-batch size (1: the per-sample Fisher)"),
                     need_int(KEY + ".seed", v["seed"]), parse_patterns(v["targets"], KEY + ".targets"),
                     need_opt_str(KEY + ".path", v["path"], f"the directory that holds {IMPORTANCE_FILE} and {CONFIG_FILE}"))


def select_targets(names, patterns):
    """The parameter names deletion.ssd.targets selects (None: every parameter), with trainable.select's matching and refusals."""
    from .trainable import select
    return select(names, patterns, key=KEY + ".targets")


def float_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS + ("siss_fisher_accumulate", "siss_absf_select"):
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: Selective Synaptic Dampening needs the kernels of csrc/ssd.hip, "
                               "csrc/ewc.hip and csrc/saliency.hip (there is no fall-back)")


def check_importance(F, name):
    """A non-finite or negative importance is refused (as ewc.fisher_stats refuses a non-finite F): no ratio is taken from it."""
    import torch
    bad = int((~torch.isfinite(F)).sum()) + int((F < 0).sum())
    if bad:
        raise ValueError(f"SSD: the {name} importance holds {bad} non-finite or negative value(s): no ratio is taken from it")


class Importances:
    """keep, forget: the two empirical Fishers, one value >= 0 per float of an engine's flat parameter buffer (zero on the alignment
    padding); ratio: siss_ssd_ratio of them (given on the ranks that receive it by broadcast).  `targets` (restrict) zeroes the ratio
    outside the named tensors."""

    def __init__(self, engine, keep, forget, *, ratio=None, keep_batches=None, forget_batches=None, batch_size=None, seed=None,
                 source="given"):
        import torch
        from . import lib
        fp = fingerprint(engine)
        dev = engine.ps.flat.device
        for name, t in (("keep", keep), ("forget", forget), ("ratio", ratio)):
            if t is None and name == "ratio":
                continue
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == fp["total"]):
                raise ValueError(f"Importances: {name} must be {fp['total']} f32 values in the flat buffer's layout")
        self.engine = engine
        self.keep, self.forget = keep.to(dev).contiguous(), forget.to(dev).contiguous()
        self.keep_batches, self.forget_batches, self.batch_size, self.seed, self.source = keep_batches, forget_batches, batch_size, seed, source
        self.total, self.tensors, self.params = fp["total"], fp["tensors"], fp["real_params"]
        self.targets, self.report = None, None
        if ratio is None:
            require_kernels()
            check_importance(self.keep, "keep")
            check_importance(self.forget, "forget")
            ratio = torch.empty_like(self.keep)
            lib.call("siss_ssd_ratio", self.keep, self.forget, ratio, self.total)
        self.ratio = ratio.to(dev).contiguous()

    @classmethod
    def from_batches(cls, stepper, keep_iter, forget_iter, n_keep, n_forget, *, prepare=None, sample_noise=None, conditioning=None,
                     timestep_low=0, generator=None, batch_size=None, seed=None):
        """F_keep from n_keep micro-batches of keep_iter, THEN F_forget from n_forget of forget_iter, at the stepper's current weights
        (variants.fisher_of_batches: one forward and one nsets = 1 backward at scale 1 / B per micro-batch, timesteps uniform in
        [timestep_low, T), noise from sample_noise, F += g^2 / batches), both drawing from the one `generator`.  No optimizer launch,
        the overlap hook off, no collective pending; on return the gradient buffers are zero and parameters, moments, step counters
        and sparse-fill records are what they were."""
        require_kernels()
        if n_keep < 1 or n_forget < 1:
            raise ValueError(f"Importances.from_batches: n_keep={n_keep!r}, n_forget={n_forget!r}")
        draw = dict(prepare=prepare, sample_noise=sample_noise, conditioning=conditioning, timestep_low=timestep_low, generator=generator)
        keep = fisher_of_batches(stepper, keep_iter, n_keep, "Importances.from_batches", **draw)
        forget = fisher_of_batches(stepper, forget_iter, n_forget, "Importances.from_batches", **draw)
        return cls(stepper.e, keep, forget, keep_batches=int(n_keep), forget_batches=int(n_forget), batch_size=batch_size, seed=seed,
                   source="computed")

    def restrict(self, names):
        """Zero the ratio outside the tensors `names` (None: nothing to do).  In place: the selection and the dampening that follow
        read the restricted ratio."""
        if names is None:
            return self
        import torch
        specs = self.engine.ps.specs
        inside = torch.zeros(self.total, dtype=torch.bool, device=self.ratio.device)
        for n in names:
            inside[specs[n].off:specs[n].off + specs[n].numel] = True
        self.ratio.masked_fill_(~inside, 0.0)
        self.targets = list(names)
        return self

    # ---------------------------------------------------------------------------------------------------------------- files
    def config(self):
        c = dict(keep_batches=self.keep_batches, forget_batches=self.forget_batches, batch_size=self.batch_size, seed=self.seed,
                 source=self.source, total=self.total, tensors=self.tensors, real_params=self.params)
        if self.report is not None:
            c.update(self.report)
        return c

    def save(self, directory):
        """ssd_importance.safetensors + ssd.json under `directory` (safetensors and JSON only)."""
        save_tensors(directory, IMPORTANCE_FILE, {"keep": self.keep, "forget": self.forget}, CONFIG_FILE, self.config())

    def save_report(self, directory, report):
        """ssd.json again, now with what the run did with the importances (the tensor file is not rewritten)."""
        self.report = dict(report)
        save_config(directory, CONFIG_FILE, self.config())

    @staticmethod
    def present(directory):
        return files_present(directory, IMPORTANCE_FILE, CONFIG_FILE)

    @classmethod
    def load(cls, directory, engine):
        """The importances saved under `directory`, for `engine`: refused when they were taken over another buffer (ps.total, the
        tensor count or the real parameter count differ)."""
        t, c = load_tensors(directory, IMPORTANCE_FILE, CONFIG_FILE, engine, "SSD importances")
        return cls(engine, t["keep"], t["forget"], keep_batches=c.get("keep_batches"), forget_batches=c.get("forget_batches"),
                   batch_size=c.get("batch_size"), seed=c.get("seed"), source="loaded")


def fraction_k(fraction, real_params):
    return max(1, int(round(check_fraction(fraction, "fraction") * int(real_params))))


def select(imp, alpha=None, fraction=None, targets=None):
    """(threshold, strict, k, count_gt, count_ge) of one of the two rules over imp.ratio, after restricting it to the tensors
    `targets` (parameter names; None: every parameter).  alpha: threshold = f32(alpha), strict (ratio > alpha), k None.  fraction:
    k = max(1, round(fraction * real_params)), threshold = the exact k-th largest ratio over the buffer (siss_absf_select: ratios are
    >= 0, so the integer key is the value's order), not strict (ties included: count_ge may exceed k); +inf is a legal threshold, 0 is
    refused -- it would select the alignment padding."""
    import numpy as np
    if (alpha is None) == (fraction is None):
        raise ValueError(f"ssd.select: exactly one of alpha and fraction is needed (alpha={alpha!r}, fraction={fraction!r})")
    imp.restrict(targets)
    r = imp.ratio
    if alpha is not None:
        thr = float(np.float32(check_alpha(alpha, "alpha")))
        return thr, True, None, int((r > thr).sum()), int((r >= thr).sum())
    from .saliency import bits_to_float, select_magnitude
    k = fraction_k(fraction, imp.params)
    s = select_magnitude(r, k)
    if s["threshold_bits"] == 0:
        raise ValueError(f"SSD: fewer than k = {k} weights have a non-zero ratio F_forget / F_keep ({s['count_gt']} of {imp.params} "
                         "parameters): a threshold of zero would select the alignment padding -- use a smaller fraction")
    return bits_to_float(s["threshold_bits"]), False, k, s["count_gt"], s["count_ge"]


def dampen(engine, imp, threshold, strict, lam, apply=True):
    """siss_ssd_dampen on the engine's flat parameter buffer: the statistics as a dict (STATS, plus fraction_selected = selected /
    real_params, mean_beta over the selected, delta_norm = sqrt(sum (p' - p)^2) and relative_change = delta_norm / |p|).  apply: the
    parameters are written and the bf16 shadow and every derived operand copy brought up to date (engine.refresh_weights); else a dry
    run that writes nothing."""
    import torch
    from . import lib
    require_kernels()
    if not same_layout(imp, engine):
        raise ValueError("ssd.dampen: the importances were taken over another parameter layout")
    p = engine.ps.flat
    partials = torch.empty(lib.query("siss_ssd_partials_words"), dtype=torch.float64, device=p.device)
    stats = torch.empty(8, dtype=torch.float64, device=p.device)
    lib.call("siss_ssd_dampen", p, imp.ratio, imp.total, float(threshold), int(bool(strict)), check_lambda(lam, "lambda"),
             int(bool(apply)), partials, stats)
    if apply:
        engine.refresh_weights(cast_shadow=True)
    return stats_dict(stats.cpu().tolist(), imp.params)


def stats_dict(s, real_params):
    out = {k: (int(s[i]) if i < 3 else float(s[i])) for i, k in enumerate(STATS)}
    out["fraction_selected"] = out["selected"] / real_params
    out["mean_beta"] = out["sum_beta"] / out["selected"] if out["selected"] else None
    out["delta_norm"] = math.sqrt(out["sum_delta2"])
    out["relative_change"] = math.sqrt(out["sum_delta2"] / out["sum_p2"]) if out["sum_p2"] > 0 else 0.0
    return out


def per_tensor(imp, threshold, strict):
    """{parameter name: selected floats} of a threshold, the tensors without a selected float left out (torch, off the hot path: one
    comparison over the buffer, one count per tensor, one copy to the host)."""
    import torch
    r = imp.ratio
    sel = (r > threshold) if strict else (r >= threshold)
    specs = imp.engine.ps.specs
    counts = torch.stack([sel[sp.off:sp.off + sp.numel].sum() for sp in specs.values()]).cpu().tolist()
    return {n: int(c) for n, c in zip(specs, counts) if c}

"""Gradient surgery between the keep and forget gradients (OPT-IN, NOT the reference's protocol): `deletion.surgery`,
`SISSStepper(surgery=...)`.

The step is g = g_x - s g_a with s > 0: where <g_x, g_a> > 0 the forget ascent undoes the keep descent.  Projection methods remove that
interference -- PCGrad (Yu et al., NeurIPS 2020), gradient-projection unlearning (Hoang et al., WACV 2024), the restricted gradient of
Ko et al. (NeurIPS 2024).  The dual-cotangent backward leaves both gradient sets side by side, so the surgery costs no backward pass: per
GROUP G of the flat buffer -- the whole buffer (`granularity: global`) or one parameter tensor with the alignment padding behind it
(`granularity: tensor`, layer-wise surgery) -- the f64 sums xx_G, aa_G, xa_G are taken once per optimizer step, after the accumulation
and the data-parallel exchange; G CONFLICTS when xa_G > 0 (strictly: zero and NaN do not; xx_G = 0 or aa_G = 0 never does), and there

    mode forget   a' = a - (xa / xx) x, x' = x     the forget direction loses the part that raises the keep loss
    mode keep     x' = x - (xa / aa) a, a' = a
    mode mutual   both, each from the ORIGINAL pair (PCGrad, the restricted gradient)

The scaling factor is the norm fix on the projected forget set, s = scaling_norm / |a'| over the whole buffer, and the update direction
clip (x' - s a') = clip (cx_G x - ca_G a) with one f32 coefficient pair per group (csrc/surgery.hip).  With no conflicting group the
step IS the plain one, bit for bit.  The scalar block gains four fields -- the number of conflicting groups, the cosine of the pair and
the shares of |a|^2 and |x|^2 the projections removed -- and `grams()` reads the per-tensor sums of the last step back on demand.
"""
from .variants import exclusive, fingerprint, need_fields

KEY = "deletion.surgery"
FIELDS = ("mode", "granularity")
MODES = ("forget", "keep", "mutual")                     # the C ABI's smode: the index
GRANULARITIES = ("global", "tensor")
DEFAULTS = dict(mode="forget", granularity="tensor")
ENTRY_POINTS = ("siss_grad_norms_scale_surgery", "siss_recombine_clip_adamw_surgery", "siss_surgery_chunk",
                "siss_surgery_partials_words", "siss_surgery_coef_words")
CONFLICTS_SLOT, COS_SLOT, REMOVED_A_SLOT, REMOVED_X_SLOT = 12, 13, 14, 15      # of the optimizer's 16-float scalar block
# the losses with two gradient sets and the norm fix; why the others are refused
LOSSES = ("importance_sampling_with_mixture", "double_forward_with_neg_del", "subscore_bernoulli")
REFUSED_LOSSES = {
    "erasediff": "its s <= 0 from eta - <g_x, g_a> / |g_a|^2 is that mode's own conflict rule",
    "simple_neg_del": "it has one gradient set: there is no pair to project",
    "naive_del": "it has one gradient set: there is no pair to project",
}


class SurgeryConfig:
    def __init__(self, mode, granularity):
        self.mode, self.granularity = mode, granularity

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS}


def _choice(key, x, choices):
    if not isinstance(x, str) or x not in choices:
        raise ValueError(f"{key}={x!r}: one of {' | '.join(choices)} is needed")
    return x


def parse_surgery(value, trainable=None, lora=None, saliency=None, ewc=None):
    """`deletion.surgery`: None (absent / null: the plain update, today's run) or a SurgeryConfig.  Refused, naming the entry: anything
    but a mapping, an unknown field, a mode that is not forget | keep | mutual, a granularity that is not global | tensor, and the key
    together with deletion.trainable, deletion.lora, deletion.saliency or deletion.ewc (those keys' values).  deletion.ssd runs once,
    before the loop, and does combine."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{mode:mutual}")
    exclusive("config", {KEY: value, "deletion.ewc": ewc, "deletion.saliency": saliency, "deletion.lora": lora,
                         "deletion.trainable": trainable})
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    return SurgeryConfig(_choice(KEY + ".mode", v["mode"], MODES), _choice(KEY + ".granularity", v["granularity"], GRANULARITIES))


def check_loss(loss_fn, where=KEY):
    """Surgery applies to the two-set losses with the norm fix; the others are refused with their reason."""
    if loss_fn in LOSSES:
        return loss_fn
    why = REFUSED_LOSSES.get(loss_fn, "it is not one of " + ", ".join(LOSSES))
    raise ValueError(f"{where} does not apply to loss_fn={loss_fn!r}: {why} (leave the key out)")


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: gradient surgery needs the kernels of csrc/surgery.hip (there is no "
                               "fall-back to the plain update)")


# ---------------------------------------------------------------------------------------------------------------- the plan (host)
def group_table(specs, total, granularity):
    """(names, offsets): the groups of a flat buffer in buffer order -- `tensor`: one per parameter tensor, from its offset to the next
    tensor's (the alignment padding belongs to the tensor before it); `global`: the whole buffer.  offsets: T + 1 ascending ints,
    offsets[0] = 0, offsets[T] = total."""
    if granularity == "global":
        return ["*"], [0, int(total)]
    order = sorted(specs.values(), key=lambda sp: sp.off)
    if not order or order[0].off != 0:
        raise ValueError("surgery: the first tensor of the buffer does not start at offset 0")
    offs = [int(sp.off) for sp in order] + [int(total)]
    for sp, a, b in zip(order, offs, offs[1:]):
        if a % 4 or b - a < sp.numel or sp.numel < 1:
            raise ValueError(f"surgery: {sp.name} at [{a}, {b}) of the buffer: a 16-byte aligned stretch that holds its {sp.numel} "
                             "parameters is needed")
    return [sp.name for sp in order], offs


def job_plan(offsets, chunk):
    """(starts, groups, first): every group cut into jobs of `chunk` floats from its start, the last one shorter; first[g] is the
    index of group g's first job (T + 1 entries: first[T] = the job count).  The jobs tile [0, offsets[-1]) exactly once."""
    starts, groups, first = [], [], [0]
    for g, (a, b) in enumerate(zip(offsets, offsets[1:])):
        for st in range(a, b, chunk):
            starts.append(st)
            groups.append(g)
        first.append(len(starts))
    return starts, groups, first


def plan_words(offsets, chunk):
    """The device plan of csrc/surgery.hip as one list of ints: job starts, job groups, first jobs, offsets.  And the job count."""
    starts, groups, first = job_plan(offsets, chunk)
    return starts + groups + first + [int(o) for o in offsets], len(starts)


class Surgery:
    """The plan of one engine's flat buffer (group table, job table) and the slabs the two passes write: one f64 row per job, the f64
    group sums, the f32 coefficient table.  All of it lives as long as the object: a captured step holds the addresses."""

    def __init__(self, engine, mode="forget", granularity="tensor"):
        import torch
        from . import lib
        require_kernels()
        self.mode = _choice("mode", mode, MODES)
        self.granularity = _choice("granularity", granularity, GRANULARITIES)
        self.engine = engine
        ps = engine.ps
        fp = fingerprint(engine)
        self.total, self.tensors, self.params = fp["total"], fp["tensors"], fp["real_params"]
        self.names, self.offsets = group_table(ps.specs, ps.total, self.granularity)
        self.chunk = int(lib.query("siss_surgery_chunk"))
        words, self.jobs = plan_words(self.offsets, self.chunk)
        dev = ps.flat.device
        self.groups = len(self.names)
        self.group_offsets = torch.tensor(self.offsets, dtype=torch.int64)                  # HOST: the entry points check it
        self.plan = torch.tensor(words, dtype=torch.int64).to(dev)
        self.partials = torch.zeros(lib.query("siss_surgery_partials_words", self.jobs), dtype=torch.float64, device=dev)
        self.group_sums = torch.zeros(3 * self.groups, dtype=torch.float64, device=dev)
        self.coef = torch.zeros(lib.query("siss_surgery_coef_words", self.groups), dtype=torch.float32, device=dev)

    @property
    def smode(self):
        return MODES.index(self.mode)

    def log_fields(self):
        """What the surgery itself adds to every log line (the four statistics come out of the step's scalar block)."""
        return dict(surgery_mode=self.mode, surgery_granularity=self.granularity, surgery_groups=self.groups)

    def stats_from(self, s):
        """The logged fields from a host copy of the optimizer's scalar block."""
        return dict(surgery_conflicts=int(s[CONFLICTS_SLOT]), surgery_cos=float(s[COS_SLOT]), surgery_removed_a=float(s[REMOVED_A_SLOT]),
                    surgery_removed_x=float(s[REMOVED_X_SLOT]), **self.log_fields())

    def grams(self):
        """{group name: (xx, aa, xa, conflicts)} of the LAST step: one device-to-host read of the f64 group sums, on demand (never inside
        a step).  The names are the parameter tensors' (`tensor`) or "*" (`global`)."""
        g = self.group_sums.cpu().view(-1, 3).tolist()
        return {name: (xx, aa, xa, bool(xa > 0 and xx > 0 and aa > 0)) for name, (xx, aa, xa) in zip(self.names, g)}

"""Teacher-target unlearning for Stable Diffusion (OPT-IN, NOT the reference's protocol): `deletion.loss_fn=teacher_target` with
`+deletion.teacher={...}`, `SISSStepper(loss_fn="teacher_target", teacher=..., teacher_cfg=...)`.

Every other objective of the loop regresses onto the drawn noise, the mixture's eps or EraseDiff's U[0, 1) stand-in.  The two most used
unlearning methods for Stable Diffusion substitute the TARGET instead, and build it from a frozen copy eps* of the pretrained UNet:

    forget: esd      y_forget = u - eta (k - u),  k = eps*(a_t, t, c), u = eps*(a_t, t, empty prompt)      (ESD, Gandikota et al., ICCV 2023)
    forget: anchor   y_forget = eps*(a_t, t, c_anchor)                              (Concept Ablation, Kumari et al., ICCV 2023)
    keep: noise      y_keep = the drawn noise        keep: teacher   y_keep = eps*(x_t, t, c)        keep: none   no keep term

    L = mean_keep |eps_theta(x_t, t, c) - y_keep|^2 + weight * mean_forget |eps_theta(a_t, t, c) - y_forget|^2
    g = g_x + weight g_a            (descent on both; then the usual clip and AdamW)

on keep latents x0, forget latents a0, one shared noise and one shared t per row, as `double_forward_with_neg_del` noises them (NOT
ESD's sampling of x_t from the model's own partial denoising).  The teacher's outputs are constants.  The teacher is a second engine
of the student's configuration and dtype with no gradient buffer and no optimizer state, run forward-only once per micro-batch on the
rows `row_layout` names; csrc/teacher.hip turns its output into the cotangent and the loss sums (siss_teacher_seed) and forms the
update's scalars with the scaling factor fixed at -weight (siss_grad_norms_weighted).
"""
import os

from .variants import fingerprint, need_fields, need_opt_str, save_config

KEY = "deletion.teacher"
LOSS = "teacher_target"
FIELDS = ("forget", "keep", "guidance", "weight", "anchor_prompt", "path")
FORGETS = ("esd", "anchor")                      # the C ABI's forget_mode: the index
KEEPS = ("noise", "teacher", "none")             # the C ABI's keep_mode: the index
DEFAULTS = dict(forget="esd", keep="noise", guidance=1.0, weight=1.0, anchor_prompt=None, path=None)
ENTRY_POINTS = ("siss_teacher_seed", "siss_teacher_partials_words", "siss_grad_norms_weighted")
# the opt-in update variants the teacher does not run with (deletion.lora does: its update goes through the same keywords)
NO_WEIGHTED_FORM = "the teacher target recombines with a fixed weight, and their pass 1 has no weighted form"


class TeacherConfig:
    def __init__(self, forget, keep, guidance, weight, anchor_prompt, path):
        self.forget, self.keep, self.guidance, self.weight = forget, keep, float(guidance), float(weight)
        self.anchor_prompt, self.path = anchor_prompt, path

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS}


def _choice(key, x, choices):
    if not isinstance(x, str) or x not in choices:
        raise ValueError(f"{key}={x!r}: one of {' | '.join(choices)} is needed")
    return x


def _number(key, x, what, ok):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x or x in (float("inf"), float("-inf")) or not ok(x):
        raise ValueError(f"{key}={x!r}: {what} is needed")
    return float(x)


def teacher_exclusive(where, key, value, others):
    """The teacher against the keys (or keywords) of the update variants it does not combine with: `others` {key: value} in the order
    the message should try them.  Raises ValueError naming both and the reason."""
    if value is None:
        return
    for k, v in others.items():
        if v is not None:
            raise ValueError(f"{where}: {key} and {k} do not combine -- {NO_WEIGHTED_FORM} (leave one of the two out)")


def fixed_weight_exclusive(where, others):
    """FlatAdamW.launch(fixed_weight=...) against ranges= / mask= / ewc= / surgery= / eta=."""
    teacher_exclusive(where, "fixed_weight=", True, others)


def parse_teacher(value, trainable=None, saliency=None, ewc=None, surgery=None):
    """`deletion.teacher`: None (absent / null: today's run) or a TeacherConfig.  Refused, naming the entry: anything but a mapping, an
    unknown field, a forget that is not esd | anchor, a keep that is not noise | teacher | none, guidance < 0, weight <= 0, forget:
    anchor without anchor_prompt, forget: esd with one, and the key together with deletion.trainable, deletion.saliency, deletion.ewc
    or deletion.surgery (those keys' values).  deletion.lora and deletion.ssd do combine."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{forget:esd,keep:teacher}")
    teacher_exclusive("config", KEY, value, {"deletion.surgery": surgery, "deletion.ewc": ewc, "deletion.saliency": saliency,
                                             "deletion.trainable": trainable})
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    forget = _choice(KEY + ".forget", v["forget"], FORGETS)
    keep = _choice(KEY + ".keep", v["keep"], KEEPS)
    guidance = _number(KEY + ".guidance", v["guidance"], "a finite number >= 0 (eta of u - eta (k - u))", lambda x: x >= 0)
    weight = _number(KEY + ".weight", v["weight"], "a finite number > 0 (the forget term's weight)", lambda x: x > 0)
    anchor = need_opt_str(KEY + ".anchor_prompt", v["anchor_prompt"], "the anchor prompt (a string, or a .pt embedding / token file)")
    path = need_opt_str(KEY + ".path", v["path"], "a directory with unet/ in the diffusers layout")
    if forget == "anchor" and not anchor:
        raise ValueError(f"{KEY}: forget: anchor needs anchor_prompt (the prompt whose prediction the forget rows are regressed onto)")
    if forget == "esd" and anchor is not None:
        raise ValueError(f"{KEY}: anchor_prompt={anchor!r} with forget: esd -- the esd target uses the empty prompt, not an anchor "
                         "(leave it out, or set forget: anchor)")
    return TeacherConfig(forget, keep, guidance, weight, anchor, path)


def check_path(path):
    """deletion.teacher.path: a directory whose unet/ holds a diffusers checkpoint."""
    d = os.path.join(str(path), "unet")
    for f in ("config.json", "diffusion_pytorch_model.safetensors"):
        if not os.path.isfile(os.path.join(d, f)):
            raise FileNotFoundError(f"{KEY}.path={path!r}: no unet/{f} under it (the teacher is read from <path>/unet in the diffusers "
                                    "layout)")
    return d


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: the teacher target needs the kernels of csrc/teacher.hip (there is "
                               "no fall-back to torch ops)")


# ---------------------------------------------------------------------------------------------------------------- the rows (host)
def row_layout(keep, forget, B):
    """The rows of the two forwards of one micro-batch of B keep and B forget samples, as lists of (samples, conditioning, rows):

        student   [keep B under c | forget B under c], or [forget B under c] with keep: none
        teacher   [keep B under c (keep: teacher only) | forget B under c (esd) or c_anchor (anchor) | forget B under the empty prompt
                  (esd only)]

    plus the counts R / Rt and, for the teacher's output, the row offsets k (the forget rows under c / c_anchor) and u (under the empty
    prompt; None for anchor) that siss_teacher_seed derives from the two modes."""
    _choice("keep", keep, KEEPS)
    _choice("forget", forget, FORGETS)
    B = int(B)
    student = ([] if keep == "none" else [("keep", "c", B)]) + [("forget", "c", B)]
    teacher = [("keep", "c", B)] if keep == "teacher" else []
    k = sum(n for _, _, n in teacher)
    teacher.append(("forget", "c" if forget == "esd" else "anchor", B))
    u = None
    if forget == "esd":
        u = k + B
        teacher.append(("forget", "empty", B))
    return dict(student=student, teacher=teacher, R=sum(n for _, _, n in student), Rt=sum(n for _, _, n in teacher), k=k, u=u)


# ---------------------------------------------------------------------------------------------------------------- the frozen network
class Teacher:
    """A frozen copy of the pretrained UNet beside the student: a second engine of the student's configuration and dtype with NO gradient
    sets and no optimizer state.  weights: None -- the student's master as it is NOW (build the teacher before anything touches the
    weights the run loaded: deletion.ssd, a step) -- or a state dict in the reference layout (`from_path`).  Nothing updates it
    afterwards: the student's refresh_weights() never reaches this engine.  It runs forward-only (`predict`), keeps nothing for a backward
    pass, and owns persistent stacked input / timestep / conditioning buffers per batch shape: a step allocates nothing after the first."""

    def __init__(self, engine, *, weights=None, source="student"):
        self.engine = type(engine)(engine.cfg, engine.device, dtype=engine.adt, grad_sets=0)
        # the student's schedule switches (plain attributes set on the instance): the teacher runs the same forward
        for k, v in vars(engine).items():
            if isinstance(v, (bool, int, float)) and (hasattr(type(engine), k) or k in ("f32_fused", "flash")):
                setattr(self.engine, k, v)
        ps, mine = engine.ps, self.engine.ps
        if (mine.total, list(mine.specs)) != (ps.total, list(ps.specs)):
            raise ValueError("Teacher: the second engine's parameter layout differs from the student's")
        if weights is None:
            mine.flat.copy_(ps.flat)                     # (same layout: the master's bytes)
            self.engine.refresh_weights(cast_shadow=True)
        else:
            self.engine.load_state_dict(weights)
        self.source = source
        self.device = engine.device
        self.empty = self.anchor = None                  # [1, L, X] f32 embeddings (set_embeddings)
        self._stacks = {}
        fp = fingerprint(self.engine)
        self.total, self.tensors, self.params = fp["total"], fp["tensors"], fp["real_params"]
        self.cfg = None

    @classmethod
    def from_path(cls, engine, path):
        """The teacher read from <path>/unet in the diffusers layout (deletion.teacher.path)."""
        from safetensors.torch import load_file
        d = check_path(path)
        return cls(engine, weights=load_file(os.path.join(d, "diffusion_pytorch_model.safetensors")), source=d)

    def set_embeddings(self, empty=None, anchor=None):
        """The [1, L, X] embeddings of the empty prompt (esd) and of the anchor prompt (anchor), kept as f32 on the teacher's device."""
        def one(e, what):
            if e is None:
                return None
            e = e.detach().to(device=self.device).float()
            if e.dim() != 3 or e.shape[0] != 1:
                raise ValueError(f"Teacher.set_embeddings({what}=...): a [1, L, X] embedding is needed, got {tuple(e.shape)}")
            return e.contiguous()
        self.empty, self.anchor = one(empty, "empty"), one(anchor, "anchor")
        return self

    @property
    def nbytes(self):
        """Device bytes the teacher's weights hold: the f32 master and its operand copy (none besides it in the f32 mode)."""
        ps = self.engine.ps
        shadow = 0 if ps.shadow is ps.flat else ps.shadow.numel() * ps.shadow.element_size()
        return int(ps.flat.numel() * 4 + shadow + ps.grads.numel() * 4)

    def check(self, cfg):
        """What a step under `cfg` needs of the teacher, before the first one (and before a capture)."""
        if cfg.forget == "esd" and self.empty is None:
            raise ValueError("Teacher: forget: esd needs the empty prompt's embedding (set_embeddings(empty=...))")
        if cfg.forget == "anchor" and self.anchor is None:
            raise ValueError("Teacher: forget: anchor needs the anchor prompt's embedding (set_embeddings(anchor=...))")

    def _stack(self, rows, x, cond):
        import torch
        key = (rows, tuple(x.shape[1:]), x.dtype, tuple(sorted((k, tuple(v.shape[1:])) for k, v in cond.items())))
        st = self._stacks.get(key)
        if st is None:
            dev = self.device
            st = (torch.zeros(rows, *x.shape[1:], dtype=x.dtype, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev),
                  {k: torch.zeros(rows, *v.shape[1:], dtype=torch.float32, device=dev) for k, v in cond.items()})
            self._stacks[key] = st
        return st

    def predict(self, cfg, x_keep, x_forget, t, cond):
        """The teacher's ONE forward of a micro-batch: x_keep / x_forget [B, C, H, W] the noised keep / forget rows (x_keep is read with
        keep: teacher only), t [B], cond the student's conditioning dict ({'encoder_hidden_states': [B, L, X]}, or {} for an
        unconditional engine).  Returns its output [Rt, C, H, W] f32 on the rows of row_layout (the engine's own buffer, valid until the
        next predict).  No gradient, nothing kept for a backward pass, no allocation after the first call of a shape."""
        import torch
        B = x_forget.shape[0]
        lay = row_layout(cfg.keep, cfg.forget, B)
        xs, ts, cs = self._stack(lay["Rt"], x_forget, cond)
        with torch.no_grad():
            r = 0
            for samples, conditioning, n in lay["teacher"]:
                xs[r:r + n].copy_(x_keep if samples == "keep" else x_forget)
                ts[r:r + n].copy_(t)
                for k, buf in cs.items():
                    if conditioning == "c":
                        buf[r:r + n].copy_(cond[k])
                    else:
                        e = self.empty if conditioning == "empty" else self.anchor
                        if k != "encoder_hidden_states" or e is None or tuple(e.shape[1:]) != tuple(buf.shape[1:]):
                            raise ValueError(f"Teacher.predict: the {conditioning} embedding {None if e is None else tuple(e.shape)} does "
                                             f"not fit the conditioning {k} {tuple(buf.shape)}")
                        buf[r:r + n].copy_(e.expand(n, *e.shape[1:]))
                r += n
            if not cs:
                raise ValueError("Teacher.predict: both forget targets are defined through prompts -- a text-conditioned engine and "
                                 "its conditioning are needed")
            eng = self.engine
            out = eng.forward(xs, ts, **cs)
            eng.tape, eng.gmap = [], {}                  # forward only: drop the backward closures
        return out

    def log_fields(self, cfg, B):
        return dict(teacher_forget=cfg.forget, teacher_keep=cfg.keep, teacher_guidance=cfg.guidance, teacher_weight=cfg.weight,
                    teacher_rows=row_layout(cfg.keep, cfg.forget, B)["Rt"])

    def save_config(self, directory, cfg=None):
        """teacher.json: the parsed fields, the teacher's bytes, where its weights came from, and the buffer's fingerprint."""
        cfg = cfg or self.cfg
        save_config(directory, "teacher.json", dict(**(cfg.as_dict() if cfg is not None else {}), bytes=self.nbytes, weights=self.source,
                                                    **fingerprint(self.engine)))

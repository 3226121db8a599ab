"""Unified Concept Editing (OPT-IN, not the reference's protocol): `deletion.uce`.

UCE (Gandikota, Orgad, Belinkov, Materzynska & Bau, WACV 2024) erases concepts WITHOUT gradient steps, images or optimizer state: it
rewrites only the cross-attention key / value projections (`attn2.to_k` / `attn2.to_v`, W [C, X] with X = cross_attention_dim), in
closed form, so that the keys and values of the prompts to erase become those of a destination prompt -- the empty prompt or an
anchor -- while a list of preserved prompts keeps its keys and values.  With the token rows of the prompts stacked,

    C_e [n_e, X]  the rows of the prompts to erase          C_t [n_e, X]  the rows of their destinations, row for row
    C_p [n_p, X]  the rows of the preserved prompts (may be empty)         lambda > 0, s_e > 0, s_p > 0

    M  = lambda I + s_e C_e^T C_e + s_p C_p^T C_p           (X x X, symmetric positive definite because lambda > 0)
    D  = s_e (C_t - C_e)^T C_e                              (X x X)
    dT = D M^-1,      W' = W + W dT                         for EVERY target weight W [C, X]

which is UCE's W' = (lambda W + s_e sum W c* c^T + s_p sum W c c^T)(lambda I + s_e sum c c^T + s_p sum c c^T)^-1 rearranged: dT is ONE
X x X matrix shared by all sites whatever their width C, and only the increment W dT is formed -- the whole weight is never rebuilt
from a product.  M and D are formed in f64; dT comes from a Cholesky solve on the host (as attribution.Attributor's preconditioner);
E = dT^T is rounded ONCE to f32, [X, X] row-major, and delta[r, j] = <W[r, :], E[j, :]> is the exact f32 chain of csrc/uce.hip.

DEVIATION from the authors' code: their scripts pick the token rows that count differently per script (the last subject token, the
tokens behind the first, ...); here EVERY one of the L rows of an embedding counts, for the edited, the destination and the preserved
prompts alike.  Not built: that per-script token selection, the debiasing and moderation presets, editing the text encoder, and UCE
under `deletion.lora`.

UCE is no update variant: it runs once, before the loop (and before `deletion.ssd`), on the weights the run loaded; the teacher of
`deletion.teacher` is built before it and stays pretrained; the saliency mask, the Fisher anchor and the step-0 metrics see the edited
model.  `training_steps=0` makes it a method of its own.

The files: `uce_edit.safetensors` (keys `E` f32, `M`, `D` f64) beside `uce.json` (the parsed key, the prompt lists, the row counts,
cond(M), the statistics of the add and the residuals per tensor, under a fingerprint of X and the embeddings).
"""
import hashlib
import math
import os

from .variants import files_present, need_fields, need_opt_str, save_config, save_tensors

KEY = "deletion.uce"
EDIT_FILE, CONFIG_FILE = "uce_edit.safetensors", "uce.json"
FIELDS = ("edit", "preserve", "preserve_file", "lambda", "edit_scale", "preserve_scale", "targets", "path")
DEFAULT_TARGETS = [r"attn2\.to_[kv]\.weight"]
DEFAULTS = {"edit": None, "preserve": None, "preserve_file": None, "lambda": 0.1, "edit_scale": 1.0, "preserve_scale": 1.0,
            "targets": DEFAULT_TARGETS, "path": None}
ENTRY_POINTS = ("siss_uce_partials_words", "siss_uce_delta", "siss_uce_apply")
STATS = ("sum_delta2", "sum_p2", "max_delta", "floats")                # stats[0..3] of siss_uce_apply
JOB_BYTES = 64


class UCEConfig:
    def __init__(self, edit, preserve, preserve_file, lam, edit_scale, preserve_scale, targets, path):
        self.edit, self.preserve, self.preserve_file = edit, preserve, preserve_file      # edit: [(prompt, target or None), ...]
        self.lam, self.edit_scale, self.preserve_scale = lam, edit_scale, preserve_scale
        self.targets, self.path = targets, path                                         # targets: compiled expressions

    def as_dict(self):
        return {"edit": [{"prompt": p, "target": t} for p, t in self.edit], "preserve": list(self.preserve),
                "preserve_file": self.preserve_file, "lambda": self.lam, "edit_scale": self.edit_scale,
                "preserve_scale": self.preserve_scale, "targets": [p.pattern for p in self.targets], "path": self.path}

    def preserved_prompts(self):
        """`preserve`, then the non-empty lines of `preserve_file` (read now: the file may be written after the key is parsed)."""
        out = list(self.preserve)
        if self.preserve_file is not None:
            if not os.path.isfile(self.preserve_file):
                raise FileNotFoundError(f"{KEY}.preserve_file={self.preserve_file!r}: no such file (one prompt per line)")
            with open(self.preserve_file) as f:
                out += [line.strip() for line in f if line.strip()]
        return out


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def check_positive(x, key, what):
    if not _number(x) or not math.isfinite(x) or not x > 0:
        raise ValueError(f"{key}={x!r}: a finite number > 0 is needed -- {what}")
    return float(x)


def check_lambda(lam, key=KEY + ".lambda"):
    return check_positive(lam, key, "lambda I keeps lambda I + s_e C_e^T C_e + s_p C_p^T C_p positive definite and the unnamed "
                                    "directions of the weights where they are")


def _prompt(x, key):
    if not isinstance(x, str) or x == "":
        raise ValueError(f"{key}={x!r}: a prompt (a non-empty string) is needed")
    return x


def parse_uce(value, lora=None):
    """`deletion.uce`: None (absent / null: no edit, today's run) or a UCEConfig.  Refused, naming the entry: anything but a mapping, an
    unknown field, a missing or empty `edit`, an edit entry that is no {prompt, target} mapping with a prompt (target: null for the
    empty prompt, or a prompt), a preserve that is no list of prompts, a preserve_file or path that is no string, lambda / edit_scale /
    preserve_scale <= 0 or not finite, a malformed targets, and the key together with deletion.lora (`lora`: that key's value)."""
    if value is None:
        return None
    value = need_fields(KEY, value, FIELDS, "{edit:[{prompt:a photo of X,target:null}]}")
    if lora is not None:
        raise ValueError(f"config: {KEY} and deletion.lora do not combine -- the adapter's base copy of its targets is taken before the "
                         "edit, and its merge would write the unedited weights back (UCE under LoRA is not built; leave one of the two out)")
    v = dict(DEFAULTS, **{k: x for k, x in value.items() if x is not None})
    edit = v["edit"]
    if isinstance(edit, (str, bytes)) or not isinstance(edit, (list, tuple)) or len(edit) == 0:
        raise ValueError(f"{KEY}.edit={edit!r}: a non-empty LIST of {{prompt, target}} is needed (target: null for the empty prompt)")
    pairs = []
    for i, entry in enumerate(edit):
        if not hasattr(entry, "keys") or set(entry) - {"prompt", "target"} or "prompt" not in entry:
            raise ValueError(f"{KEY}.edit[{i}]={entry!r}: a mapping {{prompt, target}} is needed")
        t = entry.get("target")
        pairs.append((_prompt(entry["prompt"], f"{KEY}.edit[{i}].prompt"), None if t is None else _prompt(t, f"{KEY}.edit[{i}].target")))
    pres = v["preserve"] if v["preserve"] is not None else []
    if isinstance(pres, (str, bytes)) or not isinstance(pres, (list, tuple)):
        raise ValueError(f"{KEY}.preserve={pres!r}: null or a LIST of prompts is needed")
    pres = [_prompt(p, f"{KEY}.preserve[{i}]") for i, p in enumerate(pres)]
    from .trainable import parse_patterns
    return UCEConfig(pairs, pres, need_opt_str(KEY + ".preserve_file", v["preserve_file"], "a file with one prompt per line"),
                     check_lambda(v["lambda"]),
                     check_positive(v["edit_scale"], KEY + ".edit_scale", "the weight s_e of the edited rows"),
                     check_positive(v["preserve_scale"], KEY + ".preserve_scale", "the weight s_p of the preserved rows"),
                     parse_patterns(list(v["targets"]) if isinstance(v["targets"], tuple) else v["targets"], KEY + ".targets"),
                     need_opt_str(KEY + ".path", v["path"], f"the directory that holds {EDIT_FILE} and {CONFIG_FILE}"))


def select_targets(names, patterns):
    """The parameter names deletion.uce.targets selects, matched as deletion.trainable matches (trainable.select's refusals)."""
    from .trainable import select
    names = list(names)
    got = select(names, patterns, key=KEY + ".targets", announce=False)
    return names if got is None else got


def check_targets(specs, names, X):
    """Refuse a name that is no parameter, or no `mat` of [*, X] (the edit multiplies from the right by an X x X matrix)."""
    for n in names:
        if n not in specs:
            raise KeyError(f"{KEY}: no parameter named {n!r}")
        sp = specs[n]
        if sp.kind != "mat" or len(sp.native_shape) != 2 or int(sp.native_shape[1]) != int(X):
            raise ValueError(f"{KEY}: target {n!r} is a {sp.kind} of shape {tuple(sp.native_shape)}, not a matrix [*, {X}] over the text "
                             "embedding (the edit serves the cross-attention to_k / to_v projections)")
    if len(set(names)) != len(list(names)):
        raise ValueError(f"{KEY}: a target is named twice")
    return list(names)


def require_kernels():
    from . import lib
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: Unified Concept Editing needs the kernels of csrc/uce.hip (there is "
                               "no fall-back)")


# ---------------------------------------------------------------------------------------------------------------- the edit matrix
def _rows(x, name, X=None):
    """An embedding or a stack of them as [n, X] f64 on the host; a non-finite value is refused."""
    import numpy as np
    a = np.asarray(x.detach().cpu().double().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
    if a.ndim < 2 and a.size == 0 and X is not None:
        a = a.reshape(0, X)
    if a.ndim < 2:
        raise ValueError(f"uce.edit_matrix: {name} must be rows [n, X], got shape {a.shape}")
    a = a.reshape(-1, a.shape[-1])
    if X is not None and a.shape[1] != X:
        raise ValueError(f"uce.edit_matrix: {name} has rows of {a.shape[1]}, C_e of {X}")
    if not np.isfinite(a).all():
        raise ValueError(f"uce.edit_matrix: {name} holds {int((~np.isfinite(a)).sum())} non-finite value(s): no edit is taken from it")
    return a


class UCEEdit:
    """E [X, X] f32 (= dT^T, rounded once), M and D [X, X] f64 on the host, the row counts and cond(M) (2-norm, from M's eigenvalues)."""

    def __init__(self, E, M, D, n_edit, n_preserve, lam, edit_scale, preserve_scale, cond, digest=None, source="computed"):
        self.E, self.M, self.D = E, M, D
        self.X = int(E.shape[0])
        self.n_edit, self.n_preserve = int(n_edit), int(n_preserve)
        self.lam, self.edit_scale, self.preserve_scale, self.cond = float(lam), float(edit_scale), float(preserve_scale), float(cond)
        self.digest, self.source = digest, source
        self.report = None
        self.E_dev = None                                   # E on a device, where a run keeps one (the tensor a broadcast fills)

    def config(self):
        c = dict(X=self.X, edit_rows=self.n_edit, preserve_rows=self.n_preserve, cond=self.cond, embeddings=self.digest,
                 source=self.source, **{"lambda": self.lam, "edit_scale": self.edit_scale, "preserve_scale": self.preserve_scale})
        if self.report is not None:
            c.update(self.report)
        return c

    def save(self, directory):
        """uce_edit.safetensors + uce.json under `directory` (safetensors and JSON only)."""
        import torch
        save_tensors(directory, EDIT_FILE, {k: torch.from_numpy(getattr(self, k).copy()) for k in ("E", "M", "D")}, CONFIG_FILE,
                     self.config())

    def save_report(self, directory, report):
        """uce.json again, now with what the run did with the edit (the tensor file is not rewritten)."""
        self.report = dict(report)
        save_config(directory, CONFIG_FILE, self.config())


def embeddings_digest(X, *row_sets):
    """sha256 over X and the f64 bytes of the row sets: the fingerprint a saved edit is filed under."""
    h = hashlib.sha256(str(int(X)).encode())
    for a in row_sets:
        h.update(b"|" + str(tuple(a.shape)).encode() + b"|" + a.tobytes())
    return h.hexdigest()


def edit_matrix(C_e, C_t, C_p=None, lam=0.1, s_e=1.0, s_p=1.0):
    """The UCEEdit of the stacked rows (module docstring).  Refused: a non-finite input, lambda or a scale <= 0, a C_t of another shape
    than C_e's, no edited row."""
    import numpy as np
    lam = check_lambda(lam, "lambda")
    s_e = check_positive(s_e, "edit_scale", "the weight of the edited rows")
    s_p = check_positive(s_p, "preserve_scale", "the weight of the preserved rows")
    Ce = _rows(C_e, "C_e")
    X = Ce.shape[1]
    shape_t = tuple(np.shape(C_t.detach().cpu().numpy() if hasattr(C_t, "detach") else C_t))
    Ct = _rows(C_t, "C_t", X)
    if Ct.shape != Ce.shape:
        raise ValueError(f"uce.edit_matrix: C_t has shape {shape_t}, C_e {Ce.shape}: every edited row needs its destination row")
    if Ce.shape[0] == 0:
        raise ValueError("uce.edit_matrix: no row to edit")
    Cp = np.zeros((0, X)) if C_p is None else _rows(C_p, "C_p", X)
    M = lam * np.eye(X) + s_e * (Ce.T @ Ce) + s_p * (Cp.T @ Cp)
    M = 0.5 * (M + M.T)
    D = s_e * ((Ct - Ce).T @ Ce)
    chol = np.linalg.cholesky(M)                                    # raises LinAlgError when M is not positive definite
    try:
        from scipy.linalg import solve_triangular
        ET = solve_triangular(chol.T, solve_triangular(chol, D.T, lower=True), lower=False)
    except ImportError:
        ET = np.linalg.solve(chol.T, np.linalg.solve(chol, D.T))
    # dT = D M^-1, E = dT^T = M^-1 D^T (M is symmetric)
    w = np.linalg.eigvalsh(M)
    return UCEEdit(np.ascontiguousarray(ET, dtype=np.float32), M, D, Ce.shape[0], Cp.shape[0], lam, s_e, s_p, float(w[-1] / w[0]),
                   digest=embeddings_digest(X, Ce, Ct, Cp))


def present(directory):
    return files_present(directory, EDIT_FILE, CONFIG_FILE)


def save(directory, edit, report=None):
    """The two files of an edit under `directory`; `report`: what the run did with it (config, prompts, stats, residuals)."""
    if report is not None:
        edit.report = dict(report)
    edit.save(directory)


def load(directory, X):
    """The edit saved under `directory`, for a UNet whose cross_attention_dim is X: a foreign X is refused by field."""
    import json
    import numpy as np
    from safetensors.torch import load_file
    path = os.path.join(str(directory), CONFIG_FILE)
    with open(path) as f:
        c = json.load(f)
    if int(c.get("X", -1)) != int(X):
        raise ValueError(f"{path}: X = {c.get('X')!r}, this UNet's cross_attention_dim is {int(X)} -- the edit was computed for another "
                         "text encoder")
    t = load_file(os.path.join(str(directory), EDIT_FILE))
    E, M, D = (t[k].numpy() for k in ("E", "M", "D"))
    if E.shape != (X, X) or E.dtype != np.float32 or M.shape != (X, X) or D.shape != (X, X):
        raise ValueError(f"{os.path.join(str(directory), EDIT_FILE)}: E / M / D are not [{X}, {X}] (E f32)")
    return UCEEdit(np.ascontiguousarray(E), M.astype(np.float64), D.astype(np.float64), c.get("edit_rows", 0), c.get("preserve_rows", 0),
                   c["lambda"], c["edit_scale"], c["preserve_scale"], c["cond"], digest=c.get("embeddings"), source="loaded")


# ---------------------------------------------------------------------------------------------------------------- the launches
def job_table(specs, names):
    """(the rows as the bytes of csrc/uce.hip's UceJob array -- a numpy record array of 64-byte rows --, the rows of delta in all)."""
    import numpy as np
    dt = np.dtype([("w_off", "<i8"), ("row_off", "<i8"), ("rows", "<i4"), ("pad", "<i4"), ("reserved", "<i8", (5,))])
    assert dt.itemsize == JOB_BYTES
    rec = np.zeros(len(names), dtype=dt)
    row = 0
    for i, n in enumerate(names):
        sp = specs[n]
        rec[i]["w_off"], rec[i]["row_off"], rec[i]["rows"] = int(sp.off), row, int(sp.native_shape[0])
        row += int(sp.native_shape[0])
    return rec, row


def _E_device(edit, device):
    import torch
    E = edit.E_dev                                        # (the copy a rank received by broadcast; else the host matrix)
    if E is None:
        E = edit.E if torch.is_tensor(edit.E) else torch.from_numpy(edit.E)
    if E.dtype != torch.float32 or E.dim() != 2 or E.shape[0] != E.shape[1]:
        raise ValueError(f"uce.apply: E must be a square f32 matrix, got {tuple(E.shape)} {E.dtype}")
    return E.to(device).contiguous()


def apply(engine, edit, names, apply=True):
    """The two launches on the engine's flat parameter buffer: siss_uce_delta into a compact buffer of the targets `names`, then
    siss_uce_apply (p += delta over the targets' floats only).  Returns the statistics (STATS, plus relative_change =
    sqrt(sum delta^2 / sum p^2) with p before the edit).  apply: the parameters are written and the bf16 shadow and every derived
    operand copy brought up to date (engine.refresh_weights); else a dry run that writes nothing.  A name that is no `mat` of [*, X]
    is refused."""
    import ctypes
    import torch
    from . import lib
    require_kernels()
    p = engine.ps.flat
    E = _E_device(edit, p.device)
    X = int(E.shape[0])
    names = check_targets(engine.ps.specs, names, X)
    rec, rows = job_table(engine.ps.specs, names)
    jobs = (ctypes.c_char * rec.nbytes).from_buffer_copy(rec.tobytes())
    delta = torch.empty(rows * X, dtype=torch.float32, device=p.device)
    partials = torch.empty(lib.query("siss_uce_partials_words", rows * X, len(names)), dtype=torch.float64, device=p.device)
    stats = torch.empty(len(STATS), dtype=torch.float64, device=p.device)
    lib.call("siss_uce_delta", p, jobs, len(names), E, X, delta)
    lib.call("siss_uce_apply", p, jobs, len(names), X, delta, int(bool(apply)), partials, stats)
    if apply:
        engine.refresh_weights(cast_shadow=True)
    return stats_dict(stats.cpu().tolist())


def stats_dict(s):
    out = {k: float(s[i]) for i, k in enumerate(STATS)}
    out["floats"] = int(out["floats"])
    out["relative_change"] = math.sqrt(out["sum_delta2"] / out["sum_p2"]) if out["sum_p2"] > 0 else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- the residuals
def weights_of(engine_or_weights, names):
    """{name: W [C, X] f64 on the host} of an engine (its f32 master) or of a mapping name -> tensor / array."""
    import torch
    out = {}
    for n in names:
        w = engine_or_weights.ps.p(n) if hasattr(engine_or_weights, "ps") else engine_or_weights[n]
        out[n] = (w.detach().cpu() if torch.is_tensor(w) else torch.as_tensor(w)).double()
    return out


def values_before(engine_or_weights, names, C_t, C_p=None):
    """What `residuals` compares against, taken BEFORE the edit: {name: (W C_t^T, W C_p^T or None)} in f64."""
    import torch
    Ct = torch.from_numpy(_rows(C_t, "C_t"))
    Cp = None if C_p is None else torch.from_numpy(_rows(C_p, "C_p", Ct.shape[1]))
    W = weights_of(engine_or_weights, names)
    return {n: (W[n] @ Ct.T, None if Cp is None or Cp.shape[0] == 0 else W[n] @ Cp.T) for n in names}


def residuals(engine_or_weights, names, before, C_e, C_p=None):
    """After the edit (torch f64, off the hot path): per tensor and overall, the edit residual |W' C_e^T - W C_t^T| / |W C_t^T| and the
    preserve drift |W' C_p^T - W C_p^T| / |W C_p^T| (Frobenius norms; None without preserved rows), `before` = values_before(...) of
    the weights before the edit.  {"edit_residual", "preserve_drift", "per_tensor": {name: {...}}}."""
    import torch
    Ce = torch.from_numpy(_rows(C_e, "C_e"))
    Cp = None if C_p is None else torch.from_numpy(_rows(C_p, "C_p", Ce.shape[1]))
    W = weights_of(engine_or_weights, names)
    per, acc = {}, [0.0, 0.0, 0.0, 0.0]
    for n in names:
        vt, vp = before[n]
        num_e, den_e = float(((W[n] @ Ce.T - vt) ** 2).sum()), float((vt ** 2).sum())
        row = {"edit_residual": math.sqrt(num_e / den_e) if den_e > 0 else None, "preserve_drift": None}
        acc[0] += num_e
        acc[1] += den_e
        if vp is not None:
            num_p, den_p = float(((W[n] @ Cp.T - vp) ** 2).sum()), float((vp ** 2).sum())
            row["preserve_drift"] = math.sqrt(num_p / den_p) if den_p > 0 else None
            acc[2] += num_p
            acc[3] += den_p
        per[n] = row
    return {"edit_residual": math.sqrt(acc[0] / acc[1]) if acc[1] > 0 else None,
            "preserve_drift": math.sqrt(acc[2] / acc[3]) if acc[3] > 0 else None, "per_tensor": per}

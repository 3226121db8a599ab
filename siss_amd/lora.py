"""Opt-in LoRA unlearning on the UNet's linear projections and 3x3 convolutions: `deletion.lora: {rank, alpha, targets, conv_targets,
seed}`, LoRAState and the adapter file.  (Not the reference's protocol, like deletion.trainable: the key is absent from every YAML
and nothing changes without it.)

The base weights stay frozen; every target weight W [O, I] is parametrised as W0 + s B A with A [r, I], B [O, r], s = alpha / r.  The
engine runs forward and backward on the MERGED weight, unchanged, so the dual-cotangent backward leaves dW_k of every target in
ParamStore.grads; the chain rule through the parametrisation is dB_k = s dW_k A^T, dA_k = s B^T dW_k (siss_lora_project), the two-pass
optimizer runs on the LoRA flat buffer and its [2, L] gradient pair, and one merge pass rewrites the targets' stretches of the master
and of its bf16 shadow (siss_lora_merge) -- csrc/lora.hip, driven by ONE device job table built here.

The adapter file: `pytorch_lora_weights.safetensors` with peft-style keys `unet.<module path>.lora_A.weight` [r, I] and
`unet.<module path>.lora_B.weight` [O, r], beside `lora_config.json` (rank, alpha, target names, base checkpoint, step count).

`conv_targets` puts peft's Conv2d adapter on 3x3 convolutions (PSpec kind conv3, stored tap-major as [9, Co, Ci]):
W[t] = W0[t] + s B A[t] with B [Co, r] shared by the nine taps and A [9, r, Ci] -- peft's lora_B.weight [Co, r, 1, 1] and
lora_A.weight [r, Ci, 3, 3], which is how the adapter file holds them.  dB = s sum_t dW[t] A[t]^T, dA[t] = s B^T dW[t]
(siss_lora_project_conv / siss_lora_merge_conv over a job table of their own).  The conv adapters lie in the SAME flat buffers,
behind the linear ones, so the optimizer, the all-reduce and the step see one buffer; a state without conv targets is today's.
"""
import json
import math
import os

from .trainable import parse_patterns, select
from .variants import exclusive, need_fields, need_int

MAX_RANK = 64
TILE = 64                       # rows / columns of a target one block owns (csrc/lora.hip kTile; checked against siss_lora_tile)
LINEAR_KINDS = ("mat", "conv1")  # PSpec.kind of a weight whose native layout is the plain [O, I] matrix
WEIGHTS_FILE, CONFIG_FILE = "pytorch_lora_weights.safetensors", "lora_config.json"
KEY = "deletion.lora"


class LoRAConfig:
    """patterns / conv_patterns: the compiled `targets` / `conv_targets` (None: the list is absent; at least one is given)."""

    def __init__(self, rank, alpha, patterns, seed, conv_patterns=None):
        self.rank, self.alpha, self.patterns, self.seed, self.conv_patterns = rank, alpha, patterns, seed, conv_patterns

    @property
    def scale(self):
        return self.alpha / self.rank


def parse_lora(value, trainable=None):
    """`deletion.lora`: None (absent / null: no adapter) or a LoRAConfig.  Refused, naming the entry: anything but a mapping, a rank
    outside 1..64, a non-positive or non-numeric alpha, targets / conv_targets that are not a non-empty list of regular expressions
    (at least one of the two is needed; rank, alpha and seed are shared by both kinds), an unknown field, and the key together with
    deletion.trainable (`trainable`: that key's value)."""
    if value is None:
        return None
    value = need_fields(KEY, value, ("rank", "alpha", "targets", "conv_targets", "seed"), "{rank:4,targets:[attn]}")
    exclusive("config", {KEY: value, "deletion.trainable": trainable})
    rank = value.get("rank")
    if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
        raise ValueError(f"{KEY}.rank={rank!r}: an integer in 1..{MAX_RANK} is needed")
    alpha = value.get("alpha", rank)
    if alpha is None:
        alpha = rank
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha <= 0:
        raise ValueError(f"{KEY}.alpha={alpha!r}: a positive number is needed (default: the rank)")
    seed = value.get("seed", 0)
    if seed is None:
        seed = 0
    need_int(KEY + ".seed", seed)
    if value.get("targets") is None and value.get("conv_targets") is None:
        raise ValueError(f"{KEY}.targets is missing: a list of regular expressions over the parameter names (e.g. [attn]) -- or "
                         f"{KEY}.conv_targets, the same for the 3x3 convolutions (e.g. ['resnets\\.\\d+\\.conv[12]\\.weight'])")
    patterns = parse_patterns(value.get("targets"), key=KEY + ".targets")
    conv_patterns = parse_patterns(value.get("conv_targets"), key=KEY + ".conv_targets")
    return LoRAConfig(rank, float(alpha), patterns, seed, conv_patterns)


def select_targets(specs, patterns):
    """The target weights `patterns` select among the PSpecs of a UNet, in the order of `specs`: the `.weight`s of plain linear / 1x1
    projections (native shape [O, I]).  Refused by name: an entry that matches nothing (trainable.select), an entry that matches a 3x3
    convolution's or conv_in's weight, and an entry that matches biases / norm parameters ONLY."""
    names = list(specs)
    select(names, patterns, key=KEY + ".targets", announce=False)          # (an entry that matches nothing)
    eligible = lambda n: n.endswith(".weight") and specs[n].kind in LINEAR_KINDS
    what = {"conv3": "a 3x3 convolution", "conv_in": "the input convolution", "vec": "a bias / norm parameter"}
    hint = (": narrow the expression (e.g. attn[12]\\.to_(q|k|v|out\\.0)\\.weight); a 3x3 convolution other than the input "
            f"convolution carries an adapter through {KEY}.conv_targets")
    hit = set()
    for pat in patterns:
        mine = [n for n in names if pat.search(n)]
        # a convolution weight has no [O, I] form: refused wherever it is matched.  The biases and norm parameters an expression written
        # for MODULES (`attn`) matches beside their projections carry no adapter and are passed over; an expression that matches
        # nothing else is refused
        conv = [n for n in mine if specs[n].kind in ("conv3", "conv_in")]
        if conv or not any(eligible(n) for n in mine):
            bad = conv or mine
            raise ValueError(f"{KEY}.targets: entry {pat.pattern!r} selects {len(bad)} tensor(s) that are no weight of a linear or 1x1 "
                             "projection, e.g. " + ", ".join(f"{n} ({what.get(specs[n].kind, specs[n].kind)})" for n in bad[:3]) + hint)
        hit.update(n for n in mine if eligible(n))
    return [n for n in names if n in hit]


def select_conv_targets(specs, patterns):
    """The mirror of select_targets for `conv_targets`: the `.weight`s of kind conv3 (native [9, Co, Ci]: resnet conv1 / conv2, the
    downsamplers' and upsamplers' convolutions, conv_out) `patterns` select, in the order of `specs`; the biases and norm parameters
    an expression also matches are passed over.  Refused by name: an entry that matches nothing, an entry that matches a linear /
    1x1 weight (those belong in `targets`) or conv_in.weight (a padded [Co, 64]-column matrix with three live channels: no adapter),
    and an entry that matches no 3x3 convolution's weight at all."""
    key = KEY + ".conv_targets"
    names = list(specs)
    select(names, patterns, key=key, announce=False)                        # (an entry that matches nothing)
    eligible = lambda n: n.endswith(".weight") and specs[n].kind == "conv3"
    what = {"mat": f"a linear projection: {KEY}.targets", "conv1": f"a 1x1 convolution: {KEY}.targets",
            "conv_in": "the input convolution: it carries no adapter", "vec": "a bias / norm parameter"}
    hit = set()
    for pat in patterns:
        mine = [n for n in names if pat.search(n)]
        other = [n for n in mine if n.endswith(".weight") and specs[n].kind in LINEAR_KINDS + ("conv_in",)]
        if other or not any(eligible(n) for n in mine):
            bad = other or mine
            raise ValueError(f"{key}: entry {pat.pattern!r} selects {len(bad)} tensor(s) that are no weight of a 3x3 convolution, e.g. "
                             + ", ".join(f"{n} ({what.get(specs[n].kind, specs[n].kind)})" for n in bad[:3])
                             + ": narrow the expression (e.g. resnets\\.\\d+\\.conv[12]\\.weight)")
        hit.update(n for n in mine if eligible(n))
    return [n for n in names if n in hit]


def resolve_targets(specs, cfg):
    """(linear target names, conv target names) of a LoRAConfig over the PSpecs of a UNet: either list may be empty, not both."""
    return ([] if cfg.patterns is None else select_targets(specs, cfg.patterns),
            [] if cfg.conv_patterns is None else select_conv_targets(specs, cfg.conv_patterns))


def roundup(n, align):
    return -(-n // align) * align


TAPS = 9                        # a conv3 weight is [9, Co, Ci] natively, t = kh * 3 + kw (ops.conv_w_to_native)


def _layout(shapes, rank, align, taps, base, w0_base):
    """The block of targets [taps, O, I] from `base` of the LoRA flat buffer: every A [taps, r, I], then every B [O, r], each padded
    to `align` floats; W0 packed from `w0_base`; ceil(O / 64) + taps ceil(I / 64) project and taps ceil(O / 64) ceil(I / 64) merge tiles
    a target.  Returns (rows of 9 with the tap count last, end of the block, end of W0, project tiles, merge tiles)."""
    a_off, off = [], base
    for _, O, I in shapes:
        a_off.append(off)
        off += roundup(taps * rank * I, align)
    b_off = []
    for _, O, I in shapes:
        b_off.append(off)
        off += roundup(O * rank, align)
    rows, w0, pt, mt = [], w0_base, 0, 0
    for (w_off, O, I), a, b in zip(shapes, a_off, b_off):
        rows.append((w_off, a, b, w0, O, I, pt, mt, taps))
        w0 += roundup(taps * O * I, align)
        pt += -(-O // TILE) + taps * -(-I // TILE)
        mt += taps * -(-O // TILE) * -(-I // TILE)
    return rows, off, w0, pt, mt


def layout(shapes, rank, align):
    """The LoRA flat buffer and the job rows of targets with native shapes `shapes` = [(weight offset, O, I), ...]: every A [r, I], then
    every B [O, r], each padded to `align` floats; W0 packed in the same order.  Returns (rows, L, W0 floats, project tiles, merge
    tiles), rows = [(w_off, a_off, b_off, w0_off, O, I, first project tile, first merge tile), ...]."""
    rows, *rest = _layout(shapes, rank, align, 1, 0, 0)
    return ([row[:8] for row in rows], *rest)


def job_table(rows):
    """The rows as the bytes of csrc/lora.hip's LoraJob array (a numpy record array)."""
    import numpy as np
    dt = np.dtype([("w_off", "<i8"), ("a_off", "<i8"), ("b_off", "<i8"), ("w0_off", "<i8"), ("O", "<i4"), ("I", "<i4"),
                   ("ptile0", "<i4"), ("mtile0", "<i4")])
    rec = np.zeros(len(rows), dtype=dt)
    for i, row in enumerate(rows):
        rec[i] = row
    assert dt.itemsize == 48
    return rec


def conv_layout(shapes, rank, align, base=0, w0_base=0):
    """layout() for conv targets with native shapes [9, O, I], `shapes` = [(weight offset, O, I), ...]: their block of the LoRA flat
    buffer starts at `base` (behind the linear block): every A [9, r, I], then every B [O, r]; W0 [9, O, I] packed from `w0_base`.
    Returns (rows, end of the block = L, end of W0, project tiles, merge tiles), rows = [(w_off, a_off, b_off, w0_off, O, I, first
    project tile, first merge tile, taps), ...]; a target owns ceil(O / 64) + 9 ceil(I / 64) project tiles and
    9 ceil(O / 64) ceil(I / 64) merge tiles."""
    return _layout(shapes, rank, align, TAPS, base, w0_base)


def conv_job_table(rows):
    """The conv rows as the bytes of csrc/lora.hip's LoraConvJob array: the 48 bytes of job_table's record followed by
    {int taps; int pad[3]} (zero) -- 64 bytes a row."""
    import numpy as np
    dt = np.dtype([("w_off", "<i8"), ("a_off", "<i8"), ("b_off", "<i8"), ("w0_off", "<i8"), ("O", "<i4"), ("I", "<i4"),
                   ("ptile0", "<i4"), ("mtile0", "<i4"), ("taps", "<i4"), ("pad", "<i4", (3,))])
    rec = np.zeros(len(rows), dtype=dt)
    for i, row in enumerate(rows):
        rec[i] = (*row, (0, 0, 0))
    assert dt.itemsize == 64
    return rec


def conv_a_to_ref(a_native):
    """A [9, r, Ci] (native, t = kh * 3 + kw) -> peft's lora_A.weight [r, Ci, 3, 3]"""
    t, r, ci = a_native.shape
    return a_native.reshape(3, 3, r, ci).permute(2, 3, 0, 1).contiguous()


def conv_a_to_native(a_ref):
    """peft's lora_A.weight [r, Ci, 3, 3] -> A [9, r, Ci]: ops.conv_w_to_native of it"""
    r, ci, kh, kw = a_ref.shape
    return a_ref.permute(2, 3, 0, 1).reshape(kh * kw, r, ci).contiguous()


def adapter_keys(name):
    """(key of A, key of B) of target weight `name` in the adapter file."""
    assert name.endswith(".weight")
    mod = name[:-len(".weight")]
    return f"unet.{mod}.lora_A.weight", f"unet.{mod}.lora_B.weight"


def check_state_dict(sd, names, shapes, rank, conv_names=(), conv_shapes=()):
    """Strict: exactly the keys of `names` and `conv_names`, each of the shape its target implies ([r, I] / [O, r]; a conv target's
    [r, Ci, 3, 3] / [Co, r, 1, 1]).  Raises KeyError / ValueError naming the entry."""
    want = {}
    for n, (_, O, I) in zip(names, shapes):
        ka, kb = adapter_keys(n)
        want[ka], want[kb] = (rank, I), (O, rank)
    for n, (_, O, I) in zip(conv_names, conv_shapes):
        ka, kb = adapter_keys(n)
        want[ka], want[kb] = (rank, I, 3, 3), (O, rank, 1, 1)
    missing, extra = [k for k in want if k not in sd], [k for k in sd if k not in want]
    if missing or extra:
        raise KeyError(f"LoRA adapter: missing {missing[:3]} ({len(missing)}), unexpected {extra[:3]} ({len(extra)})")
    for k, shp in want.items():
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"LoRA adapter: {k} has shape {tuple(sd[k].shape)}, the target needs {shp}")


def read_config(directory):
    with open(os.path.join(directory, CONFIG_FILE)) as f:
        c = json.load(f)
    for k in ("rank", "alpha", "targets"):
        if k not in c:
            raise KeyError(f"{os.path.join(directory, CONFIG_FILE)}: no {k!r}")
    return c


def require_kernels(tile=False, conv=False):
    """Raise unless the loaded library has the LoRA entry points (an older build loaded for an A/B may lack them): no fall-back.
    tile: also hold the library's tile against the one the job table is built for (once, when a state is built).  conv: the state
    has conv targets -- their two entry points are needed too."""
    from . import lib
    if not lib.has("siss_lora_project") or not lib.has("siss_lora_merge"):
        raise RuntimeError("this libsiss_hip.so has no siss_lora_project / siss_lora_merge: LoRA needs the kernels of csrc/lora.hip "
                           "(there is no fall-back to the full update)")
    if conv and not (lib.has("siss_lora_project_conv") and lib.has("siss_lora_merge_conv")):
        raise RuntimeError("this libsiss_hip.so has no siss_lora_project_conv / siss_lora_merge_conv: conv_targets need the kernels of "
                           "csrc/lora.hip (there is no fall-back to the full update)")
    if tile and int(lib.query("siss_lora_tile")) != TILE:
        raise RuntimeError(f"siss_lora_tile() = {lib.query('siss_lora_tile')}, siss_amd/lora.py tiles by {TILE}")


class LoRAState:
    """The adapters of the target weights `names` of `engine` (a UNetEngine / UNetCondEngine with its weights loaded): p [L] (every
    A, then every B, each padded to ALIGN with zeros that stay zero), g [2, L], the packed W0 (copied from the master HERE) and the
    device job table (built once: a captured step holds its address).  Init as peft: A ~ U(-1/sqrt(I), 1/sqrt(I)) from a CPU
    generator seeded with `seed` (the same on every rank), B = 0 -- the merged weight is W0 until the first update.

    conv_names: the 3x3 convolution weights (kind conv3) that carry an adapter beside them (`names` may then be empty): conv_rows and
    a job table of their own (conv_jobs), and a block of the SAME p / g behind the linear block -- every A [9, r, I], then every
    B [O, r], padded alike; L is the whole length.  Their W0 is packed behind the linear targets'.  Init as peft's Conv2d adapter:
    A ~ U(-1/sqrt(9 I), 1/sqrt(9 I)), drawn as [r, I, 3, 3] from the same generator AFTER the linear targets' draws, B = 0."""

    def __init__(self, engine, names, rank, alpha=None, seed=0, conv_names=()):
        import torch
        from .unet import ALIGN
        names, conv_names = list(names), list(conv_names)
        if torch.device(engine.device).type == "cuda":          # (a host-side state -- the adapter file alone -- needs no library)
            require_kernels(tile=True, conv=bool(conv_names))
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
            raise ValueError(f"LoRA rank {rank!r}: an integer in 1..{MAX_RANK} is needed")
        ps = engine.ps
        unknown = [n for n in names + conv_names if n not in ps.specs]
        if unknown or not (names or conv_names) or len(set(names + conv_names)) != len(names) + len(conv_names):
            raise KeyError(f"LoRA targets: unknown {unknown[:3]}, or an empty / repeated list")
        bad = [n for n in names if not (n.endswith(".weight") and ps.specs[n].kind in LINEAR_KINDS)]
        if bad:
            raise ValueError(f"LoRA targets must be weights of linear / 1x1 projections: {bad[:3]}")
        bad = [n for n in conv_names if not (n.endswith(".weight") and ps.specs[n].kind == "conv3")]
        if bad:
            raise ValueError(f"LoRA conv targets must be weights of 3x3 convolutions (not conv_in): {bad[:3]}")
        self.engine, self.rank = engine, rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scale = self.alpha / rank
        self.seed = int(seed)
        self.names = tuple(sorted(names, key=lambda n: ps.specs[n].off))
        self.shapes = [(ps.specs[n].off, *ps.specs[n].native_shape) for n in self.names]
        self.rows, lin_L, lin_w0, self.project_tiles, self.merge_tiles = layout(self.shapes, rank, ALIGN)
        self.conv_names = tuple(sorted(conv_names, key=lambda n: ps.specs[n].off))
        self.conv_shapes = [(ps.specs[n].off, *ps.specs[n].native_shape[1:]) for n in self.conv_names]
        self.conv_rows, self.L, w0_floats, self.conv_project_tiles, self.conv_merge_tiles = conv_layout(
            self.conv_shapes, rank, ALIGN, base=lin_L, w0_base=lin_w0)
        dev = engine.device
        self.p = torch.zeros(self.L, dtype=torch.float32, device=dev)
        self.g = torch.zeros(2, self.L, dtype=torch.float32, device=dev)
        self.w0 = torch.zeros(w0_floats, dtype=torch.float32, device=dev)
        self.jobs = torch.from_numpy(job_table(self.rows).view("uint8")).to(dev)
        self.conv_jobs = torch.from_numpy(conv_job_table(self.conv_rows).view("uint8").reshape(-1)).to(dev)
        self.params = sum(rank * (O + I) for _, O, I in self.shapes) + sum(rank * (O + TAPS * I) for _, O, I in self.conv_shapes)
        self.tensors = 2 * (len(self.names) + len(self.conv_names))
        gen = torch.Generator().manual_seed(self.seed)
        for (w_off, a, b, w0, O, I, _, _) in self.rows:
            self.w0[w0:w0 + O * I].copy_(ps.flat[w_off:w_off + O * I])
            bound = 1.0 / math.sqrt(I)
            self.p[a:a + rank * I].copy_(((torch.rand(rank, I, generator=gen) * 2 - 1) * bound).reshape(-1))
        for (w_off, a, b, w0, O, I, _, _, T) in self.conv_rows:
            self.w0[w0:w0 + T * O * I].copy_(ps.flat[w_off:w_off + T * O * I])
            bound = 1.0 / math.sqrt(T * I)                       # kaiming-uniform, a = sqrt 5, over the fan-in 9 I
            a_ref = (torch.rand(rank, I, 3, 3, generator=gen) * 2 - 1) * bound
            self.p[a:a + T * rank * I].copy_(conv_a_to_native(a_ref).reshape(-1))
        self.steps = 0
        self.base = None                    # path of the base checkpoint (lora_config.json)

    # ---- views ---------------------------------------------------------------------------------------------------------------
    def A(self, i, of=None):
        _, a, _, _, O, I, _, _ = self.rows[i]
        return (self.p if of is None else of)[..., a:a + self.rank * I].unflatten(-1, (self.rank, I))

    def B(self, i, of=None):
        _, _, b, _, O, I, _, _ = self.rows[i]
        return (self.p if of is None else of)[..., b:b + O * self.rank].unflatten(-1, (O, self.rank))

    def conv_A(self, i, of=None):
        """A of conv target i, native [9, r, I]"""
        _, a, _, _, O, I, _, _, T = self.conv_rows[i]
        return (self.p if of is None else of)[..., a:a + T * self.rank * I].unflatten(-1, (T, self.rank, I))

    def conv_B(self, i, of=None):
        _, _, b, _, O, I, _, _, T = self.conv_rows[i]
        return (self.p if of is None else of)[..., b:b + O * self.rank].unflatten(-1, (O, self.rank))

    def optimizer_state_bytes(self):
        return 2 * 4 * self.L

    # ---- the two launches ----------------------------------------------------------------------------------------------------
    def project(self, nsets=2):
        """g[k] <- (dA_k, dB_k) of every target from the engine's weight gradients (overwritten; nsets = 1: g[1] <- 0).  No host sync."""
        from . import lib
        require_kernels(conv=bool(self.conv_rows))
        grads = self.engine.ps.grads
        if self.rows:
            lib.call("siss_lora_project", grads, grads.stride(0), int(nsets), self.p, self.g, self.L, self.jobs, len(self.rows),
                     self.rank, self.scale, self.project_tiles)
        if self.conv_rows:
            lib.call("siss_lora_project_conv", grads, grads.stride(0), int(nsets), self.p, self.g, self.L, self.conv_jobs,
                     len(self.conv_rows), self.rank, self.scale, self.conv_project_tiles)

    def merge(self, scale=1.0):
        """master (and bf16 shadow) of every target <- W0 + (s * scale) B A; scale = 0 restores W0 bit for bit.  No host sync."""
        from . import lib
        require_kernels(conv=bool(self.conv_rows))
        ps = self.engine.ps
        shadow = None if ps.shadow is ps.flat else ps.shadow
        if self.rows:
            lib.call("siss_lora_merge", ps.flat, shadow, self.w0, self.p, self.jobs, len(self.rows), self.rank,
                     self.scale * float(scale), self.merge_tiles)
        if self.conv_rows:
            lib.call("siss_lora_merge_conv", ps.flat, shadow, self.w0, self.p, self.conv_jobs, len(self.conv_rows), self.rank,
                     self.scale * float(scale), self.conv_merge_tiles)

    # ---- the adapter file ----------------------------------------------------------------------------------------------------
    def state_dict(self):
        """peft-style keys: [r, I] / [O, r] of a linear target, [r, Ci, 3, 3] / [Co, r, 1, 1] of a conv target."""
        sd = {}
        for i, n in enumerate(self.names):
            ka, kb = adapter_keys(n)
            sd[ka], sd[kb] = self.A(i).detach().cpu().clone(), self.B(i).detach().cpu().clone()
        for i, n in enumerate(self.conv_names):
            ka, kb = adapter_keys(n)
            sd[ka] = conv_a_to_ref(self.conv_A(i).detach().cpu())
            sd[kb] = self.conv_B(i).detach().cpu().clone()[:, :, None, None]
        return sd

    def load_state_dict(self, sd):
        import torch
        check_state_dict(sd, self.names, self.shapes, self.rank, self.conv_names, self.conv_shapes)
        for i, n in enumerate(self.names):
            ka, kb = adapter_keys(n)
            self.A(i).copy_(sd[ka].to(device=self.p.device, dtype=torch.float32))
            self.B(i).copy_(sd[kb].to(device=self.p.device, dtype=torch.float32))
        for i, n in enumerate(self.conv_names):
            ka, kb = adapter_keys(n)
            self.conv_A(i).copy_(conv_a_to_native(sd[ka].to(torch.float32)).to(self.p.device))
            self.conv_B(i).copy_(sd[kb].to(device=self.p.device, dtype=torch.float32)[:, :, 0, 0])

    def config(self):
        c = dict(rank=self.rank, alpha=self.alpha, targets=list(self.names), seed=self.seed, base_checkpoint=self.base,
                 steps=int(self.steps), lora_params=self.params)
        if self.conv_names:                 # (a state without conv targets writes today's file)
            c["conv_targets"] = list(self.conv_names)
        return c

    def log_fields(self):
        """What every log line of a LoRA run carries (lora_conv_tensors only with conv targets)."""
        f = dict(lora_rank=self.rank, lora_alpha=self.alpha, lora_params=self.params, lora_tensors=self.tensors)
        if self.conv_names:
            f["lora_conv_tensors"] = 2 * len(self.conv_names)
        return f

    def save(self, directory):
        """pytorch_lora_weights.safetensors + lora_config.json under `directory` (safetensors and JSON only)."""
        from safetensors.torch import save_file
        os.makedirs(directory, exist_ok=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(directory, WEIGHTS_FILE))
        with open(os.path.join(directory, CONFIG_FILE), "w") as f:
            json.dump(self.config(), f, indent=1)

    @classmethod
    def load(cls, engine, directory):
        """The adapter saved under `directory` over `engine`'s CURRENT weights as W0: names and shapes are checked strictly."""
        from safetensors.torch import load_file
        c = read_config(directory)
        st = cls(engine, c["targets"], int(c["rank"]), float(c["alpha"]), int(c.get("seed") or 0),
                 conv_names=c.get("conv_targets") or ())
        st.load_state_dict(load_file(os.path.join(directory, WEIGHTS_FILE)))
        st.steps, st.base = int(c.get("steps") or 0), c.get("base_checkpoint")
        return st

"""Opt-in LoRA unlearning on the UNet's linear projections: `deletion.lora: {rank, alpha, targets, seed}`, LoRAState and the adapter
file.  (Not the reference's protocol, like deletion.trainable: the key is absent from every YAML and nothing changes without it.)

The base weights stay frozen; every target weight W [O, I] is parametrised as W0 + s B A with A [r, I], B [O, r], s = alpha / r.  The
engine runs forward and backward on the MERGED weight, unchanged, so the dual-cotangent backward leaves dW_k of every target in
ParamStore.grads; the chain rule through the parametrisation is dB_k = s dW_k A^T, dA_k = s B^T dW_k (siss_lora_project), the two-pass
optimizer runs on the LoRA flat buffer and its [2, L] gradient pair, and one merge pass rewrites the targets' stretches of the master
and of its bf16 shadow (siss_lora_merge) -- csrc/lora.hip, driven by ONE device job table built here.

The adapter file: `pytorch_lora_weights.safetensors` with peft-style keys `unet.<module path>.lora_A.weight` [r, I] and
`unet.<module path>.lora_B.weight` [O, r], beside `lora_config.json` (rank, alpha, target names, base checkpoint, step count).
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
    def __init__(self, rank, alpha, patterns, seed):
        self.rank, self.alpha, self.patterns, self.seed = rank, alpha, patterns, seed

    @property
    def scale(self):
        return self.alpha / self.rank


def parse_lora(value, trainable=None):
    """`deletion.lora`: None (absent / null: no adapter) or a LoRAConfig.  Refused, naming the entry: anything but a mapping, a rank
    outside 1..64, a non-positive or non-numeric alpha, targets that are not a non-empty list of regular expressions, an unknown
    field, and the key together with deletion.trainable (`trainable`: that key's value)."""
    if value is None:
        return None
    value = need_fields(KEY, value, ("rank", "alpha", "targets", "seed"), "{rank:4,targets:[attn]}")
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
    if "targets" not in value or value["targets"] is None:
        raise ValueError(f"{KEY}.targets is missing: a list of regular expressions over the parameter names (e.g. [attn])")
    patterns = parse_patterns(value["targets"], key=KEY + ".targets")
    return LoRAConfig(rank, float(alpha), patterns, seed)


def select_targets(specs, patterns):
    """The target weights `patterns` select among the PSpecs of a UNet, in the order of `specs`: the `.weight`s of plain linear / 1x1
    projections (native shape [O, I]).  Refused by name: an entry that matches nothing (trainable.select), an entry that matches a 3x3
    convolution's or conv_in's weight, and an entry that matches biases / norm parameters ONLY."""
    names = list(specs)
    select(names, patterns, key=KEY + ".targets", announce=False)          # (an entry that matches nothing)
    eligible = lambda n: n.endswith(".weight") and specs[n].kind in LINEAR_KINDS
    what = {"conv3": "a 3x3 convolution", "conv_in": "the input convolution", "vec": "a bias / norm parameter"}
    hint = ": narrow the expression (e.g. attn[12]\\.to_(q|k|v|out\\.0)\\.weight)"
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


def roundup(n, align):
    return -(-n // align) * align


def layout(shapes, rank, align):
    """The LoRA flat buffer and the job rows of targets with native shapes `shapes` = [(weight offset, O, I), ...]: every A [r, I], then
    every B [O, r], each padded to `align` floats; W0 packed in the same order.  Returns (rows, L, W0 floats, project tiles, merge
    tiles), rows = [(w_off, a_off, b_off, w0_off, O, I, first project tile, first merge tile), ...]."""
    a_off, off = [], 0
    for _, O, I in shapes:
        a_off.append(off)
        off += roundup(rank * I, align)
    b_off = []
    for _, O, I in shapes:
        b_off.append(off)
        off += roundup(O * rank, align)
    rows, w0, pt, mt = [], 0, 0, 0
    for (w_off, O, I), a, b in zip(shapes, a_off, b_off):
        rows.append((w_off, a, b, w0, O, I, pt, mt))
        w0 += roundup(O * I, align)
        pt += -(-O // TILE) + -(-I // TILE)
        mt += -(-O // TILE) * -(-I // TILE)
    return rows, off, w0, pt, mt


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


def adapter_keys(name):
    """(key of A, key of B) of target weight `name` in the adapter file."""
    assert name.endswith(".weight")
    mod = name[:-len(".weight")]
    return f"unet.{mod}.lora_A.weight", f"unet.{mod}.lora_B.weight"


def check_state_dict(sd, names, shapes, rank):
    """Strict: exactly the keys of `names`, each of the shape its target implies.  Raises KeyError / ValueError naming the entry."""
    want = {}
    for n, (_, O, I) in zip(names, shapes):
        ka, kb = adapter_keys(n)
        want[ka], want[kb] = (rank, I), (O, rank)
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


def require_kernels(tile=False):
    """Raise unless the loaded library has the LoRA entry points (an older build loaded for an A/B may lack them): no fall-back.
    tile: also hold the library's tile against the one the job table is built for (once, when a state is built)."""
    from . import lib
    if not lib.has("siss_lora_project") or not lib.has("siss_lora_merge"):
        raise RuntimeError("this libsiss_hip.so has no siss_lora_project / siss_lora_merge: LoRA needs the kernels of csrc/lora.hip "
                           "(there is no fall-back to the full update)")
    if tile and int(lib.query("siss_lora_tile")) != TILE:
        raise RuntimeError(f"siss_lora_tile() = {lib.query('siss_lora_tile')}, siss_amd/lora.py tiles by {TILE}")


class LoRAState:
    """The adapters of the target weights `names` of `engine` (a UNetEngine / UNetCondEngine with its weights loaded): p [L] (every
    A, then every B, each padded to ALIGN with zeros that stay zero), g [2, L], the packed W0 (copied from the master HERE) and the
    device job table (built once: a captured step holds its address).  Init as peft: A ~ U(-1/sqrt(I), 1/sqrt(I)) from a CPU
    generator seeded with `seed` (the same on every rank), B = 0 -- the merged weight is W0 until the first update."""

    def __init__(self, engine, names, rank, alpha=None, seed=0):
        import torch
        from .unet import ALIGN
        if torch.device(engine.device).type == "cuda":          # (a host-side state -- the adapter file alone -- needs no library)
            require_kernels(tile=True)
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
            raise ValueError(f"LoRA rank {rank!r}: an integer in 1..{MAX_RANK} is needed")
        ps = engine.ps
        names = list(names)
        unknown = [n for n in names if n not in ps.specs]
        if unknown or not names or len(set(names)) != len(names):
            raise KeyError(f"LoRA targets: unknown {unknown[:3]}, or an empty / repeated list")
        bad = [n for n in names if not (n.endswith(".weight") and ps.specs[n].kind in LINEAR_KINDS)]
        if bad:
            raise ValueError(f"LoRA targets must be weights of linear / 1x1 projections: {bad[:3]}")
        self.engine, self.rank = engine, rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scale = self.alpha / rank
        self.seed = int(seed)
        self.names = tuple(sorted(names, key=lambda n: ps.specs[n].off))
        self.shapes = [(ps.specs[n].off, *ps.specs[n].native_shape) for n in self.names]
        self.rows, self.L, w0_floats, self.project_tiles, self.merge_tiles = layout(self.shapes, rank, ALIGN)
        dev = engine.device
        self.p = torch.zeros(self.L, dtype=torch.float32, device=dev)
        self.g = torch.zeros(2, self.L, dtype=torch.float32, device=dev)
        self.w0 = torch.zeros(w0_floats, dtype=torch.float32, device=dev)
        self.jobs = torch.from_numpy(job_table(self.rows).view("uint8")).to(dev)
        self.params = sum(rank * (O + I) for _, O, I in self.shapes)
        self.tensors = 2 * len(self.names)
        gen = torch.Generator().manual_seed(self.seed)
        for (w_off, a, b, w0, O, I, _, _) in self.rows:
            self.w0[w0:w0 + O * I].copy_(ps.flat[w_off:w_off + O * I])
            bound = 1.0 / math.sqrt(I)
            self.p[a:a + rank * I].copy_(((torch.rand(rank, I, generator=gen) * 2 - 1) * bound).reshape(-1))
        self.steps = 0
        self.base = None                    # path of the base checkpoint (lora_config.json)

    # ---- views ---------------------------------------------------------------------------------------------------------------
    def A(self, i, of=None):
        _, a, _, _, O, I, _, _ = self.rows[i]
        return (self.p if of is None else of)[..., a:a + self.rank * I].unflatten(-1, (self.rank, I))

    def B(self, i, of=None):
        _, _, b, _, O, I, _, _ = self.rows[i]
        return (self.p if of is None else of)[..., b:b + O * self.rank].unflatten(-1, (O, self.rank))

    def optimizer_state_bytes(self):
        return 2 * 4 * self.L

    # ---- the two launches ----------------------------------------------------------------------------------------------------
    def project(self, nsets=2):
        """g[k] <- (dA_k, dB_k) of every target from the engine's weight gradients (overwritten; nsets = 1: g[1] <- 0).  No host sync."""
        from . import lib
        require_kernels()
        grads = self.engine.ps.grads
        lib.call("siss_lora_project", grads, grads.stride(0), int(nsets), self.p, self.g, self.L, self.jobs, len(self.rows), self.rank,
                 self.scale, self.project_tiles)

    def merge(self, scale=1.0):
        """master (and bf16 shadow) of every target <- W0 + (s * scale) B A; scale = 0 restores W0 bit for bit.  No host sync."""
        from . import lib
        require_kernels()
        ps = self.engine.ps
        shadow = None if ps.shadow is ps.flat else ps.shadow
        lib.call("siss_lora_merge", ps.flat, shadow, self.w0, self.p, self.jobs, len(self.rows), self.rank,
                 self.scale * float(scale), self.merge_tiles)

    # ---- the adapter file ----------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = {}
        for i, n in enumerate(self.names):
            ka, kb = adapter_keys(n)
            sd[ka], sd[kb] = self.A(i).detach().cpu().clone(), self.B(i).detach().cpu().clone()
        return sd

    def load_state_dict(self, sd):
        import torch
        check_state_dict(sd, self.names, self.shapes, self.rank)
        for i, n in enumerate(self.names):
            ka, kb = adapter_keys(n)
            self.A(i).copy_(sd[ka].to(device=self.p.device, dtype=torch.float32))
            self.B(i).copy_(sd[kb].to(device=self.p.device, dtype=torch.float32))

    def config(self):
        return dict(rank=self.rank, alpha=self.alpha, targets=list(self.names), seed=self.seed, base_checkpoint=self.base,
                    steps=int(self.steps), lora_params=self.params)

    def log_fields(self):
        """What every log line of a LoRA run carries."""
        return dict(lora_rank=self.rank, lora_alpha=self.alpha, lora_params=self.params, lora_tensors=self.tensors)

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
        st = cls(engine, c["targets"], int(c["rank"]), float(c["alpha"]), int(c.get("seed") or 0))
        st.load_state_dict(load_file(os.path.join(directory, WEIGHTS_FILE)))
        st.steps, st.base = int(c.get("steps") or 0), c.get("base_checkpoint")
        return st

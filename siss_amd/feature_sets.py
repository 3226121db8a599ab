"""Set-level figures on the FID features: the Kernel Inception Distance and precision / recall / density / coverage, on the kernels of
csrc/feature_sets.hip.  NOT the reference's protocol, which reports FID only.

`metrics.fid` folds the [N, 2048] f32 features of its Inception-v3 into two sums and drops them.  This module keeps them and does the
pairwise work FID cannot: polynomial-kernel sums over subsets (KID, Binkowski et al. 2018, with torchmetrics' KernelInceptionDistance
surface -- unbiased, so usable at 1,000 to 2,000 samples where FID needs 10,000) and k-th-neighbour balls (precision / recall,
Kynkaanniemi et al. 2019; density / coverage, Naeem et al. 2020 -- "do samples still look real" apart from "did the model lose part of
the distribution").  No N x M matrix is formed and no feature travels to the host.

    sqnorm / knn_radius / ball_stats / kid_sums     the four launchers, on device tensors
    FeatureBank                                     one preallocated [capacity, D] f32 buffer; save / load under a fingerprint
    KernelInceptionDistance                         update_features(f, real), compute() -> (mean, std), reset()
    PRDC                                            compute(real_bank, fake_bank) -> {precision, recall, density, coverage}
    FeatureSets                                     the sink `metrics.fid.sets` hangs behind FIDEvaluator / FIDTracker

There is no fall-back: a library without the entry points raises.  A distance is one f32 value that depends on its two rows alone
(the launchers' contract), so the two directions of a pair agree bit for bit.
"""
import hashlib
import json
import os
import time

import torch

from . import lib
from .records import finite_or_none

ENTRY_POINTS = ("siss_feat_sqnorm", "siss_feat_knn_ws_bytes", "siss_feat_knn_radius", "siss_feat_ball_ws_bytes", "siss_feat_ball_stats",
                "siss_kid_ws_bytes", "siss_kid_sums")
FORMAT = 1
MAX_K = 16
MAX_D = 4096
MAX_SUBSETS = 21845         # 3 sums per subset on a grid axis of 65,535


def require_kernels():
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: the feature-set figures need the kernels of csrc/feature_sets.hip "
                               "(there is no fall-back to a matrix product)")


def _ws_bytes(name, *args):
    n = int(lib.query(name, *(int(a) for a in args)))
    if n < 0:
        raise ValueError(f"{name}{tuple(int(a) for a in args)} refused its arguments")
    return n


def _launch(name, *args):
    """lib.call for device tensors only: a host pointer must never reach a kernel."""
    for a in args:
        if torch.is_tensor(a) and not a.is_cuda:
            raise RuntimeError(f"{name}: a tensor on {a.device}; the feature-set kernels run on the device only")
    return lib.call(name, *args)


def _rows(x, what, d=None):
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1:
        raise ValueError(f"{what}: f32 rows [n >= 1, d] are needed, got {getattr(x, 'dtype', None)} {tuple(getattr(x, 'shape', ()))}")
    if d is not None and x.shape[1] != d:
        raise ValueError(f"{what}: rows of {d} are needed, got {tuple(x.shape)}")
    if not 4 <= x.shape[1] <= MAX_D or x.shape[1] % 4:
        raise ValueError(f"{what}: d = {x.shape[1]}; the kernels take 4 <= d <= {MAX_D}, d % 4 == 0")
    return x.contiguous()


def _check_k(k, what="k"):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}={k!r}: an integer in 1 .. {MAX_K} is needed")
    return k


def _work(nbytes, device):
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.int64)


def sqnorm(x):
    """sq [n] f32: per row the sum of squares, taken in f64 over ascending k and rounded once."""
    require_kernels()
    x = _rows(x, "sqnorm")
    sq = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    _launch("siss_feat_sqnorm", x, x.shape[0], x.shape[1], sq)
    return sq


def knn_radius(x, sq, k):
    """radius [n] f32: per row the k-th smallest squared distance to ANOTHER row (the self pair is left out by index), +inf when the
    set has fewer than k + 1 rows."""
    require_kernels()
    x, k = _rows(x, "knn_radius"), _check_k(k)
    n, d = x.shape
    radius = torch.empty(n, device=x.device, dtype=torch.float32)
    ws = _work(_ws_bytes("siss_feat_knn_ws_bytes", n, k), x.device)
    _launch("siss_feat_knn_radius", x, n, d, sq, k, radius, ws, ws.numel() * 8)
    return radius


def ball_stats(q, sq_q, g, sq_g, radius_g=None, self0=-1):
    """(inside [nq] int32 or None, min_d2 [nq] f32, argmin [nq] int32): per query row the number of gallery rows j whose ball holds
    it (d2 <= radius_g[j]; None without radii), the smallest squared distance and the lowest row attaining it."""
    require_kernels()
    g = _rows(g, "ball_stats gallery")
    q = _rows(q, "ball_stats queries", g.shape[1])
    nq, ng, dev = q.shape[0], g.shape[0], g.device
    inside = torch.empty(nq, device=dev, dtype=torch.int32) if radius_g is not None else None
    min_d2 = torch.empty(nq, device=dev, dtype=torch.float32)
    argmin = torch.empty(nq, device=dev, dtype=torch.int32)
    ws = _work(_ws_bytes("siss_feat_ball_ws_bytes", nq, ng), dev)
    _launch("siss_feat_ball_stats", q, nq, sq_q, g, ng, sq_g, radius_g, g.shape[1], int(self0), inside, min_d2, argmin, ws, ws.numel() * 8)
    return inside, min_d2, argmin


def kid_sums(x, idx_x, y, idx_y, gamma, coef):
    """out [S, 3] f64 on the device: per subset b the kernel sums (xx without the diagonal, yy without the diagonal, xy) of the
    cubic polynomial kernel over the rows idx_x[b] of x and idx_y[b] of y.  idx_x / idx_y: [S, s] integer HOST tables (checked against
    the row counts here, then copied once, together)."""
    require_kernels()
    x = _rows(x, "kid_sums x")
    y = _rows(y, "kid_sums y", x.shape[1])
    ix, iy = torch.as_tensor(idx_x), torch.as_tensor(idx_y)
    if ix.dim() != 2 or ix.shape != iy.shape or ix.shape[0] < 1 or ix.shape[1] < 1 or ix.is_floating_point() or iy.is_floating_point():
        raise ValueError(f"kid_sums: two integer row tables [S, s] of one shape are needed, got {tuple(ix.shape)} and {tuple(iy.shape)}")
    S, s = ix.shape
    if S > MAX_SUBSETS:
        raise ValueError(f"kid_sums: {S} subsets; one launch takes at most {MAX_SUBSETS}")
    for t, n, what in ((ix, x.shape[0], "idx_x"), (iy, y.shape[0], "idx_y")):
        if int(t.min()) < 0 or int(t.max()) >= n:
            raise ValueError(f"kid_sums: {what} names rows outside 0 .. {n - 1}")
    tables = torch.stack([ix.cpu().to(torch.int32), iy.cpu().to(torch.int32)]).to(x.device)       # the tables go up as one copy
    out = torch.empty(S, 3, device=x.device, dtype=torch.float64)
    ws = _work(_ws_bytes("siss_kid_ws_bytes", S, s), x.device)
    _launch("siss_kid_sums", x, x.shape[0], tables[0], y, y.shape[0], tables[1], x.shape[1], S, s, float(gamma), float(coef), out, ws,
            ws.numel() * 8)
    return out


# ---------------------------------------------------------------- fingerprints
def weights_fingerprint(model):
    """sha256 over a metric network's parameters (name, shape and bytes in state-dict order): the Inception checkpoint's hash."""
    h = hashlib.sha256()
    h.update(b"siss_amd.feature_sets/%d\0" % FORMAT)
    for k, v in model.state_dict().items():
        h.update(k.encode() + b"\0" + repr(tuple(v.shape)).encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def real_fingerprint(model, paths):
    """What a bank of real features depends on: the network's weights and the image files with their sizes and mtimes."""
    from .sscd_search import files_fingerprint
    return {"model": weights_fingerprint(model), "files": files_fingerprint(paths), "n": len(paths)}


# ---------------------------------------------------------------- the bank
class FeatureBank:
    """One preallocated [capacity, D] f32 buffer on `device` with a fill count.  `cache` holds what PRDC derives from the rows (their
    squared norms and radii); it is dropped whenever the rows change."""

    def __init__(self, num_features, capacity, device):
        num_features, capacity = int(num_features), int(capacity)
        if not 4 <= num_features <= MAX_D or num_features % 4:
            raise ValueError(f"FeatureBank: num_features = {num_features}; the kernels take 4 <= d <= {MAX_D}, d % 4 == 0")
        if capacity < 1:
            raise ValueError(f"FeatureBank: capacity = {capacity}: at least one row is needed")
        self.num_features, self.capacity, self.device = num_features, capacity, torch.device(device)
        self.buf = torch.empty(capacity, num_features, device=self.device, dtype=torch.float32)
        self.n, self.cache = 0, {}

    def __len__(self):
        return self.n

    @property
    def rows(self):
        return self.buf[:self.n]

    def append(self, f):
        if f.dim() != 2 or f.shape[1] != self.num_features:
            raise ValueError(f"FeatureBank.append: [N, {self.num_features}] features are needed, got {tuple(f.shape)}")
        m = int(f.shape[0])
        if self.n + m > self.capacity:
            raise ValueError(f"FeatureBank.append: {self.n} + {m} rows do not fit the capacity of {self.capacity}")
        self.buf[self.n:self.n + m].copy_(f)
        self.n += m
        self.cache.clear()

    def clear(self):
        self.n = 0
        self.cache.clear()

    def save(self, path, fingerprint):
        """`path` (safetensors: the rows) and `path + '.json'` (the fingerprint)."""
        from safetensors.torch import save_file
        path = str(path)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = f"{path}.tmp{os.getpid()}"
        save_file({"features": self.rows.detach().cpu().contiguous()}, tmp)
        os.replace(tmp, path)
        with open(path + ".json", "w") as f:
            json.dump({"format": FORMAT, "n": self.n, "num_features": self.num_features, "fingerprint": fingerprint}, f)
        return path

    @staticmethod
    def exists(path):
        return os.path.isfile(str(path)) and os.path.isfile(str(path) + ".json")

    @staticmethod
    def matches(path, fingerprint):
        """Whether the file under `path` was written under `fingerprint`."""
        try:
            with open(str(path) + ".json") as f:
                meta = json.load(f)
        except (OSError, ValueError):
            return False
        return meta.get("format") == FORMAT and meta.get("fingerprint") == fingerprint

    @classmethod
    def load(cls, path, fingerprint, device="cpu", capacity=None):
        """The bank save() wrote; ValueError when it was written under another fingerprint (other weights, other files)."""
        from safetensors.torch import load_file
        path = str(path)
        with open(path + ".json") as f:
            meta = json.load(f)
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a feature bank of format {FORMAT}")
        if meta.get("fingerprint") != fingerprint:
            raise ValueError(f"{path}: the features were written under another fingerprint (other Inception weights or other image "
                             "files, sizes or mtimes): remove the file or name another path")
        f = load_file(path)["features"]
        if f.dtype != torch.float32 or tuple(f.shape) != (meta["n"], meta["num_features"]):
            raise ValueError(f"{path}: the header describes {meta['n']} rows of {meta['num_features']}, the file holds {tuple(f.shape)}")
        bank = cls(f.shape[1], max(int(capacity or 0), f.shape[0], 1), device)
        bank.append(f.to(device))
        return bank


# ---------------------------------------------------------------- KID
def subset_tables(n_real, n_fake, subsets, subset_size, seed):
    """(idx_real, idx_fake) [subsets, subset_size] int64 host tables, drawn as torchmetrics draws them -- per subset
    torch.randperm(n_real)[:subset_size], then torch.randperm(n_fake)[:subset_size] -- from a host generator seeded with `seed`."""
    g = torch.Generator().manual_seed(int(seed))
    real, fake = [], []
    for _ in range(subsets):
        real.append(torch.randperm(n_real, generator=g)[:subset_size])
        fake.append(torch.randperm(n_fake, generator=g)[:subset_size])
    return torch.stack(real), torch.stack(fake)


def kid_from_sums(sums, m):
    """(mean, std) f64 tensors of the per-subset values (kxx + kyy) / (m (m - 1)) - 2 kxy / m^2 over sums [S, 3]; std is the
    population standard deviation (unbiased=False), as torchmetrics computes it."""
    sums = sums.to(torch.float64)
    vals = (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)
    return vals.mean(), vals.std(unbiased=False)


class KernelInceptionDistance:
    """torchmetrics.image.kid.KernelInceptionDistance on given features, cubic polynomial kernel: `update_features(f, real)`,
    `compute() -> (mean, std)`, `reset()` (the fake side only).  The subset tables are drawn again from `seed` at every compute():
    two evaluations with equal counts use the same tables, and their difference is the model's.  `banks`: (real, fake) FeatureBanks to
    read instead of keeping the features here."""

    def __init__(self, subsets=100, subset_size=1000, degree=3, gamma=None, coef=1.0, seed=0, banks=None):
        if not isinstance(subsets, int) or isinstance(subsets, bool) or not 1 <= subsets <= MAX_SUBSETS:
            raise ValueError(f"Argument `subsets`={subsets!r}: an integer in 1 .. {MAX_SUBSETS} is needed")
        if not isinstance(subset_size, int) or isinstance(subset_size, bool) or subset_size < 2:
            raise ValueError(f"Argument `subset_size`={subset_size!r}: an integer of at least 2 is needed")
        if degree != 3:
            raise ValueError(f"Argument `degree`={degree!r}: only the cubic kernel (degree 3) is built")
        if gamma is not None and not (isinstance(gamma, float) and gamma > 0):
            raise ValueError(f"Argument `gamma`={gamma!r}: None (1 / D) or a positive float is needed")
        if not isinstance(coef, float) or coef <= 0:
            raise ValueError(f"Argument `coef`={coef!r}: a positive float is needed")
        if not isinstance(seed, int) or isinstance(seed, bool):
            raise ValueError(f"Argument `seed`={seed!r}: an integer is needed")
        self.subsets, self.subset_size, self.degree, self.gamma, self.coef, self.seed = subsets, subset_size, 3, gamma, coef, seed
        self.banks = banks
        self._real, self._fake = [], []

    def update_features(self, f, real):
        if self.banks is not None:
            self.banks[0 if real else 1].append(f)
        elif f.shape[0]:
            (self._real if real else self._fake).append(f.to(torch.float32))

    def _sides(self):
        if self.banks is not None:
            return self.banks[0].rows, self.banks[1].rows
        for side in (self._real, self._fake):
            if len(side) > 1:
                side[:] = [torch.cat(side)]
        return (self._real[0] if self._real else None), (self._fake[0] if self._fake else None)

    def compute(self):
        real, fake = self._sides()
        n_real, n_fake = (0 if real is None else real.shape[0]), (0 if fake is None else fake.shape[0])
        if n_real < self.subset_size or n_fake < self.subset_size:
            raise ValueError("Argument `subset_size` should be smaller than the number of samples")
        ir, if_ = subset_tables(n_real, n_fake, self.subsets, self.subset_size, self.seed)
        gamma = 1.0 / real.shape[1] if self.gamma is None else self.gamma
        return kid_from_sums(kid_sums(real, ir, fake, if_, gamma, self.coef), self.subset_size)

    def reset(self):
        if self.banks is not None:
            self.banks[1].clear()
        self._fake = []


# ---------------------------------------------------------------- PRDC
class PRDC:
    """Precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of a fake bank against a real bank,
    with SQUARED distances, r_R / r_F the k-th-neighbour radii of the N real / M fake rows:

        precision = mean_j [exists i: d2(F_j, R_i) <= r_R[i]]          recall   = mean_i [exists j: d2(R_i, F_j) <= r_F[j]]
        density   = (1 / (k M)) sum_j #{i: d2(F_j, R_i) <= r_R[i]}     coverage = mean_i [min_j d2(R_i, F_j) <= r_R[i]]

    Comparisons use `<=`, Kynkaanniemi's statement; the `prdc` package's code uses `<`.  The two differ on exact ties only.  Two
    radius launches and two ball_stats launches; the real side's squared norms and radii are cached on its bank, so they are computed
    once per run, not per evaluation."""

    def __init__(self, k=5):
        self.k = _check_k(k, "PRDC: k")

    def _side(self, bank):
        key = ("prdc", self.k)
        if key not in bank.cache:
            sq = bank.cache.get("sq")
            if sq is None:
                sq = bank.cache["sq"] = sqnorm(bank.rows)
            bank.cache[key] = knn_radius(bank.rows, sq, self.k)
        return bank.cache["sq"], bank.cache[key]

    def compute(self, real_bank, fake_bank):
        N, M = len(real_bank), len(fake_bank)
        if N < self.k + 1 or M < self.k + 1:
            raise ValueError(f"PRDC: k = {self.k} needs at least {self.k + 1} rows on each side, got {N} real and {M} fake")
        sq_r, r_r = self._side(real_bank)
        sq_f, r_f = self._side(fake_bank)
        in_f, _, _ = ball_stats(fake_bank.rows, sq_f, real_bank.rows, sq_r, r_r)
        in_r, min_r, _ = ball_stats(real_bank.rows, sq_r, fake_bank.rows, sq_f, r_f)
        out = torch.stack([(in_f > 0).double().mean(), (in_r > 0).double().mean(), in_f.double().sum() / (self.k * M),
                           (min_r <= r_r).double().mean()]).cpu().tolist()
        return dict(zip(("precision", "recall", "density", "coverage"), out))


# ---------------------------------------------------------------- the `metrics.fid.sets` key
KEYS = ("kid", "prdc", "real_features_path", "max_bytes")
KID_KEYS = ("subsets", "subset_size", "seed", "gamma", "coef")
PRDC_KEYS = ("k",)
DEFAULT_MAX_BYTES = 2_000_000_000
RECORD_FIELDS = ("kid_mean", "kid_std", "kid_subsets", "kid_subset_size", "precision", "recall", "density", "coverage", "prdc_k",
                 "sets_seconds")


def _mapping(node, what, keys):
    if not isinstance(node, dict):
        raise ValueError(f"{what}={node!r}: a mapping {{{', '.join(keys)}}} is needed")
    unknown = sorted(set(node) - set(keys))
    if unknown:
        raise ValueError(f"{what}: unknown field(s) {unknown}; the fields are {list(keys)}")
    return node


def parse_config(node, num_images, num_features=2048):
    """`metrics.fid.sets: {kid: {subsets, subset_size, seed, gamma, coef}, prdc: {k}, real_features_path, max_bytes}` (null / absent:
    None) -> plain settings.  A host-side check, before the first step: ValueError for a node that is no mapping or has an unknown
    field, for k outside 1 .. 16 or k >= num_images, subset_size > num_images, and for a fake bank that alone does not fit max_bytes
    (the real side is checked when it is loaded)."""
    if node is None:
        return None
    what = "metrics.fid.sets"
    node = dict(_mapping(node, what, KEYS))
    out = {"kid": None, "prdc": None, "real_features_path": node.get("real_features_path") or None}
    mb = node.get("max_bytes", DEFAULT_MAX_BYTES)
    if not isinstance(mb, int) or isinstance(mb, bool) or mb < 1:
        raise ValueError(f"{what}.max_bytes={mb!r}: a positive byte count is needed")
    out["max_bytes"] = mb
    if node.get("kid") is not None:
        kid = dict(_mapping(node["kid"], what + ".kid", KID_KEYS))
        try:
            KernelInceptionDistance(**kid)
        except ValueError as e:
            raise ValueError(f"{what}.kid: {e}") from None
        kid.setdefault("subsets", 100), kid.setdefault("subset_size", 1000), kid.setdefault("seed", 0)
        if kid["subset_size"] > num_images:
            raise ValueError(f"{what}.kid.subset_size={kid['subset_size']} is larger than metrics.fid.num_imgs_to_generate={num_images}")
        out["kid"] = kid
    if node.get("prdc") is not None:
        prdc = dict(_mapping(node["prdc"], what + ".prdc", PRDC_KEYS))
        k = _check_k(prdc.get("k", 5), what + ".prdc.k")
        if k >= num_images:
            raise ValueError(f"{what}.prdc.k={k}: metrics.fid.num_imgs_to_generate={num_images} images have no {k}-th other neighbour")
        out["prdc"] = {"k": k}
    if num_images * num_features * 4 > mb:
        raise ValueError(f"{what}: the bank of {num_images} generated rows ({num_images * num_features * 4} bytes) does not fit "
                         f"max_bytes={mb}")
    return out


class FeatureSets:
    """What `metrics.fid.sets` hangs behind the FID: a sink for the features FrechetInceptionDistance.update_features already holds
    (`sets(f, real)`), the two banks, and `evaluate()`, the fields FIDTracker adds to its record.  The fake bank is allocated here; the
    real bank by `open_real(n)` or `adopt_real(bank)` once the real side's size is known."""

    def __init__(self, settings, num_images, device, num_features=2048):
        require_kernels()
        self.settings, self.device, self.num_features, self.num_images = settings, torch.device(device), int(num_features), int(num_images)
        self.fake = FeatureBank(num_features, num_images, device)
        self.real = None
        self.kid_cfg, self.prdc = settings["kid"], (PRDC(settings["prdc"]["k"]) if settings["prdc"] else None)
        self.real_features_path = settings["real_features_path"]

    def _fits(self, n_real):
        need = (int(n_real) + self.num_images) * self.num_features * 4
        if need > self.settings["max_bytes"]:
            raise ValueError(f"metrics.fid.sets: the banks of {n_real} real and {self.num_images} generated rows ({need} bytes) do not fit "
                             f"max_bytes={self.settings['max_bytes']}")
        if self.kid_cfg and self.kid_cfg["subset_size"] > n_real:
            raise ValueError(f"metrics.fid.sets.kid.subset_size={self.kid_cfg['subset_size']} is larger than the real set of {n_real} images")
        if self.prdc and self.prdc.k >= n_real:
            raise ValueError(f"metrics.fid.sets.prdc.k={self.prdc.k}: the real set of {n_real} images has no {self.prdc.k}-th other neighbour")

    def open_real(self, n_real):
        self._fits(n_real)
        self.real = FeatureBank(self.num_features, max(int(n_real), 1), self.device)

    def adopt_real(self, bank):
        self._fits(len(bank))
        self.real = bank

    def __call__(self, f, real):
        bank = self.real if real else self.fake
        if bank is not None:
            bank.append(f)

    def begin(self):
        """Before an evaluation's first fake batch."""
        self.fake.clear()

    def evaluate(self):
        """The record fields of one evaluation.  A fake side that filter_fake left too small for a figure gives null fields and
        `sets_skipped` with the reason instead of an exception."""
        t0 = time.perf_counter()
        out, skipped = {}, []
        M = len(self.fake)
        if self.kid_cfg:
            c = self.kid_cfg
            mean = std = None
            if M < c["subset_size"]:
                skipped.append(f"kid: {M} generated rows are fewer than subset_size={c['subset_size']}")
            else:
                kid = KernelInceptionDistance(**c, banks=(self.real, self.fake))
                mean, std = (finite_or_none(float(v)) for v in kid.compute())
            out.update(kid_mean=mean, kid_std=std, kid_subsets=c["subsets"], kid_subset_size=c["subset_size"])
        if self.prdc:
            vals = dict.fromkeys(("precision", "recall", "density", "coverage"))
            if M < self.prdc.k + 1:
                skipped.append(f"prdc: {M} generated rows are fewer than k + 1 = {self.prdc.k + 1}")
            else:
                vals = {k: finite_or_none(v) for k, v in self.prdc.compute(self.real, self.fake).items()}
            out.update(**vals, prdc_k=self.prdc.k)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out["sets_seconds"] = time.perf_counter() - t0
        if skipped:
            out["sets_skipped"] = "; ".join(skipped)
        return out

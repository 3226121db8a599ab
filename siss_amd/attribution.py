"""Gradient-feature data attribution: WHICH training images stand behind a sample (TRAK, Park et al., ICML 2023; D-TRAK, Zheng et al.,
ICLR 2024) -- the step in front of an unlearning run, on csrc/attribution.hip.

    phi(x)    = R^T grad_theta L(x) / sqrt(k)         R: n x k Rademacher signs from a counter hash, never in memory
    tau(q, i) = phi(q)^T (Phi^T Phi / N + lambda I)^-1 phi_i

    Projector          the projection of a flat gradient buffer (or of a trainable.Subset of it) to k dimensions; owns the workspace
    GradientFeatures   one row per image: S noisings of the image at fixed timesteps, one backward into gradient set 0, one projection
    FeatureStore       [N, k] f32 rows on the device with their names; save / load under a fingerprint
    Attributor         the preconditioner (f64, Cholesky on the host, once per store), scores, top-k (siss_amd/sscd_search.py) and
                       self-influence

NOT the reference's protocol (its runs are handed the images to forget); ONE model, no ensemble over checkpoints; dense Rademacher
signs only; D-TRAK's form without TRAK's per-sample output weights.  There is no fall-back: a library without the entry points raises.
Host code only until a tensor is touched.
"""
import hashlib
import json
import math
import os

from . import lib, variants

ENTRY_POINTS = ("siss_jl_project", "siss_jl_ws_bytes", "siss_jl_chunk")
FORMAT = 1
K_MIN, K_MAX, K_STEP = 32, 8192, 32
MAX_TOTAL = 1 << 40
OUTPUTS = ("loss", "square")
HASH = "rademacher/lowbias32-v1"          # R[i, j] of csrc/attribution.hip (restated in tests/attribution_ref.py)
ROWS_FILE, META_FILE = "features.safetensors", "features.json"


def require_kernels():
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: the attribution features need the kernels of csrc/attribution.hip "
                               "(there is no fall-back to a matrix product)")


def check_k(k):
    if not variants.is_int(k) or not K_MIN <= k <= K_MAX or k % K_STEP:
        raise ValueError(f"k = {k!r}: a multiple of {K_STEP} in {K_MIN} .. {K_MAX} is needed")
    return k


def timestep_table(timesteps, T):
    """t_s = floor((s + 1/2) T / S) for s < S: the S = `timesteps` midpoints of an even split of [0, T)."""
    S, T = variants.need_int("timesteps", timesteps, positive=True), variants.need_int("T", T, positive=True)
    if S > T:
        raise ValueError(f"timesteps = {S}: at most the schedule's {T} steps")
    return [((2 * s + 1) * T) // (2 * S) for s in range(S)]


def row_seed(seed, index):
    """The seed of the device generator of one row: a function of (seed, index) alone, so that a row does not depend on the order or
    the company it is computed in.  sha256 of the pair, 63 bits."""
    if not variants.is_int(seed) or not variants.is_int(index) or seed < 0 or index < 0:
        raise ValueError(f"row_seed({seed!r}, {index!r}): two integers >= 0 are needed")
    return int.from_bytes(hashlib.sha256(f"siss_amd.attribution/{seed}/{index}".encode()).digest()[:8], "little") >> 1


def damping_term(damping, mean_diag):
    """lambda = damping * mean(diag(Phi^T Phi / N)); damping <= 0 or not finite is refused."""
    d = float(damping) if isinstance(damping, (int, float)) and not isinstance(damping, bool) else float("nan")
    if not (math.isfinite(d) and d > 0):
        raise ValueError(f"damping = {damping!r}: a finite number > 0 is needed (the preconditioner must be positive definite)")
    return d * float(mean_diag)


class Projector:
    """out = R^T g / sqrt(k) over a flat f32 buffer of `total` floats, or over the stretches of `subset` (a trainable.Subset of the same
    buffer; the hash index stays the flat offset, so the result is the full projection of the gradient zeroed elsewhere)."""

    def __init__(self, total, k, seed=0, subset=None, device="cuda:0"):
        self.k = check_k(k)
        if not variants.is_int(total) or not 0 < total <= MAX_TOTAL:
            raise ValueError(f"total = {total!r}: 1 .. 2^40 floats")
        if not variants.is_int(seed) or not 0 <= seed < 1 << 32:
            raise ValueError(f"seed = {seed!r}: an integer in 0 .. 2^32 - 1 is needed")
        if subset is not None and int(subset.total) != total:
            raise ValueError(f"subset: stretches of a buffer of {subset.total} floats, the projector's has {total}")
        self.total, self.seed, self.subset, self.device = total, seed, subset, device
        self._ws = None

    def fingerprint(self):
        """What identifies the projection: the hash, k, the seed, the buffer length and the stretches it runs over."""
        st = None if self.subset is None else hashlib.sha256(repr(tuple(self.subset.stretches)).encode()).hexdigest()
        return dict(hash=HASH, k=self.k, seed=self.seed, total=self.total, stretches=st)

    def project(self, g, out_row):
        """out_row[0:k] = the projection of g ([total] f32 on the device); nothing else is written."""
        import torch
        pair = (("g", g, self.total), ("out_row", out_row, self.k))
        for what, t, n in pair:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
                raise ValueError(f"project: {what} must be a contiguous f32 vector of {n}, got {getattr(t, 'dtype', None)} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        for what, t, n in pair:
            if t.data_ptr() % 16:
                raise ValueError(f"project: {what} is not 16-byte aligned (the projection reads and writes whole granules)")
        for what, t, n in pair:
            if not t.is_cuda:
                raise RuntimeError(f"project: {what} is on {t.device}; the projection runs on the device only")
        require_kernels()
        if self._ws is None:
            need = int(lib.query("siss_jl_ws_bytes", self.total, self.k))
            assert need > 0
            self._ws = torch.empty(need // 8, dtype=torch.float64, device=g.device)
            self._table = (None, 0) if self.subset is None else self.subset.table(g.device)[:2]
        tab, n_ranges = self._table
        lib.call("siss_jl_project", g, self.total, tab, n_ranges, self.k, self.seed, self._ws, self._ws.numel() * 8, out_row)
        return out_row


class GradientFeatures:
    """phi(x) of one image at the stepper's current weights.  `output`: "loss" -- TRAK's eps-MSE; "square" -- D-TRAK's ||eps_theta||^2
    (a zero target).  The S = `timesteps` noisings of ONE image run as one batch, or as accumulated micro-batches of `batch_size`
    (backward_batch's first / accumulate rule); timesteps timestep_table(S, T); the noise (and whatever `prepare` draws) from a device
    generator seeded by row_seed(seed, index).  `conditioning`: None, the dict splatted into the forward (rows of the micro-batch
    size), or a callable B -> dict."""

    def __init__(self, stepper, projector, timesteps=10, output="loss", batch_size=None, seed=0, prepare=None, conditioning=None,
                 sample_noise=None):
        if output not in OUTPUTS:
            raise ValueError(f"output = {output!r}: one of {OUTPUTS}")
        T = int(stepper.ac.numel())
        self.t = timestep_table(timesteps, T)
        self.S = len(self.t)
        self.batch_size = self.S if batch_size is None else variants.need_int("batch_size", batch_size, positive=True)
        if projector.total != int(stepper.e.ps.total):
            raise ValueError(f"projector: a buffer of {projector.total} floats, this UNet's has {stepper.e.ps.total}")
        row_seed(seed, 0)
        self.stepper, self.projector, self.output, self.seed = stepper, projector, output, seed
        self.prepare, self.conditioning, self.sample_noise = prepare, conditioning, sample_noise

    def weights_digest(self):
        """sha256 over the f32 master weights of the flat buffer."""
        return hashlib.sha256(self.stepper.e.ps.flat.detach().cpu().numpy().tobytes()).hexdigest()

    def fingerprint(self, names=None):
        """What a store of these rows was computed from: the weights, the buffer's layout, the projection, the noisings, the names."""
        fp = dict(format=FORMAT, weights=self.weights_digest(), layout=variants.fingerprint(self.stepper.e), projector=self.projector.fingerprint(),
                  timesteps=self.S, output=self.output, seed=self.seed)
        if names is not None:
            fp["names"] = hashlib.sha256("\0".join(str(n) for n in names).encode()).hexdigest()
        return fp

    def _cond(self, B):
        c = self.conditioning
        return dict((c(B) if callable(c) else c) or {})

    def _fill(self, image, index):
        """The gradient of the row's output into gradient set 0 (inside quiet_backward)."""
        import torch
        from .loss import mixture_fwd, mse_bwd_seed
        st = self.stepper
        e, dev, S = st.e, st.e.device, self.S
        gen = torch.Generator(device=dev).manual_seed(row_seed(self.seed, int(index)))
        a0 = image.to(dev)
        a0 = a0[None] if (torch.is_tensor(a0) and a0.dim() == 3) else a0
        if self.prepare is not None:
            a0 = self.prepare(a0, gen)
        a0 = a0.to(device=dev, dtype=st.io_dtype)
        a0 = a0.expand(S, *a0.shape[1:]).contiguous()
        noise = (self.sample_noise(a0.shape, dev, gen) if self.sample_noise is not None
                 else torch.randn(a0.shape, device=dev, generator=gen)).to(st.io_dtype).contiguous()
        t = torch.tensor(self.t, device=dev, dtype=torch.int64)
        for b0 in range(0, S, self.batch_size):
            b1 = min(S, b0 + self.batch_size)
            first = b0 == 0
            e.wgrad_overwrite = first and st.wgrad_overwrite
            if first:
                e.zero_grad()
            a, nz, tt = a0[b0:b1].contiguous(), noise[b0:b1].contiguous(), t[b0:b1].contiguous()
            m = mixture_fwd(a, a, nz, tt, torch.zeros(b1 - b0, device=dev), st.ac, st.gamma_tab, st.sigma_tab, 0.5)
            pred = e.forward(m.x_mix, tt, **self._cond(b1 - b0))
            cot, _, _ = mse_bwd_seed(pred, nz if self.output == "loss" else torch.zeros_like(nz), 1.0 / S)
            e.backward(cot, nsets=1)

    def row(self, image, index, out):
        """out[0:k] = phi(image) with the noise of dataset index `index`.  Raises in the middle of an accumulation, as quiet_backward
        does; on return the gradient buffers are zero, the weights, moments and operand copies keep every bit."""
        with variants.quiet_backward(self.stepper, "attribution features"):
            self._fill(image, index)
            self.projector.project(self.stepper.e.ps.grads[0], out)
        return out

    def rows(self, dataset, indices, store, first_row=0):
        """store.rows[first_row + r] = row(dataset[indices[r]], indices[r]) (an item that is a tuple: its first entry, the image)."""
        for r, i in enumerate(indices):
            item = dataset[int(i)]
            self.row(item[0] if isinstance(item, (tuple, list)) else item, int(i), store.rows[first_row + r])
        return store


class FeatureStore:
    """`rows` [N, k] f32, preallocated (zero) on `device`, a name per row and the fingerprint of what computed them."""

    def __init__(self, n, k, names=None, device="cuda:0", max_bytes=None, fingerprint=None):
        import torch
        n, k = variants.need_int("n", n, positive=True), check_k(k)
        need = 4 * n * k
        if max_bytes is not None and need > int(max_bytes):
            raise ValueError(f"FeatureStore: {n} rows of {k} take {need} bytes, more than max_bytes = {int(max_bytes)} (a smaller k, "
                             "fewer rows, or a larger max_bytes)")
        self.names = [str(i) for i in range(n)] if names is None else [str(x) for x in names]
        if len(self.names) != n:
            raise ValueError(f"FeatureStore: {n} rows, {len(self.names)} names")
        self.rows = torch.zeros(n, k, dtype=torch.float32, device=device)
        self.fingerprint = dict(fingerprint or {})

    def __len__(self):
        return self.rows.shape[0]

    @property
    def k(self):
        return self.rows.shape[1]

    def save(self, directory):
        """features.safetensors (the rows) and features.json (names, fingerprint) under `directory`."""
        variants.save_tensor(str(directory), ROWS_FILE, "rows", self.rows.detach(), META_FILE,
                             dict(format=FORMAT, n=len(self), k=self.k, names=self.names, fingerprint=self.fingerprint))
        return str(directory)

    @staticmethod
    def read_meta(directory):
        with open(os.path.join(str(directory), META_FILE)) as f:
            return json.load(f)

    @classmethod
    def load(cls, directory, expect=None, device="cpu"):
        """The store save() wrote.  expect: a fingerprint (GradientFeatures.fingerprint); the first field of it that the stored one
        does not equal is named in the ValueError (a field of `expect` that is None is not compared)."""
        from safetensors.torch import load_file
        directory = str(directory)
        meta = cls.read_meta(directory)
        if meta.get("format") != FORMAT:
            raise ValueError(f"{directory}: not a feature store of format {FORMAT}")
        rows = load_file(os.path.join(directory, ROWS_FILE))["rows"]
        if tuple(rows.shape) != (meta["n"], meta["k"]) or len(meta["names"]) != meta["n"]:
            raise ValueError(f"{directory}: {META_FILE} describes {meta['n']} rows of {meta['k']}, {ROWS_FILE} holds {tuple(rows.shape)}")
        have = meta.get("fingerprint") or {}
        for key, want in (expect or {}).items():
            if want is not None and have.get(key) != want:
                raise ValueError(f"{directory}: the store's {key} is {_short(have.get(key))}, this run's is {_short(want)} -- the rows were "
                                 "computed from something else and cannot be compared with rows of this run")
        store = cls(meta["n"], meta["k"], meta["names"], device=device, fingerprint=have)
        store.rows.copy_(rows)
        return store


def _short(v):
    s = json.dumps(v, sort_keys=True) if isinstance(v, dict) else repr(v)
    return s if len(s) <= 48 else s[:45] + "..."


class Attributor:
    """tau(q, i) = phi(q)^T K^-1 phi_i with K = Phi^T Phi / N + lambda I, lambda = damping * mean(diag(Phi^T Phi / N)).  The Gram matrix
    is formed in f64 by torch on the rows' device; its Cholesky factor and every solve are f64 on the host, once per store."""

    def __init__(self, store, damping=1e-2):
        import numpy as np
        import torch
        self.store = store
        damping_term(damping, 1.0)                                  # (refused before any work)
        phi = store.rows.double()
        gram = (phi.T @ phi) / len(store)
        self.mean_diag = float(torch.diagonal(gram).mean())
        self.damping = float(damping)
        self.lam = damping_term(damping, self.mean_diag)
        k = store.k
        K = gram.cpu().numpy() + self.lam * np.eye(k)
        self._chol = np.linalg.cholesky(K)                          # raises LinAlgError when K is not positive definite

    def precondition(self, query_rows):
        """K^-1 q per query row, [Q, k] f64 on the host (two triangular solves against the Cholesky factor)."""
        import numpy as np
        q = np.asarray(query_rows.detach().cpu().double().numpy() if hasattr(query_rows, "detach") else query_rows, dtype=np.float64)
        if q.ndim != 2 or q.shape[1] != self.store.k:
            raise ValueError(f"query rows: [Q, {self.store.k}] are needed, got {q.shape}")
        try:
            from scipy.linalg import solve_triangular
            y = solve_triangular(self._chol, q.T, lower=True)
            return solve_triangular(self._chol.T, y, lower=False).T
        except ImportError:
            return np.linalg.solve(self._chol.T, np.linalg.solve(self._chol, q.T)).T

    def _v32(self, query_rows):
        import torch
        return torch.from_numpy(self.precondition(query_rows)).to(torch.float32).to(self.store.rows.device).contiguous()

    def scores(self, query_rows):
        """[Q, N] f32 on the rows' device: the f32 dot products of the preconditioned queries (rounded to f32) with the rows."""
        return self._v32(query_rows) @ self.store.rows.T

    def topk(self, query_rows, k_top):
        """(val [Q, k_top] f32, idx [Q, k_top] int32): the rows of largest score per query, through sscd_search.topk (k_top <= 32)."""
        from . import sscd_search
        return sscd_search.topk(self._v32(query_rows), self.store.rows, k_top)

    def self_influence(self):
        """[N] f64 on the host: tau(i, i) = phi_i^T K^-1 phi_i."""
        import numpy as np
        phi = self.store.rows.detach().cpu().double().numpy()
        return np.einsum("ij,ij->i", phi, self.precondition(phi))

"""The SD experiment's k-means classifier on the device (csrc/kmeans.hip): the deletion fraction of delete_sd.py:224-225,:269-275
(`kmeans_classifier.predict(255 * image_tensors.permute(0, 2, 3, 1).flatten(1))`, `preds.mean()`) and the fit that produces the
classifier file, which the reference only consumes.

Features are the uint8 pixels of an image in HWC order, D = H * W * 3.  The reference feeds `255 * ToTensor(PIL)` in f32:
f32(f32(v / 255) * 255) == v for every v in 0..255 (tests/test_kmeans_host.py checks all 256), so the kernels take the integer
directly.  Distances are sums of f32-rounded (x - c)^2 terms accumulated in f64 in fixed orders, centres the correctly rounded f32
of exact integer means: every result is bitwise repeatable.

Deviations from scikit-learn, on purpose:
  * `k-means++` here is plain D^2 sampling (no greedy local trials) driven by a torch generator on the host: the same algorithm
    family, NOT the same random stream -- seeds do not reproduce sklearn's centres;
  * a cluster that becomes empty raises (sklearn relocates its centre to the farthest point);
  * with tol = 0 sklearn also stops when no centre moved although labels changed; that exit is not modelled (it can only cost one
    more pass with identical results and an n_iter_ one higher);
  * centres are held in f32 (sklearn keeps f64 for f64 input): they agree to half an f32 ulp.
"""
import os

import numpy as np
import torch

from . import lib
from .records import append_jsonl

MAX_CLUSTERS = 16           # csrc/kmeans.hip: 1 <= K <= 16
MAX_ROWS = (1 << 24) - 1    # uint32 feature sums: 255 * rows < 2^32


def _check_k(k):
    if not 1 <= int(k) <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters={k}: the device kernels take 1 <= K <= {MAX_CLUSTERS}")
    return int(k)


def _rows(x, device=None):
    """uint8 [N, D] on the device from a tensor / array of uint8 rows or [N, H, W, 3] images."""
    t = torch.as_tensor(x)
    if t.dtype != torch.uint8:
        raise TypeError(f"uint8 rows are needed, got {t.dtype} (decoder output goes through from_decoded)")
    if t.dim() < 2:
        raise ValueError(f"rows [N, D] or images [N, H, W, 3] are needed, got shape {tuple(t.shape)}")
    t = t.reshape(t.shape[0], -1)
    if not t.is_cuda:
        t = t.to(device or "cuda")
    return t.contiguous()


def _centres(c, device):
    c = torch.as_tensor(np.asarray(c, dtype=np.float32) if not torch.is_tensor(c) else c).to(device=device, dtype=torch.float32)
    if c.dim() != 2:
        raise ValueError(f"centres [K, D] are needed, got shape {tuple(c.shape)}")
    _check_k(c.shape[0])
    return c.contiguous()


class _Scratch:
    """The buffers of assign / update for one (N, D, K): allocated once per fit or per classified batch shape."""

    def __init__(self, n, d, k, device, update=False):
        self.n, self.d, self.k = n, d, k
        self.nblk = int(lib.query("siss_kmeans_assign_blocks", d, k))
        f64 = dict(dtype=torch.float64, device=device)
        self.slab = torch.empty(n, k, self.nblk, **f64)
        self.dist = torch.empty(n, k, **f64)
        self.row_min = torch.empty(n, **f64)
        self.inertia = torch.empty(1, **f64)
        if update:
            if n > MAX_ROWS:
                raise ValueError(f"{n} rows: the update's uint32 feature sums take at most {MAX_ROWS}")
            self.nseg = int(lib.query("siss_kmeans_update_segments", n, d, k))
            self.sums = torch.empty(self.nseg, k, d, dtype=torch.int32, device=device)       # (uint32 storage)
            self.cnts = torch.empty(self.nseg, k, dtype=torch.int64, device=device)
            self.counts = torch.empty(k, dtype=torch.int64, device=device)


def assign(rows, centres, labels=None, status=None, scratch=None):
    """Squared distances [N, K] (f64) of uint8 rows [N, D] to f32 centres [K, D], labels (int32 argmin, lowest index on ties; when
    `labels` is given it holds the previous pass's and is overwritten), the row minima and their sum -- all device tensors; the low
    word of `status` (int64 [1]) receives the number of labels that changed.  K = 1 is the distance to one centre."""
    n, d = rows.shape
    k = centres.shape[0]
    assert rows.dtype == torch.uint8 and rows.is_cuda and rows.is_contiguous()
    assert centres.dtype == torch.float32 and centres.is_contiguous() and centres.shape[1] == d and centres.device == rows.device
    s = scratch or _Scratch(n, d, k, rows.device)
    assert (s.n, s.d, s.k) == (n, d, k)
    if labels is None:
        labels = torch.full((n,), -1, dtype=torch.int32, device=rows.device)
    assert labels.dtype == torch.int32 and labels.numel() == n and labels.is_contiguous()
    lib.call("siss_kmeans_assign", rows, centres, n, d, k, s.slab, s.nblk, s.dist, labels, s.row_min, s.inertia, status)
    return s.dist, labels, s.row_min, s.inertia


def update(rows, labels, centres, status=None, scratch=None):
    """centres[k] <- the mean of the rows labelled k (exact integer sums, correctly rounded to f32), in place; returns the counts
    [K] (int64, device).  An empty cluster keeps its centre and is counted in the high word of `status`."""
    n, d = rows.shape
    k = centres.shape[0]
    s = scratch if scratch is not None and hasattr(scratch, "sums") else _Scratch(n, d, k, rows.device, update=True)
    assert (s.n, s.d, s.k) == (n, d, k) and labels.dtype == torch.int32 and labels.numel() == n
    lib.call("siss_kmeans_update", rows, labels, n, d, k, centres, s.sums, s.cnts, s.nseg, s.counts, status)
    return s.counts


class KMeansClassifier:
    """Nearest-centre classifier over uint8 HWC pixels: what `joblib.load(classifier_path).predict` is to the reference.

    `cluster_centers_`: float32 [K, D] (numpy), D = H * W * 3 in the reference's flatten order `permute(0, 2, 3, 1).flatten(1)`.
    After `fit` also `labels_` (int32 device tensor), `inertia_` and `n_iter_`."""

    def __init__(self, cluster_centers, device=None):
        c = np.ascontiguousarray(np.asarray(cluster_centers.detach().cpu() if torch.is_tensor(cluster_centers) else cluster_centers,
                                            dtype=np.float32))
        if c.ndim != 2:
            raise ValueError(f"cluster centres [K, D] are needed, got shape {c.shape}")
        _check_k(c.shape[0])
        self.cluster_centers_ = c
        self.device = device
        self._dev = None
        self.labels_ = self.inertia_ = self.n_iter_ = None

    @property
    def n_clusters(self):
        return self.cluster_centers_.shape[0]

    @property
    def n_features(self):
        return self.cluster_centers_.shape[1]

    @classmethod
    def load(cls, path, device=None):
        """`.joblib` / `.pkl`: a pickled scikit-learn KMeans (the reference's file), its `cluster_centers_`; `.npz`: the key
        `cluster_centers` (what `save` writes)."""
        path = str(path)
        ext = os.path.splitext(path)[1].lower()
        if ext == ".npz":
            with np.load(path) as z:
                if "cluster_centers" not in z:
                    raise KeyError(f"{path}: no array `cluster_centers` in it")
                return cls(z["cluster_centers"], device)
        if ext in (".joblib", ".pkl"):
            try:
                import joblib
                import sklearn  # noqa: F401  (unpickling a KMeans needs it)
            except ImportError as e:
                raise ImportError(f"{path}: a pickled scikit-learn KMeans needs joblib and scikit-learn to load ({e}); convert it "
                                  "once where they are installed: KMeansClassifier.load(path).save('kmeans_classifier.npz')") from e
            return cls(np.asarray(joblib.load(path).cluster_centers_), device)
        raise ValueError(f"{path}: a .joblib / .pkl (scikit-learn KMeans) or .npz (cluster_centers) file is needed")

    def save(self, path):
        path = str(path)
        if not path.endswith(".npz"):
            raise ValueError(f"{path}: the classifier is written as .npz")
        np.savez(path, cluster_centers=self.cluster_centers_)
        return path

    def centres(self, device):
        device = torch.device(device)
        if self._dev is None or self._dev.device != device:
            self._dev = torch.from_numpy(self.cluster_centers_).to(device).contiguous()
        return self._dev

    def predict(self, u8_rows):
        """(u8 rows [N, D] on the device, labels int32 [N], squared distances f64 [N, K]) of uint8 rows / [N, H, W, 3] images."""
        rows = _rows(u8_rows, self.device)
        if rows.shape[1] != self.n_features:
            raise ValueError(f"rows of {rows.shape[1]} features, centres of {self.n_features}")
        dist, labels, _, _ = assign(rows, self.centres(rows.device))
        return rows, labels, dist

    def from_decoded(self, img):
        """(uint8 images [n, H, W, 3], labels int32 [n], squared distances f64 [n, K]) of the VAE decoder's output [n, 3, H, W]
        (f32 or bf16, about [-1, 1]): ONE fused launch writes the image -- bitwise `((img / 2 + 0.5).clamp(0, 1) * 255).round()
        .to(uint8).permute(0, 2, 3, 1)` -- and the distance partials, one more turns them into labels.  All on the device."""
        if not (torch.is_tensor(img) and img.is_cuda and img.dim() == 4 and img.shape[1] == 3):
            raise ValueError("the decoder's output [n, 3, H, W] on the device is needed")
        if img.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"decoder output of dtype {img.dtype}: float32 or bfloat16")
        img = img.contiguous()
        n, _, h, w = img.shape
        if 3 * h * w != self.n_features:
            raise ValueError(f"images of 3 x {h} x {w} = {3 * h * w} features, centres of {self.n_features}")
        k, dev = self.n_clusters, img.device
        nblk = int(lib.query("siss_kmeans_decoded_blocks", h * w))
        u8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
        slab = torch.empty(n, k, nblk, dtype=torch.float64, device=dev)
        dist = torch.empty(n, k, dtype=torch.float64, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        lib.call("siss_kmeans_decoded", img, int(img.dtype == torch.bfloat16), self.centres(dev), n, h, w, k, u8, slab, nblk)
        lib.call("siss_kmeans_finalize", slab, n, k, nblk, dist, labels, None, None, None)
        return u8, labels, dist


def _lloyd(rows, centres, max_iter):
    """Lloyd's iterations from `centres` (modified in place).  Per iteration ONE int64 leaves the device: the changed-label count
    (low word) and the empty-cluster count of the previous update (high word)."""
    n, d = rows.shape
    k = centres.shape[0]
    s = _Scratch(n, d, k, rows.device, update=True)
    labels = torch.full((n,), -1, dtype=torch.int32, device=rows.device)
    status = torch.zeros(1, dtype=torch.int64, device=rows.device)

    def step():
        assign(rows, centres, labels, status, s)
        word = int(status.item())
        if word >> 32:
            raise RuntimeError(f"k-means: {word >> 32} of {k} clusters became empty (scikit-learn relocates such a centre; this fit "
                               "does not: choose another init / seed or fewer clusters)")
        return word & 0xFFFFFFFF

    converged, n_iter = False, 0
    for i in range(max_iter):
        n_iter = i + 1
        if step() == 0:                     # sklearn's strict convergence: this pass's labels equal the previous pass's, and
            converged = True                # the centres already are the means of exactly these labels
            break
        update(rows, labels, centres, status, s)
    if not converged:
        step()                              # labels consistent with the last centres (sklearn's closing E-step)
    return labels, float(s.inertia.item()), n_iter


def kmeans_plusplus(rows, n_clusters, generator=None):
    """[K, D] f32 centres that are rows of `rows`: the first uniform, each next one drawn with probability proportional to its
    squared distance to the nearest centre so far (the K = 1 assign pass gives the distances to the newest centre).  The uniform
    draws come from `generator` (a torch generator on the host); the row indices stay on the device."""
    n, d = rows.shape
    k = _check_k(n_clusters)
    s = _Scratch(n, d, 1, rows.device)
    centres = torch.empty(k, d, dtype=torch.float32, device=rows.device)
    first = int(torch.randint(n, (1,), generator=generator))
    centres[0] = rows[first].float()
    nearest = None
    for j in range(1, k):
        dist, _, _, _ = assign(rows, centres[j - 1:j].contiguous(), scratch=s)
        nearest = dist[:, 0].clone() if nearest is None else torch.minimum(nearest, dist[:, 0])
        cum = torch.cumsum(nearest, 0)
        u = torch.rand(1, generator=generator, dtype=torch.float64).to(rows.device)
        idx = torch.searchsorted(cum, u * cum[-1], right=True).clamp_(max=n - 1)      # the first row whose mass passes the draw
        centres[j] = rows[idx[0]].float()
    return centres


def fit(u8_rows, n_clusters=2, init="k-means++", max_iter=300, n_init=1, generator=None, device=None):
    """Lloyd's k-means over uint8 rows [N, D] (or images [N, H, W, 3]) on the device, with scikit-learn's strict convergence
    (`KMeans(tol=0, algorithm="lloyd")`): it stops at the first pass whose labels equal the previous pass's; `n_iter_` counts passes
    as sklearn does.  `init`: an explicit [K, D] array, or "k-means++" (see kmeans_plusplus: not sklearn's random stream); with the
    latter `n_init` restarts keep the lowest inertia.  Returns a KMeansClassifier with labels_, inertia_, n_iter_."""
    rows = _rows(u8_rows, device)
    k = _check_k(n_clusters)
    if rows.shape[0] < k:
        raise ValueError(f"{rows.shape[0]} rows for {k} clusters")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter={max_iter}: at least one pass")
    explicit = not isinstance(init, str)
    if not explicit and init != "k-means++":
        raise ValueError(f"init={init!r}: an explicit [K, D] array or 'k-means++'")
    best = None
    for _ in range(1 if explicit else max(1, int(n_init))):
        if explicit:
            centres = _centres(init, rows.device).clone()
            if tuple(centres.shape) != (k, rows.shape[1]):
                raise ValueError(f"init of shape {tuple(centres.shape)}, need ({k}, {rows.shape[1]})")
        else:
            centres = kmeans_plusplus(rows, k, generator)
        labels, inertia, n_iter = _lloyd(rows, centres, int(max_iter))
        if best is None or inertia < best[1]:
            best = (centres, inertia, labels, n_iter)
    out = KMeansClassifier(best[0], rows.device)
    out.inertia_, out.labels_, out.n_iter_ = best[1], best[2], best[3]
    return out


class DeletionFraction:
    """delete_sd.py:269-275 for one rank: `record(prompt, labels, step)` takes the labels of one validation prompt's images,
    appends {global_step, deletion_fraction_<i>} to `out_path` and adds deletion_steps_<i> = step the FIRST time that prompt's
    fraction is 0 (the reference writes it into the run summary once).  `score_decoded` / `score_u8` are the classifier's labels in
    the shape the other scorers of the SD evaluation have (metric_net.score_chain)."""

    def __init__(self, classifier, out_path):
        self.classifier, self.out_path = classifier, out_path
        self.deletion_steps = {}
        self.extra = None                                # fields added to every record (pipeline.sampler: name and step count)

    def score_decoded(self, img):
        """(labels [n], uint8 images [n, H, W, 3]), both on the device, of the decoder's output (one fused launch, then the labels)."""
        u8, labels, _ = self.classifier.from_decoded(img)
        return labels, u8

    def score_u8(self, u8):
        """Labels [n] (device) of uint8 images [n, H, W, 3]."""
        return self.classifier.predict(u8)[1]

    def record(self, prompt, labels, step):
        labels = torch.as_tensor(labels)
        frac = float(labels.double().mean())                   # preds.mean(): a fraction for two clusters
        rec = {"global_step": int(step), f"deletion_fraction_{prompt}": frac}
        if frac == 0 and prompt not in self.deletion_steps:
            self.deletion_steps[prompt] = rec[f"deletion_steps_{prompt}"] = int(step)
        rec.update(self.extra or {})
        return append_jsonl(self.out_path, rec)

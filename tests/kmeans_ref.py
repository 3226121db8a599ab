"""Float64 host restatement of the Lloyd loop of scikit-learn's `KMeans(init=init, n_init=1, tol=0, algorithm="lloyd")`
(sklearn/cluster/_kmeans.py `_kmeans_single_lloyd`), for tests: direct (x - c)^2 distances, argmin with the lowest index on ties,
centres = mean of the rows of a label, strict convergence (stop at the first pass whose labels equal the previous pass's), and
n_iter_ counted as sklearn counts it.  Also the synthetic sets of tests/golden/kmeans_ref.npz."""
import numpy as np


def distances(X, centres):
    """[N, K] f64 squared distances."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(centres, dtype=np.float64)
    return ((X[:, None, :] - C[None, :, :]) ** 2).sum(-1)


def relative_gap(d):
    """Per row (second smallest - smallest) / second smallest distance; 1 for K = 1."""
    if d.shape[1] < 2:
        return np.ones(d.shape[0])
    s = np.sort(d, axis=1)
    return (s[:, 1] - s[:, 0]) / np.maximum(s[:, 1], 1e-300)


def lloyd_f64(X, init, max_iter=300):
    """-> dict(labels, centres [K, D] f64, inertia, n_iter, min_gap): min_gap is the smallest relative gap between the two nearest
    centres over every row and every pass (how far any label is from flipping under a distance error)."""
    X = np.asarray(X, dtype=np.float64)
    centres = np.array(init, dtype=np.float64)
    k = centres.shape[0]
    old = np.full(X.shape[0], -1)
    min_gap, strict, n_iter = np.inf, False, 0
    for i in range(max_iter):
        n_iter = i + 1
        d = distances(X, centres)
        min_gap = min(min_gap, relative_gap(d).min())
        labels = d.argmin(1)
        if np.array_equal(labels, old):
            strict = True
            break
        for j in range(k):
            members = X[labels == j]
            if len(members) == 0:
                raise RuntimeError(f"cluster {j} became empty")
            centres[j] = members.sum(0) / len(members)
        old = labels
    if not strict:
        d = distances(X, centres)
        min_gap = min(min_gap, relative_gap(d).min())
        labels = d.argmin(1)
    return dict(labels=labels, centres=centres, inertia=float(d.min(1).sum()), n_iter=n_iter, min_gap=float(min_gap))


N, N_HELD, SHAPE, SIGMA, BASE, STEP = 160, 40, (8, 8, 3), 40.0, 116, 20


def synthetic_set(k, seed):
    """(X uint8 [N, D], held-out uint8 [N_HELD, D], init f64 [K, D]): K flat grey images STEP levels (half a sigma) apart plus
    sigma = SIGMA noise, rounded and clipped to 0..255.  The init is K distinct rows of X that all come from the FIRST component: a
    poor start, so that Lloyd needs several passes (4 to 7 on the kept seeds) to pull the centres apart, while the components stay
    far enough from each other for the two nearest centres of every row to differ by >= 1e-3 (relative) at every pass on some
    seeds -- with the components closer, hardly any seed keeps that gap over a whole run."""
    rng = np.random.RandomState(seed)
    d = int(np.prod(SHAPE))
    levels = BASE + STEP * np.arange(k)
    drawn = []

    def draw(n):
        which = rng.randint(k, size=n)
        drawn.append(which)
        return np.clip(np.rint(levels[which][:, None] + SIGMA * rng.randn(n, d)), 0, 255).astype(np.uint8)

    X, held = draw(N), draw(N_HELD)
    init = X[rng.choice(np.flatnonzero(drawn[0] == 0), size=k, replace=False)].astype(np.float64)
    return X, held, init


class HostKMeans:
    """What siss_amd.kmeans.fit returns, restated on the host for tests of the code around the fit: cluster_centers_ (f32), labels_,
    inertia_, n_iter_ and predict(rows) -> (rows, labels, distances)."""

    def __init__(self, centres, labels=None, inertia=None, n_iter=None):
        self.cluster_centers_ = np.asarray(centres, dtype=np.float32)
        self.labels_, self.inertia_, self.n_iter_ = labels, inertia, n_iter

    def predict(self, rows):
        rows = np.asarray(rows).reshape(len(rows), -1)
        d = distances(rows, self.cluster_centers_)
        return rows, d.argmin(1).astype(np.int32), d


def host_fit(rows, n_clusters=2, init="k-means++", max_iter=300, n_init=1, generator=None):
    """fit() of siss_amd.kmeans on the host in f64 (plain D^2 seeding from a torch generator, n_init restarts, lowest inertia)."""
    import torch
    X = np.asarray(rows).reshape(len(rows), -1).astype(np.float64)
    best = None
    for _ in range(1 if not isinstance(init, str) else max(1, n_init)):
        if isinstance(init, str):
            idx = [int(torch.randint(len(X), (1,), generator=generator))]
            for _j in range(1, n_clusters):
                cum = np.cumsum(distances(X, X[idx]).min(1))
                u = float(torch.rand(1, generator=generator, dtype=torch.float64))
                idx.append(min(int(np.searchsorted(cum, u * cum[-1], side="right")), len(X) - 1))
            start = X[idx]
        else:
            start = np.asarray(init, dtype=np.float64)
        r = lloyd_f64(X, start, max_iter)
        if best is None or r["inertia"] < best["inertia"]:
            best = r
    return HostKMeans(best["centres"], best["labels"].astype(np.int32), best["inertia"], best["n_iter"])

"""Writes tests/golden/kmeans_ref.npz with scikit-learn (1.7 here): for K = 2 and K = 3 the first three data seeds from 100 upward
whose relative gap between the two nearest centres is >= GAP for every row at every Lloyd pass (and for the held-out rows), with
`KMeans(init=init, n_init=1, tol=0, algorithm="lloyd")` on float64 as the recorded truth.  The float64 host restatement
(tests/kmeans_ref.py) must reproduce sklearn's labels and n_iter_ on every kept case -- asserted here -- and supplies the per-pass
gaps sklearn does not expose.

    python tests/make_kmeans_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from kmeans_ref import distances, lloyd_f64, relative_gap, synthetic_set  # noqa: E402

GAP = 1e-3
PER_K = 3
MIN_LONG_ITERS = 5


def main():
    from sklearn.cluster import KMeans
    out, summary = {}, []
    for k in (2, 3):
        kept, seed = 0, 100
        longest = 0
        while kept < PER_K:
            assert seed < 400, f"K={k}: no {PER_K} seeds with gap >= {GAP} below 400"
            X, held, init = synthetic_set(k, seed)
            host = lloyd_f64(X, init)
            held_gap = relative_gap(distances(held, host["centres"])).min()
            if min(host["min_gap"], held_gap) < GAP:
                seed += 1
                continue
            km = KMeans(n_clusters=k, init=init, n_init=1, tol=0, algorithm="lloyd", max_iter=300).fit(X.astype(np.float64))
            # the restatement IS sklearn on these cases: same labels, same pass count, centres to f64 rounding
            assert np.array_equal(km.labels_, host["labels"]) and km.n_iter_ == host["n_iter"], (k, seed)
            assert np.abs(km.cluster_centers_ - host["centres"]).max() <= 1e-9, (k, seed)
            assert abs(km.inertia_ - host["inertia"]) <= 1e-9 * host["inertia"], (k, seed)
            name = f"k{k}_s{seed}"
            out[name + "_X"], out[name + "_held"], out[name + "_init"] = X, held, init
            out[name + "_labels"] = km.labels_.astype(np.int32)
            out[name + "_centres"] = km.cluster_centers_
            out[name + "_inertia"] = np.float64(km.inertia_)
            out[name + "_n_iter"] = np.int64(km.n_iter_)
            out[name + "_held_labels"] = km.predict(held.astype(np.float64)).astype(np.int32)
            out[name + "_min_gap"] = np.float64(min(host["min_gap"], held_gap))
            summary.append((name, km.n_iter_, float(out[name + "_min_gap"])))
            longest = max(longest, km.n_iter_)
            kept += 1
            seed += 1
        assert longest >= MIN_LONG_ITERS, f"K={k}: no kept case runs {MIN_LONG_ITERS} passes ({summary})"
    out["cases"] = np.array([s[0] for s in summary])
    path = os.path.join(HERE, "golden", "kmeans_ref.npz")
    np.savez_compressed(path, **out)
    for s in summary:
        print("%s  n_iter %d  min gap %.3g" % s)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

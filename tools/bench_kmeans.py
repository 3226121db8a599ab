#!/usr/bin/env python
"""The SD k-means classifier on one GPU, 512 x 512 images (D = 786,432 features), K = 2: prints ONE JSON line.

    python tools/bench_kmeans.py [--decoded 8 64] [--rows 256 2048] [--min-seconds 0.5] [--rounds 3] [--size 512] [--no-host]

classify (per n in --decoded): the decoder's output [n, 3, S, S] f32 on the device -> uint8 images + labels
  * fused: KMeansClassifier.from_decoded (siss_kmeans_decoded + siss_kmeans_finalize), the labels read on the host;
  * composed: what it replaces -- sd_sampler.py:144's torch chain on the device, the uint8 images copied to the host, nearest centre
    there (scikit-learn's KMeans.predict on 255 * ToTensor-style f32 rows as delete_sd.py:271 calls it when sklearn imports, else a
    numpy f32 restatement);
  bytes = 5 n D + 4 K D (f32 in, uint8 out, centres once), GB/s = bytes / fused device time.
lloyd (per N in --rows): one Lloyd pass = assignment + update over uint8 rows [N, D] on the device
  * hip: siss_kmeans_assign + siss_kmeans_update (bytes = 2 N D + 12 K D: the rows twice, centres read and written);
  * host: scikit-learn's lloyd on f32 rows on the host's cores (threadpool as the environment sets it), per pass = (fit with
    max_iter = 3 - fit with max_iter = 1) / 2, when sklearn imports; else torch on the same GPU (f32 cdist-style expansion + index_add).
Device times are medians over --rounds of host-synchronised windows of at least --min-seconds, every shape warmed first; `spread`
is (max - min) / median over the rounds.  HBM_PEAK_GBPS is the figure DESIGN.md quotes (8 TB/s)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBPS = 8000.0


def measure(fn, min_seconds):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n


def median_spread(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
    return med, (ts[-1] - ts[0]) / med


def host_predictor(centres):
    """rows f32 [n, D] -> labels, on the host."""
    try:
        from sklearn.cluster import KMeans
        km = KMeans(n_clusters=centres.shape[0], init=centres, n_init=1, max_iter=1).fit(centres)   # centres of itself
        km.cluster_centers_ = centres.astype(np.float32)
        return "sklearn KMeans.predict", lambda rows: km.predict(rows)
    except ImportError:
        c = centres.astype(np.float32)
        return "numpy f32", lambda rows: np.stack([((rows - c[k]) ** 2).sum(1) for k in range(len(c))], 1).argmin(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decoded", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host / torch sides (device figures only)")
    a = ap.parse_args()
    from siss_amd import kmeans as KM
    dev = torch.device("cuda", 0)
    S, K = a.size, 2
    D = 3 * S * S
    g = torch.Generator(device=dev).manual_seed(0)
    proto = torch.randint(0, 256, (K, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    clf = KM.KMeansClassifier(proto.flatten(1).float())
    res = {"metric": "sd_kmeans", "size": S, "features": D, "clusters": K, "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK_GBPS, "classify": {}, "lloyd": {}}
    name, predict = host_predictor(clf.cluster_centers_)
    res["host_classifier"] = name
    for n in a.decoded:
        which = torch.arange(n, device=dev) % K
        img = ((proto[which].float() + 30 * torch.randn(n, S, S, 3, generator=g, device=dev)) / 255 * 2 - 1).permute(0, 3, 1, 2).contiguous()

        def fused():
            u8, labels, _ = clf.from_decoded(img)
            return u8, labels.cpu()

        def composed():
            u8 = ((img / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
            return u8, predict(u8.reshape(n, -1).astype(np.float32))

        (u8_f, l_f) = fused()
        paths = {"fused": fused}
        if not a.no_host:
            (u8_c, l_c) = composed()
            assert np.array_equal(u8_f.cpu().numpy(), u8_c) and np.array_equal(l_f.numpy(), np.asarray(l_c)), "paths disagree"
            paths["composed"] = composed
        times = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                times[k].append(measure(fn, a.min_seconds))
        nbytes = 5.0 * n * D + 4.0 * K * D
        out = {}
        for k, ts in times.items():
            med, spread = median_spread(ts)
            out[k] = {"ms": round(1e3 * med, 4), "spread": round(spread, 4)}
        out["fused"]["GBps"] = round(nbytes / (out["fused"]["ms"] * 1e-3) / 1e9, 1)
        out["fused"]["share_of_hbm_peak"] = round(out["fused"]["GBps"] / HBM_PEAK_GBPS, 4)
        if "composed" in out:
            out["composed_over_fused"] = round(out["composed"]["ms"] / out["fused"]["ms"], 2)
        res["classify"][str(n)] = out
    for N in a.rows:
        rows = torch.randint(0, 256, (N, D), generator=g, device=dev, dtype=torch.uint8)
        rows[::2] = ((rows[::2].float() + proto[0].flatten().float()) / 2).to(torch.uint8)      # two loose groups
        init = rows[:K].float()
        scratch = KM._Scratch(N, D, K, dev, update=True)
        labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        centres = init.clone()

        def hip_pass():
            KM.assign(rows, centres, labels, status, scratch)
            KM.update(rows, labels, centres, status, scratch)

        def hip_assign():
            KM.assign(rows, centres, labels, status, scratch)

        hip_pass()
        paths = {"hip_pass": hip_pass, "hip_assign": hip_assign}
        other = None
        if not a.no_host:
            try:
                from sklearn.cluster import KMeans
                X = rows.cpu().numpy().astype(np.float32)

                def fit_time(iters):
                    t0 = time.perf_counter()
                    KMeans(n_clusters=K, init=init.cpu().numpy(), n_init=1, tol=0, algorithm="lloyd", max_iter=iters).fit(X)
                    return time.perf_counter() - t0
                fit_time(1)
                per = [(fit_time(3) - fit_time(1)) / 2 for _ in range(max(1, a.rounds - 1))]
                med, spread = median_spread(per)
                other = {"what": f"sklearn lloyd, f32 rows, {os.environ.get('OMP_NUM_THREADS', 'all')} host threads",
                         "ms": round(1e3 * med, 2), "spread": round(spread, 4)}
                del X
            except ImportError:
                xf = rows.float()

                def torch_pass():
                    c = init
                    d = (xf * xf).sum(1, keepdim=True) - 2 * xf @ c.t() + (c * c).sum(1)
                    lab = d.argmin(1)
                    torch.zeros(K, D, device=dev).index_add_(0, lab, xf) / torch.bincount(lab, minlength=K).clamp_min(1)[:, None]
                torch_pass()
                per = [measure(torch_pass, a.min_seconds) for _ in range(a.rounds)]
                med, spread = median_spread(per)
                other = {"what": "torch f32 on the same GPU (expanded distances + index_add)", "ms": round(1e3 * med, 3),
                         "spread": round(spread, 4)}
                del xf
        times = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                times[k].append(measure(fn, a.min_seconds))
        out = {}
        for k, ts in times.items():
            med, spread = median_spread(ts)
            nbytes = (2.0 if k == "hip_pass" else 1.0) * N * D + (12.0 if k == "hip_pass" else 4.0) * K * D
            out[k] = {"ms": round(1e3 * med, 4), "spread": round(spread, 4), "GBps": round(nbytes / med / 1e9, 1),
                      "share_of_hbm_peak": round(nbytes / med / 1e9 / HBM_PEAK_GBPS, 4)}
        if other:
            out["other"] = other
            out["other_over_hip_pass"] = round(other["ms"] / out["hip_pass"]["ms"], 1)
        res["lloyd"][str(N)] = out
        del rows, scratch
    print(json.dumps(res))


if __name__ == "__main__":
    main()

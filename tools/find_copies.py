#!/usr/bin/env python
"""Find copied images by their SSCD embeddings, on the device (notebooks/sscd.ipynb of the reference: embed a directory, form all
pairwise similarities on the host, list what lies above a threshold).

    python tools/find_copies.py --images DIR --model sscd_disc_mixup.torchscript.pt [--threshold 0.5] [--out copies.json]
        all pairs of DIR at or above the threshold and the connected components they form (the candidate forget clusters)
    python tools/find_copies.py --images DIR --gallery DIR|INDEX_DIR --model ... [--topk 5]
        for each image of DIR its --topk nearest rows of the gallery (a directory of images, or an index saved with --save-index)

The search runs on csrc/sscd_search.hip (siss_amd/sscd_search.py): the queries x gallery matrix is never formed and no similarity but
the reported ones reaches the host.  --allow-random-init runs without the checkpoint on random weights, loudly: the figures then say
nothing about copies.  Writes pairs and components, not a labels file for the k-means classifier."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pairs_report(index, threshold):
    """All pairs of the index at or above the threshold, and their connected components, by name."""
    from siss_amd.sscd_search import components
    i, j, v = index.pairs(threshold)
    names = index.names
    return {"mode": "pairs", "images": len(index), "threshold": float(threshold),
            "pairs": [[names[a], names[b], float(s)] for a, b, s in zip(i.tolist(), j.tolist(), v.tolist())],
            "components": [[names[a] for a in comp] for comp in components(len(index), i, j)]}


def gallery_report(index, emb, names, k, threshold):
    """Per query its k nearest rows of the index, by name, and whether the nearest reaches the threshold."""
    val, idx = index.topk(emb, k)
    out = []
    for name, vr, ir in zip(names, val.cpu().tolist(), idx.cpu().tolist()):
        top = [[index.names[j], float(v)] for v, j in zip(vr, ir) if j >= 0]
        out.append({"name": name, "copy": bool(top and top[0][1] >= threshold), "top": top})
    return {"mode": "gallery", "images": len(names), "gallery": len(index), "threshold": float(threshold), "topk": int(k), "queries": out}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", required=True, help="directory of the images to examine")
    ap.add_argument("--model", required=True, help="the SSCD checkpoint (TorchScript archive or state dict)")
    ap.add_argument("--gallery", help="a directory of images, or an index directory written by --save-index; absent: all pairs of --images")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--out", default="copies.json")
    ap.add_argument("--save-index", help="write the index of the gallery (or of --images) to this directory")
    ap.add_argument("--allow-random-init", action="store_true", help="random weights when --model is not on disk (NOT a copy detector)")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--mean", type=float, nargs="+", default=[0.485, 0.456, 0.406], help="Normalize mean (SSCD's: ImageNet)")
    ap.add_argument("--std", type=float, nargs="+", default=[0.229, 0.224, 0.225])
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    import torch
    from siss_amd.sscd_search import SSCDIndex, list_images
    from siss_amd.tasks import _load_sscd
    model = _load_sscd(a.model, a.allow_random_init, "--model")
    model.batch_size = a.batch_size
    model = model.to(torch.device(a.device)).eval()
    images = list_images(a.images)
    if not images:
        raise FileNotFoundError(f"--images {a.images!r}: no image files")
    if a.gallery is None:
        index = SSCDIndex.build(model, images, a.mean, a.std, a.batch_size)
        report = pairs_report(index, a.threshold)
    else:
        if SSCDIndex.exists(a.gallery):
            index = SSCDIndex.load(a.gallery, model=model)
        else:
            index = SSCDIndex.build(model, list_images(a.gallery), a.mean, a.std, a.batch_size)
        queries = SSCDIndex.build(model, images, index.meta.get("mean") or a.mean, index.meta.get("std") or a.std, a.batch_size)
        report = gallery_report(index, queries.emb, queries.names, a.topk, a.threshold)
    if a.save_index:
        index.save(a.save_index)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    n = len(report["pairs"]) if report["mode"] == "pairs" else sum(q["copy"] for q in report["queries"])
    print(f"{report['mode']}: {report['images']} images, {n} at or above {a.threshold}; written to {a.out}")
    return report


if __name__ == "__main__":
    main()

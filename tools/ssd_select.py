#!/usr/bin/env python
"""Sweep the selection of Selective Synaptic Dampening without repeating the backward passes: from a directory that holds
ssd_importance.safetensors + ssd.json (written by a run with `deletion.ssd`) and the checkpoint those importances were taken at,
DRY-RUN siss_ssd_dampen for a list of alpha and fraction values and print one line of statistics per value.  Nothing is written.

    python tools/ssd_select.py IMPORTANCE_DIR CHECKPOINT [--cond] [--subfolder unet] [--alpha 5 10 50] [--fraction 0.001 0.01]
                               [--lambda 1] [--targets REGEX ...] [--json]

CHECKPOINT: a diffusers directory (its `unet` subfolder by default); --cond: the Stable Diffusion (conditional) UNet.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLUMNS = ("selected", "fraction_selected", "dampened", "zeroed", "mean_beta", "delta_norm", "relative_change")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("importance_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--cond", action="store_true", help="the checkpoint is a UNet2DConditionModel (Stable Diffusion)")
    ap.add_argument("--subfolder", default="unet")
    ap.add_argument("--alpha", type=float, nargs="*", default=[])
    ap.add_argument("--fraction", type=float, nargs="*", default=[])
    ap.add_argument("--lambda", dest="lam", type=float, default=1.0)
    ap.add_argument("--targets", nargs="*", default=None, help="regular expressions over the parameter names (deletion.ssd.targets)")
    ap.add_argument("--json", action="store_true", help="one JSON line per value instead of the table")
    a = ap.parse_args(argv)
    if not a.alpha and not a.fraction:
        ap.error("give at least one --alpha or --fraction value")
    import torch
    from siss_amd import ssd
    from siss_amd.model import UNet2DConditionModel, UNet2DModel
    from siss_amd.trainable import parse_patterns
    assert torch.cuda.is_available(), "ssd_select.py needs a GPU: the selection and the dry run are HIP kernels (there is no fall-back)"
    cls = UNet2DConditionModel if a.cond else UNet2DModel
    eng = cls.from_pretrained(a.checkpoint, subfolder=a.subfolder or None, device="cuda:0", compute_dtype=torch.bfloat16).engine
    imp = ssd.Importances.load(a.importance_dir, eng)
    names = ssd.select_targets(list(eng.ps.specs), parse_patterns(a.targets, "--targets"))
    rows = []
    for mode, values in (("alpha", a.alpha), ("fraction", a.fraction)):
        for v in values:
            thr, strict, k, gt, ge = ssd.select(imp, targets=names, **{mode: v})
            st = ssd.dampen(eng, imp, thr, strict, a.lam, apply=False)
            rows.append(dict({mode: v}, threshold=thr, strict=strict, k=k, **{"lambda": a.lam}, **st))
    if a.json:
        for r in rows:
            print(json.dumps(r))
        return rows
    print(f"{'rule':>18} {'threshold':>12} " + " ".join(f"{c:>17}" for c in COLUMNS))
    for r in rows:
        rule = f"alpha {r['alpha']:g}" if "alpha" in r else f"fraction {r['fraction']:g}"
        print(f"{rule:>18} {r['threshold']:>12.6g} " + " ".join(
            f"{r[c]:>17d}" if isinstance(r[c], int) else f"{'-':>17}" if r[c] is None else f"{r[c]:>17.6g}" for c in COLUMNS))
    return rows


if __name__ == "__main__":
    main()

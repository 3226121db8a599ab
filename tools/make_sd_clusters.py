#!/usr/bin/env python
"""Produce the three files the SD experiment reads and the reference ships no code for: sample N images of one prompt, cluster
them into two groups on the device (siss_amd.kmeans.fit) and write

    <img_dir>/<images_name>_NNN.png     the images (skipped with --from-dir: cluster PNGs that already exist)
    data_files.labels_path              kmeans_labels.json      file name -> 0 / 1, 1 = memorized   (data.SDData reads it)
    data_files.clustering_info_path     clustering_info.json    frac_deletion = share of label 1, mem_idx = NNN of the image
                                                                nearest to centre 1                 (DeleteSD.fill_cfg reads it)
    metrics.fraction_deletion.classifier_path, or <base_dir>/kmeans_classifier.npz
                                        the classifier, centre 1 = memorized                        (DeleteSD.evaluate reads it)

Label 1 is the cluster with the smaller mean distance of its members to their centre (memorized generations are near-duplicates
of one image), or with --mem-image PATH the cluster whose centre is nearest to that image.

    python tools/make_sd_clusters.py --n 256 [--batch 8] [--steps 50] [--prompt "..."] [--from-dir] [--mem-image PATH]
                                     [--sampler dpmsolver++ [--solver-order 2]]
                                     [--config-name delete_sd] [--config-path config] [key=value ...]

--sampler dpmsolver++ samples with the opt-in DPM-Solver++ (2M) solver (pipeline.sampler of config/delete_sd.yaml) in --steps
steps instead of DDIM; clustering_info.json then says so ("sampler", "num_inference_steps").

The prompt defaults to validation_prompts[0].  Sampling needs the checkpoint directory (unet/, vae/, text_encoder/ + tokenizer/
or a .pt prompt embedding), as the validation pass of delete_sd does."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def image_names(img_dir, images_name):
    """[(NNN, file name)] of <images_name>_NNN.png in img_dir, by NNN."""
    pat = re.compile(re.escape(images_name) + r"_(\d+)\.png$")
    found = sorted((int(m.group(1)), f) for f in os.listdir(img_dir) for m in [pat.match(f)] if m)
    if not found:
        raise FileNotFoundError(f"no {images_name}_NNN.png under {img_dir!r}")
    return found


def load_rows(img_dir, names):
    """uint8 [N, H * W * 3] (HWC, the classifier's feature order) of the named PNGs; they must share one size."""
    from PIL import Image
    rows, shape = [], None
    for f in names:
        with Image.open(os.path.join(img_dir, f)) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if shape is not None and a.shape != shape:
            raise ValueError(f"{f}: {a.shape}, the images before it {shape}")
        shape = a.shape
        rows.append(a.reshape(-1))
    return np.stack(rows), shape


def choose_memorized(labels, dist, centres, mem_row=None):
    """Index (0 / 1) of the memorized cluster: nearest centre to mem_row when given, else the smaller mean member-to-centre
    distance (ties: cluster 0)."""
    if mem_row is not None:
        d = ((centres.astype(np.float64) - mem_row.astype(np.float64)[None]) ** 2).sum(1)
        return int(d.argmin())
    spread = [np.sqrt(dist[labels == j, j]).mean() for j in (0, 1)]
    return int(spread[1] < spread[0])


def cluster(rows, numbered, fit, mem_row=None, generator=None, n_init=4):
    """-> (labels {name: 0 / 1}, info {frac_deletion, mem_idx}, centres f32 [2, D] with the memorized cluster at index 1)."""
    model = fit(rows, n_clusters=2, init="k-means++", n_init=n_init, generator=generator)
    _, labels, dist = model.predict(rows)
    labels, dist = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels), np.asarray(dist.cpu() if hasattr(dist, "cpu") else dist)
    centres = np.asarray(model.cluster_centers_, dtype=np.float32)
    mem = choose_memorized(labels, dist, centres, mem_row)
    order = [1 - mem, mem]                                  # the memorized cluster becomes index 1
    centres, dist = centres[order], dist[:, order]
    labels = (labels == mem).astype(np.int64)
    nearest = int(dist[:, 1].argmin())
    info = {"frac_deletion": float(labels.mean()), "mem_idx": int(numbered[nearest][0])}
    return {f: int(l) for (_, f), l in zip(numbered, labels)}, info, centres


def sample_images(cfg, prompt, n, batch, steps, img_dir, images_name):
    """N images of one prompt from the configured checkpoint through the validation pipeline, written as PNGs."""
    import torch
    from PIL import Image
    from siss_amd.tasks import DeleteSD
    task = DeleteSD(cfg)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    unet = task.load_unet(device)
    sampler = task._validation_pipeline(unet, device)
    if sampler.vae is None:
        raise FileNotFoundError("sampling images needs vae/ in the checkpoint directory")
    e = task._prompt_embedding(prompt, device)
    g = torch.Generator(device=device).manual_seed(task.seed())
    os.makedirs(img_dir, exist_ok=True)
    done = 0
    with sampler.holding_graphs():
        while done < n:
            b = min(batch, n - done)
            imgs, _ = sampler(e, negative_prompt_embeds=task._negative_embeds, num_inference_steps=steps, guidance_scale=7.5,
                              num_images_per_prompt=b, generator=g, output_type="np")
            for a in imgs:
                Image.fromarray(a).save(os.path.join(img_dir, f"{images_name}_{done:03d}.png"))
                done += 1


def main(argv=None, fit=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-name", default="delete_sd")
    ap.add_argument("--config-path", default=os.path.join(ROOT, "config"))
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--from-dir", action="store_true")
    ap.add_argument("--mem-image", default=None)
    ap.add_argument("--n-init", type=int, default=4)
    ap.add_argument("--sampler", default=None, help="dpmsolver++: the opt-in solver instead of DDIM (pipeline.sampler)")
    ap.add_argument("--solver-order", type=int, default=2)
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    import torch
    from siss_amd import hydra_lite
    cfg = hydra_lite.compose(a.config_name, a.config_path, a.overrides)
    fields = {}
    if a.sampler is not None:                               # the validation pipeline reads the key; a bad name is refused there
        cfg.pipeline = dict(cfg.get("pipeline") or {}, num_inference_steps=a.steps,
                            sampler=dict(name=a.sampler, solver_order=a.solver_order))
        from siss_amd.scheduler import DPMSolverMultistepScheduler
        DPMSolverMultistepScheduler.from_sampler_config(cfg.pipeline.sampler)      # (a name / order it does not have: refused now)
        if not a.from_dir:
            fields ={"sampler": f"{a.sampler}{a.solver_order}m", "num_inference_steps": a.steps}
    df = cfg.get("data_files") or {}
    img_dir, labels_path, info_path = df.get("img_dir"), df.get("labels_path"), df.get("clustering_info_path")
    if not (img_dir and labels_path and info_path):
        raise ValueError("data_files.img_dir, labels_path and clustering_info_path are needed")
    fd = (cfg.get("metrics") or {}).get("fraction_deletion") or {}
    clf_path = str(fd.get("classifier_path") or os.path.join(str(cfg.base_dir), "kmeans_classifier.npz"))
    if not clf_path.endswith(".npz"):
        clf_path = os.path.splitext(clf_path)[0] + ".npz"   # (the reference's .joblib name: scikit-learn's pickle is not written here)
    name = str(cfg.images_name)
    if not a.from_dir:
        vp = cfg.get("validation_prompts")
        sample_images(cfg, a.prompt or (vp[0] if vp else None), a.n, a.batch, a.steps, str(img_dir), name)
    numbered = image_names(str(img_dir), name)
    rows, shape = load_rows(str(img_dir), [f for _, f in numbered])
    mem_row = None
    if a.mem_image:
        mem_row, mem_shape = load_rows(os.path.dirname(a.mem_image) or ".", [os.path.basename(a.mem_image)])
        if mem_shape != shape:
            raise ValueError(f"--mem-image is {mem_shape}, the images {shape}")
        mem_row = mem_row[0]
    if fit is None:
        from siss_amd.kmeans import fit
    labels, info, centres = cluster(rows, numbered, fit, mem_row, torch.Generator().manual_seed(int(cfg.get("seed", 42))), a.n_init)
    from siss_amd.kmeans import KMeansClassifier
    for p in (labels_path, info_path, clf_path):
        os.makedirs(os.path.dirname(os.path.abspath(str(p))), exist_ok=True)
    with open(str(labels_path), "w") as f:
        json.dump(labels, f, indent=1)
    with open(str(info_path), "w") as f:
        json.dump({**info, **fields}, f, indent=1)
    KMeansClassifier(centres).save(clf_path)
    print(f"{len(labels)} images of {shape}: frac_deletion {info['frac_deletion']:.4f}, mem_idx {info['mem_idx']}; wrote {labels_path}, "
          f"{info_path}, {clf_path}")
    return labels, info, clf_path


if __name__ == "__main__":
    main()

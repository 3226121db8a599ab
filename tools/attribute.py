#!/usr/bin/env python
"""Data attribution in front of an unlearning run: which training images stand behind a sample (D-TRAK gradient features on
csrc/attribution.hip; siss_amd/attribution.py).  NOT the reference's protocol; one model, no ensemble over checkpoints.

    python tools/attribute.py build --config-name=delete_celeb|delete_tshirt [key=value ...] --out DIR [--k 2048] [--timesteps 10]
                                    [--output square|loss] [--targets REGEX ...] [--indices FILE] [--seed 0] [--batch-size B]
                                    [--max-bytes N]
        one feature row per image of the task's keep dataset (`dataset_all`; deletion.img_name=[] keeps every image in it), at the
        task's own weights (load_unet), through its prepare_batch; DIR receives features.safetensors, features.json and
        build.json (the command's configuration, for `query`).  --indices: a file of dataset indices, one per line.

    python tools/attribute.py query --store DIR (--images PATH ... | --dataset-index I ...) [--top 20] [--damping 0.01]
                                    [--write-forget-list FILE]
        the rows of the queries (files through the task's transform, seeded by their position; or dataset images, seeded by their
        index), scored against the store; DIR receives attribution.json; FILE the union of the top names, one per line: the list
        `deletion.img_name` (the datasets' remove_img_names) takes.

Stable Diffusion goes through the library (GradientFeatures(prepare=, conditioning=)), not this tool.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TASKS = ("delete_celeb", "delete_tshirt")
BUILD_FILE, RESULT_FILE = "build.json", "attribution.json"


def dataset_names(ds):
    """A name per dataset item: the file's base name where the dataset has files, else the index."""
    paths = getattr(ds, "paths", None)
    if paths is not None:
        return [os.path.basename(p) for p in paths]
    return [str(i) for i in range(len(ds))]


def write_forget_list(path, names):
    """One name per line, each once, in the given order: what `deletion.img_name` / remove_img_names takes."""
    seen, out = set(), []
    for n in names:
        if n not in seen:
            seen.add(n)
            out.append(str(n))
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in out))
    return out


def read_forget_list(path):
    with open(path) as f:
        return [line.rstrip("\n") for line in f if line.strip()]


def open_task(config_name, config_path, overrides, device):
    """(task, unet, stepper, keep dataset) of a task configuration: its own load_unet and datasets; allow_random_init /
    allow_synthetic are honoured as loudly as the task honours them."""
    from siss_amd import hydra_lite
    from siss_amd.step import SISSStepper
    if config_name not in TASKS:
        raise ValueError(f"--config-name={config_name}: one of {TASKS} (Stable Diffusion goes through siss_amd.attribution itself)")
    cfg = hydra_lite.compose(config_name, config_path, list(overrides))
    task = hydra_lite.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.fill_cfg()
    unet = task.load_unet(device)
    sched = task.load_scheduler()
    lr, betas, eps, wd = task.optimizer_args()
    stepper = SISSStepper(unet.engine, sched.alphas_cumprod, lr=lr, betas=betas, eps=eps, weight_decay=wd, scaling_norm=1.0,
                          train_batch_size=int(cfg.train_batch_size), mixed_precision=cfg.get("mixed_precision"))
    shape = (unet.config.in_channels, unet.config.sample_size, unet.config.sample_size)
    ds_all, _ = task.datasets(shape)
    return task, unet, stepper, ds_all


def features_of(task, stepper, a, device):
    from siss_amd import attribution as A
    from siss_amd.trainable import Subset, parse_patterns, select
    from siss_amd.unet import ALIGN
    ps = stepper.e.ps
    names = select(list(ps.specs), parse_patterns(a["targets"], "--targets"), "--targets")
    subset = None if names is None else Subset(ps.specs, names, ps.total, ALIGN)
    proj = A.Projector(int(ps.total), a["k"], a["seed"], subset, device)
    return A.GradientFeatures(stepper, proj, a["timesteps"], a["output"], a["batch_size"], a["seed"], prepare=task.prepare_batch,
                              conditioning=lambda B: task.conditioning(B, device), sample_noise=task.sample_noise)


def build(a, overrides):
    import torch
    from siss_amd import attribution as A
    assert torch.cuda.is_available(), "attribute.py needs a GPU: the features are HIP kernels (there is no fall-back)"
    device = torch.device("cuda", 0)
    task, unet, stepper, ds = open_task(a.config_name, a.config_path, overrides, device)
    names = dataset_names(ds)
    if a.indices:
        with open(a.indices) as f:
            indices = [int(line) for line in f if line.strip()]
    else:
        indices = list(range(len(ds)))
    bad = [i for i in indices if not 0 <= i < len(ds)]
    if bad or not indices:
        raise ValueError(f"--indices: {bad[:3]} outside the dataset's 0 .. {len(ds) - 1}" if bad else "--indices: no index")
    settings = dict(k=a.k, timesteps=a.timesteps, output=a.output, seed=a.seed, batch_size=a.batch_size, targets=a.targets)
    feats = features_of(task, stepper, settings, device)
    row_names = [names[i] for i in indices]
    store = A.FeatureStore(len(indices), a.k, row_names, device, a.max_bytes, feats.fingerprint(row_names))
    feats.rows(ds, indices, store)
    torch.cuda.synchronize()
    store.save(a.out)
    with open(os.path.join(a.out, BUILD_FILE), "w") as f:
        json.dump(dict(config_name=a.config_name, config_path=a.config_path, overrides=list(overrides), indices=indices, **settings), f,
                  indent=1)
    print(f"[attribute] {len(store)} rows of {a.k} ({a.output}, {a.timesteps} timesteps) -> {a.out}")
    return store


def query(a):
    import numpy as np
    import torch
    from siss_amd import attribution as A
    assert torch.cuda.is_available(), "attribute.py needs a GPU: the features are HIP kernels (there is no fall-back)"
    device = torch.device("cuda", 0)
    with open(os.path.join(a.store, BUILD_FILE)) as f:
        b = json.load(f)
    task, unet, stepper, ds = open_task(b["config_name"], b["config_path"], b["overrides"], device)
    feats = features_of(task, stepper, b, device)
    meta = A.FeatureStore.read_meta(a.store)
    store = A.FeatureStore.load(a.store, feats.fingerprint(meta["names"]), device)       # (changed weights: refused by field)
    if bool(a.images) == bool(a.dataset_index):
        raise ValueError("query: give --images or --dataset-index (one of the two)")
    if a.images:
        from siss_amd import hydra_lite
        from PIL import Image
        transform = hydra_lite.instantiate(task.cfg.transform)
        what = [(os.path.basename(p), transform(Image.open(p).convert("RGB")), i) for i, p in enumerate(a.images)]
    else:
        item = lambda i: ds[i][0] if isinstance(ds[i], (tuple, list)) else ds[i]
        what = [(f"dataset[{i}]", item(i), i) for i in a.dataset_index]
    q = torch.zeros(len(what), store.k, device=device)
    for r, (_, image, index) in enumerate(what):
        feats.row(image, index, q[r])
    att = A.Attributor(store, a.damping)
    top = min(a.top, len(store), 32)
    val, idx = att.topk(q, top)
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    si = att.self_influence()
    rank = np.empty(len(si), dtype=np.int64)
    rank[np.argsort(-si, kind="stable")] = np.arange(len(si))
    out = dict(store=os.path.abspath(a.store), damping=att.damping, damping_term=att.lam, top=top, queries=[])
    for r, (name, _, index) in enumerate(what):
        keep = idx[r] >= 0
        out["queries"].append(dict(query=name, index=index, names=[store.names[i] for i in idx[r][keep]],
                                   scores=[float(v) for v in val[r][keep]],
                                   self_influence_rank=[int(rank[i]) for i in idx[r][keep]]))
    with open(os.path.join(a.store, RESULT_FILE), "w") as f:
        json.dump(out, f, indent=1)
    if a.write_forget_list:
        listed = write_forget_list(a.write_forget_list, [n for qr in out["queries"] for n in qr["names"]])
        print(f"[attribute] {len(listed)} names -> {a.write_forget_list} (deletion.img_name=[{','.join(listed[:3])}{',...' if len(listed) > 3 else ''}])")
    out["rows"] = q
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build")
    b.add_argument("--config-name", required=True)
    b.add_argument("--config-path", default=os.path.join(ROOT, "config"))
    b.add_argument("--out", required=True)
    b.add_argument("--k", type=int, default=2048)
    b.add_argument("--timesteps", type=int, default=10)
    b.add_argument("--output", choices=("square", "loss"), default="square")
    b.add_argument("--targets", nargs="*", default=None, help="regular expressions over the parameter names: project their gradients only")
    b.add_argument("--indices", default=None, help="a file of dataset indices, one per line (default: the whole dataset)")
    b.add_argument("--seed", type=int, default=0)
    b.add_argument("--batch-size", type=int, default=None, help="noisings per micro-batch (default: all of --timesteps)")
    b.add_argument("--max-bytes", type=int, default=None)
    q = sub.add_parser("query")
    q.add_argument("--store", required=True)
    q.add_argument("--images", nargs="*", default=None)
    q.add_argument("--dataset-index", type=int, nargs="*", default=None)
    q.add_argument("--top", type=int, default=20)
    q.add_argument("--damping", type=float, default=1e-2)
    q.add_argument("--write-forget-list", default=None)
    a, overrides = ap.parse_known_args(argv)
    if a.cmd == "build":
        return build(a, overrides)
    if overrides:
        ap.error(f"query: unknown arguments {overrides}")
    return query(a)


if __name__ == "__main__":
    main()

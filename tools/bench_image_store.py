#!/usr/bin/env python
"""The input side of the pixel-space loops on one GPU, today's path against the image store: prints ONE JSON line.

    python tools/bench_image_store.py [--shapes celeb,mnist] [--out profiles/<name>.json]

Synthetic uint8 data written to a temporary directory -- JPEG files of 256 x 256 (smooth random images, quality 90) for the CelebA
shape at B = 16, an npz of 28 x 28 images for the MNIST shape at B = 128 -- and, per shape:

  * host: milliseconds per micro-batch spent producing the batch on the device, each micro-batch on a host clock that ends in a
    device synchronise, back to back (no step in between: the rate the producer sustains).  celeb: (x0, a0) as _DeleteBase.run takes
    them -- today ``next(Prefetcher)`` + ``next(batches(forget, RepeatedSampler))`` + ``.to(device)``, with the store two
    ``ImageStore.images(IndexBatch)`` over the same samplers; the store's batches are split into those with misses (decodes) and
    without.  mnist: x0 as TrainUnconditional.run takes it -- today ``torch.stack([ds[i] for i in idx]).to(device)``, with the store
    one ``images(idx)`` over the same EpochSampler.  Medians, with the 10th / 90th percentiles.
  * kernel: siss_image_gather alone at the batch shape, device events around groups of back-to-back launches after warm-up, the
    median group; bytes = n * chw * (1 + 4) (one byte read, one f32 written) over that time.  At the batch shape that is the time
    BETWEEN launches (the host's enqueue rate covers the kernel), so the same is taken at a large n (256 / 32768 images), where it
    is the kernel's.  The celeb store of this step holds 2048 random rows (403 MB, more than the 256 MB last-level cache) and every
    launch draws other rows; the mnist store is the data set.
  * loop: steps/s of the task's own eager loop (DeleteCeleb / TrainUnconditional .run(), bf16, random-init weights) with the store
    off and on, alternating off, on, off, on, from the `elapsed_s` the loop logs per optimizer step (the first `--loop-skip` steps
    left out); the spread is the difference between the two runs of the same setting.

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the tool there.
The shader clock is read after the timed work of each step.  No threshold is attached to any of it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"celeb": dict(B=16, chw=(3, 256, 256), images=192, big=256), "mnist": dict(B=128, chw=(1, 28, 28), images=8192, big=32768)}
LIMITS = {"host": 240, "kernel": 120, "loop": 300}       # seconds per child


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()][:2] or "not recorded"
    except Exception:
        return "not recorded"


def _stats(ms):
    if not ms:
        return None
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4),
            "batches": len(s)}


# ---------------------------------------------------------------- data (driver, no GPU)
def write_data(root, shapes):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    if "celeb" in shapes:
        d = os.path.join(root, "celeb")
        os.makedirs(d)
        for i in range(SHAPES["celeb"]["images"] + 1):     # the last one is the forget image
            low = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
            Image.fromarray(low, "RGB").resize((256, 256), Image.BICUBIC).save(os.path.join(d, f"{i:05d}.jpg"), quality=90)
    if "mnist" in shapes:
        d = os.path.join(root, "mnist")
        os.makedirs(d)
        n = SHAPES["mnist"]["images"]
        np.savez(os.path.join(d, "train.npz"), image=rng.integers(0, 256, (n, 28, 28), dtype=np.uint8), label=np.arange(n) % 11)


def _datasets(shape, data):
    from siss_amd.data import CelebAHQ, Compose, HFDataset, Normalize, ToTensor
    tr = Compose([ToTensor(), Normalize([0.5], [0.5])])
    if shape == "celeb":
        forget = [f"{SHAPES['celeb']['images']:05d}.jpg"]
        d = os.path.join(data, "celeb")
        return CelebAHQ("nondeletion", d, forget, transform=tr), CelebAHQ("deletion", d, forget, transform=tr)
    return HFDataset("all", os.path.join(data, "mnist"), "train", transform=tr), None


# ---------------------------------------------------------------- the steps (children)
def step_host(shape, data, a):
    import torch
    from siss_amd.data import EpochSampler, InfiniteSampler, Prefetcher, RepeatedSampler, batches, index_batches
    from siss_amd.image_store import ImageStore
    dev = torch.device("cuda", 0)
    B = SHAPES[shape]["B"]
    keep, forget = _datasets(shape, data)

    def timed(produce, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = produce()
            torch.cuda.synchronize()
            out.append(((time.perf_counter() - t0) * 1e3, extra))
        return out

    res = {}
    if shape == "celeb":
        it_all = Prefetcher(keep, InfiniteSampler(keep), B, device=dev, workers=4)
        it_del = batches(forget, RepeatedSampler(forget, 1 << 30), B)

        def today():
            x0, a0 = next(it_all).to(dev, non_blocking=True), next(it_del).to(dev, non_blocking=True)
            return x0.shape[0] + a0.shape[0]
        timed(today, a.warmup)
        res["today"] = _stats([ms for ms, _ in timed(today, a.batches)])
        it_all.close()
        ks, fs = ImageStore(keep, device=dev), ImageStore(forget, device=dev)
        ik, jf = index_batches(InfiniteSampler(keep), B, ks), index_batches(RepeatedSampler(forget, 1 << 30), B, fs)

        def store():
            before = ks.decoded + fs.decoded
            xb, ab = next(ik), next(jf)
            xb.cache.images(xb), ab.cache.images(ab)
            return ks.decoded + fs.decoded - before
        rows = timed(store, a.warmup + 3 * a.batches)[a.warmup:]
        res["store_with_misses"] = _stats([ms for ms, miss in rows if miss])
        res["store_all_hits"] = _stats([ms for ms, miss in rows if not miss])
        res["store_decoded"], res["store_images"] = ks.decoded + fs.decoded, len(keep) + len(forget)
    else:
        sampler = iter(EpochSampler(len(keep), B, 0, 1 << 20))
        def today():
            return torch.stack([keep[i] for i in next(sampler)[2]]).to(dev, non_blocking=True).shape[0]
        timed(today, a.warmup)
        res["today"] = _stats([ms for ms, _ in timed(today, a.batches)])
        st = ImageStore(keep, device=dev)
        sampler = iter(EpochSampler(len(keep), B, 0, 1 << 20))
        def store():
            return st.images(next(sampler)[2]).shape[0]
        timed(store, a.warmup)
        res["store_all_hits"] = _stats([ms for ms, _ in timed(store, a.batches)])
    return res


def step_kernel(shape, data, a):
    import torch
    from siss_amd.image_store import byte_table, gather_blocks, image_gather
    from siss_amd.data import Compose, Normalize, ToTensor
    dev = torch.device("cuda", 0)
    B, (C, H, W) = SHAPES[shape]["B"], SHAPES[shape]["chw"]
    rows = 2048 if shape == "celeb" else SHAPES[shape]["images"]
    g = torch.Generator(device=dev).manual_seed(0)
    store = torch.randint(0, 256, (rows, C, H, W), dtype=torch.uint8, device=dev, generator=g)
    table = byte_table(Compose([ToTensor(), Normalize([0.5], [0.5])]), C).to(dev)
    res = {"store_bytes": store.numel(), "launches_per_group": a.reps_kernel,
           "timing": "back-to-back launches between two events: launch gaps are in it"}
    for n in (B, SHAPES[shape]["big"]):                       # the batch, and one large enough that the launch gap does not cover it
        idxs = [torch.randint(0, rows, (n,), device=dev, generator=g) for _ in range(a.reps_kernel)]
        out = torch.empty((n, C, H, W), device=dev)
        for idx in idxs[:10]:
            image_gather(store, idx, table, out=out)
        groups = []
        for _ in range(a.groups):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for idx in idxs:
                image_gather(store, idx, table, out=out)
            s1.record()
            torch.cuda.synchronize()
            groups.append(s0.elapsed_time(s1) / len(idxs))
        ms = statistics.median(groups)
        nbytes = n * C * H * W * 5
        res[f"n{n}"] = {"kernel_ms": round(ms, 5), "groups_ms": [round(v, 5) for v in groups], "bytes": nbytes,
                        "bytes_per_s": round(nbytes / (ms * 1e-3)), "blocks": [gather_blocks(n, C * H * W), n]}
        del out
    return res


def step_loop(shape, data, a, on, out_dir):
    from siss_amd import hydra_lite as H
    B = SHAPES[shape]["B"]
    common = [f"train_batch_size={B}", "gradient_accumulation_steps=1", "mixed_precision=bf16", f"output_dir={out_dir}",
              *(["+image_store.enabled=true"] if on else [])]
    if shape == "celeb":
        cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"),
                        [*common, f"data_dir={data}/celeb", f"deletion.img_name=[{SHAPES['celeb']['images']:05d}.jpg]",
                         "checkpoint_path=/nonexistent", "allow_random_init=true", "save_final=false", f"training_steps={a.loop_steps}",
                         "+dataloader_num_workers=4"])
        key = "global_step"
    else:
        epochs = -(-a.loop_steps * B // SHAPES["mnist"]["images"])
        cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"),
                        [*common, f"dataset.name={data}/mnist", f"num_epochs={epochs}", "sampling_steps=null", "checkpointing_steps=null"])
        key = "step"
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.run()
    lines = [json.loads(l) for l in open(os.path.join(out_dir, "train_log_rank0.jsonl"))]
    t = {r[key]: r["elapsed_s"] for r in lines}
    first, last = a.loop_skip, max(t)
    stores = [s for s in (getattr(task, n, None) for n in ("keep_store", "forget_store", "train_store")) if s is not None]
    assert bool(stores) == on
    return {"steps_per_s": round((last - first) / (t[last] - t[first]), 3), "steps_timed": last - first,
            "decoded": sum(s.decoded for s in stores), "launches": sum(s.launches for s in stores)}


# ---------------------------------------------------------------- the driver
def child(step, shape, data, a, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--shape", shape, "--data", data, "--batches", str(a.batches),
           "--warmup", str(a.warmup), "--reps-kernel", str(a.reps_kernel), "--groups", str(a.groups), "--loop-steps", str(a.loop_steps),
           "--loop-skip", str(a.loop_skip), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step.split("-")[0]])
    if r.returncode != 0:
        raise SystemExit(f"step {step} ({shape}) ended with status {r.returncode}: nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    print(f"[bench_image_store] {shape} {step} {' '.join(extra)}: done", file=sys.stderr, flush=True)     # progress, not the result
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="celeb,mnist")
    ap.add_argument("--batches", type=int, default=60, help="timed micro-batches of the host step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps-kernel", type=int, default=200)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--loop-steps", type=int, default=60)
    ap.add_argument("--loop-skip", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON there")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--data", default=None)
    ap.add_argument("--on", type=int, default=0)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "bench_image_store.py needs a GPU"
        from siss_amd import lib
        lib.load()
        res = {"host": lambda: step_host(a.shape, a.data, a), "kernel": lambda: step_kernel(a.shape, a.data, a),
               "loop": lambda: step_loop(a.shape, a.data, a, bool(a.on), a.out_dir)}[a.step]()
        res["sclk"] = _clock()                               # read right after the timed work
        print(json.dumps(res))
        return
    shapes = [s for s in a.shapes.split(",") if s]
    assert all(s in SHAPES for s in shapes), a.shapes
    res = {"tool": "bench_image_store", "weights": "random-init", "dtype": "bf16 engine, f32 batches",
           "args": {k: getattr(a, k.replace("-", "_")) for k in ("batches", "warmup", "reps-kernel", "groups", "loop-steps", "loop-skip")},
           "shapes": {}}
    with tempfile.TemporaryDirectory() as data:
        write_data(data, shapes)
        for shape in shapes:
            row = {"B": SHAPES[shape]["B"], "image": list(SHAPES[shape]["chw"]), "images": SHAPES[shape]["images"]}
            row["host"] = child("host", shape, data, a)
            row["kernel"] = child("kernel", shape, data, a)
            runs = []
            for k, on in enumerate((0, 1, 0, 1)):            # alternating: other people's work shares the host
                runs.append(child("loop", shape, data, a, ["--on", str(on), "--out-dir", os.path.join(data, f"run_{shape}_{k}")]))
            off, on_ = [runs[0]["steps_per_s"], runs[2]["steps_per_s"]], [runs[1]["steps_per_s"], runs[3]["steps_per_s"]]
            row["loop"] = {"off_steps_per_s": off, "on_steps_per_s": on_, "spread_steps_per_s": round(max(abs(off[0] - off[1]), abs(on_[0] - on_[1])), 3),
                           "off_step_ms": round(2e3 / sum(off), 3), "on_step_ms": round(2e3 / sum(on_), 3), "runs": runs}
            res["shapes"][shape] = row
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

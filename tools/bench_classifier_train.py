#!/usr/bin/env python
"""Time one training step of the MNIST ResNet-18 classifier at B = 128, 28 x 28, on the GPU: the HIP trainer
(siss_amd.classifier_train.ResNet18Trainer.step) and, in the same call and alternating with it, a PyTorch-ROCm eager step of
tests/classifier_ref.py::ResNet18Ref (train mode, F.cross_entropy, torch.optim.Adam) on the same batch.  Device events around
`--steps` steps (at least 200) after `--warmup`, `--repeats` times each; one JSON line with the per-step medians and the spread.

    python tools/bench_classifier_train.py [--steps 200] [--warmup 20] [--repeats 5] [--batch 128] [--only hip|torch]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    a = ap.parse_args(argv)
    if a.steps < 200 and a.only is None:
        ap.error("--steps >= 200 is needed for a timing")
    import torch
    import torch.nn.functional as F
    from classifier_ref import ResNet18Ref
    from siss_amd.classifier_train import ResNet18Trainer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(a.batch, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (a.batch,), generator=g).to(dev)
    trainer = ResNet18Trainer(device=dev)
    ref = ResNet18Ref().to(dev).train()
    ref.load_state_dict(trainer.state_dict())
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)

    def hip_step():
        trainer.step(x, y)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(ref(x), y).backward()
        opt.step()

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / n

    runs = [(n, f) for n, f in (("hip", hip_step), ("torch", torch_step)) if a.only in (None, n)]
    for _, fn in runs:
        timed(fn, a.warmup)
    times = {n: [] for n, _ in runs}
    for _ in range(a.repeats):
        for n, fn in runs:                                      # alternating: both see the same clocks and neighbours
            times[n].append(timed(fn, a.steps))
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for n, ts in times.items():
        ts = sorted(ts)
        out[f"{n}_step_ms"] = ts[len(ts) // 2]
        out[f"{n}_min_ms"], out[f"{n}_max_ms"] = ts[0], ts[-1]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

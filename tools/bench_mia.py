#!/usr/bin/env python
"""The membership inference attacks on one GPU, RANDOM-INIT weights, synthetic images: prints ONE JSON line.

    python tools/bench_mia.py [--images 8] [--batch 8] [--min-seconds 1.0] [--rounds 2] [--models celebahq256 tshirt] [--dtypes bf16 f32]

Per architecture (CelebA-HQ 256 x 256, the T-shirt MNIST 28 x 28), compute dtype and attack (the defaults of siss_amd/mia.py: SecMI
t_sec = 100 / stride 10 = 12 forwards per image, PIA 2, loss 4):
  * graph / eager: siss_amd.mia.MembershipAttack.scores, each batch's chain replayed from its captured hipGraph / launched eagerly;
  * torch: the same chain written with torch's element-wise operations around the SAME engine forward, eagerly -- what a user
    writes without the metric;
  * forward_share: (forwards per evaluation) x (one captured forward of the same batch, timed alone) / the graph path's time.
Every number is ms per image.  Timing: a synchronised host clock around whole evaluations; every shape is warmed (graphs captured)
first; each measurement repeats the evaluation until --min-seconds have passed; the paths are alternated --rounds times in one call
and the median is reported with the spread between identical runs (max - min over rounds, relative).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_chains(eng, ab, x0, noise, settings, b):
    """{attack: f64 [N]} of the three chains in eager torch on the engine's forward, b rows per forward."""
    from siss_amd.mia import transfer_coefficients as tc
    out = {k: [] for k in settings}
    fw = lambda x, t: eng.forward(x.contiguous(), torch.full((x.shape[0],), t, dtype=torch.long, device=x.device))
    rows = lambda v: v.reshape(v.shape[0], -1).double().sum(dim=1)
    for s0 in range(0, x0.shape[0], b):
        x = x0[s0:s0 + b]
        if "secmi" in settings:
            t_sec, stride = settings["secmi"]["t_sec"], settings["secmi"]["stride"]
            y = x
            for s in range(0, t_sec, stride):
                cx, ce = tc(ab, "transfer", s, s + stride)
                y = cx * y + ce * fw(y, s)
            cx, ce = tc(ab, "transfer", t_sec, t_sec + stride)
            yf = cx * y + ce * fw(y, t_sec)
            cx, ce = tc(ab, "transfer", t_sec + stride, t_sec)
            out["secmi"].append(rows(((cx * yf + ce * fw(yf, t_sec + stride)) - y) ** 2))
        if "pia" in settings:
            t, p = settings["pia"]["t"], settings["pia"]["p"]
            e0 = fw(x, 0).clone()                                  # (the engine's prediction buffer is overwritten by the next forward)
            cx, ce = tc(ab, "noise", None, t)
            out["pia"].append(rows((e0 - fw(cx * x + ce * e0, t)).abs() ** p))
        if "loss" in settings:
            t = settings["loss"]["t"]
            cx, ce = tc(ab, "noise", None, t)
            out["loss"].append(torch.stack([rows((fw(cx * x + ce * n[None], t) - n[None]) ** 2) for n in noise], dim=1).mean(dim=1))
    return {k: torch.cat(v) for k, v in out.items()}


def measure(fn, min_seconds):
    """Seconds per call of fn (a whole evaluation, host-synchronised), repeated until min_seconds have passed."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n


def forward_seconds(eng, b, shape, dev, min_seconds):
    """Seconds of one captured forward of b rows, replayed alone."""
    xs, ts = torch.zeros((b, *shape), device=dev), torch.zeros(b, dtype=torch.long, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eng.forward(xs, ts)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.forward(xs, ts)
    torch.cuda.current_stream().wait_stream(side)
    return measure(graph.replay, min_seconds)


def median_spread(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
    return med, (ts[-1] - ts[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=["celebahq256", "tshirt"], choices=["celebahq256", "tshirt"])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "f32"], choices=["bf16", "f32"])
    a = ap.parse_args()
    from siss_amd.config import UNet2DConfig
    from siss_amd.data import SyntheticImages
    from siss_amd.mia import ATTACKS, DEFAULTS, MembershipAttack
    from siss_amd.model import UNet2DModel
    from siss_amd.scheduler import DDPMScheduler
    dev = torch.device("cuda", 0)
    sched = DDPMScheduler()
    ab = sched.alphas_cumprod
    N, b = a.images, a.batch
    res = {"metric": "mia", "weights": "random-init", "images": N, "batch_size": b, "settings": DEFAULTS, "unit": "ms per image",
           "device": torch.cuda.get_device_name(0), "runs": {}}
    for model in a.models:
        cfg = UNet2DConfig.celebahq256() if model == "celebahq256" else UNet2DConfig.mnist_tshirt()
        shape = (cfg.in_channels, cfg.sample_size, cfg.sample_size)
        images = torch.stack([SyntheticImages(N, shape, seed=1)[i] for i in range(N)]).to(dev)
        for dtype in a.dtypes:
            unet = UNet2DModel(cfg, device=dev, compute_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
            unet.engine.init_random(seed=0)
            eng = unet.engine
            fwd = forward_seconds(eng, b, shape, dev, a.min_seconds)
            out = {"ms_per_forward_of_batch": round(1e3 * fwd, 3)}
            for attack in ATTACKS:
                gen = lambda: torch.Generator(device=dev).manual_seed(0)
                ms = {"graph": MembershipAttack(unet, sched, dev, attacks=(attack,), batch_size=b),
                      "eager": MembershipAttack(unet, sched, dev, attacks=(attack,), batch_size=b, use_graph=False)}
                paths = {k: (lambda m=m: m.scores(images, generator=gen())) for k, m in ms.items()}
                noise = torch.randn((DEFAULTS["loss"]["noises"], *shape), device=dev, generator=gen())

                def plain():
                    with torch.no_grad():
                        return torch_chains(eng, ab, images, noise, {attack: DEFAULTS[attack]}, b)
                paths["torch"] = plain
                got = {k: fn()[attack].cpu() for k, fn in paths.items()}            # every shape warmed, every graph captured
                times = {k: [] for k in paths}
                for _ in range(a.rounds):                                           # alternated in one call
                    for k in ("graph", "torch", "eager"):
                        times[k].append(measure(paths[k], a.min_seconds))
                forwards = ms["graph"].forwards[attack]
                rec = {"forwards_per_evaluation": forwards,
                       "rel_diff_vs_torch": float(((got["graph"] - got["torch"]).abs() / got["torch"].abs()).max())}
                for k, ts in times.items():
                    med, spread = median_spread(ts)
                    rec[k] = {"ms_per_image": round(1e3 * med / N, 3), "spread": round(spread, 4)}
                med = median_spread(times["graph"])[0]
                rec["forward_share"] = round(forwards * fwd / med, 4)
                rec["graph_over_eager"] = round(median_spread(times["eager"])[0] / med, 4)
                rec["graph_over_torch"] = round(median_spread(times["torch"])[0] / med, 4)
                out[attack] = rec
                print(f"[bench_mia] {model} {dtype} {attack}: {rec['graph']['ms_per_image']} ms per image", file=sys.stderr)
                del ms, paths
            res["runs"][f"{model}_{dtype}"] = out
            del unet, eng
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

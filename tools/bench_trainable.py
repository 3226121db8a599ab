#!/usr/bin/env python
"""The replayed SISS step with a trainable SUBSET on one GPU: prints ONE JSON line (and writes it with --out).

    python tools/bench_trainable.py --config sd15 --batch 4 [--reps 10] [--rounds 2] [--out profiles/trainable_subset_sd15.json]
    python tools/bench_trainable.py --config celebahq256 --batch 16

bf16, random-init weights (the times do not depend on them), the synthetic inputs of bench.py.  Legs, each a stepper of its own over
ONE engine, its step captured into a hipGraph:

  * full                        the full update (what bench.py times; the check that the default path did not move is bench.py
                                against the parent commit's library: tools/ab_bench.sh)
  * <selection> / skip          SISSStepper(trainable=...), weight-gradient products with frozen outputs dropped (the default)
  * <selection> / keep          the same with UNetEngine.skip_frozen_wgrad = False: the full backward pass, the subset optimizer

Selections: `attn2` (the conditional UNet only), `attentions`, and the last up block.  Every leg is replayed --reps times between
two device events, the legs interleaved, --rounds rounds: ms per step of every round are reported, their spread is the run-to-run
spread the differences are to be read against.  Beside the step times: the trainable share of the parameters, the products
described / dropped in one backward pass, and the two optimizer launches' times from device events around each launch of one eager
step, with the bytes they move (pass 1 reads g_x, g_a: 8 B per trainable float; pass 2 reads g_x, g_a, p, m, v and writes p, m, v and
the bf16 shadow: 34 B) over the 8 TB/s of the data sheet.  The shader clock is read after each leg's timed work.  No threshold is
attached to any of it.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:1] or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15", choices=["sd15", "celebahq256", "small"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trainable.py needs a GPU"
    from siss_amd import lib
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.step import SISSStepper
    from siss_amd.unet import UNetEngine
    dev = torch.device("cuda", 0)
    sd = a.config == "sd15"
    if sd:
        from siss_amd.unet_cond import UNetCondEngine
        cfg = UNet2DConditionConfig.sd15()
        eng = UNetCondEngine(cfg, dev)
    else:
        cfg = UNet2DConfig.celebahq256() if a.config == "celebahq256" else UNet2DConfig(
            sample_size=64, block_out_channels=(128, 128, 256), down_block_types=("DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "AttnUpBlock2D", "UpBlock2D"))
        eng = UNetEngine(cfg, dev)
    eng.init_random(seed=42)
    names = list(eng.ps.specs)
    last_up = f"^up_blocks\\.{len(cfg.block_out_channels) - 1}\\."
    selections = {"attentions": "attentions", "last_up_block": last_up}
    if sd:
        selections = {"attn2": "attn2", **selections}
    B, hw, cin = a.batch, cfg.sample_size, cfg.in_channels
    g = torch.Generator(device=dev).manual_seed(42)
    cond = None
    if sd:
        ac = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2, 0)
        kw = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=750.0)
        x0 = (0.18215 * torch.randn(B, cin, hw, hw, generator=g, device=dev)).to(torch.bfloat16)
        a0 = (0.18215 * torch.randn(1, cin, hw, hw, generator=g, device=dev)).repeat(B, 1, 1, 1).to(torch.bfloat16)
        cond = {"encoder_hidden_states": torch.randn(1, 77, cfg.cross_attention_dim, generator=g, device=dev).repeat(B, 1, 1).to(torch.bfloat16)}
    else:
        ac = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32), 0)
        kw = dict(lr=5e-6, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6, scaling_norm=500.0)
        x0 = (torch.rand(B, cin, hw, hw, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        a0 = (torch.rand(1, cin, hw, hw, generator=g, device=dev) * 2 - 1).repeat(B, 1, 1, 1).to(torch.bfloat16)
    torch.cuda.manual_seed(1234)
    total_params = sum(int(sp.numel) for sp in eng.ps.specs.values())

    legs = {}

    def make(name, trainable, skip):
        """A stepper, its products / optimizer figures from one profiled eager step, and its captured step."""
        st = SISSStepper(eng, ac, lambd=0.5, train_batch_size=B, mixed_precision="bf16", trainable=trainable, **kw)
        eng.skip_frozen_wgrad = skip

        def one_step():
            noise = torch.randn(B, cin, hw, hw, device=dev, dtype=torch.bfloat16)
            t = torch.randint(999, 1000, (B,), device=dev)
            u = torch.rand(B, device=dev)
            st.micro_step(x0, a0, noise, t, u, cond)
        for _ in range(2):
            one_step()
        torch.cuda.synchronize()
        i0, d0 = eng.wgrads.issued, eng.wgrads.dropped
        lib.PROF = []
        one_step()
        torch.cuda.synchronize()
        prof, lib.PROF = lib.PROF, None
        floats = st.subset.floats if st.subset is not None else eng.ps.total
        opt = {}
        for rec in prof:
            if rec[0].startswith(("siss_grad_norms_scale", "siss_recombine_clip_adamw")):
                per = 8.0 if "norms" in rec[0] else 34.0
                ms = rec[1].elapsed_time(rec[2])
                opt[rec[0]] = {"ms": round(ms, 4), "bytes": per * floats, "of_8TBs": round(per * floats / (ms * 1e-3) / PEAK, 3)}
        info = {"trainable_params": st.trainable_counts()[0], "trainable_tensors": st.trainable_counts()[1],
                "trainable_share": round(st.trainable_counts()[0] / total_params, 5), "stretches": 0 if st.subset is None else len(st.subset.stretches),
                "products_described": eng.wgrads.issued - i0 + eng.wgrads.dropped - d0, "products_dropped": eng.wgrads.dropped - d0,
                "optimizer": opt, "ms_per_step": []}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one_step()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                one_step()
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        legs[name] = (st, graph, info)

    make("full", None, True)
    for sel, pat in selections.items():
        chosen = [n for n in names if re.search(pat, n)]
        for mode, skip in (("skip", True), ("keep", False)):
            make(f"{sel}/{mode}", chosen, skip)
    for _ in range(a.rounds):
        for name, (st, graph, info) in legs.items():
            graph.replay()
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.reps):
                graph.replay()
            s1.record()
            torch.cuda.synchronize()
            info["ms_per_step"].append(round(s0.elapsed_time(s1) / a.reps, 3))
            info["sclk"] = _clock() or "not recorded"
    res = {"tool": "bench_trainable", "device": torch.cuda.get_device_name(0), "config": a.config, "batch": B, "weights": "random-init",
           "dtype": "bf16", "parameters": total_params, "reps": a.reps, "rounds": a.rounds,
           "timing": "device events around `reps` replays of each leg's hipGraph, legs interleaved, one figure per round",
           "selections": selections, "legs": {k: v[2] for k, v in legs.items()}}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

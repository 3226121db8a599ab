#!/usr/bin/env python
"""The replayed SISS step with LoRA adapters on one GPU: prints ONE JSON line (and writes it with --out).

    python tools/bench_lora.py --config sd15 --batch 4 [--reps 10] [--rounds 2] [--out profiles/lora_sd15.json]
    python tools/bench_lora.py --config celebahq256 --batch 16

bf16, random-init weights (the times do not depend on them), the synthetic inputs of bench.py; no dataset.  Legs, each a stepper of
its own over ONE engine, its step captured into a hipGraph:

  * full            the full update (what bench.py times)
  * trainable       SISSStepper(trainable=the LoRA targets): the same weight-gradient products, the subset optimizer, full-size m / v
  * lora_r4/16/64   SISSStepper(lora=LoRAState(rank r)) on targets `attn[12]\\.to_(q|k|v|out\\.0)\\.weight` (SD) /
                    `attentions\\.\\d+\\.to_(q|k|v|out\\.0)\\.weight` (the pixel UNets)

Every leg is replayed --reps times between two device events, the legs interleaved, --rounds rounds: ms per step of every round are
reported; their spread is the run-to-run spread the differences are to be read against.  Beside the step times, each launch of the
update ALONE (--launch-reps back-to-back launches between two device events, after two warm-up launches): the full-buffer FlatAdamW.launch
of the full leg, and siss_lora_project / FlatAdamW.launch on the adapter buffer / siss_lora_merge of every LoRA leg, with the bytes
they move over the 8 TB/s of the data sheet (project reads dW of both sets TWICE -- once by row tiles for dB, once by column tiles for
dA: 16 B per target float; merge reads W0 and writes the master and its bf16 shadow: 10 B), and the bytes of optimizer state (m + v).
The shader clock is read after each leg's timed work.  One condition is checked and recorded, not enforced: the three LoRA launches
together take less time than the full-buffer FlatAdamW.launch they replace.

    python tools/bench_lora.py --config celebahq256 --batch 16 --conv-targets [--out profiles/lora_conv_celebahq256.json]
    python tools/bench_lora.py --config sd15 --batch 4 --conv-targets

--conv-targets puts the adapters on the 3x3 convolutions as well (deletion.lora.conv_targets; peft's Conv2d adapter): every resnet
conv1 / conv2 -- on the pixel UNets INSTEAD of the attention projections (nearly all of their parameters are convolutions), on SD
BESIDE them.  The launches timed alone are then the pair of each kind (siss_lora_project + siss_lora_project_conv, the two merges) as
LoRAState.project() / merge() issue them; a conv target's floats move like a linear target's (dW of both sets read twice, W0 read,
master and shadow written).  No condition is attached to these figures: a LoRA over every convolution reads every dW twice.
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
RANKS = (4, 16, 64)


def _clock():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        lines = [l.strip() for l in r.stdout.splitlines() if "sclk" in l.lower()]
        return lines[:1] or None
    except Exception:
        return None


def timed(fn, reps):
    """ms per call of `reps` back-to-back calls between two device events, after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(reps):
        fn()
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15", choices=["sd15", "celebahq256", "small"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--launch-reps", type=int, default=50, help="back-to-back launches of each update launch timed alone")
    ap.add_argument("--conv-targets", action="store_true",
                    help="adapters on every resnet conv1 / conv2 (pixel UNets: instead of the attention projections; sd15: beside them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py needs a GPU"
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from siss_amd.unet import UNetEngine
    dev = torch.device("cuda", 0)
    sd = a.config == "sd15"
    if sd:
        from siss_amd.unet_cond import UNetCondEngine
        cfg = UNet2DConditionConfig.sd15()
        eng = UNetCondEngine(cfg, dev)
        pattern = r"attn[12]\.to_(q|k|v|out\.0)\.weight"
    else:
        cfg = UNet2DConfig.celebahq256() if a.config == "celebahq256" else UNet2DConfig(
            sample_size=64, block_out_channels=(128, 128, 256), down_block_types=("DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "AttnUpBlock2D", "UpBlock2D"))
        eng = UNetEngine(cfg, dev)
        pattern = r"attentions\.\d+\.to_(q|k|v|out\.0)\.weight"
    eng.init_random(seed=42)
    targets = [n for n in eng.ps.specs if re.search(pattern, n)]
    conv_pattern, conv_targets = None, []
    if a.conv_targets:
        conv_pattern = r"resnets\.\d+\.conv[12]\.weight"
        conv_targets = [n for n in eng.ps.specs if re.search(conv_pattern, n)]
        assert conv_targets and all(eng.ps.specs[n].kind == "conv3" for n in conv_targets)
        if not sd:
            pattern, targets = None, []
    target_floats = sum(int(eng.ps.specs[n].numel) for n in targets + conv_targets)
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

    def make(name, **skw):
        st = SISSStepper(eng, ac, lambd=0.5, train_batch_size=B, mixed_precision="bf16", **skw, **kw)

        def one_step():
            noise = torch.randn(B, cin, hw, hw, device=dev, dtype=torch.bfloat16)
            t = torch.randint(999, 1000, (B,), device=dev)
            u = torch.rand(B, device=dev)
            st.micro_step(x0, a0, noise, t, u, cond)
        for _ in range(2):
            one_step()
        torch.cuda.synchronize()
        okw = dict(scaling_norm=kw["scaling_norm"])
        info = {"trainable_params": st.trainable_counts()[0], "trainable_tensors": st.trainable_counts()[1],
                "optimizer_state_bytes": 8 * st.opt.m.numel(), "ms_per_step": []}
        if st.lora is not None:
            lo = st.lora
            info["rank"], info["adapter_floats"], info["project_tiles"], info["merge_tiles"] = lo.rank, lo.L, lo.project_tiles, lo.merge_tiles
            info["adapter_bytes"] = 4 * lo.params
            if lo.conv_names:
                info["conv_project_tiles"], info["conv_merge_tiles"] = lo.conv_project_tiles, lo.conv_merge_tiles
            pm, om, mm = timed(lo.project, a.launch_reps), timed(lambda: st.opt.launch(lo.g, **okw), a.launch_reps), timed(lo.merge, a.launch_reps)
            info["launches_ms"] = {"siss_lora_project": round(pm, 4), "adamw_on_adapters": round(om, 4), "siss_lora_merge": round(mm, 4),
                                   "sum": round(pm + om + mm, 4)}
            info["rates_of_8TBs"] = {"siss_lora_project": round(16.0 * target_floats / (pm * 1e-3) / PEAK, 3),
                                     "siss_lora_merge": round(10.0 * target_floats / (mm * 1e-3) / PEAK, 3)}
            lo.merge()
        elif st.subset is None:
            info["launches_ms"] = {"flat_adamw_full_buffer": round(timed(lambda: st.opt.launch(eng.ps.grads, **okw), a.launch_reps), 4)}
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

    make("full")
    make("trainable", trainable=targets + conv_targets)
    for r in RANKS:
        make(f"lora_r{r}", lora=LoRAState(eng, targets, r, float(r), seed=0, conv_names=conv_targets))
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
    full_ms = legs["full"][2]["launches_ms"]["flat_adamw_full_buffer"]
    res = {"tool": "bench_lora", "device": torch.cuda.get_device_name(0), "config": a.config, "batch": B, "weights": "random-init",
           "dtype": "bf16", "parameters": total_params, "targets": pattern, "target_tensors": len(targets), "target_floats": target_floats,
           **({"conv_targets": conv_pattern, "conv_target_tensors": len(conv_targets)} if conv_targets else {}),
           "reps": a.reps, "rounds": a.rounds, "launch_reps": a.launch_reps,
           "timing": "device events around `reps` replays of each leg's hipGraph, legs interleaved, one figure per round; launches_ms: "
                     "`launch_reps` back-to-back eager launches between two device events after two warm-up launches",
           "project_variants": "ONE built: dW read twice (row tiles for dB, column tiles for dA, one launch); the read-once form was not built",
           "lora_launches_below_full_adamw": {k: bool(v[2]["launches_ms"]["sum"] < full_ms) for k, v in legs.items() if "rank" in v[2]},
           "legs": {k: v[2] for k, v in legs.items()}}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

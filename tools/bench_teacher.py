#!/usr/bin/env python
"""The teacher-target step (siss_amd/teacher.py, csrc/teacher.hip) against `double_forward_with_neg_del` on the same build: writes ONE
JSON (profiles/teacher.json).

    python tools/bench_teacher.py [--batch 4] [--iters 10] [--rounds 3] [--only sd15|tiny] [--out profiles/teacher.json]

Per network (the SD v1.5 UNet at 64 x 64 latents with a 77 x 768 prompt, and the small test configuration: 16 x 16, two blocks, a
64-wide prompt), random-init weights, bf16, B keep + B forget rows, in ONE process:

  * step_ms              a whole optimizer step, eager, for `double_forward_with_neg_del` (the yardstick) and for the four useful teacher
                         settings: esd and anchor, each with keep: noise and keep: teacher;
  * teacher_forward_ms   the teacher's forward alone, on the rows each setting gives it;
  * seed                 siss_teacher_seed against the same arithmetic written as eager torch ops on the same device and buffers;
  * teacher_bytes        what the frozen copy holds (f32 master + bf16 operand copy; no gradient sets, no optimizer state).

Every leg is timed between two device events over --iters calls after a warm-up, the legs interleaved over --rounds rounds; every
round's figure is reported and a leg's spread over the rounds is what its differences are to be read against.  No threshold is attached
to any figure: where torch is faster, the JSON says so.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = [("esd", "noise"), ("esd", "teacher"), ("anchor", "noise"), ("anchor", "teacher")]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def spread(xs):
    return dict(ms=[round(x, 4) for x in xs], min=round(min(xs), 4), max=round(max(xs), 4), median=round(sorted(xs)[len(xs) // 2], 4))


def configs():
    from siss_amd.config import UNet2DConditionConfig
    tiny = UNet2DConditionConfig(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(64, 128),
                                 down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
                                 layers_per_block=1, attention_head_dim=2, cross_attention_dim=64)
    return {"sd15": (UNet2DConditionConfig.sd15(), 64, 768), "tiny": (tiny, 16, 64)}


def torch_seed(pred, noise, teach, B, keep, forget, eta, scale, cot):
    """siss_teacher_seed's arithmetic as eager torch ops (keep: noise | teacher; the same buffers): cot and the per-row sums."""
    k0 = B if keep == "teacher" else 0
    k = teach[k0:k0 + B]
    yf = k
    if forget == "esd":
        u = teach[k0 + B:k0 + 2 * B]
        yf = u - eta * (k - u)
    y = torch.cat([noise.float() if keep == "noise" else teach[:B], yf], 0)
    d = pred - y
    torch.mul(d, 2.0 * scale, out=cot)
    return d.double().square().flatten(1).sum(1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=[None, "sd15", "tiny"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_teacher.py needs a GPU"
    from siss_amd import lib
    from siss_amd.loss import teacher_seed
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.step import SISSStepper
    from siss_amd.teacher import Teacher, parse_teacher, row_layout
    from siss_amd.unet_cond import UNetCondEngine
    dev = torch.device("cuda", 0)
    B = a.batch
    ac = DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear").alphas_cumprod
    result = dict(batch=B, iters=a.iters, rounds=a.rounds, device=torch.cuda.get_device_name(0), dtype="bf16", networks={}, not_measured=[])
    for name, (cfg, hw, X) in configs().items():
        if a.only and name != a.only:
            result["not_measured"].append(f"{name}: left out by --only")
            continue
        gen = torch.Generator().manual_seed(0)
        rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
        x0, a0, noise = rnd(B, 4, hw, hw), rnd(1, 4, hw, hw).repeat(B, 1, 1, 1), rnd(B, 4, hw, hw)
        t, u = torch.randint(0, 1000, (B,), generator=gen).to(dev), torch.rand(B, generator=gen).to(dev)
        prompt, empty, anchor = rnd(1, 77, X), rnd(1, 77, X), rnd(1, 77, X)
        cond = {"encoder_hidden_states": prompt.repeat(B, 1, 1)}
        eng = UNetCondEngine(cfg, dev)
        eng.init_random(seed=1)
        teacher = Teacher(eng).set_embeddings(empty=empty, anchor=anchor)
        kw = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=750.0, train_batch_size=B, mixed_precision="bf16")
        out = dict(sample=hw, prompt=[77, X], params=sum(int(sp.numel) for sp in eng.ps.specs.values()), teacher_bytes=teacher.nbytes,
                   student_bytes=int(eng.ps.flat.numel() * 4 + eng.ps.shadow.numel() * 2 + eng.ps.grads.numel() * 4))
        # (one stepper at a time over the engine: each owns m and v of the whole buffer)
        fwd, step_times = {}, {}

        def run(stp):
            stp.step(x0, a0, noise, t, u, cond)
        order = [("double_forward_with_neg_del", None)] + [(f"{f}/{k}", parse_teacher(dict(forget=f, keep=k, anchor_prompt="x" if f == "anchor" else None)))
                                                          for f, k in SETTINGS]
        for leg, tc in order:
            stp = SISSStepper(eng, ac, loss_fn="teacher_target" if tc else "double_forward_with_neg_del",
                              **(dict(teacher=teacher, teacher_cfg=tc) if tc else {}), **kw)
            run(stp); run(stp)
            torch.cuda.synchronize()
            step_times[leg] = [timed(lambda: run(stp), a.iters) for _ in range(a.rounds)]
            if tc:
                lay = row_layout(tc.keep, tc.forget, B)
                xk = x0.to(torch.bfloat16)
                f = lambda: teacher.predict(tc, xk, xk, t, cond)
                f()
                torch.cuda.synchronize()
                fwd[leg] = dict(rows=lay["Rt"], **spread([timed(f, a.iters) for _ in range(a.rounds)]))
            del stp
            torch.cuda.empty_cache()
        base = sorted(step_times["double_forward_with_neg_del"])[a.rounds // 2]
        out["step_ms"] = {leg: dict(spread(ts), over_double_forward=round(sorted(ts)[a.rounds // 2] / base, 4)) for leg, ts in step_times.items()}
        out["teacher_forward_ms"] = fwd
        # the seed kernel against eager torch, on [2 B, chw] rows
        chw = 4 * hw * hw
        pred, teach = rnd(2 * B, chw), rnd(3 * B, chw)
        nz = noise.flatten(1).to(torch.bfloat16)
        cot, cot_t = torch.empty_like(pred), torch.empty_like(pred)
        sums = torch.empty(2 * B, device=dev)
        partials = torch.empty(lib.query("siss_teacher_partials_words", 2 * B, chw), dtype=torch.float64, device=dev)
        seed = {}
        for fgt, keep in SETTINGS:
            tc = parse_teacher(dict(forget=fgt, keep=keep, guidance=1.0, anchor_prompt="x" if fgt == "anchor" else None))
            hipf = lambda: teacher_seed(pred, nz, teach, B, tc, 0.125, cot=cot, sums=sums, partials=partials)
            torf = lambda: torch_seed(pred, nz, teach, B, keep, fgt, 1.0, 0.125, cot_t)
            s1, s2 = hipf(), torf()
            torch.cuda.synchronize()
            reps = 200
            hs, ts = zip(*[(timed(hipf, reps), timed(torf, reps)) for _ in range(a.rounds)])
            seed[f"{fgt}/{keep}"] = dict(hip=spread(hs), torch_eager=spread(ts), hip_over_torch=round(sorted(hs)[a.rounds // 2] / sorted(ts)[a.rounds // 2], 4),
                                         max_abs_cot_diff=float((cot - cot_t).abs().max()), max_rel_sum_diff=float(((s1 - s2).abs() / s2).max()))
        out["seed"] = dict(rows=2 * B, chw=chw, calls_per_timing=200, settings=seed)
        result["networks"][name] = out
        del eng, teacher
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

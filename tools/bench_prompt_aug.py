#!/usr/bin/env python
"""Time one iteration of the augmented-prompt optimisation (siss_amd/prompt_aug.py) at SD v1.5 size, n = 1 and n = 4 text samples:
the text forward, UNetCondEngine.context_vjp (the data-gradient-only backward with the text gradient), the loss / cotangent launch
pair and the embedding update -- and, beside them, backward(nsets=1) of the same forward on the same build (what the iteration would
cost without the data-only mode; its gradient fill is outside the timed region) and the 16 context products + their sum alone (what
context_vjp adds to the data-only backward).  Eager launches (capturing the iteration is future work), device time between events, median of
--reps after --warmup.  One JSON line per batch; --out appends them to a file under profiles/.

    python tools/bench_prompt_aug.py [--n 1 4] [--reps 5] [--warmup 2] [--out profiles/prompt_aug_sd15.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def ctx_products(eng, n, L, X):
    """The launches context_vjp adds to the data-only backward, alone: one siss_ctx_dgrad per cross-attention site at the site's
    width (operands of the engine's element type, the values do not matter) and the one siss_ctx_reduce over the slabs."""
    import torch
    from siss_amd import lib
    widths = [eng.ps.specs[k].ref_shape[0] for k in eng.ps.specs if k.endswith(".attn2.to_k.weight")]
    rows = n * L
    dkv = {C: torch.zeros(rows, 2 * C, dtype=eng.adt, device=eng.device) for C in set(widths)}
    w = {C: torch.zeros(2, X, C, dtype=eng.adt, device=eng.device) for C in set(widths)}
    slabs = torch.zeros(len(widths), rows, X, device=eng.device)
    out = torch.zeros(L, X, device=eng.device)

    def run():
        for s, C in enumerate(widths):
            lib.call("siss_ctx_dgrad", dkv[C][:, :C], dkv[C][:, C:], 2 * C, w[C][0], w[C][1], slabs[s], rows, C, X, int(eng.f32))
        lib.call("siss_ctx_reduce", slabs, out, len(widths), n, L * X, 1)
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from siss_amd import prompt_aug
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.unet_cond import UNetCondEngine
    dev = torch.device("cuda", 0)
    eng = UNetCondEngine(UNet2DConditionConfig.sd15(), dev)
    eng.init_random(seed=0)
    eng.refresh_weights(cast_shadow=True)
    g = torch.Generator(device=dev).manual_seed(0)
    L, X = 77, eng.cfg.cross_attention_dim
    lines = []
    for n in a.n:
        z = torch.randn(n, 4, 64, 64, device=dev, generator=g)
        t = torch.full((n,), 981, dtype=torch.long, device=dev)
        e = torch.randn(L, X, device=dev, generator=g)
        e0, m, v, grad = e.clone(), torch.zeros_like(e), torch.zeros_like(e), torch.empty_like(e)
        dist = torch.zeros(L, dtype=torch.float64, device=dev)
        e_n = e.unsqueeze(0).repeat(n, 1, 1).contiguous()
        u = eng.forward(z, t, torch.randn(n, L, X, device=dev, generator=g)).clone()
        cot, loss = torch.empty_like(z), torch.zeros(1, device=dev)
        p = eng.forward(z, t, e_n)
        prompt_aug.noise_norm_cot(p, u, cot, loss)
        rec = {"what": "prompt_aug iteration, SD v1.5, eager", "n": n,
               "text_forward_ms": timed(lambda: eng.forward(z, t, e_n), a.reps, a.warmup),
               "context_vjp_ms": timed(lambda: eng.context_vjp(cot, out=grad, reduce=True), a.reps, a.warmup),
               "loss_cot_ms": timed(lambda: prompt_aug.noise_norm_cot(p, u, cot, loss), a.reps, a.warmup),
               "update_ms": timed(lambda: prompt_aug.embed_update(e, e0, grad, m, v, dist, 1, 0.1, 0.5, 0.0), a.reps, a.warmup)}

        # backward(nsets=1) accumulates into the gradient buffer: filled once, outside the timed region
        eng.zero_grad()
        rec["backward_nsets1_ms"] = timed(lambda: eng.backward(cot, nsets=1), a.reps, a.warmup)
        rec["ctx_products_ms"] = timed(ctx_products(eng, n, L, X), a.reps, a.warmup)
        rec["iteration_ms"] = rec["text_forward_ms"] + rec["context_vjp_ms"] + rec["loss_cot_ms"] + rec["update_ms"]
        rec = {k: (round(val, 4) if isinstance(val, float) else val) for k, val in rec.items()}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return lines


if __name__ == "__main__":
    main()

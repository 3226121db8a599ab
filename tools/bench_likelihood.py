#!/usr/bin/env python
"""Forget-set likelihood (bits/dim on the probability-flow ODE) on one GPU: prints ONE JSON line.

    python tools/bench_likelihood.py [--reps 20] [--no-ref]

Cases: MNIST 28 x 28 (config/train_tshirt_mnist.yaml's unet: the reference's T-shirt case) and CelebA-HQ 256 x 256
(google/ddpm-celebahq-256's architecture), B = 1, the f32 engine, RANDOM-INIT weights.  Per case:
  * fe_ms_graph / fe_ms_eager: one function evaluation (forward + input VJP + drift / divergence) replayed from the captured
    hipGraph / launched eagerly;
  * fused_us: siss_pflow_drift_div + siss_slab_rowsum_f64 alone;
  * eval_s / nfe: one full bits/dim evaluation (device RK45, rtol = atol = 1e-5; CelebA-HQ only with --celeb-full);
  * with scipy importable (and not --no-ref): ref_fe_ms / ref_eval_s / ref_nfe -- the reference-shaped composition: oracle.unet in
    torch f32 on this GPU with the autograd divergence, scipy's solve_ivp on the host, a numpy round trip per evaluation
    (MNIST only; at 256 x 256 it would take hours).
nfe of random-init weights is NOT representative of a trained model's: the per-evaluation times are the comparable numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _reference(cfg, sd, x, eps, sde):
    """The reference's composition (metrics/song_likelihood/likelihood.py) on oracle.unet in f32: (ms per evaluation, s, nfe)."""
    from scipy import integrate
    from oracle.unet import OracleUNet2D, UNetConfig
    net = OracleUNet2D(UNetConfig(**vars(cfg))).cuda().float()
    net.load_state_dict({k: v.float() for k, v in sd.items()})
    net.requires_grad_(False)
    shape, dev = tuple(x.shape), x.device
    table = sde.sqrt_1m_alphas_cumprod.to(dev)
    times = []

    def drift_fn(xx, vec_t):
        beta_t = sde.beta_0 + vec_t * (sde.beta_1 - sde.beta_0)
        drift = -0.5 * beta_t[:, None, None, None] * xx
        labels = vec_t * (sde.N - 1)
        score = -net(xx, labels.long())[0] / table[labels.long()][:, None, None, None]
        return drift - torch.sqrt(beta_t)[:, None, None, None] ** 2 * score * 0.5

    def ode_func(t, y):
        t0 = time.perf_counter()
        sample = torch.from_numpy(y[:-shape[0]].reshape(shape)).to(dev).type(torch.float32)
        vec_t = torch.ones(shape[0], device=dev) * t
        with torch.enable_grad():
            sample.requires_grad_(True)
            d = drift_fn(sample, vec_t)
            g = torch.autograd.grad(torch.sum(d * eps), sample)[0]
        div = torch.sum(g * eps, dim=(1, 2, 3))
        out = np.concatenate([d.detach().cpu().numpy().reshape(-1), div.cpu().numpy().reshape(-1)])
        times.append(time.perf_counter() - t0)
        return out

    init = np.concatenate([x.cpu().numpy().reshape(-1), np.zeros(shape[0])])
    t0 = time.perf_counter()
    sol = integrate.solve_ivp(ode_func, (1e-5, 1.0), init, rtol=1e-5, atol=1e-5, method="RK45")
    return 1e3 * float(np.median(times[2:] or times)), time.perf_counter() - t0, int(sol.nfev)


def case(name, cfg, reps, with_ref, full=True):
    from siss_amd import lib
    from siss_amd.likelihood import LikelihoodEvaluator, PFlowODE, VPSDE
    from siss_amd.unet import UNetEngine
    dev = torch.device("cuda", 0)
    eng = UNetEngine(cfg, dev, dtype=torch.float32)
    sd = eng.init_random(seed=0)
    sde = VPSDE()
    shape = (1, cfg.in_channels, cfg.sample_size, cfg.sample_size)
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand(shape, device=dev, generator=g) * 2 - 1).contiguous()
    eps = torch.randint(0, 2, shape, device=dev, generator=g).float() * 2 - 1
    out = {}
    for graph in (True, False):
        ode = PFlowODE(eng, sde, shape, use_graph=graph)
        ode.xs.copy_(x)
        ode.eps.copy_(eps)
        out["fe_ms_graph" if graph else "fe_ms_eager"] = round(_time(lambda: ode(0.5), reps), 4)
    ode.set_time(0.5)
    out["fused_us"] = round(1e3 * _time(lambda: (
        lib.call("siss_pflow_drift_div", ode.xs, ode.eng._buf("pred", shape), ode.v, ode.eps, ode.par, ode.out, ode.partials,
                 1, ode.chw, ode.nblk),
        lib.call("siss_slab_rowsum_f64", ode.partials, ode.out[ode.n:], 1, ode.nblk)), reps * 10), 2)
    if not full:
        return out
    ev = LikelihoodEvaluator(sde)
    ev.evaluate_likelihood(eng, x, epsilon=eps)                  # (capture)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bpd, _, nfe = ev.evaluate_likelihood(eng, x, epsilon=eps)
    torch.cuda.synchronize()
    out.update(eval_s=round(time.perf_counter() - t0, 3), nfe=int(nfe), bpd=round(float(bpd[0]), 5))
    if with_ref:
        ms, s, n = _reference(cfg, sd, x, eps, sde)
        out.update(ref_fe_ms=round(ms, 3), ref_eval_s=round(s, 2), ref_nfe=n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--celeb-full", action="store_true", help="also one full CelebA-HQ evaluation (random-init weights: thousands of "
                    "function evaluations, minutes)")
    a = ap.parse_args()
    from siss_amd.config import UNet2DConfig
    try:
        import scipy.integrate  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    res = {"metric": "likelihood_bpd", "engine": "f32", "batch": 1, "weights": "random-init (nfe not representative)",
           "device": torch.cuda.get_device_name(0)}
    res["mnist28"] = case("mnist28", UNet2DConfig.mnist_tshirt(), a.reps, have_scipy and not a.no_ref)
    res["celebahq256"] = case("celebahq256", UNet2DConfig.celebahq256(), max(2, a.reps // 5), False, full=a.celeb_full)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

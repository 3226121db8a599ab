"""The host side of the augmented prompt (no GPU): tests/prompt_aug_ref.py -- the restatement the GPU tests compare against -- held
to finite differences and to the properties the method's description states, and the tool's file against its consumer."""
import os
import sys

import pytest
import torch

import prompt_aug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@pytest.fixture(scope="module")
def small():
    """a network smaller than the GPU cases (two levels of 32 / 64 channels, 8 x 8 latents, 5 tokens of width 16), f64"""
    from oracle.unet_cond import OracleUNet2DCondition, UNetCondConfig
    torch.manual_seed(3)
    oc = UNetCondConfig.tiny(ch=(32, 64), heads=2, cross_dim=16, sample_size=8, in_channels=4)
    oc.layers_per_block = 1
    net = OracleUNet2DCondition(oc).eval().double()
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 4, 8, 8, generator=g, dtype=F64)
    e, e_neg = torch.randn(1, 5, 16, generator=g, dtype=F64), torch.randn(1, 5, 16, generator=g, dtype=F64)
    return net, z, torch.tensor([981, 981]), e, e_neg


def test_gradient_agrees_with_central_finite_differences(small):
    net, z, t, e, e_neg = small
    _, g = R.loss_grad(net, z, t, e, e_neg)
    scale = float(g.abs().max())
    h = 1e-5
    for (l, x) in [(0, 0), (1, 3), (2, 15), (4, 7), (3, 0)]:
        d = torch.zeros_like(e)
        d[0, l, x] = h
        with torch.no_grad():
            fd = (R.noise_norm(net, z, t, e + d, e_neg=e_neg)[0] - R.noise_norm(net, z, t, e - d, e_neg=e_neg)[0]) / (2 * h)
        assert abs(float(fd) - float(g[0, l, x])) <= 1e-5 * scale, (l, x, float(fd), float(g[0, l, x]), scale)


def test_row_zero_takes_the_decoupled_decay_only(small):
    net, z, t, e, e_neg = small
    k, lr = 3, 0.1
    out, tr = R.aug_prompt(net, z, t, e, e_neg, lr=lr, optim_iters=k)
    assert tr["iterations"] == k
    want = e[0, 0].clone()
    for _ in range(k):
        want = want * (1 - lr * 1e-2)
    assert torch.equal(out[0, 0], want)
    assert float((out[0, 1:] - e[0, 1:]).abs().min()) > 0.5 * lr          # Adam's first steps: every other coordinate moved by ~lr


def test_target_loss_stops_before_the_update(small):
    net, z, t, e, e_neg = small
    first = R.aug_prompt(net, z, t, e, e_neg, optim_iters=1)[1]["noise_norm"][0]
    out, tr = R.aug_prompt(net, z, t, e, e_neg, optim_iters=4, target_loss=first * 1.5)
    assert tr["stopped_early"] and tr["iterations"] == 0 and tr["noise_norm"] == [first]
    assert torch.equal(out, e)
    _, tr = R.aug_prompt(net, z, t, e, e_neg, optim_iters=2, target_loss=first * 1e-3)
    assert not tr["stopped_early"] and tr["iterations"] == 2


def test_penalty_switches_on_from_the_second_iteration(small):
    """optim_epsilon = 0: in the first iteration the distance is 0, which is not > 0"""
    net, z, t, e, e_neg = small
    _, tr = R.aug_prompt(net, z, t, e, e_neg, optim_iters=3, optim_epsilon=0.0, alpha=0.5)
    assert tr["penalised"] == [False, True, True]


def test_end_to_end_seed_keeps_enough_coordinates():
    """The GPU end-to-end test compares only coordinates whose reference gradient exceeds 1e-3 of the largest in every iteration;
    with its seed that must keep at least 90 % of the coordinates of rows 1.."""
    net, _ = R.seeded_oracle("tiny", R.AUG_SEED)
    z, e, e_neg = R.aug_inputs("tiny")
    t = torch.full((R.AUG_N,), R.AUG_T)
    _, tr = R.aug_prompt(net, z.double(), t, e.double(), e_neg.double(), lr=R.AUG_LR, optim_iters=R.AUG_ITERS)
    keep = R.kept_coordinates(tr)
    share = float(keep[1:].double().mean())
    print(f"\nkept coordinates of rows 1..: {share:.4f}; noise norms {tr['noise_norm']}")
    assert share >= 0.9, share
    # the early-stop case places target_loss between the first two norms, clear of both by the bf16 engine's 3e-2 tolerance
    target = R.early_stop_target(tr["noise_norm"][0], tr["noise_norm"][1])
    assert target is not None and tr["noise_norm"][1] * (1 + R.BF16_NORM_REL) < target < tr["noise_norm"][0] * (1 - R.BF16_NORM_REL)
    assert R.early_stop_target(1.0, 0.951) is None and abs(R.early_stop_target(1.0, 0.8) - 0.897) < 1e-12


def test_saved_embedding_loads_through_the_task(tmp_path):
    sys.path.insert(0, ROOT)
    from siss_amd import hydra_lite as H
    from siss_amd.prompt_aug import save_aug_prompt
    e = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(0))
    path, side = save_aug_prompt(str(tmp_path / "aug" / "prompt.pt"), e, {"noise_norm": [3.0, 2.0], "iterations": 2},
                                 token_grads=torch.arange(77.0))
    import json
    rec = json.load(open(side))
    assert rec["shape"] == [1, 77, 64] and rec["noise_norm"] == [3.0, 2.0] and len(rec["token_grad_norms"]) == 77
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"), ["pretrained_model_name_or_path=/nonexistent", "using_augmented_prompt=true"])
    cfg.validation_prompts = [path]
    cfg.unet = dict(cross_attention_dim=64)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    got = task._prompt_embedding(cfg.validation_prompts[0], torch.device("cpu"))
    assert got.dtype == torch.float32 and torch.equal(got, e)


# ---------------------------------------------------------------- the loop's wiring, launchers and engine emulated on the host
class _HostEngine:
    """forward / context_vjp of the HIP engine's surface on a torch network (f64 inside, f32 at the surface), counting its calls"""

    def __init__(self, net):
        self.net, self.calls = net, []

    def refresh_weights(self, **kw):
        pass

    def forward(self, x, t, e):
        self.calls.append(("forward", int(x.shape[0])))
        self._e = e.detach().double().requires_grad_(True)
        with torch.enable_grad():
            self._out = self.net(x.double(), t, self._e)[0]
        return self._out.detach().float()

    def context_vjp(self, cot, out=None, reduce=False):
        self.calls.append(("context_vjp", int(cot.shape[0])))
        (g,) = torch.autograd.grad(self._out, self._e, cot.double(), retain_graph=True)
        out.copy_((g.sum(0) if reduce else g).float())
        return out


def _host_sampler(monkeypatch, net):
    from siss_amd import prompt_aug as PA
    from siss_amd.sd_sampler import SDSampler

    def noise_norm_cot(p, u, cot, loss, partials=None):
        d = p.double() - u.double()
        n = d.square().sum().sqrt()
        loss.copy_(n.float().reshape(1))
        cot.copy_((d / n if float(n) > 0 else torch.zeros_like(d)).float())
        return cot

    def embed_update(e, e0, g, m, v, dist, step, lr, alpha=0.5, optim_epsilon=None, betas=PA.ADAMW_BETAS, eps=PA.ADAMW_EPS,
                     weight_decay=PA.ADAMW_WEIGHT_DECAY):
        L = e.shape[0]
        geff = g.double().clone()
        if optim_epsilon is not None:
            d = (e.double() - e0.double()).square().sum(-1).sqrt()
            dist[:L] = d
            if float(d[1:].mean()) > optim_epsilon:
                unit = torch.where(d[:, None] > 0, (e.double() - e0.double()) / d[:, None].clamp_min(1e-300), torch.zeros_like(geff))
                geff = alpha * geff + (1 - alpha) / (L - 1) * unit
        geff[0] = 0
        bc1, bc2s = PA.bias_corrections(step, betas)
        p = e.double() * (1 - lr * weight_decay)
        m2 = m.double() + (geff - m.double()) * (1 - betas[0])
        v2 = v.double() * betas[1] + geff * geff * (1 - betas[1])
        p = p - lr / bc1 * m2 / (v2.sqrt() / bc2s + eps)
        e.copy_(p.float()); m.copy_(m2.float()); v.copy_(v2.float())

    def cfg_ddim_step(eps, x, out, coeffs, guidance, clip=0.0, norms=None):
        sa, sb, pa, pb = coeffs
        u, p = eps.chunk(2)
        ee = u + guidance * (p - u)
        out.copy_(pa * (x - sb * ee) / sa + pb * ee)
        return out
    monkeypatch.setattr(PA, "noise_norm_cot", noise_norm_cot)
    monkeypatch.setattr(PA, "embed_update", embed_update)
    monkeypatch.setattr(PA, "cfg_ddim_step", cfg_ddim_step)
    eng = _HostEngine(net)
    unet = type("U", (), {})()
    unet.engine, unet.device = eng, torch.device("cpu")
    unet.config = type("C", (), dict(in_channels=4, sample_size=8))()
    return SDSampler(unet, use_graph=False), eng, cfg_ddim_step


@pytest.mark.parametrize("optim_epsilon", [None, 0.0], ids=["plain", "penalty"])
def test_loop_wiring_with_emulated_launchers(small, monkeypatch, optim_epsilon):
    """siss_amd/prompt_aug.py's loop against the restatement with the engine and the three launchers emulated by torch on the host:
    the order of the forwards (u once, the text forward last before every context_vjp), the step counter, the penalty's arguments,
    the early stop and the trace."""
    net, z, t, e, e_neg = small
    s, eng, _ = _host_sampler(monkeypatch, net)
    kw = dict(prompt_embeds=e.float(), negative_prompt_embeds=e_neg.float(), latents=z.float(), num_images_per_prompt=2,
              height=64, width=64, lr=0.1, optim_iters=3, optim_epsilon=optim_epsilon, return_trace=True)
    ref_e, ref_tr = R.aug_prompt(net, z.float().double(), t, e.float().double(), e_neg.float().double(), lr=0.1, optim_iters=3,
                                 optim_epsilon=optim_epsilon)
    out, tr = s.aug_prompt(**kw)
    assert eng.calls == [("forward", 2)] + [("forward", 2), ("context_vjp", 2)] * 3
    assert tr["iterations"] == 3 and not tr["stopped_early"] and tr["step"] == 0 and tr["timestep"] == 981
    assert all(abs(a - b) <= 1e-5 * b for a, b in zip(tr["noise_norm"], ref_tr["noise_norm"])), (tr["noise_norm"], ref_tr["noise_norm"])
    keep = R.kept_coordinates(ref_tr)
    assert float((out[0].double() - ref_e[0]).abs()[keep].max()) <= 1e-3 and tuple(out.shape) == (1, 5, 16)
    # early stop between the first two norms: one update
    eng.calls.clear()
    out2, tr2 = s.aug_prompt(target_loss=0.5 * (ref_tr["noise_norm"][0] + ref_tr["noise_norm"][1]), **kw)
    assert ref_tr["noise_norm"][1] < ref_tr["noise_norm"][0]
    assert tr2["stopped_early"] and tr2["iterations"] == 1 and len(tr2["noise_norm"]) == 2
    assert eng.calls == [("forward", 2), ("forward", 2), ("context_vjp", 2), ("forward", 2)]


def test_text_cond_grad_wiring_with_emulated_launchers(small, monkeypatch):
    net, z, t, e, e_neg = small
    s, eng, ddim = _host_sampler(monkeypatch, net)
    kw = dict(prompt_embeds=e.float(), negative_prompt_embeds=e_neg.float(), latents=z.float(), num_images_per_prompt=2, height=64, width=64)
    got = s.get_text_cond_grad(target_steps=[0], **kw)
    ref = R.token_grad_norms(net, z.float().double(), t, e.float().double(), e_neg.float().double())
    assert tuple(got.shape) == (5,) and float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert eng.calls == [("forward", 2), ("forward", 2), ("context_vjp", 2)]
    both, tr = s.get_text_cond_grad(target_steps=[0, 1], return_trace=True, **kw)
    assert torch.equal(tr["per_step"][0], got) and torch.equal(both, torch.stack(tr["per_step"]).mean(0))
    zf, n = z.float(), 2
    u = eng.forward(zf, t, e_neg.float().repeat(n, 1, 1))
    p = eng.forward(zf, t, e.float().repeat(n, 1, 1))
    x1 = ddim(torch.cat([u, p]), zf, torch.empty_like(zf), s.scheduler.coeffs(981), 7.5)
    assert torch.equal(tr["latents"][0], zf) and torch.equal(tr["latents"][1], x1)
    t1 = torch.full((n,), s.scheduler.set_timesteps(50)[1])
    ref1 = R.token_grad_norms(net, x1.double(), t1, e.float().double(), e_neg.float().double())
    assert float((tr["per_step"][1].double() - ref1).abs().max()) <= 1e-5 * float(ref1.abs().max())
    for f in (s.aug_prompt, s.get_text_cond_grad):
        with pytest.raises(NotImplementedError, match="eta"):
            f(eta=0.5, **kw)
        with pytest.raises(NotImplementedError, match="prompt_embeds"):
            f(prompt="a photo", **kw)
        with pytest.raises(ValueError, match="guidance"):
            f(guidance_scale=1.0, **kw)
        with pytest.raises(ValueError, match="target_steps"):
            f(target_steps=[50], **kw)


def test_guided_advance_to_a_later_target_step(small, monkeypatch):
    """target_steps=[1]: the latents first take one DDIM step under guidance with the ORIGINAL embedding -- one forward over the 2n
    batch, uncond rows first, through the sampler's own evaluator -- and the optimisation then runs at the second timestep; and
    get_text_cond_grad with a gap before its target step advances the same way.  The sampler's evaluator is dropped afterwards."""
    net, z, t, e, e_neg = small
    s, eng, ddim = _host_sampler(monkeypatch, net)
    kw = dict(prompt_embeds=e.float(), negative_prompt_embeds=e_neg.float(), latents=z.float(), num_images_per_prompt=2, height=64, width=64)
    out, tr = s.aug_prompt(target_steps=[1, 3], lr=0.1, optim_iters=2, return_trace=True, **kw)
    assert eng.calls == [("forward", 4), ("forward", 2)] + [("forward", 2), ("context_vjp", 2)] * 2
    steps = s.scheduler.set_timesteps(50)
    assert tr["step"] == 1 and tr["timestep"] == steps[1] == 961 and s._ev is None
    # the same by hand: one guided step from the restatement's two predictions, then the restatement at the second timestep
    zd, ed, nd = z.float().double(), e.float().double(), e_neg.float().double()
    with torch.no_grad():
        u0, p0 = net(zd, t, nd.repeat(2, 1, 1))[0], net(zd, t, ed.repeat(2, 1, 1))[0]
    z1 = ddim(torch.cat([u0, p0]), zd, torch.empty_like(zd), s.scheduler.coeffs(steps[0]), 7.5)
    t1 = torch.full((2,), steps[1])
    ref_e, ref_tr = R.aug_prompt(net, z1, t1, ed, nd, lr=0.1, optim_iters=2)
    assert all(abs(a - b) <= 1e-5 * b for a, b in zip(tr["noise_norm"], ref_tr["noise_norm"])), (tr["noise_norm"], ref_tr["noise_norm"])
    assert float((out[0].double() - ref_e[0]).abs()[R.kept_coordinates(ref_tr)].max()) <= 1e-3
    eng.calls.clear()
    got = s.get_text_cond_grad(target_steps=[1], **kw)
    assert eng.calls == [("forward", 4), ("forward", 2), ("forward", 2), ("context_vjp", 2)]
    ref = R.token_grad_norms(net, z1, t1, ed, nd)
    assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    with s.holding_graphs():                               # inside the block the evaluator is kept for the next call
        s.get_text_cond_grad(target_steps=[1], **kw)
        assert s._ev is not None
    assert s._ev is None

"""Host reference of the prompt-embedding gradients and the augmented prompt (test infrastructure only): the semantics of
``SDSampler.aug_prompt`` / ``get_text_cond_grad`` restated in plain torch over a torch network called as ``net(x, t, ctx)[0]``
(oracle.unet_cond.OracleUNet2DCondition), with autograd and ``torch.optim.AdamW``, in whatever dtype the network and the inputs have
(f64 for the parity tests).  Written from the description of the method, not from any implementation:

    e_neg, e : [1, L, X] the empty prompt's and the prompt's embedding;  z : [n, 4, h, w] latents at the target step;  t : [n] ints
    loss(e) = || net(z, t, e.repeat(n)) - net(z, t, e_neg.repeat(n)) ||_2   over ALL n * chw elements (one scalar)
    per iteration: if optim_epsilon is set and mean_{r >= 1} ||e0_r - e_r||_2 > optim_epsilon: loss <- alpha loss + (1 - alpha) mean;
                   if target_loss is set and the NOISE NORM <= target_loss: stop before the update;
                   grad = d loss / d e, row 0 zeroed; AdamW(lr, defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2) step.
"""
import torch

# the two SD-shaped networks of tests/test_hip_unet_cond.py (CASES there)
CASES = {
    "tiny": dict(ch=(64, 128), heads=2, cross_dim=64, sample_size=16, layers=2),
    "sd_widths": dict(ch=(320, 640), heads=8, cross_dim=768, sample_size=16, layers=1),
}
# The end-to-end case's seed: the SMALLEST seed >= 0 at which the f64 restatement alone (tests/test_prompt_aug_host.py checks both) keeps at
# least 90 % of the coordinates of rows 1.. (kept_coordinates) and leaves room for early_stop_target between its first two noise norms.
AUG_SEED = 1
BF16_NORM_REL = 3e-2        # the bf16 engine's noise norm is held to this, relative, against the f64 trace
AUG_N, AUG_ITERS, AUG_LR, AUG_T = 2, 3, 0.1, 981     # (981: the first of 50 "leading" DDIM steps with steps_offset 1)


def configs(case):
    """(siss_amd UNet2DConditionConfig, oracle UNetCondConfig) of a case."""
    from siss_amd.config import UNet2DConditionConfig
    from oracle.unet_cond import UNetCondConfig
    c = CASES[case]
    oc = UNetCondConfig.tiny(ch=c["ch"], heads=c["heads"], cross_dim=c["cross_dim"], sample_size=c["sample_size"], in_channels=4)
    oc.layers_per_block = c["layers"]
    kw = {k: getattr(oc, k) for k in ("sample_size", "in_channels", "out_channels", "block_out_channels", "down_block_types",
                                      "up_block_types", "layers_per_block", "attention_head_dim", "cross_attention_dim",
                                      "norm_num_groups", "norm_eps", "downsample_padding", "flip_sin_to_cos", "freq_shift")}
    return UNet2DConditionConfig(**kw), oc


def seeded_oracle(case, seed, dtype=torch.float64):
    """The oracle network of a case with torch's default initialisation under torch.manual_seed(seed); its f32 state dict is what
    the HIP engine loads."""
    from oracle.unet_cond import OracleUNet2DCondition
    torch.manual_seed(int(seed))
    net = OracleUNet2DCondition(configs(case)[1]).eval()
    sd = {k: v.detach().clone().float() for k, v in net.state_dict().items()}
    return net.to(dtype), sd


def aug_inputs(case, seed=AUG_SEED, n=AUG_N, L=77):
    """(z [n, 4, h, w], e [1, L, X], e_neg [1, L, X]) f32, seeded."""
    c = CASES[case]
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(n, 4, c["sample_size"], c["sample_size"], generator=g)
    e = torch.randn(1, L, c["cross_dim"], generator=g)
    e_neg = torch.randn(1, L, c["cross_dim"], generator=g)
    return z, e, e_neg


def noise_norm(net, z, t, e, u=None, e_neg=None):
    n = z.shape[0]
    if u is None:
        with torch.no_grad():
            u = net(z, t, e_neg.repeat(n, 1, 1))[0]
    p = net(z, t, e.repeat(n, 1, 1))[0]
    return torch.norm(p - u, p=2), u


def loss_grad(net, z, t, e, e_neg):
    """(noise norm, d noise norm / d e [1, L, X])"""
    e = e.detach().clone().requires_grad_(True)
    loss, _ = noise_norm(net, z, t, e, e_neg=e_neg)
    (g,) = torch.autograd.grad(loss, [e])
    return loss.detach(), g


def token_grad_norms(net, z, t, e, e_neg):
    """[L]: the per-token L2 norm of the noise norm's gradient with respect to the text embedding."""
    return loss_grad(net, z, t, e, e_neg)[1].norm(p=2, dim=-1).mean(dim=0)


def aug_prompt(net, z, t, e, e_neg, lr=0.1, optim_iters=10, target_loss=None, optim_epsilon=None, alpha=0.5):
    """-> (e [1, L, X], trace): trace["noise_norm"] per iteration entered, ["grads"] the noise norm's gradient per update (before the
    row mask), ["penalised"] per update, ["iterations"] updates done, ["stopped_early"]."""
    e = e.detach().clone().requires_grad_(True)
    e0 = e.detach().clone()
    opt = torch.optim.AdamW([e], lr=lr)
    trace = {"noise_norm": [], "grads": [], "penalised": [], "iterations": 0, "stopped_early": False}
    u = None
    for _ in range(optim_iters):
        nn_, u = noise_norm(net, z, t, e, u=u, e_neg=e_neg)
        trace["noise_norm"].append(float(nn_.detach()))
        loss, pen = nn_, False
        if optim_epsilon is not None:
            with torch.no_grad():
                l2 = torch.norm(e0[:, 1:] - e[:, 1:], p=2, dim=-1).mean()
            if l2 > optim_epsilon:
                loss = alpha * nn_ + (1 - alpha) * torch.norm(e0[:, 1:] - e[:, 1:], p=2, dim=-1).mean()
                pen = True
        if target_loss is not None and trace["noise_norm"][-1] <= target_loss:
            trace["stopped_early"] = True
            break
        (gn,) = torch.autograd.grad(nn_, [e], retain_graph=True)
        (g,) = torch.autograd.grad(loss, [e])
        trace["grads"].append(gn.detach().clone())
        trace["penalised"].append(pen)
        g = g.clone()
        g[:, 0] = 0
        e.grad = g
        opt.step()
        opt.zero_grad()
        trace["iterations"] += 1
    return e.detach(), trace


def kept_coordinates(trace, rel=1e-3):
    """bool [L, X]: rows 1.. coordinates whose reference gradient exceeds rel of the largest in EVERY iteration (Adam's first steps
    have magnitude lr whatever the gradient's size: a coordinate whose gradient is near zero moves by +-lr on a rounding difference)."""
    keep = None
    for g in trace["grads"]:
        k = g[0].abs() > rel * g[0, 1:].abs().max()
        keep = k if keep is None else keep & k
    keep[0] = False
    return keep



def early_stop_target(r0, r1, rel=BF16_NORM_REL):
    """A target_loss between the first two reference noise norms r0 > r1 that separates them for ANY engine whose norms lie within
    `rel` of the reference's: the middle of [r1 (1 + rel), r0 (1 - rel)].  None when that interval is empty: the case is then
    unfit for an early-stop check at that tolerance."""
    lo, hi = r1 * (1 + rel), r0 * (1 - rel)
    return 0.5 * (lo + hi) if lo < hi else None

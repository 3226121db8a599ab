"""Host reference of the membership inference attacks (test infrastructure only): the SecMI / PIA / loss-threshold chains of
siss_amd/mia.py restated in torch on any eps-predictor, in the dtype of their input (f64 for the reference, f32 / autocast for the
yardsticks), the brute-force pair counting the statistics are held against, and the exact denoiser of point-mass data."""
import math

import numpy as np
import torch


def coefficients(ab, t_from, t_to):
    """(cx, ce) of the deterministic DDIM transfer from level ab[t_from] to ab[t_to], in f64 (Python floats)."""
    a, c = float(ab[t_from]), float(ab[t_to])
    return math.sqrt(c / a), math.sqrt(1.0 - c) - math.sqrt(c * (1.0 - a) / a)


def transfer(x, e, ab, t_from, t_to):
    cx, ce = coefficients(ab, t_from, t_to)
    return cx * x + ce * e


def row_sums(v):
    return v.double().reshape(v.shape[0], -1).sum(dim=1)


def secmi(eps, ab, x0, t_sec, stride):
    """f64 [N]: ||x^ - x_t||^2 of the round trip t_sec -> t_sec + stride -> t_sec after the inversion of x0 (taken at level ab[0])."""
    x = x0
    for s in range(0, t_sec, stride):
        x = transfer(x, eps(x, s), ab, s, s + stride)
    xt = x
    xf = transfer(xt, eps(xt, t_sec), ab, t_sec, t_sec + stride)
    xb = transfer(xf, eps(xf, t_sec + stride), ab, t_sec + stride, t_sec)
    return row_sums((xb - xt) ** 2)


def pia(eps, ab, x0, t, p):
    """f64 [N]: sum |e0 - eps(x_t, t)|^p with x_t noised by the network's own e0 = eps(x0, 0)."""
    e0 = eps(x0, 0)
    a = float(ab[t])
    xt = math.sqrt(a) * x0 + math.sqrt(1.0 - a) * e0
    return row_sums((e0 - eps(xt, t)).abs() ** p)


def loss(eps, ab, x0, noise, t, per_noise=False):
    """f64 [N]: the mean over the shared noises [J, C, H, W] of ||eps(x_t, t) - noise||^2 (per_noise: [N, J])."""
    a = float(ab[t])
    out = []
    for n in noise:
        n = n.to(x0.dtype)[None]
        out.append(row_sums((eps(math.sqrt(a) * x0 + math.sqrt(1.0 - a) * n, t) - n) ** 2))
    out = torch.stack(out, dim=1)
    return out if per_noise else out.mean(dim=1)


def net_eps(net, autocast=None, batch=16):
    """eps(x, t) of a torch network called as net(x, t)[0] with one integer timestep for the batch; the output in x's dtype.
    autocast: a dtype to run the network under torch.autocast on x's device."""
    @torch.no_grad()
    def eps(x, t):
        out = []
        for s in range(0, x.shape[0], batch):
            xs = x[s:s + batch]
            tt = torch.full((xs.shape[0],), int(t), dtype=torch.long, device=x.device)
            if autocast is not None:
                with torch.autocast(x.device.type, dtype=autocast):
                    out.append(net(xs, tt)[0].to(x.dtype))
            else:
                out.append(net(xs, tt)[0].to(x.dtype))
        return torch.cat(out)
    return eps


def all_scores(eps, ab, x0, noise, settings):
    """{attack: f64 [N]} of the three chains under `settings` = {secmi: {t_sec, stride}, pia: {t, p}, loss: {t, noises}}."""
    s = settings
    return {"secmi": secmi(eps, ab, x0, s["secmi"]["t_sec"], s["secmi"]["stride"]),
            "pia": pia(eps, ab, x0, s["pia"]["t"], s["pia"]["p"]),
            "loss": loss(eps, ab, x0, noise[:s["loss"]["noises"]], s["loss"]["t"])}


def point_mass_eps(ab, mu):
    """The exact denoiser of data concentrated at mu: eps*(x, t) = (x - sqrt(ab_t) mu) / sqrt(1 - ab_t)."""
    def eps(x, t):
        a = float(ab[t])
        return (x - math.sqrt(a) * mu) / math.sqrt(1.0 - a)
    return eps


# ---------------------------------------------------------------------------------------------------------------- statistics
def brute_auc(member, holdout):
    """(#{s_m < s_h} + 0.5 #{s_m = s_h}) / (n_m n_h), pair by pair."""
    wins = sum((m < h) + 0.5 * (m == h) for m in member for h in holdout)
    return wins / (len(member) * len(holdout))


def brute_flagged(scores, holdout, alpha):
    """(share of `scores` flagged, realised FPR) at level alpha: flagged iff strictly below the (k + 1)-th smallest holdout score,
    k = floor(alpha n_h), found by counting instead of sorting: the smallest holdout value with more than k holdout values <= it."""
    n_h = len(holdout)
    k = int(math.floor(alpha * n_h + 1e-9))
    thr = min(h for h in holdout if sum(g <= h for g in holdout) > k)
    return sum(s < thr for s in scores) / len(scores), sum(h < thr for h in holdout) / n_h


def brute_percentile(forget, holdout):
    return sum((h < f) + 0.5 * (h == f) for f in forget for h in holdout) / (len(forget) * len(holdout))

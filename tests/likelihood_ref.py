"""Host references of the likelihood metric (test infrastructure only).

  * ``rk45_host``: scipy.integrate.solve_ivp(method="RK45") restated in numpy f64 (scipy 1.15's rk.py / common.py algorithm, the
    same expressions), usable where scipy is not installed;
  * ``likelihood_f64``: the reference's likelihood_fn composition in f64 -- the oracle UNet (oracle.unet.OracleUNet2D) in torch f64,
    the divergence by autograd (Hutchinson), the host integrator with a numpy round trip per function evaluation.
"""
import numpy as np
import torch

C = np.array([0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1])
A = np.array([
    [0, 0, 0, 0, 0],
    [1 / 5, 0, 0, 0, 0],
    [3 / 40, 9 / 40, 0, 0, 0],
    [44 / 45, -56 / 15, 32 / 9, 0, 0],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729, 0],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]])
B = np.array([35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])
E = np.array([-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])
SAFETY, MIN_FACTOR, MAX_FACTOR, ORDER = 0.9, 0.2, 10, 4


def _norm(x):
    return np.linalg.norm(x) / x.size ** 0.5


class Result:
    def __init__(self, y, t, nfev):
        self.y, self.t, self.nfev = y, t, nfev


def rk45_host(fun, t0, y0, t_bound, rtol=1e-3, atol=1e-6):
    """Returns Result(y at t_bound, accepted times with t0 first, nfev)."""
    y = np.asarray(y0, dtype=np.float64).copy()
    n = y.size
    nfev = [0]

    def f(t, v):
        nfev[0] += 1
        return np.asarray(fun(t, v), dtype=np.float64)

    t = float(t0)
    direction = np.sign(t_bound - t0) if t_bound != t0 else 1
    fy = f(t, y)
    # select_initial_step
    interval = abs(t_bound - t0)
    if interval == 0.0:
        h_abs = 0.0
    else:
        scale = atol + np.abs(y) * rtol
        d0, d1 = _norm(y / scale), _norm(fy / scale)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        h0 = min(h0, interval)
        y1 = y + h0 * direction * fy
        f1 = f(t + h0 * direction, y1)
        d2 = _norm((f1 - fy) / scale) / h0
        h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1 / (ORDER + 1))
        h_abs = min(100 * h0, h1, interval, np.inf)
    K = np.empty((7, n))
    exponent = -1 / (ORDER + 1)
    ts = [t]
    while not (n == 0 or t == t_bound):
        min_step = 10 * np.abs(np.nextafter(t, direction * np.inf) - t)
        if h_abs < min_step:
            h_abs = min_step
        rejected = False
        while True:
            if h_abs < min_step:
                raise RuntimeError("step size too small")
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = np.abs(h)
            K[0] = fy
            for s, (a, c) in enumerate(zip(A[1:], C[1:]), start=1):
                dy = np.dot(K[:s].T, a[:s]) * h
                K[s] = f(t + c * h, y + dy)
            y_new = y + h * np.dot(K[:-1].T, B)
            f_new = f(t + h, y_new)
            K[-1] = f_new
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            err = _norm(np.dot(K.T, E) * h / scale)
            if err < 1:
                factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** exponent)
                if rejected:
                    factor = min(1, factor)
                h_abs *= factor
                break
            h_abs *= max(MIN_FACTOR, SAFETY * err ** exponent)
            rejected = True
        y, fy, t = y_new, f_new, t_new
        ts.append(t)
        if direction * (t - t_bound) >= 0:
            break
    return Result(y, ts, nfev[0])


def likelihood_f64(net, x, eps, sde, rtol=1e-5, atol=1e-5, t_eps=1e-5, drop_divergence=False):
    """bits/dim of x [B, C, H, W] under `net` (an f64 torch UNet: net(sample, t)[0]) with probe eps: the reference's likelihood_fn
    with beta(t), std(t) in f64 and the label t * (N - 1) floored as the reference does (f32).  Returns (bpd [B] f64, nfev)."""
    x = x.detach().double().cpu()
    eps = eps.detach().double().cpu()
    shape, Bn = tuple(x.shape), x.shape[0]
    n = x.numel()
    table = torch.sqrt(1 - torch.cumprod(1 - torch.linspace(sde.beta_0 / sde.N, sde.beta_1 / sde.N, sde.N, dtype=torch.float64), 0))

    def fun(t, y):
        _, _, label = sde.coefficients(t)
        beta = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
        std = float(table[label])
        xs = torch.from_numpy(y[:n].copy()).view(shape).requires_grad_(True)
        lab = torch.full((Bn,), label, dtype=torch.long)
        with torch.enable_grad():
            drift = -0.5 * beta * xs + 0.5 * beta / std * net(xs, lab)[0]
            g = torch.autograd.grad((drift * eps).sum(), xs)[0]
        div = (g * eps).sum(dim=(1, 2, 3))
        if drop_divergence:
            div = torch.zeros_like(div)
        return np.concatenate([drift.detach().reshape(-1).numpy(), div.numpy()])

    y0 = np.concatenate([x.reshape(-1).numpy(), np.zeros(Bn)])
    res = rk45_host(fun, t_eps, y0, 1.0, rtol=rtol, atol=atol)
    z = torch.from_numpy(res.y[:n]).view(shape)
    delta = torch.from_numpy(res.y[n:])
    N = int(np.prod(shape[1:]))
    prior = -N / 2.0 * np.log(2 * np.pi) - (z ** 2).sum(dim=(1, 2, 3)) / 2.0
    return -(prior + delta) / np.log(2) / N + 7.0, res.nfev

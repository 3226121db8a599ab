"""Float64 restatement of the DPM-Solver++ multistep sampler (orders 1 and 2, "2M": Lu et al. 2022, Algorithm 2; diffusers'
DPMSolverMultistepScheduler with algorithm_type="dpmsolver++", solver_type="midpoint", final_sigmas_type="zero"), written from the
formulas and not from siss_amd/scheduler.py: the contract the scheduler class, the kernel and the pipelines are held to (diffusers is
not installed).  numpy only; `ac` is alphas_cumprod as a float64 array."""
import numpy as np


def betas_ac(beta_schedule="linear", beta_start=1e-4, beta_end=0.02, T=1000):
    """alphas_cumprod as the package's DDPMScheduler forms it (f32 betas, f32 cumprod), widened to f64."""
    import torch
    if beta_schedule == "linear":
        b = torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
    else:
        b = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - b, dim=0).double().numpy()


def timesteps(K, T=1000, spacing="linspace", offset=0):
    if spacing == "linspace":
        return [int(v) for v in np.linspace(0, T - 1, K + 1).round()[::-1][:-1]]
    assert spacing == "leading"
    return [int(v) for v in (np.arange(0, K + 1) * (T // (K + 1)))[::-1][:-1] + offset]


def asl(ac, t):
    """(alpha_t, sigma_t, lambda_t = ln alpha_t - ln sigma_t)."""
    a, s = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])
    return a, s, np.log(a) - np.log(s)


def coeffs(ac, ts, i, order, first=None):
    """(1 / a_s, s_s / a_s, c_x, c_0, c_1) of step i of the grid ts, f64: m = x / a_s - (s_s / a_s) e, x' = c_x x + c_0 m + c_1 m1."""
    first = (i == 0) if first is None else first
    a_s, s_s, l_s = asl(ac, ts[i])
    if i == len(ts) - 1:                                     # to sigma = 0: x' = m
        return 1.0 / a_s, s_s / a_s, 0.0, 1.0, 0.0
    a_t, s_t, l_t = asl(ac, ts[i + 1])
    h = l_t - l_s
    E = a_t * (1.0 - np.exp(-h))
    if order == 1 or first:
        return 1.0 / a_s, s_s / a_s, s_t / s_s, E, 0.0
    r = (l_s - asl(ac, ts[i - 1])[2]) / h
    return 1.0 / a_s, s_s / a_s, s_t / s_s, E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r)


def guide(eps, n, g):
    """(e, ||e_uncond|| per sample, ||e_text - e_uncond|| per sample) of eps [2n, ...] under guidance g > 1; (eps, None, None) else."""
    eps = np.asarray(eps, dtype=np.float64)
    if not g > 1.0:
        return eps, None, None
    u, d = eps[:n], eps[n:] - eps[:n]
    norm = lambda v: np.sqrt((v.reshape(n, -1) ** 2).sum(1))
    return u + g * d, norm(u), norm(d)


def step(e, x, m1, co):
    """(x', m) of one update from the guided eps `e`, f64.  m1 is read only when c_1 != 0."""
    a, b, cx, c0, c1 = (float(v) for v in co)
    x = np.asarray(x, dtype=np.float64)
    m = a * x - b * np.asarray(e, dtype=np.float64)
    out = cx * x + c0 * m
    if c1 != 0.0:
        out = out + c1 * np.asarray(m1, dtype=np.float64)
    return out, m


def trajectory(ac, ts, x, eps_fn, order, start=0):
    """The states after each step of ts[start:] from x at ts[start] under eps_fn(x, t) -> guided eps (f64): [x_1, ..., x_end]; the
    first step run is of order 1."""
    x, m1, out = np.asarray(x, dtype=np.float64), None, []
    for i in range(start, len(ts)):
        x, m1 = step(eps_fn(x, ts[i]), x, m1, coeffs(ac, ts, i, order, first=(i == start)))
        out.append(x)
    return out


def step_f32(eps, x, m1, n, g, co):
    """The kernel's own arithmetic on torch f32 tensors (any device), one rounding per product / sum in its order:
    d = e_t - e_u; e = e_u + g d; m = a x - b e; x' = (c_x x + c_0 m) + c_1 m1 (the last term only when c_1 != 0).  Returns (x', m)."""
    import torch
    a, b, cx, c0, c1 = (torch.tensor(float(v), dtype=torch.float32, device=x.device) for v in co)
    if g > 1.0:
        u = eps[:n]
        d = eps[n:] - u
        e = u + torch.tensor(float(g), dtype=torch.float32, device=x.device) * d
    else:
        e = eps
    m = a * x - b * e
    out = cx * x + c0 * m
    if float(c1) != 0.0:
        out = out + c1 * m1
    return out, m


def error_bound(eps, x, m1, n, g, co):
    """A-priori bounds (err_x, err_m) on |kernel - step()| from the kernel's rounding count, each f32 operation at most u = 2^-24
    relative: e takes 3 (d, g d, the sum), m takes 3 more (a x, b e, the difference), x' takes 4 or 6 (the products and sums)."""
    u = 2.0 ** -24
    a, b, cx, c0, c1 = (abs(float(v)) for v in co)
    e, _, _ = guide(eps, n, g)
    mx = lambda v: float(np.abs(v).max())
    x = np.asarray(x, dtype=np.float64)
    err_e = 0.0
    if g > 1.0:
        d = np.asarray(eps[n:], dtype=np.float64) - np.asarray(eps[:n], dtype=np.float64)
        err_e = u * (2.0 * g * mx(d) + mx(e))
    xo, m = step(e, x, m1, co)
    err_m = u * (a * mx(x) + b * mx(e) + mx(m)) + b * err_e
    last = c1 * mx(m1) if c1 != 0.0 else 0.0
    err_x = u * (cx * mx(x) + c0 * mx(m) + last) + c0 * err_m + 2.0 * u * (cx * mx(x) + c0 * mx(m) + last)
    return err_x, err_m

"""Restatements for the injection check's tests (tests/test_injection_host.py, tests/test_hip_injection.py), written from the
formulas alone:

    init_timestep = min(int(N * strength), N);  t_start = max(N - init_timestep, 0);  timesteps[t_start:], N - t_start

    j = i mod m
    z_j = (mean_j + exp(0.5 * clamp(logvar_j, -30, 20)) * eps_z_j) * scaling
    x_i = a * z_j + b * eps_t_i

in float64 from the f32 (or bf16) inputs and the f32 scalars, the f32 error bound of that chain, an f32 torch emulation of the
launcher for the host tests, and float64 guidance + DDIM (eta = 0)."""
import torch

U = 2.0 ** -24              # f32 unit roundoff: one rounding to nearest changes a value by at most U * |value|
ULP = 2.0 ** -23            # one f32 ulp of a value v is at most ULP * |v|
EXPF_ULP = 1                # the maximum error HIP's math API documents for expf
ROUNDINGS = 7               # 0.5 * lv, std * eps_z, mean + ., . * scaling  |  a * z, b * eps_t, their sum


def f32(v):
    """The f32 nearest to v, as a Python float (what a c_float argument carries)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def scalars(alphas_cumprod, t):
    """(a, b) = (sqrt(ac[t]), sqrt(1 - ac[t])) formed in f32, as DDIMScheduler.add_noise forms them."""
    ac = alphas_cumprod[int(t)].float()
    return float(ac ** 0.5), float((1 - ac) ** 0.5)


def timesteps_ref(all_timesteps, num_inference_steps, strength):
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    return list(all_timesteps)[t_start:], num_inference_steps - t_start


def tile_index(m, n, order="mod"):
    """Which image output i reads: i mod m (torch.cat([z] * k)), or -- the WRONG order, for the negative control -- i // (n / m)."""
    i = torch.arange(n)
    return i % m if order == "mod" else i // (n // m)


def inject_f64(moments, eps_z, eps_t, scaling, a, b, order="mod"):
    """(x [n, C, h, w] in f64, the bound's magnitudes (M, S)): M = (|mean| + |std eps_z|) scaling a + |b eps_t| and
    S = |std eps_z| scaling a, per element of x."""
    m, n, C = moments.shape[0], eps_t.shape[0], moments.shape[1] // 2
    mom = moments.double().cpu()
    mean, logvar = mom[:, :C], mom[:, C:]
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    ez, et = eps_z.double().cpu(), eps_t.double().cpu()
    scaling, a, b = float(scaling), float(a), float(b)
    z = (mean + std * ez) * scaling
    idx = tile_index(m, n, order)
    x = a * z[idx] + b * et
    S = (std * ez).abs()[idx] * abs(scaling) * abs(a)
    M = mean.abs()[idx] * abs(scaling) * abs(a) + S + (b * et).abs()
    return x, M, S


def inject_bound(M, S):
    """First-order f32 error of the kernel's chain against inject_f64: every one of its ROUNDINGS products and sums rounds once
    (each at most U relative to the magnitude M it feeds), and expf is off by at most EXPF_ULP ulp, which reaches x through the
    std term alone (S)."""
    return ROUNDINGS * U * M + EXPF_ULP * ULP * S


def inject_emul(moments, eps_z, eps_t, scaling, a, b):
    """The launcher in f32 torch on the host (for tests without a GPU): same tiling, same order of operations."""
    m, n, C = moments.shape[0], eps_t.shape[0], moments.shape[1] // 2
    if n % m:
        raise RuntimeError("siss_latent_inject failed with status 1 (bad argument)")
    mom = moments.float()
    z = (mom[:, :C] + torch.exp(0.5 * mom[:, C:].clamp(-30.0, 20.0)) * eps_z) * f32(scaling)
    return f32(a) * z[tile_index(m, n)] + f32(b) * eps_t


def ddim_f64(eps, x, n, g, co, clip=0.0):
    """Float64 guidance + DDIM (eta = 0) step, and the per-sample norms of eps_uncond and eps_text - eps_uncond (None without
    guidance).  co = (sqrt a_t, sqrt(1 - a_t), sqrt a_prev, sqrt(1 - a_prev))."""
    e = eps.double()
    sa, sb, sap, sbp = co
    norms = None
    if g > 1.0:
        u, d = e[:n], e[n:] - e[:n]
        e = u + g * d
        norms = (u.flatten(1).norm(dim=1), d.flatten(1).norm(dim=1))
    x0 = (x.double() - sb * e) / sa
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    return sap * x0 + sbp * e, norms

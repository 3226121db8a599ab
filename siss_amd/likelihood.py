"""Forget-set likelihood (the paper's NLL metric, bits/dim) on the probability-flow ODE of a VP-SDE.

Restates the reference's ``metrics.likelihood.LikelihoodEvaluator`` over ``metrics/song_likelihood`` (``likelihood_fn``:
integrate the probability-flow ODE of the image from t = eps to T = 1 together with the log-density change, estimated along one
Hutchinson probe per sample; add the prior log-density at T; convert to bits/dim, + 7).  The reference drives scipy's
``solve_ivp(method="RK45")`` on the host with a numpy round trip per function evaluation; here:

  * one function evaluation = the UNet forward + its input VJP (``UNetEngine.input_vjp``) + ``siss_pflow_drift_div`` (the drift
    and the per-block divergence partials) + ``siss_slab_rowsum_f64``, captured once per input shape into a hipGraph and replayed;
  * the integrator (``rk45``) is scipy 1.15's RK45 -- Dormand-Prince tableau, FSAL, ``select_initial_step``, the same step
    controller -- with every state vector on the device in f64 (``siss_rk_combine``, ``siss_rk_norm``); the host reads the
    per-block partials of one error norm per attempted step and nothing else.

The ODE runs on an f32 engine: a bf16 drift feeds the controller at rtol = atol = 1e-5 its rounding noise (measured once, MNIST 28 x 28,
random-init weights, same probe: 4868 function evaluations and bits/dim +4.0e-3 against 3614 on the f32 engine).  For a bf16 model
the evaluator owns an f32 ``UNetEngine`` of the same configuration and copies the model's flat f32 master into it before each
evaluation.
"""
import math
import time

import numpy as np
import torch

from . import lib
from .records import append_jsonl

# scipy.integrate RK45 (scipy/integrate/_ivp/rk.py, 1.15): the Dormand-Prince 5(4) pair and the step controller's constants
RK45_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
RK45_A = ((), (1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9),
          (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
          (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
RK45_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
RK45_E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)
SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10
ERROR_ESTIMATOR_ORDER = 4
ERROR_EXPONENT = -1 / (ERROR_ESTIMATOR_ORDER + 1)


class RK45Result:
    def __init__(self, y, t_events, nfev, n_attempted):
        self.y, self.t, self.nfev, self.n_attempted = y, t_events, nfev, n_attempted


def rk45(fun, t0, y0, t_bound, rtol=1e-3, atol=1e-6, out32=None, n32=0):
    """scipy.integrate.solve_ivp(fun, (t0, t_bound), y0, method="RK45", rtol=rtol, atol=atol) with the state on the device.

    fun(t, y) -> f64 device vector of y's length (copied at once: fun may return the same buffer every call).  y0: f64 device vector.
    out32 / n32: every state fun is evaluated at is also cast to f32 over its first n32 entries into out32 (the model input of
    the likelihood ODE) before fun runs.  Returns y at t_bound (device f64), the accepted times (t0 first), nfev and the number
    of attempted steps; nfev = 2 + 6 x attempted steps, as scipy counts."""
    assert y0.dtype == torch.float64 and y0.is_cuda and y0.dim() == 1
    n = y0.numel()
    t0, t_bound = float(t0), float(t_bound)
    direction = float(np.sign(t_bound - t0)) if t_bound != t0 else 1.0
    K = torch.empty(7, n, dtype=torch.float64, device=y0.device)
    kr = [K[i] for i in range(7)]                 # rows in stage order; FSAL rotates the first and the last
    y, y_new, ys = y0.clone(), torch.empty_like(y0), torch.empty_like(y0)
    nblk = max(1, min(256, -(-n // 2048)))
    part = torch.empty(nblk, dtype=torch.float64, device=y0.device)
    nfev = 0

    def stage(pairs, h, base, out):
        terms = lib.RkTerms.of(pairs)
        lib.call("siss_rk_combine", lib.C.byref(terms), base, float(h), out, out32, int(n32), n)

    def evaluate(t, yv, dst):
        nonlocal nfev
        nfev += 1
        dst.copy_(fun(t, yv))

    def norm(pairs, h, ya, yb=None):
        terms = lib.RkTerms.of(pairs)
        lib.call("siss_rk_norm", lib.C.byref(terms), float(h), ya, yb, float(rtol), float(atol), n, part, nblk)
        return math.sqrt(sum(part.tolist())) / n ** 0.5

    # initial derivative and select_initial_step (scipy/integrate/_ivp/common.py)
    if n32:
        stage([], 0.0, y, None)
    evaluate(t0, y, kr[0])
    interval = abs(t_bound - t0)
    if interval == 0.0:
        h_abs = 0.0
    else:
        d0 = norm([(1.0, y)], 1.0, y)
        d1 = norm([(1.0, kr[0])], 1.0, y)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        h0 = min(h0, interval)
        stage([(1.0, kr[0])], h0 * direction, y, ys)
        evaluate(t0 + h0 * direction, ys, kr[1])
        d2 = norm([(1.0, kr[1]), (-1.0, kr[0])], 1.0, y) / h0
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(1e-6, h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1 / (ERROR_ESTIMATOR_ORDER + 1))
        h_abs = min(100 * h0, h1, interval)
    t, ts, attempted = t0, [t0], 0
    while not (n == 0 or t == t_bound):
        min_step = 10 * abs(np.nextafter(t, direction * np.inf) - t)
        if h_abs < min_step:
            h_abs = min_step
        rejected = False
        while True:
            if h_abs < min_step:
                raise RuntimeError(f"rk45: required step size is less than spacing between numbers (t = {t})")
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            attempted += 1
            for s in range(1, 6):
                stage([(a, kr[j]) for j, a in enumerate(RK45_A[s]) if a != 0.0], h, y, ys)
                evaluate(t + RK45_C[s] * h, ys, kr[s])
            stage([(b, kr[j]) for j, b in enumerate(RK45_B) if b != 0.0], h, y, y_new)
            evaluate(t + h, y_new, kr[6])
            err = norm([(e, kr[j]) for j, e in enumerate(RK45_E) if e != 0.0], h, y, y_new)
            if err < 1:
                factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** ERROR_EXPONENT)
                if rejected:
                    factor = min(1, factor)
                h_abs *= factor
                break
            h_abs *= max(MIN_FACTOR, SAFETY * err ** ERROR_EXPONENT)
            rejected = True
        y, y_new = y_new, y
        kr[0], kr[6] = kr[6], kr[0]
        t = t_new
        ts.append(t)
        if direction * (t - t_bound) >= 0:
            break
    return RK45Result(y, ts, nfev, attempted)


# ---------------------------------------------------------------------------------------------------------------- the SDE
class VPSDE:
    """The variance-preserving SDE of score_sde (metrics/song_likelihood/sde_lib.py), as the likelihood ODE uses it: beta(t) and the
    discrete-time score scale sqrt(1 - alphas_cumprod)[t * (N - 1)] in f32, the N(0, I) prior."""

    def __init__(self, beta_min=0.1, beta_max=20, N=1000):
        self.beta_0, self.beta_1, self.N = float(beta_min), float(beta_max), int(N)
        # float64, rounded ONCE to float32: a float32 linspace / cumprod / sqrt would depend on the host's vector ISA
        betas = torch.linspace(self.beta_0 / self.N, self.beta_1 / self.N, self.N, dtype=torch.float64)
        ac = torch.cumprod(1.0 - betas, dim=0)
        self.discrete_betas = betas.float()
        self.alphas_cumprod = ac.float()
        self.sqrt_1m_alphas_cumprod = torch.sqrt(1.0 - ac).float()

    @property
    def T(self):
        return 1

    def coefficients(self, t):
        """(beta(t), std(t), label) with the reference's f32 arithmetic: vec_t = f32(t); beta_0 + vec_t * (beta_1 - beta_0);
        labels = (vec_t * (N - 1)).long(); std = sqrt_1m_alphas_cumprod[labels]."""
        t32 = np.float32(t)
        beta = np.float32(self.beta_0) + t32 * np.float32(self.beta_1 - self.beta_0)
        label = int(t32 * np.float32(self.N - 1))
        return np.float32(beta), np.float32(self.sqrt_1m_alphas_cumprod[label]), label

    def prior_logp(self, z):
        """log N(z; 0, I) per sample, in f64."""
        N = int(np.prod(z.shape[1:]))
        return -N / 2.0 * np.log(2 * np.pi) - torch.sum(z.double() ** 2, dim=tuple(range(1, z.dim()))) / 2.0


class VESDE:
    """metrics.song_likelihood.sde_lib.VESDE: not built."""

    def __init__(self, *a, **k):
        raise NotImplementedError("VESDE: the likelihood metric is built for the VP-SDE only (the T-shirt config's sde)")


class subVPSDE:
    """metrics.song_likelihood.sde_lib.subVPSDE: not built."""

    def __init__(self, *a, **k):
        raise NotImplementedError("subVPSDE: the likelihood metric is built for the VP-SDE only (the T-shirt config's sde)")


def bits_per_dim(z, delta_logp, sde):
    """The reference's bpd of likelihood_fn: -(prior_logp(z) + delta_logp) / ln 2 / N + 7 (offset), in f64 over f32 z."""
    N = int(np.prod(z.shape[1:]))
    return -(sde.prior_logp(z.float()) + delta_logp.double()) / np.log(2) / N + 7.0


# ---------------------------------------------------------------------------------------------------------------- the drift
class PFlowODE:
    """The right-hand side of the likelihood ODE over the joint state [x_flat ; delta_logp] on one f32 engine and one input shape:
    fun(t, y) -> f64 [n + B].  Its model input (`xs`, f32) is written by the integrator (rk45's out32)."""

    def __init__(self, eng, sde, shape, use_graph=True):
        assert eng.f32, "the likelihood ODE runs on an f32 engine"
        self.eng, self.sde, self.shape = eng, sde, tuple(shape)
        dev = eng.device
        B = self.shape[0]
        self.chw = int(np.prod(self.shape[1:]))
        self.n = B * self.chw
        self.nblk = max(1, min(1024, self.chw // 2048))
        self.xs = torch.zeros(self.shape, dtype=torch.float32, device=dev)
        self.ts = torch.zeros(B, dtype=torch.long, device=dev)
        self.par = torch.zeros(3, dtype=torch.float32, device=dev)                 # [beta(t), std(t), sqrt(beta(t)) ** 2]
        self.eps = torch.zeros(self.shape, dtype=torch.float32, device=dev)        # the Hutchinson probe
        self.v = torch.zeros(self.shape, dtype=torch.float32, device=dev)          # J^T eps
        self.out = torch.zeros(self.n + B, dtype=torch.float64, device=dev)
        self.partials = torch.zeros(B, self.nblk, dtype=torch.float64, device=dev)
        self.use_graph = use_graph
        self.graph = None

    def body(self):
        B = self.shape[0]
        pred = self.eng.forward(self.xs, self.ts)
        self.eng.input_vjp(self.eps, out=self.v)
        lib.call("siss_pflow_drift_div", self.xs, pred, self.v, self.eps, self.par, self.out, self.partials, B, self.chw, self.nblk)
        lib.call("siss_slab_rowsum_f64", self.partials, self.out[self.n:], B, self.nblk)

    def capture(self):
        side = torch.cuda.Stream(device=self.eng.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.body()                                     # settle every buffer of this shape before the capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                self.body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = graph

    def set_time(self, t):
        beta, std, label = self.sde.coefficients(t)
        g = np.sqrt(beta)                                   # (numpy f32: IEEE, as torch's sqrt on the device)
        self.par[0].fill_(float(beta))
        self.par[1].fill_(float(std))
        self.par[2].fill_(float(np.float32(g * g)))
        self.ts.fill_(label)

    def __call__(self, t, y=None):
        self.set_time(t)
        if self.use_graph:
            if self.graph is None:
                self.capture()
            self.graph.replay()
        else:
            self.body()
        return self.out


def same_layout(a, b):
    """Whether two ParamStores lay their parameters out identically (the flat master can be copied across)."""
    key = lambda ps: (ps.total, [(n, sp.kind, sp.off, sp.numel, sp.native_shape) for n, sp in ps.specs.items()])
    return key(a) == key(b)


class LikelihoodEvaluator:
    """metrics.likelihood.LikelihoodEvaluator: ``evaluate_likelihood(model, img_batch) -> (bpd [B], z, nfe)``."""

    def __init__(self, sde=None, hutchinson_type="Rademacher", rtol=1e-5, atol=1e-5, method="RK45", eps=1e-5, use_graph=True):
        sde = VPSDE() if sde is None else sde
        if not isinstance(sde, VPSDE):
            raise NotImplementedError(f"{type(sde).__name__}: the likelihood metric is built for the VP-SDE only")
        if method != "RK45":
            raise NotImplementedError(f"method={method!r}: only scipy's RK45 is restated on the device")
        if hutchinson_type not in ("Rademacher", "Gaussian"):
            raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")
        self.sde, self.hutchinson_type, self.rtol, self.atol, self.method, self.eps = sde, hutchinson_type, rtol, atol, method, eps
        self.use_graph = use_graph
        self._eng, self._odes = None, {}

    def engine_for(self, model):
        """The evaluator's own f32 engine, holding the model's current weights (its flat f32 master, copied)."""
        from .unet import UNetEngine
        src = getattr(model, "engine", model)
        if type(src) is not UNetEngine:
            raise NotImplementedError(f"{type(src).__name__}: the likelihood metric is built for the unconditional UNet2DModel only")
        if self._eng is None or self._eng.cfg != src.cfg or self._eng.device != src.device:
            self._eng, self._odes = UNetEngine(src.cfg, src.device, dtype=torch.float32), {}
        eng = self._eng
        assert same_layout(eng.ps, src.ps), "likelihood: the f32 engine's parameter layout differs from the model's"
        eng.ps.flat.copy_(src.ps.flat)
        eng.refresh_weights(cast_shadow=True)
        return eng

    def probe(self, shape, device, generator=None):
        if self.hutchinson_type == "Gaussian":
            return torch.randn(shape, device=device, generator=generator)
        return torch.randint(0, 2, shape, device=device, generator=generator).float() * 2 - 1.0

    def evaluate_likelihood(self, model, img_batch, epsilon=None, generator=None):
        """bits/dim of each image of img_batch [B, C, H, W] (already normalised as the model's training data), the latent z at T
        and the number of function evaluations -- the reference's likelihood_fn.  epsilon: the Hutchinson probe (else drawn
        from `generator`)."""
        eng = self.engine_for(model)
        data = img_batch.to(eng.device).float().contiguous()
        shape = tuple(data.shape)
        ode = self._odes.get(shape)
        if ode is None:
            ode = self._odes[shape] = PFlowODE(eng, self.sde, shape, use_graph=self.use_graph)
        ode.eps.copy_(self.probe(shape, eng.device, generator) if epsilon is None else epsilon.to(eng.device).float())
        B = shape[0]
        y0 = torch.cat([data.reshape(-1).double(), torch.zeros(B, dtype=torch.float64, device=eng.device)])
        res = rk45(ode, self.eps, y0, self.sde.T, rtol=self.rtol, atol=self.atol, out32=ode.xs.view(-1), n32=ode.n)
        z = res.y[:ode.n].float().view(shape)
        delta_logp = res.y[ode.n:]
        return bits_per_dim(z, delta_logp, self.sde), z, res.nfev


def log_likelihood(evaluator, model, image, global_step, path, generator):
    """One evaluation of the forget image, appended to `path` as a JSON line {global_step, bpd, nfe, seconds} (tasks.py)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bpd, _, nfe = evaluator.evaluate_likelihood(model, image.unsqueeze(0) if image.dim() == 3 else image, generator=generator)
    rec = dict(global_step=int(global_step), bpd=float(bpd[0]), nfe=int(nfe), seconds=time.perf_counter() - t0)
    append_jsonl(path, rec)
    print(f"[siss_amd] likelihood at step {global_step}: {rec['bpd']:.4f} bits/dim ({nfe} function evaluations, "
          f"{rec['seconds']:.1f} s)")
    return rec

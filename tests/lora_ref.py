"""f64 restatement of the LoRA pieces (siss_amd/lora.py, csrc/lora.hip): the chain rule through W = W0 + s B A, the merge, and one
adapter-space optimizer step composed with tests/optimizer_ref.py.  numpy / torch on the CPU; test infrastructure only.

Tables here are lists of (w_off, a_off, b_off, w0_off, O, I, ptile0, mtile0) -- the rows siss_amd.lora.layout builds.
"""
import numpy as np
import torch

import optimizer_ref as R

f64 = np.float64
U = 2.0 ** -24


def views(buf, row, r):
    """(A [r, I], B [O, r]) of a job row as views of the flat LoRA buffer `buf` (last axis)."""
    _, a, b, _, O, I, _, _ = row
    return buf[..., a:a + r * I].reshape(*buf.shape[:-1], r, I), buf[..., b:b + O * r].reshape(*buf.shape[:-1], O, r)


def project(grads, rows, lora_p, r, s, nsets):
    """(g [2, L] f64, bound [2, L]): dA_k = s B^T dW_k, dB_k = s dW_k A^T of every row from grads [>= nsets, P]; set k >= nsets and the
    padding between tensors are zero.  bound: the dot-product bound of the f32 kernel, (K + 2) u s (|B|^T |dW|) resp. (|dW| |A|^T), with
    K the reduction length (O resp. I): K - 1 additions and a product per term (gamma_K), the scaling by s one more rounding."""
    p = np.asarray(lora_p, f64)
    g = np.zeros((2, p.size), f64)
    bound = np.zeros((2, p.size), f64)
    for row in rows:
        w_off, a, b, _, O, I, _, _ = row
        A, B = views(p, row, r)
        for k in range(nsets):
            dW = np.asarray(grads[k][w_off:w_off + O * I], f64).reshape(O, I)
            g[k, a:a + r * I] = (s * (B.T @ dW)).reshape(-1)
            g[k, b:b + O * r] = (s * (dW @ A.T)).reshape(-1)
            bound[k, a:a + r * I] = ((O + 2) * U * s * (np.abs(B).T @ np.abs(dW))).reshape(-1)
            bound[k, b:b + O * r] = ((I + 2) * U * s * (np.abs(dW) @ np.abs(A).T)).reshape(-1)
    return g, bound


def merge(flat, rows, w0, lora_p, r, s):
    """(flat f64 with W0 + s B A on every row's stretch, bound of the same shape (zero outside the stretches): (r + 2) u (|W0| + s |B| |A|))."""
    out = np.asarray(flat, f64).copy()
    bound = np.zeros_like(out)
    p, w0 = np.asarray(lora_p, f64), np.asarray(w0, f64)
    for row in rows:
        w_off, _, _, w0_off, O, I, _, _ = row
        A, B = views(p, row, r)
        base = w0[w0_off:w0_off + O * I].reshape(O, I)
        out[w_off:w_off + O * I] = (base + s * (B @ A)).reshape(-1)
        bound[w_off:w_off + O * I] = ((r + 2) * U * (np.abs(base) + s * (np.abs(B) @ np.abs(A)))).reshape(-1)
    return out, bound


def target_mask(n, rows):
    m = np.zeros(n, bool)
    for w_off, _, _, _, O, I, _, _ in rows:
        m[w_off:w_off + O * I] = True
    return m


def used_mask(L, rows, r):
    """bool [L]: the floats of the LoRA buffer that belong to an A or a B (the rest is alignment padding)"""
    m = np.zeros(L, bool)
    for _, a, b, _, O, I, _, _ in rows:
        m[a:a + r * I] = True
        m[b:b + O * r] = True
    return m


def adapter_step(gx, ga, p, m, v, step, hp, mode, knob, max_norm):
    """One adapter-space update in f64: optimizer_ref.step_f64 on the LoRA flat buffer and its gradient pair.  Returns ((p, m, v, g), scalars)."""
    return R.step_f64(gx, ga, p, m, v, step, hp, mode, knob, max_norm)


class LoRAOracle(torch.nn.Module):
    """An oracle UNet whose target weights are W0 + s B A under autograd: named_parameters() are the adapters alone (W0 and every other
    tensor are constants), the call goes through torch.func.functional_call with the merged weights."""

    def __init__(self, net, names, r, s, A, B):
        super().__init__()
        self.__dict__["net"] = net                      # (not registered: its parameters are not this module's)
        self.names, self.r, self.s = list(names), r, s
        self.base = {n: p.detach().clone() for n, p in net.named_parameters()}
        self.A = torch.nn.ParameterList([torch.nn.Parameter(a.detach().clone().to(torch.float64)) for a in A])
        self.B = torch.nn.ParameterList([torch.nn.Parameter(b.detach().clone().to(torch.float64)) for b in B])

    def merged(self):
        w = dict(self.base)
        for n, a, b in zip(self.names, self.A, self.B):
            w[n] = self.base[n] + self.s * (b @ a).reshape(self.base[n].shape)
        return w

    def forward(self, *args, **kw):
        return torch.func.functional_call(self.net, self.merged(), args, kw)

    def flat(self, tensors_a, tensors_b, rows, L):
        """The per-target tensors laid into a flat [L] f64 numpy buffer by the rows' offsets."""
        out = np.zeros(L, f64)
        for row, a, b in zip(rows, tensors_a, tensors_b):
            _, ao, bo, _, O, I, _, _ = row
            out[ao:ao + self.r * I] = a.detach().double().numpy().reshape(-1)
            out[bo:bo + O * self.r] = b.detach().double().numpy().reshape(-1)
        return out


def oracle_gradients(model, loss_obj, loss_fn, ac, micro_batches, train_batch_size, loss_params=None, conditioning=None):
    """(g_x, g_a) of one optimizer step as lists over model.parameters(), by torch.autograd.grad: the loop body of oracle/step.py
    (loss normalised by train_batch_size and the number of micro-batches) without the optimizer; a loss that returns ONE objective
    (naive_del, simple_neg_del) gives g_a = 0."""
    from oracle.step import prep_inputs
    params = list(model.parameters())
    gx = [torch.zeros_like(p) for p in params]
    ga = [torch.zeros_like(p) for p in params]
    n = len(micro_batches)
    fn = getattr(loss_obj, loss_fn)
    for mb in micro_batches:
        keep, forget = prep_inputs(ac, mb["x0"], mb["a0"], mb["noise"], mb["t"])
        kw = dict(loss_params or {})
        if mb.get("u") is not None and loss_fn in ("importance_sampling_with_mixture", "subscore_bernoulli"):
            kw["u"] = mb["u"]
        loss, _, _, _, _, wlx, wla = fn(model, mb["t"], mb["noise"], conditioning or {}, keep, forget, **kw)
        if loss is not None:
            for acc, g in zip(gx, torch.autograd.grad(loss.sum() / train_batch_size / n, params)):
                acc += g
            continue
        for acc, g in zip(gx, torch.autograd.grad(wlx.sum() / train_batch_size / n, params, retain_graph=True, allow_unused=True)):
            acc += 0 if g is None else g
        for acc, g in zip(ga, torch.autograd.grad(wla.sum() / train_batch_size / n, params, allow_unused=True)):
            acc += 0 if g is None else g
    return gx, ga

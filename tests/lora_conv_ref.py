"""f64 restatement of the conv LoRA pieces (siss_amd/lora.py conv_targets, csrc/lora.hip siss_lora_project_conv / siss_lora_merge_conv)
on the native tap-major layout: W [9, O, I] = W0 + s B A[t] with B [O, r] shared by the taps and A [9, r, I] -- peft's Conv2d adapter
(lora_ref.LoRAOracle's `(b @ a).reshape(base.shape)` with a = lora_A.weight.flatten(1)).  numpy / torch on the CPU; test
infrastructure only.

Tables here are lists of (w_off, a_off, b_off, w0_off, O, I, ptile0, mtile0, taps) -- the rows siss_amd.lora.conv_layout builds.
"""
import numpy as np

from lora_ref import U, f64


def views(buf, row, r):
    """(A [T, r, I], B [O, r]) of a conv job row as views of the flat LoRA buffer `buf` (last axis)."""
    _, a, b, _, O, I, _, _, T = row
    return buf[..., a:a + T * r * I].reshape(*buf.shape[:-1], T, r, I), buf[..., b:b + O * r].reshape(*buf.shape[:-1], O, r)


def project(grads, rows, lora_p, r, s, nsets):
    """(g [2, L] f64, bound [2, L]) over the conv rows: dB = s sum_t dW[t] A[t]^T (ONE reduction of length T I),
    dA[t] = s B^T dW[t]; set k >= nsets and everything outside the rows' A / B are zero.  bound: (K + 2) u s (sum of absolute
    products), K = T I for dB and O for dA: K - 1 additions and a product per term, the scaling by s one more rounding."""
    p = np.asarray(lora_p, f64)
    g = np.zeros((2, p.size), f64)
    bound = np.zeros((2, p.size), f64)
    for row in rows:
        w_off, a, b, _, O, I, _, _, T = row
        A, B = views(p, row, r)
        for k in range(nsets):
            dW = np.asarray(grads[k][w_off:w_off + T * O * I], f64).reshape(T, O, I)
            g[k, a:a + T * r * I] = (s * np.einsum("om,toi->tmi", B, dW)).reshape(-1)
            g[k, b:b + O * r] = (s * np.einsum("toi,tni->on", dW, A)).reshape(-1)
            bound[k, a:a + T * r * I] = ((O + 2) * U * s * np.einsum("om,toi->tmi", np.abs(B), np.abs(dW))).reshape(-1)
            bound[k, b:b + O * r] = ((T * I + 2) * U * s * np.einsum("toi,tni->on", np.abs(dW), np.abs(A))).reshape(-1)
    return g, bound


def merge(flat, rows, w0, lora_p, r, s):
    """(flat f64 with W0[t] + s B A[t] on every row's [T, O, I] stretch, bound of the same shape (zero outside the stretches):
    (r + 2) u (|W0| + s |B| |A[t]|))."""
    out = np.asarray(flat, f64).copy()
    bound = np.zeros_like(out)
    p, w0 = np.asarray(lora_p, f64), np.asarray(w0, f64)
    for row in rows:
        w_off, _, _, w0_off, O, I, _, _, T = row
        A, B = views(p, row, r)
        base = w0[w0_off:w0_off + T * O * I].reshape(T, O, I)
        out[w_off:w_off + T * O * I] = (base + s * np.einsum("ok,tki->toi", B, A)).reshape(-1)
        bound[w_off:w_off + T * O * I] = ((r + 2) * U * (np.abs(base) + s * np.einsum("ok,tki->toi", np.abs(B), np.abs(A)))).reshape(-1)
    return out, bound


def target_mask(n, rows):
    m = np.zeros(n, bool)
    for w_off, _, _, _, O, I, _, _, T in rows:
        m[w_off:w_off + T * O * I] = True
    return m


def used_mask(L, rows, r):
    """bool [L]: the floats of the LoRA buffer that belong to a conv target's A or B"""
    m = np.zeros(L, bool)
    for _, a, b, _, O, I, _, _, T in rows:
        m[a:a + T * r * I] = True
        m[b:b + O * r] = True
    return m


def a_native_to_ref(a):
    """A [9, r, I] (t = kh * 3 + kw) -> lora_A.weight [r, I, 3, 3] (numpy)"""
    T, r, I = a.shape
    return np.ascontiguousarray(a.reshape(3, 3, r, I).transpose(2, 3, 0, 1))


def flat(tensors_a_ref, tensors_b, rows, L, r, into=None):
    """Per-target reference-layout tensors (A [r, I, 3, 3] or [r, 9 I] in reference order; B [O, r] or [O, r, 1, 1]) laid into a flat
    [L] f64 numpy buffer by the conv rows' offsets, A converted to native."""
    out = np.zeros(L, f64) if into is None else into
    for row, a, b in zip(rows, tensors_a_ref, tensors_b):
        _, ao, bo, _, O, I, _, _, T = row
        a = np.asarray(a.detach().double().numpy() if hasattr(a, "detach") else a, f64).reshape(r, I, 3, 3)
        b = np.asarray(b.detach().double().numpy() if hasattr(b, "detach") else b, f64).reshape(O, r)
        out[ao:ao + T * r * I] = a.transpose(2, 3, 0, 1).reshape(-1)
        out[bo:bo + O * r] = b.reshape(-1)
    return out

"""tests/optimizer_ref.py against torch's own operators on the CPU, and the f32 restatement ALONE against every bound that
tests/test_hip_optimizer.py applies to the kernels, on that test's exact seeded inputs: a wrong reference must not bless a wrong
kernel, and a bound that the reference's own arithmetic cannot keep would fail here, not on the GPU.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optimizer_ref as R

F64 = torch.float64
f32 = np.float32
SMALL = [n for n in R.SIZES if n <= 100_003]


@pytest.mark.parametrize("name", list(R.HYPER))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_f64_reference_is_torch_adamw_with_clip_grad_norm(name, mode):
    """Three carried steps of norm fixing / erasediff / the inf guard + clip_grad_norm_ + torch.optim.AdamW(foreach=False), all in f64
    on the same f32 inputs and the f32-rounded hyper-parameters: within 1e-12 of the update (weight decay acts on a p0 of that size)."""
    hp, n, knob, max_norm = R.hyper(*R.HYPER[name]), 1027, (1e-2 if mode == 1 else 5.0), 1.0
    lr, b1, b2, eps, wd = R.wide(hp)
    p0 = (lr * np.random.default_rng(1).standard_normal(n)).astype(f32)     # of one update's size: 1e-12 of the update stays above f64's ulp of p
    tp = torch.from_numpy(p0).double().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        gx, ga = R.gauss_pair(n, 10 * step + mode)
        if mode == 2:
            ga[:] = 0
        x, a = torch.from_numpy(gx).double(), torch.from_numpy(ga).double()
        if mode == 1:
            s = -max(float(f32(knob)) - float(x @ a) / float(a @ a), 0.0)
        else:
            s = float(f32(knob)) / float(a.norm()) if float(a.norm()) else 0.0
        tp.grad = x - s * a
        before = tp.detach().clone()
        pre = torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        (p_new, m, v, g), sc = R.step_f64(gx, ga, p, m, v, step, hp, mode, knob, max_norm)
        upd = float((tp.detach() - before).abs().max())
        assert abs(sc["pre_clip_norm"] - float(pre)) <= 1e-12 * float(pre)
        assert float((torch.from_numpy(g) - tp.grad).abs().max()) <= 1e-12 * float(tp.grad.abs().max())
        assert float((torch.from_numpy(p_new) - tp.detach()).abs().max()) <= 1e-12 * upd, (step, upd)
        st = opt.state[tp]
        assert float((torch.from_numpy(m) - st["exp_avg"]).abs().max()) <= 1e-12 * float(st["exp_avg"].abs().max())
        assert float((torch.from_numpy(v) - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max())
        p = p_new


def test_effective_beta2_is_the_f32_value():
    hp = R.hyper(*R.HYPER["celeb"])
    assert abs(float(hp[2]) - 0.99900001287) < 1e-11 and float(f32(1) - hp[2]) == 1.0 - float(hp[2])   # 1 - beta is exact in f32


def test_bf16_rounding_is_torchs():
    x = np.random.default_rng(2).standard_normal(100_003).astype(f32) * f32(3)
    sp = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,
                   0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000], np.uint32).view(f32)
    for t in (x, sp):
        want = torch.from_numpy(t.copy()).to(torch.bfloat16)
        assert torch.equal(R.bf16(t).view(torch.int16), want.view(torch.int16))
    assert R.bf16_bits(sp).tolist()[4:8] == [0x0000, 0x0002, 0x3F80, 0x3F82] and R.bf16_bits(sp)[12] == 0x7F80
    nan = np.array([0x7FC00000, 0x7F800001, 0xFFC12345], np.uint32).view(f32)
    assert bool(R.bf16(nan).float().isnan().all())


@pytest.mark.parametrize("t,co,ci", [(9, 12, 20), (1, 5, 64), (1, 1, 1), (9, 33, 31)])
def test_dgrad_weight_copy_is_flip_and_permute(t, co, ci):
    w = torch.randn(t, co, ci, generator=torch.Generator().manual_seed(3))
    assert torch.equal(torch.from_numpy(R.dgrad_weight(w.numpy())), w.flip(0).permute(0, 2, 1).contiguous())


def _phase_conv(x, wf, plane):
    """plane (py, px) of the sub-pixel form: out[Y, X] = sum_ab wf[plane * 4 + a * 2 + b] x[Y - 1 + py + a, X - 1 + px + b], zero padded"""
    py, px = plane >> 1, plane & 1
    H, W = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    w = wf[plane * 4:plane * 4 + 4].reshape(2, 2, *wf.shape[1:]).permute(2, 3, 0, 1)         # [Co][Ci][a][b]
    return F.conv2d(xp[..., py:py + H + 1, px:px + W + 1], w)


@pytest.mark.parametrize("Co,Ci,H,W", [(1, 1, 1, 1), (3, 5, 4, 6), (4, 2, 5, 3)])
def test_phase_weights_give_the_nearest_upsample_convolution_exactly(Co, Ci, H, W):
    g = torch.Generator().manual_seed(4)
    w = torch.randint(-4, 5, (9, Co, Ci), generator=g).double()
    x = torch.randint(-4, 5, (2, Ci, H, W), generator=g).double()
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w.reshape(3, 3, Co, Ci).permute(2, 3, 0, 1), padding=1)
    wf = torch.from_numpy(R.phase_weights(w.numpy())).double()
    got = torch.zeros_like(want)
    for plane in range(4):
        got[..., plane >> 1::2, plane & 1::2] = _phase_conv(x, wf, plane)
    assert torch.equal(got, want)


@pytest.mark.parametrize("Co,Ci", [(1, 1), (3, 5)])
def test_fold_is_the_adjoint_of_the_phase_map(Co, Ci):
    g = torch.Generator().manual_seed(5)
    W = torch.randint(-4, 5, (9, Co, Ci), generator=g).float().numpy()
    D = torch.randint(-4, 5, (16, Co, Ci), generator=g).float().numpy()
    fold = R.phase_fold(D, np.zeros_like(W))
    assert float((fold.astype(np.float64) * W).sum()) == float((D.astype(np.float64) * R.phase_weights(W)).sum())
    pre = torch.randint(-4, 5, (9, Co, Ci), generator=g).float().numpy()
    assert np.array_equal(R.phase_fold(D, pre), pre + fold)                                    # it ADDS to dW


def test_zero_mask_and_table():
    tab, total = R.zero_table([5, 0, 9], [2, 1, 1])
    assert tab.tolist() == [5, 0, 9, 0, 2, 3, 4] and total == 4
    m = R.zero_mask(48, [5, 0, 9], [2, 1, 1])
    assert m.reshape(12, 4).all(1).tolist() == [True, False, False, False, False, True, True, False, False, True, False, False]
    with pytest.raises(AssertionError):
        R.zero_mask(48, [0, 1], [2, 1])


def test_grid_for():
    assert [R.grid_for(n) for n in (1, 3, 4, 1024, 1027, 1028, 100_003, R.SIZES[-1])] == [1, 1, 1, 1, 1, 2, 98, 2048]


def test_exact_pairs_are_what_they_claim():
    for n in SMALL:
        gx, ga, knob = R.cancelling_int_pair(n)
        xx, aa, xa = R.int_sums(gx, ga)
        s = knob / math.sqrt(aa)
        assert s == 2 and xx - 2 * s * xa + s * s * aa == 0
        for r10 in (5, -3):
            xx, aa, xa = R.int_sums(*R.ratio_pair(n, r10))
            assert 10 * xa == r10 * aa, (n, r10)


# ------------------------------------------------------------------ the reference alone inside the GPU test's bounds
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", R.SIZES)
def test_f32_restatement_keeps_the_scalar_bounds_on_gaussian_data(n, mode):
    knob = 1e-2 if mode == 1 else 5.0
    gx, ga = R.gauss_pair(n, n + mode)
    blk = R.scalars_f32(*R.norm_sums_f32(gx, ga), mode, knob, 1.0, 0.95, 0.999, 0)
    worst = R.scalar_errors(blk, R.scalar_bounds(gx, ga, mode, knob, 1.0))
    print(f"[optimizer-host] n {n} mode {mode}: error / allowed " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n", R.SIZES)
def test_f32_restatement_keeps_the_bounds_on_a_near_cancelling_pair(n):
    gx, ga = R.near_cancelling_pair(n, n + 3, 5.0)
    blk = R.scalars_f32(*R.norm_sums_f32(gx, ga), 0, 5.0, 1.0, 0.95, 0.999, 0)
    worst = R.scalar_errors(blk, R.scalar_bounds(gx, ga, 0, 5.0, 1.0))
    print(f"[optimizer-host] near-cancelling n {n}: error / allowed " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n", SMALL)
def test_f32_restatement_on_integer_data_is_exact(n):
    gx, ga = R.int_pair(n, n)
    xx, aa, xa = R.int_sums(gx, ga)
    assert R.norm_sums_f32(gx, ga) == (float(xx), float(aa), float(xa))
    gx, ga, knob = R.cancelling_int_pair(n)
    blk = R.scalars_f32(*R.norm_sums_f32(gx, ga), 0, knob, 1.0, 0.95, 0.999, 0)
    assert blk[4] == 0 and blk[5] == 1 and blk[3] == 2 and not np.isnan(blk).any()
    blk = R.scalars_f32(*R.norm_sums_f32(*R.ratio_pair(n, 5)), 1, 1e-2, 1.0, 0.95, 0.999, 0)
    assert blk[3] == 0
    blk = R.scalars_f32(*R.norm_sums_f32(*R.ratio_pair(n, -3)), 1, 1e-2, 1.0, 0.95, 0.999, 0)
    assert blk[3] == f32(-(float(f32(1e-2)) + 0.3))


@pytest.mark.parametrize("b1,b2", R.BETAS)
def test_bias_corrections_in_double_are_within_2u_and_in_f32_are_not(b1, b2):
    worst64, worst32 = 0.0, {}
    for k in [1, 2, 3, 6, 31, 100, 1000, 100_000]:
        e64 = R.bias_correction_errors(R.scalars_f32(1.0, 1.0, 0.0, 2, 5.0, 1.0, b1, b2, k - 1, pow64=True), b1, b2, k)
        e32 = R.bias_correction_errors(R.scalars_f32(1.0, 1.0, 0.0, 2, 5.0, 1.0, b1, b2, k - 1, pow64=False), b1, b2, k)
        print(f"[optimizer-host] betas {b1, b2} step {k}: |bc1 err| / u, |bc2_sqrt err| / u: double pow {e64[0]:.2f} {e64[1]:.2f}; f32 pow {e32[0]:.2f} {e32[1]:.2f}")
        worst64, worst32[k] = max(worst64, *e64), max(e32)
    assert worst64 <= 2.0
    assert all(worst32[k] > 2.0 for k in (2, 3, 6)), worst32


# ------------------------------------------------------------------ the step-precision test's reference side, and the predicted defect
@pytest.mark.parametrize("zero_init", [True, False], ids=["p0=0", "p0~N(0,1)"])
@pytest.mark.parametrize("name", ["lr5e-3", "sd"])
def test_f32_restatement_keeps_4x_torch_and_the_f32_pow_does_not(name, zero_init):
    """Against the f64 update, relative to the update's size: torch's own f32 CPU AdamW (e_ref), the restatement with
    `1.f - powf(beta, step)` (numpy's correctly rounded f32 pow standing in for the device's) and the restatement with the bias
    corrections in double.  The latter stays within 4 x e_ref at every step; the former exceeds it at steps 2, 3 and 6 where p0 = 0
    isolates the update."""
    hp = R.hyper(*R.HYPER[name])
    for k in R.STEPS:
        g, p0, m, v = R.precision_case(k, hp, zero_init)
        z = np.zeros_like(g)
        (pr, mr, vr, _), _ = R.step_f64(g, z, p0, m, v, k, hp, 2, 5.0, 1e30)
        e_ref = R.update_errors(R.torch_adamw(g, p0, m, v, k, hp, torch.float32), (pr, mr, vr), p0)
        xx = R.norm_sums_f32(g, z)
        e = {}
        for pow64 in (False, True):
            blk = R.scalars_f32(*xx, 2, 5.0, 1e30, hp[1], hp[2], k - 1, pow64=pow64)
            assert blk[3] == 0 and blk[5] == 1 and blk[6] == k
            e[pow64] = R.update_errors(R.adamw_f32(g, z, p0, m, v, blk, hp)[:3], (pr, mr, vr), p0)
        print(f"[optimizer-host] {name} {'p0=0' if zero_init else 'p0~N'} step {k}: p error / update: torch f32 {e_ref[0]:.2e}, f32 pow {e[False][0]:.2e} "
              f"({e[False][0] / e_ref[0]:.1f} x), double pow {e[True][0]:.2e} ({e[True][0] / e_ref[0]:.2f} x); m {e[True][1] / e_ref[1]:.2f} x, v {e[True][2] / e_ref[2]:.2f} x")
        assert all(e[True][i] <= 4 * e_ref[i] for i in range(3)), (k, e[True], e_ref)
        if zero_init and k in (2, 3, 6):
            assert e[False][0] > 4 * e_ref[0], (k, e[False], e_ref)


def test_decay_forms():
    for name in R.HYPER:
        hp = R.hyper(*R.HYPER[name])
        two, fused = R.decay_two_roundings(hp), R.decay_fused(hp)
        print(f"[optimizer-host] {name}: decay = 1.f - lr * wd: two roundings {float(two)!r}, fused {float(fused)!r}")
        assert two.dtype == f32 and abs(float(two) - float(fused)) <= 2.0 ** -24

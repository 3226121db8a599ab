"""LoRA on the UNet's 3x3 convolutions on the GPU (csrc/lora.hip siss_lora_project_conv / siss_lora_merge_conv, siss_amd/lora.py
conv_targets, SISSStepper(lora=...), deletion.lora.conv_targets), against the f64 restatement of tests/lora_conv_ref.py.

* siss_lora_project_conv: dA[t], dB of one table of five conv targets at unequal offsets -- (48, 40), (17, 130), (3, 64): fewer rows
  than one MFMA tile, conv_out's class; (130, 5): I % 4 != 0, the scalar load path, rows not 16-byte aligned; (320, 128): several
  row tiles -- element by element within the dot-product bound (K + 2) 2^-24 s sum |.||.| with K = 9 I for dB (ONE reduction over
  the taps) and K = O for dA: K - 1 additions and one product per term, the scaling by s one more rounding; derived, not measured.
  r = 1, 3, 4, 16, 64, one and two sets; outputs overwritten; padding, the linear block in front and the guard bands untouched; two
  runs bitwise equal; bad arguments refused.
* siss_lora_merge_conv: within (r + 2) 2^-24 (|W0| + s |B| |A[t]|); B = 0 and s = 0 give W0 bit for bit; the shadow is the bf16 of the
  master; the null-shadow form; nothing outside the targets' [9, O, I] stretches changes.
* one LoRAState with linear AND conv targets: project() / merge() agree with both restatements, neither block disturbs the other.
* the step on the f32 engine (CELEB_TOY on the fused schedule, sd-tiny) against torch autograd in f64 through W0 + s B A and
  optimizer_ref on the adapter buffer, at tests/test_hip_f32_mode.py's RTOL; conv targets: a resnet's conv1 and conv2, the stride-2
  downsampler, the upsampler in its sub-pixel form, conv_out -- each with a derived operand copy of its own -- and one linear target.
* invariants of three bf16 steps, the adapter file through load_lora / unload_lora, the captured step, the task.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import lora_conv_ref as CR
import lora_ref as LR
import optimizer_ref as R
from test_hip_f32_mode import CELEB_TOY, RTOL, SD_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 64
OI = [(48, 40), (17, 130), (3, 64), (130, 5), (320, 128)]
GAPS = [192, 128, 192, 64, 320]                               # floats in front of each target: unequal offsets, all multiples of ALIGN
LINEAR = [(64, 24, 40), (64 + 24 * 40 + 64, 40, 8)]          # a linear block in front of the conv block of the same LoRA buffer
RANKS = [1, 3, 4, 16, 64]
GUARD = 1024
SENTINEL = -7.25


def _offsets():
    out, off = [], 0
    for (O, I), gap in zip(OI, GAPS):
        off += gap
        out.append((off, O, I))
        off += -(-9 * O * I // ALIGN) * ALIGN
    return out, off + 256


SHAPES, P_TOTAL = _offsets()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


_CASES = {}


def case(r):
    """The table, adapters and gradients of rank r (host side, computed once): a linear block [0, L0) in front of the conv block."""
    if r not in _CASES:
        from siss_amd import lora as LO
        lrows, L0, lw0, _, _ = LO.layout(LINEAR, r, ALIGN)
        rows, L, w0_floats, ptiles, mtiles = LO.conv_layout(SHAPES, r, ALIGN, base=L0, w0_base=lw0)
        assert rows[0][1] == L0 > 0 and rows[0][3] == lw0 > 0
        assert ptiles == sum(-(-O // 64) + 9 * -(-I // 64) for O, I in OI) and mtiles == sum(9 * -(-O // 64) * -(-I // 64) for O, I in OI)
        for row in rows:                        # every stretch the kernels may touch lies inside its buffer
            assert row[0] + 9 * row[4] * row[5] <= P_TOTAL and row[3] + 9 * row[4] * row[5] <= w0_floats
            assert row[1] + 9 * r * row[5] <= L and row[2] + row[4] * r <= L
        rng = np.random.default_rng(20 + r)
        used = CR.used_mask(L, rows, r)
        p = np.zeros(L, np.float32)
        p[used] = rng.standard_normal(int(used.sum())).astype(np.float32)
        p[:L0] = 1.5                                                         # the linear block: never read by the conv launches
        grads = rng.standard_normal((2, P_TOTAL)).astype(np.float32)
        grads[1] *= 0.5
        w0 = rng.standard_normal(w0_floats).astype(np.float32)
        _CASES[r] = dict(rows=rows, L=L, L0=L0, ptiles=ptiles, mtiles=mtiles, used=used, p=p, grads=grads, w0=w0, s=2.0 / r ** 0.5,
                         jobs=LO.conv_job_table(rows))
    return _CASES[r]


def guarded(n, dev, fill=0.0, dtype=torch.float32):
    """(whole buffer, the n elements between two sentinel guard bands)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    whole[GUARD:GUARD + n] = fill
    return whole, whole[GUARD:GUARD + n]


def table(c, dev):
    return torch.from_numpy(c["jobs"].view(np.uint8).reshape(-1)).to(dev)


def run_project(dev, r, nsets, prefill=0.0):
    from siss_amd import lib
    c = case(r)
    whole, g = guarded(2 * c["L"], dev)
    g = g.view(2, c["L"])
    if prefill:
        g[:, torch.from_numpy(c["used"]).to(dev)] = prefill       # the outputs are OVERWRITTEN, not accumulated into
    g[:, :c["L0"]] = 5.5                                          # the linear block of the same buffer
    lib.call("siss_lora_project_conv", torch.from_numpy(c["grads"]).to(dev), P_TOTAL, nsets, torch.from_numpy(c["p"]).to(dev), g, c["L"],
             table(c, dev), len(c["rows"]), r, c["s"], c["ptiles"])
    torch.cuda.synchronize()
    return whole.cpu(), g.cpu()


# ================================================================ siss_lora_project_conv
@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("r", RANKS)
def test_project_conv_within_the_dot_product_bound(dev, r, nsets):
    c = case(r)
    whole, g = run_project(dev, r, nsets, prefill=3.0)
    ref, bound = CR.project(c["grads"], c["rows"], c["p"], r, c["s"], nsets)
    err = np.abs(g.numpy().astype(np.float64) - ref)
    used = c["used"]
    worst = float((err / np.maximum(bound, 1e-300))[:, used][:nsets].max())
    print(f"[lora conv] project r {r} nsets {nsets}: worst error / bound {worst:.3f}")
    assert (err[:, used] <= bound[:, used]).all(), (r, nsets, worst)
    assert np.abs(ref[0]).max() > 1 and g[0].abs().max() > 1
    for row in c["rows"]:                                      # every tap's dA and the dB were written (nothing left at the prefill)
        assert not (g[:nsets, row[1]:row[1] + 9 * r * row[5]] == 3.0).any() and not (g[:nsets, row[2]:row[2] + row[4] * r] == 3.0).any()
    if nsets == 1:
        assert not g[1, c["L0"]:].any(), "nsets = 1: the second LoRA gradient set is zero"
    else:
        assert not torch.equal(g[0], g[1])
    assert (g[:, :c["L0"]] == 5.5).all(), "the linear block of the same buffer was written"
    pad = torch.from_numpy(~used)
    pad[:c["L0"]] = False
    assert not g[:, pad].any(), "the padding between the tensors must stay zero"
    assert (whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all(), "guard band written"
    _, again = run_project(dev, r, nsets, prefill=-1.0)
    assert torch.equal(bits(g), bits(again)), "two runs differ"


def test_conv_launchers_refuse_bad_arguments(dev):
    from siss_amd import lib
    c = case(4)
    jobs = table(c, dev)
    n = len(c["rows"])
    g, p, dw = torch.zeros(2, c["L"] + 4, device=dev), torch.zeros(c["L"] + 4, device=dev), torch.from_numpy(c["grads"]).to(dev)
    p[:c["L"]] = torch.from_numpy(c["p"]).to(dev)
    w0 = torch.zeros(c["w0"].size + 4, device=dev)
    flat = torch.zeros(P_TOTAL + 4, device=dev)
    for r, nsets in ((0, 2), (65, 2), (4, 3), (4, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_lora_project_conv", dw, P_TOTAL, nsets, p, g, c["L"], jobs, n, r, 1.0, c["ptiles"])
    for args in ((dw.view(-1)[1:], P_TOTAL, 2, p, g, c["L"]), (dw, P_TOTAL, 2, p[1:], g, c["L"]), (dw, P_TOTAL, 2, p, g.view(-1)[1:], c["L"]),
                 (dw, P_TOTAL + 2, 2, p, g, c["L"]), (dw, P_TOTAL, 2, p, g, c["L"] + 2)):        # misaligned bases / set strides
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_lora_project_conv", *args, jobs, n, 4, 1.0, c["ptiles"])
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_lora_project_conv", dw, P_TOTAL, 2, p, g, c["L"], jobs, 0, 4, 1.0, c["ptiles"])
    for r in (0, 65):
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_lora_merge_conv", flat, None, w0, p, jobs, n, r, 1.0, c["mtiles"])
    for f, w, pp in ((flat[1:], w0, p), (flat, w0[1:], p), (flat, w0, p[1:])):
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_lora_merge_conv", f, None, w, pp, jobs, n, 4, 1.0, c["mtiles"])
    torch.cuda.synchronize()
    assert not g.any() and not flat.any(), "a refused call wrote"


# ================================================================ siss_lora_merge_conv
def run_merge(dev, r, p, s, with_shadow):
    from siss_amd import lib
    c = case(r)
    fw, flat = guarded(P_TOTAL, dev, fill=SENTINEL + 1)
    sw, shadow = guarded(P_TOTAL, dev, fill=SENTINEL + 1, dtype=torch.bfloat16)
    lib.call("siss_lora_merge_conv", flat, shadow if with_shadow else None, torch.from_numpy(c["w0"]).to(dev), torch.from_numpy(p).to(dev),
             table(c, dev), len(c["rows"]), r, s, c["mtiles"])
    torch.cuda.synchronize()
    return fw.cpu(), flat.cpu(), sw.cpu(), shadow.cpu()


@pytest.mark.parametrize("with_shadow", [True, False], ids=["bf16-shadow", "null-shadow"])
@pytest.mark.parametrize("r", RANKS)
def test_merge_conv_within_the_bound_and_touches_the_targets_only(dev, r, with_shadow):
    c = case(r)
    fw, flat, sw, shadow = run_merge(dev, r, c["p"], c["s"], with_shadow)
    ref, bound = CR.merge(np.full(P_TOTAL, SENTINEL + 1), c["rows"], c["w0"], c["p"], r, c["s"])
    tm = CR.target_mask(P_TOTAL, c["rows"])
    err = np.abs(flat.numpy().astype(np.float64) - ref)
    print(f"[lora conv] merge r {r}: worst error / bound {float((err[tm] / bound[tm]).max()):.3f}")
    assert (err[tm] <= bound[tm]).all()
    outside = torch.from_numpy(~tm)
    assert (flat[outside] == SENTINEL + 1).all() and (fw[:GUARD] == SENTINEL).all() and (fw[-GUARD:] == SENTINEL).all()
    assert (sw[:GUARD] == SENTINEL).all() and (sw[-GUARD:] == SENTINEL).all() and (shadow[outside] == SENTINEL + 1).all()
    inside = torch.from_numpy(tm)
    assert not (flat[inside] == SENTINEL + 1).any(), "a float of a target was not written"
    if with_shadow:
        assert torch.equal(bits(shadow[inside]), bits(flat[inside].to(torch.bfloat16))), "the shadow is not the bf16 of the master"
        assert torch.equal(bits(shadow[inside]), bits(R.bf16(flat[inside].numpy())))
    else:
        assert (shadow == SENTINEL + 1).all()
    # B = 0 (the state a run starts from): W0, and s = 0 (unload): W0 bit for bit
    p0 = c["p"].copy()
    for row in c["rows"]:
        p0[row[2]:row[2] + row[4] * r] = 0
    for p, s in ((p0, c["s"]), (c["p"], 0.0)):
        _, flat0, _, shadow0 = run_merge(dev, r, p, s, with_shadow)
        for row in c["rows"]:
            n = 9 * row[4] * row[5]
            w0 = torch.from_numpy(c["w0"][row[3]:row[3] + n])
            assert torch.equal(bits(flat0[row[0]:row[0] + n]), bits(w0))
            if with_shadow:
                assert torch.equal(bits(shadow0[row[0]:row[0] + n]), bits(w0.to(torch.bfloat16)))


# ================================================================ one state, linear AND conv targets
LIN = {"plain": r"attentions\.0\.to_q\.weight", "cond": r"attn2\.to_k\.weight"}
CONV5 = (r"^down_blocks\.0\.resnets\.0\.conv[12]\.weight|^down_blocks\.0\.downsamplers\.0\.conv\.weight|"
         r"^up_blocks\.0\.upsamplers\.0\.conv\.weight|^conv_out\.weight")
UPCONV = "up_blocks.0.upsamplers.0.conv.weight"


def pick(specs, kind):
    """(one linear target, the five conv targets: a resnet's conv1 and conv2, the downsampler, the upsampler, conv_out)"""
    lin = [n for n in specs if re.search(LIN[kind], n)][:1]
    conv = [n for n in specs if re.search(CONV5, n)]
    assert len(lin) == 1 and len(conv) == 5 and all(specs[n].kind == "conv3" for n in conv), (lin, conv)
    return lin, conv


def test_mixed_state_project_and_merge_agree_with_both_restatements(dev):
    from siss_amd.lora import LoRAState
    from test_hip_trainable_step import make_engine, weights
    eng = make_engine("plain")
    eng.load_state_dict(weights("plain"))
    ps = eng.ps
    lin = [n for n in ps.specs if re.search(r"attentions\.\d+\.to_(q|out\.0)\.weight", n)]
    _, conv = pick(ps.specs, "plain")
    r = 5
    state = LoRAState(eng, lin, r, 10.0, seed=2, conv_names=conv)
    only_lin, only_conv = LoRAState(eng, lin, r, 10.0, seed=2), LoRAState(eng, [], r, 10.0, seed=2, conv_names=conv)
    g = torch.Generator().manual_seed(3)
    ul = torch.from_numpy(LR.used_mask(state.L, state.rows, r))
    uc = torch.from_numpy(CR.used_mask(state.L, state.conv_rows, r))
    assert not (ul & uc).any() and int((ul | uc).sum()) == state.params
    p = torch.zeros(state.L)
    p[ul | uc] = torch.randn(int((ul | uc).sum()), generator=g)
    state.p.copy_(p)
    ps.grads.copy_(torch.randn(ps.grads.shape, generator=g))
    grads = ps.grads.cpu().numpy()
    for nsets in (2, 1):
        state.g.fill_(3.0)
        state.g[:, ~(ul | uc).to(dev)] = 0.0
        state.project(nsets)
        torch.cuda.synchronize()
        got = state.g.cpu().numpy().astype(np.float64)
        ref_l, b_l = LR.project(grads, state.rows, p.numpy(), r, state.scale, nsets)
        ref_c, b_c = CR.project(grads, state.conv_rows, p.numpy(), r, state.scale, nsets)
        assert (np.abs(got - (ref_l + ref_c)) <= b_l + b_c).all(), nsets
        assert np.abs(ref_l).max() > 0.1 and np.abs(ref_c).max() > 0.1
    # each block is, bit for bit, what a state with that kind alone computes: neither launch disturbs the other
    only_lin.p.copy_(state.p[:only_lin.L])
    only_lin.project(1)
    assert torch.equal(bits(only_lin.g), bits(state.g[:, :only_lin.L]))
    for i in range(len(conv)):
        only_conv.conv_A(i).copy_(state.conv_A(i)); only_conv.conv_B(i).copy_(state.conv_B(i))
    only_conv.project(1)
    for i in range(len(conv)):
        assert torch.equal(bits(only_conv.conv_A(i, only_conv.g)), bits(state.conv_A(i, state.g)))
        assert torch.equal(bits(only_conv.conv_B(i, only_conv.g)), bits(state.conv_B(i, state.g)))
    flat0, shadow0 = ps.flat.clone(), ps.shadow.clone()
    state.merge()
    torch.cuda.synchronize()
    ref, b1 = LR.merge(flat0.cpu().numpy(), state.rows, state.w0.cpu().numpy(), p.numpy(), r, state.scale)
    ref, b2 = CR.merge(ref, state.conv_rows, state.w0.cpu().numpy(), p.numpy(), r, state.scale)
    tm = torch.from_numpy(LR.target_mask(ps.total, state.rows) | CR.target_mask(ps.total, state.conv_rows)).to(dev)
    assert (np.abs(ps.flat.cpu().double().numpy() - ref) <= b1 + b2).all()
    assert torch.equal(bits(ps.flat[~tm]), bits(flat0[~tm])) and torch.equal(bits(ps.shadow[~tm]), bits(shadow0[~tm]))
    assert torch.equal(bits(ps.shadow[tm]), bits(ps.flat[tm].to(torch.bfloat16))) and not torch.equal(ps.flat[tm], flat0[tm])
    state.merge(0.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(ps.flat), bits(flat0)) and torch.equal(bits(ps.shadow), bits(shadow0)), "merge(0) does not restore W0"


# ================================================================ the step, f32 engine, against autograd in f64
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)


def f32_pair(kind, seed):
    """(f32 engine with the sub-pixel upsample on, f64 oracle network, state dict, input channels, text width or None)"""
    if kind == "plain":
        from test_hip_f32_mode import _pair
        eng, net, sd = _pair(CELEB_TOY, seed=seed, fused=True)           # the fused schedule: sub-pixel upsample from 16 pixels up
        return eng, net, sd, 3, None
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.unet_cond import UNetCondEngine
    from oracle.unet_cond import OracleUNet2DCondition, UNetCondConfig
    c = SD_CASES["sd-tiny"]
    oc = UNetCondConfig.tiny(ch=c["ch"], heads=c["heads"], cross_dim=c["cross_dim"], sample_size=c["sample_size"], in_channels=4)
    oc.layers_per_block = c["layers"]
    kw = {k: getattr(oc, k) for k in ("sample_size", "in_channels", "out_channels", "block_out_channels", "down_block_types",
                                      "up_block_types", "layers_per_block", "attention_head_dim", "cross_attention_dim",
                                      "norm_num_groups", "norm_eps", "downsample_padding", "flip_sin_to_cos", "freq_shift")}
    eng = UNetCondEngine(UNet2DConditionConfig(**kw), "cuda:0", dtype=torch.float32)
    eng.f32_fused, eng.subpixel_min_px = True, 16        # the upsampler alone takes its fused (sub-pixel) form; the other switches stay off
    sd = eng.init_random(seed=seed)
    net = OracleUNet2DCondition(oc).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    return eng, net, sd, 4, c["cross_dim"]


@pytest.mark.parametrize("loss_fn", ["importance_sampling_with_mixture", "naive_del"])
@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_f32_conv_lora_steps_match_autograd_through_the_parametrisation(dev, kind, loss_fn):
    """Two optimizer steps, the first over two micro-batches: the adapter gradients of both sets per tensor, the step scalars and the
    update of the adapter buffer against the f64 oracle (W = W0 + s B A under autograd -- peft's Conv2d merge for the convolutions --
    optimizer_ref.step_f64 on the flat adapter buffer), at the f32 mode's RTOL (tests/test_hip_f32_mode.py)."""
    from siss_amd.lora import LoRAState, conv_a_to_ref
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from oracle.loss import OracleDeletionLoss
    from parity_util import masked_update_cosine
    eng, net, sd, ch, xdim = f32_pair(kind, seed=5)
    lin, conv = pick(eng.ps.specs, kind)
    r, alpha = 4, 8.0
    state = LoRAState(eng, lin, r, alpha, seed=2, conv_names=conv)
    nl, nc = len(state.names), len(state.conv_names)
    ac = S.alphas_cumprod()
    single = loss_fn == "naive_del"
    st = SISSStepper(eng, ac, scaling_norm=5.0, lambd=0.5, train_batch_size=2, grad_accum=2, mixed_precision=None, loss_fn=loss_fn,
                     inf_guard=single, lora=state, **HPK)
    assert st.opt.p is state.p and st.opt.m.numel() == state.L and set(st.subset.names) == set(lin + conv)
    hp = R.hyper(HPK["lr"], *HPK["betas"], HPK["eps"], HPK["weight_decay"])
    loss_obj = OracleDeletionLoss(*(v.double() for v in S.gamma_sigma(ac)))
    g = torch.Generator().manual_seed(7)
    m_ref, v_ref = np.zeros(state.L), np.zeros(state.L)
    used_b = np.zeros(state.L, bool)                       # the B's: what carries a gradient in the step from B = 0
    for row in state.rows + state.conv_rows:
        used_b[row[2]:row[2] + row[4] * r] = True
    used = LR.used_mask(state.L, state.rows, r) | CR.used_mask(state.L, state.conv_rows, r)
    # every tensor of the buffer: (name, what, offset, count)
    pieces = [(n, w, o, c) for n, row in zip(state.names, state.rows) for w, o, c in (("A", row[1], r * row[5]), ("B", row[2], row[4] * r))]
    pieces += [(n, w, o, c) for n, row in zip(state.conv_names, state.conv_rows)
               for w, o, c in (("A", row[1], 9 * r * row[5]), ("B", row[2], row[4] * r))]
    for step in range(2):
        st.ga = 2 if step == 0 else 1
        mbs = []
        for _ in range(st.ga):
            mb = dict(x0=torch.rand(2, ch, 16, 16, generator=g) * 2 - 1, a0=(torch.rand(1, ch, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1),
                      noise=torch.randn(2, ch, 16, 16, generator=g), t=torch.tensor([999, 400]), u=torch.tensor([0.9, 0.2]))
            mbs.append(mb)
        ctx = None if xdim is None else torch.randn(2, 13, xdim, generator=g)
        p_before = state.p.cpu().double().numpy()
        # the oracle's parameters in peft's shapes: A [r, I] / [r, Ci * 9] in reference order, B [O, r]
        As = [state.A(i).cpu() for i in range(nl)] + [conv_a_to_ref(state.conv_A(i).cpu()).flatten(1) for i in range(nc)]
        Bs = [state.B(i).cpu() for i in range(nl)] + [state.conv_B(i).cpu() for i in range(nc)]
        model = LR.LoRAOracle(net, list(state.names) + list(state.conv_names), r, state.scale, As, Bs)
        cond64 = {} if ctx is None else {"encoder_hidden_states": ctx.double()}
        gx, ga = LR.oracle_gradients(model, loss_obj, loss_fn, ac.double(), [{k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
                                                                             for mb in mbs], 2, {"lambd": 0.5} if not single else None, cond64)
        n = nl + nc

        def lay(gs):
            out = model.flat(gs[:nl], gs[n:n + nl], state.rows, state.L)
            return CR.flat(gs[nl:n], gs[n + nl:], state.conv_rows, state.L, r, into=out)
        gxf, gaf = lay(gx), lay(ga)
        (p_ref, m_ref, v_ref, g_fin), sc = LR.adapter_step(gxf, gaf, p_before, m_ref, v_ref, step + 1, hp, 2 if single else 0,
                                                           1.0 if single else 5.0, 1.0)
        for mb in mbs:
            st.micro_step(mb["x0"], mb["a0"], mb["noise"], mb["t"].cuda(), mb["u"],
                          None if ctx is None else {"encoder_hidden_states": ctx.cuda()})
        got = st.stats()
        assert UPCONV in eng._up_w, "the upsampler did not take its sub-pixel form"
        lg = state.g.cpu().double().numpy()
        assert not lg[:, ~used].any()
        worst = (0.0, None)
        for k, ref in enumerate((gxf, gaf)):
            tot = np.linalg.norm(ref)
            for name, what, o, cnt in pieces:
                a, b = lg[k, o:o + cnt], ref[o:o + cnt]
                if np.linalg.norm(b) <= 1e-9 * tot:                       # (step 1 from B = 0: dA = 0; naive_del: the second set)
                    assert np.linalg.norm(a) <= 1e-6 * max(tot, 1e-30), (step, k, name, what)
                    continue
                worst = max(worst, (float(np.linalg.norm(a - b) / np.linalg.norm(b)), (k, name, what)))
        keys = {"pre_clip_norm": "pre_clip_norm"} if single else {"norm_loss_x": "norm_x", "norm_loss_a": "norm_a", "scaling_factor": "scale",
                                                                 "pre_clip_norm": "pre_clip_norm"}
        print(f"\n[lora conv] {kind} {loss_fn} step {step}: worst adapter-gradient rel err {worst[0]:.2e} at {worst[1]}; "
              + ", ".join(f"{k} {got[k]:.7g} / {sc[v]:.7g}" for k, v in keys.items()))
        assert worst[0] <= RTOL, worst
        for k, v in keys.items():
            assert abs(got[k] - sc[v]) <= RTOL * abs(sc[v]), (k, got[k], sc[v])
        if step == 0:
            for name, what, o, cnt in pieces:
                if what == "A":
                    assert not state.g[:, o:o + cnt].any(), f"B = 0: dA of {name} must be exactly zero"
                else:
                    assert state.g[0, o:o + cnt].any(), f"dB of {name} is zero"
        # the update, over the elements that carry a gradient in this step (the B's in the step from B = 0, every tensor afterwards)
        live = torch.from_numpy(used_b if step == 0 else used)
        sel = lambda x: {"p": torch.as_tensor(x)[live]}
        cos, frac = masked_update_cosine(sel(p_before), sel(p_ref), sel(state.p.cpu()), sel(g_fin))
        print(f"[lora conv] masked update cosine {cos:.6f} over {frac:.2f} of the elements with a gradient")
        assert cos >= 0.9999 and frac > 0.5, (cos, frac)
        assert not state.p.cpu().numpy()[~used].any(), "the padding of the adapter buffer moved"
        # the master is the merge of what the optimizer left (f32 engine: the operand IS the master)
        flat = eng.ps.flat.cpu().numpy()
        ref_w, b1 = LR.merge(flat, state.rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), r, state.scale)
        ref_w, b2 = CR.merge(ref_w, state.conv_rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), r, state.scale)
        assert (np.abs(flat.astype(np.float64) - ref_w) <= b1 + b2).all()
        tm = LR.target_mask(flat.size, state.rows) | CR.target_mask(flat.size, state.conv_rows)
        assert np.abs(flat[tm] - state_w0_image(state, flat.size)[tm]).max() > 0, "the targets did not move"


def state_w0_image(state, n):
    """[n] f32: W0 of every target at its place in the flat buffer, zero elsewhere"""
    out = np.zeros(n, np.float32)
    w0 = state.w0.cpu().numpy()
    for row in state.rows:
        out[row[0]:row[0] + row[4] * row[5]] = w0[row[3]:row[3] + row[4] * row[5]]
    for row in state.conv_rows:
        out[row[0]:row[0] + 9 * row[4] * row[5]] = w0[row[3]:row[3] + 9 * row[4] * row[5]]
    return out


# ================================================================ invariants on the bf16 engine, the adapter file
def bf16_model(dev):
    """The tiny bf16 UNet with the sub-pixel upsample on (its 8 x 8 upsampler lies below the default threshold)."""
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from test_hip_surface import KW
    from test_hip_trainable_step import weights
    model = UNet2DModel(UNet2DConfig(**KW), device=dev)
    model.engine.subpixel_min_px = 16
    model.load_state_dict(weights("plain"))
    return model


def test_bf16_invariants_and_the_adapter_file_with_conv_targets(dev, tmp_path):
    from safetensors.torch import load_file
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from test_hip_trainable_step import batch
    model = bf16_model(dev)
    eng, ps = model.engine, model.engine.ps
    lin, conv = pick(ps.specs, "plain")
    x, t = batch("plain", 9, dev)[0], torch.tensor([500, 20], device=dev)
    pred0 = eng.forward(x, t).clone()
    assert UPCONV in eng._up_w, "the upsampler did not take its sub-pixel form"
    flat0, shadow0 = ps.flat.clone(), ps.shadow.clone()
    state = LoRAState(eng, lin, 4, 8.0, seed=1, conv_names=conv)
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16", lora=state, **HPK)
    assert st.opt.m.numel() == state.L == st.opt.v.numel() and st.opt.shadow is None
    assert st.trainable_counts() == (state.params, state.tensors) and state.tensors == 12
    assert state.params == sum(4 * sum(ps.specs[n].native_shape) for n in lin) + sum(4 * (ps.specs[n].native_shape[1] + 9 * ps.specs[n].native_shape[2]) for n in conv)
    tm = torch.from_numpy(LR.target_mask(ps.total, state.rows) | CR.target_mask(ps.total, state.conv_rows)).to(dev)
    p_init = state.p.clone()
    for s in range(3):
        st.step(*batch("plain", s, dev))
        torch.cuda.synchronize()
        if s == 0:
            for i, row in enumerate(state.conv_rows):
                assert not state.conv_A(i, state.g).any(), "the first step from B = 0: dA must be exactly zero"
                assert state.conv_B(i).any() and state.conv_B(i, state.g)[0].any(), f"B of {state.conv_names[i]} did not move"
    assert torch.equal(bits(ps.flat[~tm]), bits(flat0[~tm])) and torch.equal(bits(ps.shadow[~tm]), bits(shadow0[~tm])), \
        "a float outside the targets changed"
    for row in state.conv_rows:
        n = 9 * row[4] * row[5]
        assert not torch.equal(ps.flat[row[0]:row[0] + n], flat0[row[0]:row[0] + n]), "a conv target did not move"
    assert not torch.equal(state.p, p_init)
    trained_flat, trained_shadow = ps.flat.clone(), ps.shadow.clone()
    assert torch.equal(bits(trained_shadow[tm]), bits(trained_flat[tm].to(torch.bfloat16)))
    ps.flat[tm] = 0.0                                        # ... and the targets are merge(w0, p), recomputed
    state.merge()
    torch.cuda.synchronize()
    assert torch.equal(bits(ps.flat), bits(trained_flat)) and torch.equal(bits(ps.shadow), bits(trained_shadow))
    ref_w, b1 = LR.merge(flat0.cpu().numpy(), state.rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), 4, state.scale)
    ref_w, b2 = CR.merge(ref_w, state.conv_rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), 4, state.scale)
    assert (np.abs(ps.flat.cpu().double().numpy() - ref_w) <= b1 + b2).all()
    pred_t = eng.forward(x, t).clone()
    assert not torch.equal(pred_t, pred0)
    state.base = "some/base"
    state.save(str(tmp_path / "lora"))
    sd = load_file(str(tmp_path / "lora" / "pytorch_lora_weights.safetensors"))
    for n in conv:
        co, ci = ps.specs[n].ref_shape[:2]
        mod = n[:-len(".weight")]
        assert tuple(sd[f"unet.{mod}.lora_A.weight"].shape) == (4, ci, 3, 3) and tuple(sd[f"unet.{mod}.lora_B.weight"].shape) == (co, 4, 1, 1)
    # a stock model + the adapter: the trained forward, bit for bit; without it again: the stock forward -- every derived copy (phase
    # weights, dgrad copies, the stride-2 copy, conv_out's) follows the merge
    stock = bf16_model(dev)
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred0))
    loaded = stock.load_lora(str(tmp_path / "lora"))
    assert (loaded.names, loaded.conv_names) == (state.names, state.conv_names) and torch.equal(bits(loaded.p), bits(state.p)) and loaded.steps == 3
    assert torch.equal(bits(stock.engine.ps.flat), bits(trained_flat)) and torch.equal(bits(stock.engine.ps.shadow), bits(trained_shadow))
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred_t)), "load_lora(save()) does not reproduce the trained forward"
    # ... and the operand copies only the BACKWARD pass reads (the transposed dgrad weights, the stride-2 downsampler's plane-grouped
    # copy, conv_out's) are those of a model that LOADED the merged weights as a checkpoint, and the sub-pixel phase weights too.
    # (The copies themselves are compared, each a pure function of the weights, after a backward pass has built the lazy ones.)
    cot = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev)

    def derived(engine):
        engine.forward(x, t)
        engine.zero_grad()
        engine.backward(cot, nsets=2)
        torch.cuda.synchronize()
        out = {"wT": engine._wt_all.clone(), "conv_out": engine._wd_out.clone()}
        out.update({"wds " + k: v[0].clone() for k, v in engine._wds.items()})
        out.update({f"up {k} {i}": w.clone() for k, v in engine._up_w.items() for i, w in enumerate(v)})
        assert "wds down_blocks.0.downsamplers.0" in out and f"up {UPCONV} 1" in out, sorted(out)
        return out

    def same(a, b):
        assert sorted(a) == sorted(b)
        return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]
    merged = bf16_model(dev)
    merged.load_state_dict(model.state_dict())
    assert torch.equal(bits(merged.engine.ps.flat), bits(trained_flat))
    d_merged, d_stock = derived(merged.engine), derived(bf16_model(dev).engine)
    assert len(same(d_merged, d_stock)) == len(d_stock), "a derived copy does not depend on the targets"
    assert same(derived(stock.engine), d_merged) == [], "a derived copy did not follow load_lora()"
    with pytest.raises(RuntimeError, match="unload_lora"):
        stock.load_lora(str(tmp_path / "lora"))
    stock.unload_lora()
    assert torch.equal(bits(stock.engine.ps.flat), bits(flat0)) and torch.equal(bits(stock.engine.ps.shadow), bits(shadow0))
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred0)), "the forward after unload_lora() is not the forward before"
    assert same(derived(stock.engine), d_stock) == [], "a derived copy kept the adapter after unload_lora()"
    half = stock.load_lora(str(tmp_path / "lora"), scale=0.5)            # the scale reaches the kernel
    ref_h, bh1 = LR.merge(flat0.cpu().numpy(), half.rows, half.w0.cpu().numpy(), half.p.cpu().numpy(), 4, 0.5 * half.scale)
    ref_h, bh2 = CR.merge(ref_h, half.conv_rows, half.w0.cpu().numpy(), half.p.cpu().numpy(), 4, 0.5 * half.scale)
    got_h = stock.engine.ps.flat.cpu().double().numpy()
    assert (np.abs(got_h - ref_h) <= bh1 + bh2).all()
    assert np.abs(got_h - trained_flat.cpu().double().numpy()).max() > 0 and np.abs(got_h - flat0.cpu().double().numpy()).max() > 0


def test_captured_conv_lora_step_equals_eager(dev):
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from test_hip_trainable_step import batch, make_engine, weights
    res = []
    for captured in (False, True):
        eng = make_engine("plain")
        eng.subpixel_min_px = 16
        eng.load_state_dict(weights("plain"))
        lin, conv = pick(eng.ps.specs, "plain")
        state = LoRAState(eng, lin, 4, 8.0, seed=1, conv_names=conv)
        st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16", lora=state, **HPK)
        args = batch("plain", 0, dev)
        p_init = state.p.clone()

        def reset():
            state.p.copy_(p_init)
            state.merge()
            eng.refresh_weights(cast_shadow=True)
            st.opt.m.zero_(); st.opt.v.zero_(); st.opt.scalars.zero_()
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                st.step(*args)
                st.step(*args)
                reset()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    st.step(*args)
            torch.cuda.current_stream().wait_stream(side)
            reset()
            # (the replay overwrites every adapter gradient; the alignment padding of g is zero and stays zero by contract)
            used = torch.from_numpy(LR.used_mask(state.L, state.rows, 4) | CR.used_mask(state.L, state.conv_rows, 4)).to(dev)
            state.g[:, used] = 3.0
            graph.replay()
        else:
            st.step(*args)
        torch.cuda.synchronize()
        res.append((state.p.clone(), eng.ps.flat.clone(), st.opt.scalars.clone()))
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b)), "the replayed conv LoRA step differs from the eager one"
    assert not torch.equal(res[0][0], p_init)


# ================================================================ the task
def test_delete_tshirt_with_conv_lora_writes_the_adapter_and_logs_it(dev, tmp_path):
    from safetensors.torch import load_file
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/out",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "mixed_precision=bf16",
                     "+dataloader_num_workers=1", "+deletion.lora={rank:4,conv_targets:['resnets\\.\\d+\\.conv[12]\\.weight']}"])
    cfg.unet = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
                    down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"],
                    layers_per_block=1)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    specs = UNetEngine.param_specs(UNet2DConfig.from_dict(dict(cfg.unet)))
    task.run()
    d = os.path.join(cfg.output_dir, "lora")
    assert sorted(os.listdir(d)) == ["lora_config.json", "pytorch_lora_weights.safetensors"]
    c = json.load(open(os.path.join(d, "lora_config.json")))
    want = [n for n in specs if re.search(r"resnets\.\d+\.conv[12]\.weight", n)]
    assert len(want) >= 8 and all(specs[n].kind == "conv3" for n in want)
    assert c["targets"] == [] and sorted(c["conv_targets"]) == sorted(want) and (c["rank"], c["alpha"], c["steps"]) == (4, 4.0, 2)
    sd = load_file(os.path.join(d, "pytorch_lora_weights.safetensors"))
    assert len(sd) == 2 * len(want)
    moved = 0
    for n in want:
        co, ci = specs[n].ref_shape[:2]
        mod = n[:-len(".weight")]
        a, b = sd[f"unet.{mod}.lora_A.weight"], sd[f"unet.{mod}.lora_B.weight"]
        assert tuple(a.shape) == (4, ci, 3, 3) and tuple(b.shape) == (co, 4, 1, 1)
        moved += bool(b.any())
    assert moved >= len(want) // 2 > 0
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"))]
    params = sum(4 * (specs[n].native_shape[1] + 9 * specs[n].native_shape[2]) for n in want)
    assert len(lines) == 2
    for st in lines:
        assert (st["lora_rank"], st["lora_alpha"], st["lora_params"], st["lora_tensors"]) == (4, 4.0, params, 2 * len(want))
        assert st["lora_conv_tensors"] == 2 * len(want)
        assert (st["trainable_params"], st["trainable_tensors"]) == (params, 2 * len(want))

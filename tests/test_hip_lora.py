"""The LoRA unlearning mode on the GPU (csrc/lora.hip, siss_amd/lora.py, SISSStepper(lora=...), deletion.lora), against the f64
restatement of tests/lora_ref.py.

* siss_lora_project: dA_k, dB_k of one job table with four targets of different shapes at unequal offsets, element by element within
  the dot-product bound (K + 2) 2^-24 s (|B|^T |dW|) resp. (|dW| |A|^T) -- K - 1 additions and one product per term, the scaling by s
  one more rounding; derived, not measured -- for r = 1, 3, 4, 16, 64 and one or two gradient sets; padding and guard bands untouched,
  two runs bitwise equal.
* siss_lora_merge: within (r + 2) 2^-24 (|W0| + s |B| |A|); B = 0 gives W0; the shadow is the bf16 of the master; nothing outside the
  targets' stretches changes; the null-shadow (f32 engine) form.
* the step on the f32 engine (one unconditional, one conditional tiny UNet of tests/test_hip_f32_mode.py) against torch autograd in
  f64 through W0 + s B A and optimizer_ref on the adapter buffer, at that file's RTOL.
* invariants of three bf16 steps, the adapter file through load_lora / unload_lora, the task, and the refusal without the kernels.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import lora_ref as LR
import optimizer_ref as R
from test_hip_f32_mode import CELEB_TOY, RTOL, SD_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 64
SHAPES = [(192, 48, 40), (192 + 1920 + 128, 17, 130), (8192, 320, 768), (8192 + 320 * 768 + 64 * 5, 64, 64)]      # (offset, O, I)
P_TOTAL = SHAPES[-1][0] + 64 * 64 + 256
RANKS = [1, 3, 4, 16, 64]
GUARD = 1024
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


_CASES = {}


def case(r):
    """The table, adapters and gradients of rank r (host side, computed once)."""
    if r not in _CASES:
        from siss_amd import lora as LO
        rows, L, w0_floats, ptiles, mtiles = LO.layout(SHAPES, r, ALIGN)
        rng = np.random.default_rng(10 + r)
        used = LR.used_mask(L, rows, r)
        p = np.zeros(L, np.float32)
        p[used] = rng.standard_normal(int(used.sum())).astype(np.float32)
        grads = rng.standard_normal((2, P_TOTAL)).astype(np.float32)
        grads[1] *= 0.5
        w0 = rng.standard_normal(w0_floats).astype(np.float32)
        _CASES[r] = dict(rows=rows, L=L, ptiles=ptiles, mtiles=mtiles, used=used, p=p, grads=grads, w0=w0, s=2.0 / r ** 0.5,
                         jobs=LO.job_table(rows))
    return _CASES[r]


def guarded(n, dev, fill=0.0, dtype=torch.float32):
    """(whole buffer, the n elements between two sentinel guard bands)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    whole[GUARD:GUARD + n] = fill
    return whole, whole[GUARD:GUARD + n]


def run_project(dev, r, nsets, prefill=0.0):
    from siss_amd import lib
    c = case(r)
    jobs = torch.from_numpy(c["jobs"].view(np.uint8)).to(dev)
    whole, g = guarded(2 * c["L"], dev)
    g = g.view(2, c["L"])
    if prefill:
        g[:, torch.from_numpy(c["used"]).to(dev)] = prefill       # the outputs are OVERWRITTEN, not accumulated into
    lib.call("siss_lora_project", torch.from_numpy(c["grads"]).to(dev), P_TOTAL, nsets, torch.from_numpy(c["p"]).to(dev), g, c["L"], jobs,
             len(c["rows"]), r, c["s"], c["ptiles"])
    torch.cuda.synchronize()
    return whole.cpu(), g.cpu()


# ================================================================ siss_lora_project
@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("r", RANKS)
def test_project_within_the_dot_product_bound(dev, r, nsets):
    c = case(r)
    whole, g = run_project(dev, r, nsets, prefill=3.0)
    ref, bound = LR.project(c["grads"], c["rows"], c["p"], r, c["s"], nsets)
    err = np.abs(g.numpy().astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300))[:, c["used"]][:nsets].max())
    print(f"[lora] project r {r} nsets {nsets}: worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (r, nsets, worst)
    assert np.abs(ref[0]).max() > 1 and g[0].abs().max() > 1
    if nsets == 1:
        assert not g[1].any(), "nsets = 1: the second LoRA gradient set is zero"
    else:
        assert not torch.equal(g[0], g[1])
    assert not g[:, torch.from_numpy(~c["used"])].any(), "the padding between the tensors must stay zero"
    assert (whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all(), "guard band written"
    _, again = run_project(dev, r, nsets, prefill=-1.0)
    assert torch.equal(bits(g), bits(again)), "two runs differ"


def test_project_refuses_bad_arguments(dev):
    from siss_amd import lib
    c = case(4)
    jobs = torch.from_numpy(c["jobs"].view(np.uint8)).to(dev)
    g, p, dw = torch.zeros(2, c["L"], device=dev), torch.from_numpy(c["p"]).to(dev), torch.from_numpy(c["grads"]).to(dev)
    for r, nsets in ((0, 2), (65, 2), (4, 3), (4, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_lora_project", dw, P_TOTAL, nsets, p, g, c["L"], jobs, len(c["rows"]), r, 1.0, c["ptiles"])
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_lora_merge", dw[0], None, torch.from_numpy(c["w0"]).to(dev), p, jobs, len(c["rows"]), 65, 1.0, c["mtiles"])


# ================================================================ siss_lora_merge
def run_merge(dev, r, p, s, with_shadow):
    from siss_amd import lib
    c = case(r)
    jobs = torch.from_numpy(c["jobs"].view(np.uint8)).to(dev)
    fw, flat = guarded(P_TOTAL, dev, fill=SENTINEL + 1)
    sw, shadow = guarded(P_TOTAL, dev, fill=SENTINEL + 1, dtype=torch.bfloat16)
    lib.call("siss_lora_merge", flat, shadow if with_shadow else None, torch.from_numpy(c["w0"]).to(dev), torch.from_numpy(p).to(dev), jobs,
             len(c["rows"]), r, s, c["mtiles"])
    torch.cuda.synchronize()
    return fw.cpu(), flat.cpu(), sw.cpu(), shadow.cpu()


@pytest.mark.parametrize("with_shadow", [True, False], ids=["bf16-shadow", "null-shadow"])
@pytest.mark.parametrize("r", RANKS)
def test_merge_within_the_bound_and_touches_the_targets_only(dev, r, with_shadow):
    c = case(r)
    fw, flat, sw, shadow = run_merge(dev, r, c["p"], c["s"], with_shadow)
    ref, bound = LR.merge(np.full(P_TOTAL, SENTINEL + 1), c["rows"], c["w0"], c["p"], r, c["s"])
    tm = LR.target_mask(P_TOTAL, c["rows"])
    err = np.abs(flat.numpy().astype(np.float64) - ref)
    print(f"[lora] merge r {r}: worst error / bound {float((err[tm] / bound[tm]).max()):.3f}")
    assert (err[tm] <= bound[tm]).all()
    outside = torch.from_numpy(~tm)
    assert (flat[outside] == SENTINEL + 1).all() and (fw[:GUARD] == SENTINEL).all() and (fw[-GUARD:] == SENTINEL).all()
    assert (sw[:GUARD] == SENTINEL).all() and (sw[-GUARD:] == SENTINEL).all() and (shadow[outside] == SENTINEL + 1).all()
    inside = torch.from_numpy(tm)
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
        _, flat0, _, _ = run_merge(dev, r, p, s, with_shadow)
        for row in c["rows"]:
            n = row[4] * row[5]
            assert torch.equal(flat0[row[0]:row[0] + n], torch.from_numpy(c["w0"][row[3]:row[3] + n]))


# ================================================================ the step, f32 engine, against autograd in f64
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)
TARGETS = {"plain": r"attentions\.\d+\.to_(q|k|v|out\.0)\.weight", "cond": r"attn[12]\.to_(q|k|v|out\.0)\.weight"}


def f32_pair(kind, seed):
    """(f32 engine, f64 oracle network, state dict, input channels, text width or None)"""
    if kind == "plain":
        from test_hip_f32_mode import _pair
        eng, net, sd = _pair(CELEB_TOY, seed=seed)
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
    sd = eng.init_random(seed=seed)
    net = OracleUNet2DCondition(oc).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    return eng, net, sd, 4, c["cross_dim"]


@pytest.mark.parametrize("loss_fn", ["importance_sampling_with_mixture", "naive_del"])
@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_f32_lora_steps_match_autograd_through_the_parametrisation(dev, kind, loss_fn):
    """Two optimizer steps, the first over two micro-batches: the adapter gradients of both sets per tensor, the step scalars and the
    update of the adapter buffer against the f64 oracle (W = W0 + s B A under autograd, optimizer_ref.step_f64 on the flat adapter
    buffer), at the f32 mode's RTOL (tests/test_hip_f32_mode.py)."""
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from oracle.loss import OracleDeletionLoss
    from parity_util import masked_update_cosine
    eng, net, sd, ch, xdim = f32_pair(kind, seed=5)
    names = [n for n in sd if re.search(TARGETS[kind], n)]
    r, alpha = 4, 8.0
    state = LoRAState(eng, names, r, alpha, seed=2)
    assert len(state.names) == len(names) > 4
    ac = S.alphas_cumprod()
    single = loss_fn == "naive_del"
    st = SISSStepper(eng, ac, scaling_norm=5.0, lambd=0.5, train_batch_size=2, grad_accum=2, mixed_precision=None, loss_fn=loss_fn,
                     inf_guard=single, lora=state, **HPK)
    assert st.opt.p is state.p and st.opt.m.numel() == state.L and st.subset is not None and set(st.subset.names) == set(names)
    hp = R.hyper(HPK["lr"], *HPK["betas"], HPK["eps"], HPK["weight_decay"])
    loss_obj = OracleDeletionLoss(*(v.double() for v in S.gamma_sigma(ac)))
    g = torch.Generator().manual_seed(7)
    m_ref, v_ref = np.zeros(state.L), np.zeros(state.L)
    used = LR.used_mask(state.L, state.rows, r)
    for step in range(2):
        st.ga = 2 if step == 0 else 1
        mbs = []
        for _ in range(st.ga):
            mb = dict(x0=torch.rand(2, ch, 16, 16, generator=g) * 2 - 1, a0=(torch.rand(1, ch, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1),
                      noise=torch.randn(2, ch, 16, 16, generator=g), t=torch.tensor([999, 400]), u=torch.tensor([0.9, 0.2]))
            mbs.append(mb)
        ctx = None if xdim is None else torch.randn(2, 13, xdim, generator=g)
        p_before = state.p.cpu().double().numpy()
        model = LR.LoRAOracle(net, state.names, r, state.scale, [state.A(i).cpu() for i in range(len(names))],
                              [state.B(i).cpu() for i in range(len(names))])
        cond64 = {} if ctx is None else {"encoder_hidden_states": ctx.double()}
        gx, ga = LR.oracle_gradients(model, loss_obj, loss_fn, ac.double(), [{k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
                                                                             for mb in mbs], 2, {"lambd": 0.5} if not single else None, cond64)
        n = len(names)
        gxf, gaf = model.flat(gx[:n], gx[n:], state.rows, state.L), model.flat(ga[:n], ga[n:], state.rows, state.L)
        (p_ref, m_ref, v_ref, g_fin), sc = LR.adapter_step(gxf, gaf, p_before, m_ref, v_ref, step + 1, hp, 2 if single else 0,
                                                           1.0 if single else 5.0, 1.0)
        for mb in mbs:
            st.micro_step(mb["x0"], mb["a0"], mb["noise"], mb["t"].cuda(), mb["u"],
                          None if ctx is None else {"encoder_hidden_states": ctx.cuda()})
        got = st.stats()
        lg = state.g.cpu().double().numpy()
        assert not lg[:, ~used].any()
        worst = (0.0, None)
        for k, ref in enumerate((gxf, gaf)):
            tot = np.linalg.norm(ref)
            for i, row in enumerate(state.rows):
                for what, (o, cnt) in (("A", (row[1], r * row[5])), ("B", (row[2], row[4] * r))):
                    a, b = lg[k, o:o + cnt], ref[o:o + cnt]
                    if np.linalg.norm(b) <= 1e-9 * tot:                       # (step 1 from B = 0: dA = 0; naive_del: the second set)
                        assert np.linalg.norm(a) <= 1e-6 * max(tot, 1e-30), (step, k, state.names[i], what)
                        continue
                    worst = max(worst, (float(np.linalg.norm(a - b) / np.linalg.norm(b)), (k, state.names[i], what)))
        keys = {"pre_clip_norm": "pre_clip_norm"} if single else {"norm_loss_x": "norm_x", "norm_loss_a": "norm_a", "scaling_factor": "scale",
                                                                 "pre_clip_norm": "pre_clip_norm"}
        print(f"\n[lora] {kind} {loss_fn} step {step}: worst adapter-gradient rel err {worst[0]:.2e} at {worst[1]}; "
              + ", ".join(f"{k} {got[k]:.7g} / {sc[v]:.7g}" for k, v in keys.items()))
        assert worst[0] <= RTOL, worst
        for k, v in keys.items():
            assert abs(got[k] - sc[v]) <= RTOL * abs(sc[v]), (k, got[k], sc[v])
        if step == 0:
            for i, row in enumerate(state.rows):
                assert not state.g[:, row[1]:row[1] + r * row[5]].any(), "B = 0: dA must be exactly zero"
        cos, frac = masked_update_cosine({"p": torch.from_numpy(p_before)}, {"p": torch.from_numpy(p_ref)}, {"p": state.p.cpu()},
                                         {"p": torch.from_numpy(g_fin)})
        print(f"[lora] masked update cosine {cos:.6f} over {frac:.2f} of the adapter buffer")
        # (the mask keeps the elements with a gradient: all of B -- half of this buffer, O = I and no padding -- in the step from
        #  B = 0, where dA = 0; everything from then on)
        assert cos >= 0.9999 and frac > (0.4 if step == 0 else 0.5), (cos, frac)
        assert not state.p.cpu().numpy()[~used].any(), "the padding of the adapter buffer moved"
        # the master is the merge of what the optimizer left (f32 engine: the operand IS the master)
        ref_w, bound = LR.merge(eng.ps.flat.cpu().numpy(), state.rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), r, state.scale)
        assert (np.abs(eng.ps.flat.cpu().double().numpy() - ref_w) <= bound).all()


# ================================================================ invariants on the bf16 engine, the adapter file
def test_bf16_invariants_and_the_adapter_file(dev, tmp_path):
    from siss_amd.config import UNet2DConfig
    from siss_amd.lora import LoRAState
    from siss_amd.model import UNet2DModel
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from test_hip_surface import KW
    from test_hip_trainable_step import batch, weights
    model = UNet2DModel(UNet2DConfig(**KW), device=dev)
    model.load_state_dict(weights("plain"))
    eng, ps = model.engine, model.engine.ps
    names = [n for n in ps.specs if re.search(TARGETS["plain"], n)]
    x, t = batch("plain", 9, dev)[0], torch.tensor([500, 20], device=dev)
    pred0 = eng.forward(x, t).clone()
    flat0, shadow0 = ps.flat.clone(), ps.shadow.clone()
    state = LoRAState(eng, names, 4, 8.0, seed=1)
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16", lora=state, **HPK)
    assert st.opt.m.numel() == state.L == st.opt.v.numel() and st.opt.shadow is None
    assert st.trainable_counts() == (state.params, state.tensors)
    tm = torch.from_numpy(LR.target_mask(ps.total, state.rows)).to(dev)
    p_init = state.p.clone()
    for s in range(3):
        st.step(*batch("plain", s, dev))
        torch.cuda.synchronize()
        if s == 0:
            for row in state.rows:
                assert not state.g[:, row[1]:row[1] + 4 * row[5]].any(), "the first step from B = 0: dA must be exactly zero"
                assert state.B(state.rows.index(row)).any(), "B did not move"
                assert state.g[0, row[2]:row[2] + row[4] * 4].any()
    assert torch.equal(bits(ps.flat[~tm]), bits(flat0[~tm])) and torch.equal(bits(ps.shadow[~tm]), bits(shadow0[~tm])), \
        "a float outside the targets changed"
    assert not torch.equal(ps.flat[tm], flat0[tm]) and not torch.equal(state.p, p_init)
    trained_flat, trained_shadow = ps.flat.clone(), ps.shadow.clone()
    assert torch.equal(bits(trained_shadow[tm]), bits(trained_flat[tm].to(torch.bfloat16)))
    ps.flat[tm] = 0.0                                        # ... and the targets are merge(w0, p), recomputed
    state.merge()
    torch.cuda.synchronize()
    assert torch.equal(bits(ps.flat), bits(trained_flat)) and torch.equal(bits(ps.shadow), bits(trained_shadow))
    ref_w, bound = LR.merge(flat0.cpu().numpy(), state.rows, state.w0.cpu().numpy(), state.p.cpu().numpy(), 4, state.scale)
    assert (np.abs(ps.flat.cpu().double().numpy() - ref_w) <= bound).all()
    pred_t = eng.forward(x, t).clone()
    assert not torch.equal(pred_t, pred0)
    state.base = "some/base"
    state.save(str(tmp_path / "lora"))
    # a stock model + the adapter: the trained forward, bit for bit; without it again: the stock forward
    stock = UNet2DModel(UNet2DConfig(**KW), device=dev)
    stock.load_state_dict(weights("plain"))
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred0))
    loaded = stock.load_lora(str(tmp_path / "lora"))
    assert loaded.names == state.names and torch.equal(bits(loaded.p), bits(state.p)) and loaded.steps == 3
    assert torch.equal(bits(stock.engine.ps.flat), bits(trained_flat))
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred_t)), "load_lora(save()) does not reproduce the trained forward"
    with pytest.raises(RuntimeError, match="unload_lora"):
        stock.load_lora(str(tmp_path / "lora"))
    stock.unload_lora()
    assert torch.equal(bits(stock.engine.ps.flat), bits(flat0)) and torch.equal(bits(stock.engine.ps.shadow), bits(shadow0))
    assert torch.equal(bits(stock.engine.forward(x, t)), bits(pred0)), "the forward after unload_lora() is not the forward before"
    half = stock.load_lora(str(tmp_path / "lora"), scale=0.5)            # the scale reaches the kernel
    ref_h, bound_h = LR.merge(flat0.cpu().numpy(), half.rows, half.w0.cpu().numpy(), half.p.cpu().numpy(), 4, 0.5 * half.scale)
    assert (np.abs(stock.engine.ps.flat.cpu().double().numpy() - ref_h) <= bound_h).all()
    with pytest.raises(RuntimeError, match="no adapter"):
        stock.unload_lora(); stock.unload_lora()


def test_captured_lora_step_equals_eager(dev):
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from test_hip_trainable_step import batch, make_engine, weights
    res = []
    for captured in (False, True):
        eng = make_engine("plain")
        eng.load_state_dict(weights("plain"))
        names = [n for n in eng.ps.specs if re.search(TARGETS["plain"], n)]
        state = LoRAState(eng, names, 4, 8.0, seed=1)
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
            state.g.fill_(3.0)
            graph.replay()
        else:
            st.step(*args)
        torch.cuda.synchronize()
        res.append((state.p.clone(), eng.ps.flat.clone(), st.opt.scalars.clone()))
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b)), "the replayed LoRA step differs from the eager one"


# ================================================================ the task and the surface
def test_delete_sd_with_lora_writes_the_adapter_and_logs_it(dev, tmp_path):
    from safetensors.torch import load_file
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    emb = tmp_path / "prompt.pt"
    torch.save(torch.randn(1, 77, 64), emb)
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/out",
                     "pretrained_model_name_or_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true",
                     "+deletion.lora={rank:4,targets:[attn]}"])
    cfg.validation_prompts = [str(emb)]
    cfg.unet = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=[64, 128],
                    down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"],
                    up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"], attention_head_dim=2, cross_attention_dim=64)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    stock = UNet2DConditionModel(UNet2DConditionConfig.from_dict(dict(cfg.unet)), device=dev)
    initial = stock.engine.init_random(seed=task.seed())
    task.run()
    d = os.path.join(cfg.output_dir, "lora")
    assert sorted(os.listdir(d)) == ["lora_config.json", "pytorch_lora_weights.safetensors"]
    c = json.load(open(os.path.join(d, "lora_config.json")))
    specs = stock.engine.ps.specs
    want = [n for n in specs if "attn" in n and n.endswith(".weight") and specs[n].kind in ("mat", "conv1")]
    assert sorted(c["targets"]) == sorted(want) and (c["rank"], c["alpha"], c["steps"]) == (4, 4.0, 2)
    sd = load_file(os.path.join(d, "pytorch_lora_weights.safetensors"))
    assert len(sd) == 2 * len(want) and all(re.fullmatch(r"unet\..*\.lora_[AB]\.weight", k) for k in sd)
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"))]
    params = sum(4 * sum(specs[n].native_shape) for n in want)
    assert len(lines) == 2
    for st in lines:
        assert (st["lora_rank"], st["lora_alpha"], st["lora_params"], st["lora_tensors"]) == (4, 4.0, params, 2 * len(want))
        assert (st["trainable_params"], st["trainable_tensors"]) == (params, 2 * len(want))
    # the merged model beside it: frozen tensors bit for bit, targets moved -- and the stock weights + the adapter give exactly it
    saved = load_file(os.path.join(cfg.output_dir, "unet", "diffusion_pytorch_model.safetensors"))
    moved = 0
    for n, w in initial.items():
        if n in want:
            moved += not torch.equal(saved[n], w.float())
        else:
            assert torch.equal(bits(saved[n]), bits(w.float())), f"frozen tensor {n} changed"
    assert moved >= len(want) // 2 > 0
    stock.load_lora(d)
    for n, w in stock.state_dict().items():
        assert torch.equal(bits(w), bits(saved[n])), f"{n}: stock + adapter is not the saved merged model"


def test_without_the_key_the_first_step_is_the_full_update(dev):
    """No `lora` anywhere: the parameters after one step are bitwise optimizer_ref.adamw_f32 on the step's own gradients and scalar
    block, every tensor moves and the moments are full size (this test holds with and without the LoRA mode in the tree)."""
    from test_hip_optimizer import restate
    from test_hip_trainable_step import HP, batch, stepper
    eng, st = stepper("plain", None)
    p0 = eng.ps.flat.cpu().numpy().copy()
    st.step(*batch("plain", 0, dev))
    torch.cuda.synchronize()
    assert st.subset is None and st.opt.p is eng.ps.flat and st.opt.m.numel() == eng.ps.total and st.opt.shadow is eng.ps.shadow
    gx, ga = (eng.ps.grads[k].cpu().numpy() for k in (0, 1))
    got = eng.ps.flat.cpu().numpy()
    z = np.zeros_like(p0)
    rp, *_ = restate(gx, ga, p0, z, z, st.opt.scalars.cpu().numpy(), HP, got)
    assert np.array_equal(got.view(np.int32), rp.view(np.int32))
    assert torch.equal(bits(eng.ps.shadow), bits(eng.ps.flat.to(torch.bfloat16)))
    for n, sp in eng.ps.specs.items():
        assert not np.array_equal(got[sp.off:sp.off + sp.numel], p0[sp.off:sp.off + sp.numel]), f"{n} did not move"


def test_a_library_without_the_entry_points_is_refused(dev, monkeypatch):
    from siss_amd import lib
    from siss_amd.lora import LoRAState
    from test_hip_trainable_step import make_engine, weights
    eng = make_engine("plain")
    eng.load_state_dict(weights("plain"))
    names = [n for n in eng.ps.specs if re.search(TARGETS["plain"], n)]
    state = LoRAState(eng, names, 4)
    has = lib.has
    monkeypatch.setattr(lib, "has", lambda name: False if name.startswith("siss_lora_") else has(name))
    flat = eng.ps.flat.clone()
    with pytest.raises(RuntimeError, match="siss_lora_project"):
        LoRAState(eng, names, 4)
    for fn in (state.project, state.merge):
        with pytest.raises(RuntimeError, match="no fall-back"):
            fn()
    assert torch.equal(bits(eng.ps.flat), bits(flat))


def test_lora_and_trainable_together_are_refused_by_the_stepper(dev):
    from siss_amd.lora import LoRAState
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    from test_hip_trainable_step import make_engine, weights
    eng = make_engine("plain")
    eng.load_state_dict(weights("plain"))
    names = [n for n in eng.ps.specs if re.search(TARGETS["plain"], n)]
    state = LoRAState(eng, names, 4)
    with pytest.raises(ValueError, match="trainable"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, lora=state, trainable=names, **HPK)
    with pytest.raises(ValueError, match="another engine"):
        SISSStepper(make_engine("plain"), S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, lora=state, **HPK)

"""A trainable SUBSET through the engine, the stepper, the class surface and the task loops (SISSStepper(trainable=...),
UNetEngine.skip_frozen_wgrad, deletion.trainable), on the small UNet2DModel of tests/test_hip_surface.py (attention tensors
trainable) and the small conditional UNet of tests/test_hip_unet_cond.py (cross-attention, `attn2`, trainable), B = 2.

* skip_frozen_wgrad = False (launch for launch the full update's backward pass): both gradient sets after one micro-step are BITWISE
  those of a stepper without `trainable` (but for the time-embedding gradients, which two identical FULL steps do not repeat bitwise
  either: see the test); the updated trainable parameters are bitwise optimizer_ref.adamw_f32 on them, fed the
  kernel's own scalar block; the frozen parameters are bitwise the loaded ones after three steps.
* skip_frozen_wgrad = True: the queue issued fewer products by exactly the number whose outputs are all frozen (counted here by
  recording every described product's outputs against the parameter names); the trainable stretches of both gradient sets equal
  those of the False mode -- bitwise per tensor, or, for a tensor whose product ran in another grouped launch (another split
  count, another order of its f32 additions), within the bound tests/test_hip_unet.py holds two schedules of the same products
  to: max |difference| <= 1e-5 max |gradient| (test_side_stream_weight_gradients_equal_the_main_stream_schedule).
* a step captured with torch.cuda.graph and replayed equals the eager step bitwise; sparse_fill on equals sparse_fill off bitwise
  over three steps and does not raise.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as R
from test_hip_optimizer import hold, restate
from test_hip_surface import KW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)
HP = R.hyper(HPK["lr"], *HPK["betas"], HPK["eps"], HPK["weight_decay"])
PATTERN = {"plain": "attentions", "cond": "attn2"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def make_engine(kind):
    if kind == "plain":
        from siss_amd.config import UNet2DConfig
        from siss_amd.unet import UNetEngine
        return UNetEngine(UNet2DConfig(**KW), "cuda:0")
    from siss_amd.unet_cond import UNetCondEngine
    from test_hip_unet_cond import _cfgs
    return UNetCondEngine(_cfgs("tiny")[0], "cuda:0")


_SD = {}


def weights(kind):
    """One random state dict per network, computed once and shared (never modified)."""
    if kind not in _SD:
        _SD[kind] = make_engine(kind).init_random(seed=4)
    return _SD[kind]


def names_of(kind):
    import re
    return [n for n in weights(kind) if re.search(PATTERN[kind], n)]


def batch(kind, step, dev):
    g = torch.Generator().manual_seed(100 + step)
    c = 3 if kind == "plain" else 4
    x0 = (torch.rand(2, c, 16, 16, generator=g) * 2 - 1).to(dev)
    a0 = (torch.rand(1, c, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1).to(dev)
    noise = torch.randn(2, c, 16, 16, generator=g).to(dev)
    t = torch.tensor([999, 300], device=dev)
    u = torch.tensor([0.9, 0.2], device=dev)
    cond = None if kind == "plain" else {"encoder_hidden_states": torch.randn(1, 77, 64, generator=g).repeat(2, 1, 1).to(dev)}
    return x0, a0, noise, t, u, cond


def stepper(kind, trainable, skip=True, sparse_fill=True):
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    eng = make_engine(kind)
    eng.load_state_dict(weights(kind))
    eng.skip_frozen_wgrad, eng.sparse_fill = skip, sparse_fill
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16",
                     trainable=trainable, **HPK)
    return eng, st


_RUNS = {}


def record_forms(eng, forms):
    """Install a launcher on the engine's weight-gradient queue that notes HOW every product runs -- name -> set of forms, for every
    parameter a product's dW / dbias / dbias2 overlap -- and forwards the launch.  The form is what decides the order of a product's
    f32 additions: ("own", nsplits) for a launch of its own with that explicit split count; ("grouped", nsplits field, reduction rows)
    for a member of a grouped table, capped or not (the library derives a grouped job's split count from its own rows alone,
    csrc/gemm_tn.hip, and the capped kernel walks the same blocks); ("pair", nsplits field, rows, the partner's dW offset) for a
    two-product launch, whose block split depends on the partner."""
    from siss_amd import lib
    specs, total, base = sorted(eng.ps.specs.values(), key=lambda sp: sp.off), eng.ps.total, eng.ps.grads.data_ptr()
    end = base + 4 * eng.ps.grads.numel()

    def note(form, dW, extent, N, dbias, dbias2):
        for addr, n in ((dW, extent), (dbias, N), (dbias2, N)):
            if addr and base <= addr < end:              # (a scratch output -- the sub-pixel upsampler's -- names no parameter)
                off = (addr - base) // 4 % total
                for sp in specs:
                    if sp.off < off + n and off < sp.off + sp.numel:
                        forms.setdefault(sp.name, set()).add(form)

    def of_job(j, form):
        note(form, j.dW, j.npanels * j.N * j.C, j.N, j.dbias, j.dbias2)

    def launcher(name, *args, refusable=False):
        rc = lib.call(name, *args, refusable=refusable)
        if name in ("siss_gemm_tn", "siss_gemm_tn_bs"):
            note(("own", args[16]), args[4], args[8] * args[6] * args[7], args[6], args[18], args[19])
        elif name in ("siss_gemm_tn_grouped", "siss_gemm_tn_grouped_capped"):
            for j in list(args[0])[:args[1]]:
                of_job(j, ("grouped", j.nsplits, j.row_end - j.row_begin))
        elif name == "siss_gemm_tn_pair":
            if rc == 0:
                a, b = args[0]._obj, args[1]._obj
                for j, other in ((a, b), (b, a)):
                    of_job(j, ("pair", j.nsplits, j.row_end - j.row_begin, (other.dW - base) // 4 % total))
        else:
            raise AssertionError(f"the weight-gradient queue launched {name}: unknown to this test")
        return rc
    eng.wgrads.launcher = launcher


def run(kind, trainable, skip=True, sparse_fill=True, steps=3, rep=0):
    """`steps` eager steps: (gradients of the first, parameters after each, scalar block of the first, products issued in the first,
    the form every product of the first ran in); rep: another run of the same"""
    key = (kind, None if trainable is None else "subset", skip, sparse_fill, steps, rep)
    if key not in _RUNS:
        dev = torch.device("cuda:0")
        eng, st = stepper(kind, trainable, skip, sparse_fill)
        grads, params, blk, issued = None, [], None, None
        forms = {}
        record_forms(eng, forms)
        for s in range(steps):
            if s == 1:
                eng.wgrads.launcher = None
            n0 = eng.wgrads.issued
            st.step(*batch(kind, s, dev))
            torch.cuda.synchronize()
            if s == 0:
                grads, blk, issued = eng.ps.grads.clone(), st.opt.scalars.cpu().numpy().copy(), eng.wgrads.issued - n0
            params.append(eng.ps.flat.clone())
        _RUNS[key] = dict(grads=grads, params=params, blk=blk, issued=issued, specs=eng.ps.specs, subset=st.subset,
                          loaded=None, shadow=eng.ps.shadow.clone(), forms={n: tuple(sorted(f)) for n, f in forms.items()})
        eng2 = make_engine(kind)
        eng2.load_state_dict(weights(kind))
        _RUNS[key]["loaded"] = eng2.ps.flat.clone()
    return _RUNS[key]


def mask_of(r):
    m = torch.zeros(r["loaded"].numel(), dtype=torch.bool)
    for a, b in r["subset"].stretches:
        m[a:b] = True
    return m


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_launch_for_launch_mode(dev, kind):
    full = run(kind, None)
    sub = run(kind, names_of(kind), skip=False)
    assert sub["subset"] is not None and 0 < sub["subset"].tensors < len(sub["specs"])
    # Bitwise, tensor by tensor -- except the four time-embedding gradients, which the parent's own backward pass does not repeat
    # bitwise between two identical full steps (siss_linear_multi_bwd sums the resnets' contributions in the order its blocks
    # arrive: measured on the conditional UNet, 2.4e-7 .. 9.5e-7 absolute at |g| 5 .. 12, in 15 of 16 repeated full steps against the
    # first): those are held to the bound tests/test_hip_unet.py holds two schedules of the same sums to, 1e-5 max |g|.
    differ = {}
    for n, sp in sub["specs"].items():
        a, b = sub["grads"][:, sp.off:sp.off + sp.numel], full["grads"][:, sp.off:sp.off + sp.numel]
        if n.startswith("time_embedding."):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), n
        elif not torch.equal(bits(a), bits(b)):
            differ[n] = float((a - b).abs().max())
    assert not differ, f"skip_frozen_wgrad = False: {len(differ)} gradient tensors are not the full update's: {list(differ.items())[:8]}"
    assert sub["issued"] == full["issued"]
    m = mask_of(sub).numpy()
    gx, ga = (sub["grads"][k].cpu().numpy()[m] for k in (0, 1))
    p0 = sub["loaded"].cpu().numpy()
    got = sub["params"][0].cpu().numpy()
    z = np.zeros(int(m.sum()), np.float32)
    rp, *_ = restate(gx, ga, p0[m], z, z, sub["blk"], HP, got[m])
    assert np.array_equal(got[m].view(np.int32), rp.view(np.int32)), "trainable parameters after one step: not adamw_f32 on them"
    assert not np.array_equal(got[m], p0[m]), "the trainable parameters did not move"
    for s, p in enumerate(sub["params"]):
        assert np.array_equal(p.cpu().numpy()[~m].view(np.int32), p0[~m].view(np.int32)), f"frozen parameters moved in step {s}"
    hold(sub["blk"], gx, ga, 0, 5.0, f"{kind}: the subset's scalar block")       # the logged norms are the subset's
    assert sub["blk"][0] < full["blk"][0]


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_two_full_steps_differ_in_the_time_embedding_gradients_only(dev, kind):
    """What the exception of test_launch_for_launch_mode stands on: two identical FULL steps (no selection, fresh engines) give every
    gradient bit for bit except, at most, the four time-embedding tensors (float atomicAdd in csrc/timeemb.hip), and those within the
    1e-5 max |g| of that test."""
    a, b = run(kind, None), run(kind, None, rep=1)
    for n, sp in a["specs"].items():
        x, y = a["grads"][:, sp.off:sp.off + sp.numel], b["grads"][:, sp.off:sp.off + sp.numel]
        if n.startswith("time_embedding."):
            assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max()), n
        else:
            assert torch.equal(bits(x), bits(y)), f"{n}: two identical full steps differ by {float((x - y).abs().max())}"
    assert a["forms"] == b["forms"]


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_products_dropped(dev, kind):
    off = run(kind, names_of(kind), skip=False)
    on = run(kind, names_of(kind), skip=True)
    dropped = off["issued"] - on["issued"]
    print(f"[trainable] {kind}: {off['issued']} products with skip_frozen_wgrad off, {on['issued']} with it on")
    assert 0 < dropped < off["issued"]
    specs, sub = on["specs"], on["subset"]
    # How each trainable tensor's product ran in the two passes (record_forms): the same form -- a launch of its own with the same
    # split count, a grouped job over the same rows, a pair with the same partner, or no queue product at all (a gradient some fused
    # kernel forms on the side, launched alike in both passes) -- means the same f32 additions in the same order: BITWISE.  Only a
    # tensor shown to have run in another form may take the named bound.
    same_form, other_form = [], []
    for n in sub.names:
        assert (n in off["forms"]) == (n in on["forms"]), f"{n}: a product in one pass and none in the other"
        (same_form if off["forms"].get(n, ("side",)) == on["forms"].get(n, ("side",)) else other_form).append(n)
    print(f"[trainable] {kind}: {len(same_form)} trainable tensors ran in the same form in both passes, {len(other_form)} in another: "
          f"{[(n, off['forms'][n], on['forms'][n]) for n in other_form[:6]]}")
    assert same_form and sum(n in on["forms"] for n in same_form) > 0, "no product to compare bitwise"
    for n in sub.names:
        sp = specs[n]
        a, b = off["grads"][:, sp.off:sp.off + sp.numel], on["grads"][:, sp.off:sp.off + sp.numel]
        if n in same_form:
            assert torch.equal(bits(a), bits(b)), (n, on["forms"].get(n), float((a - b).abs().max()))
        else:
            scale = float(a.abs().max())
            assert float((a - b).abs().max()) <= 1e-5 * scale, (n, off["forms"][n], on["forms"][n], float((a - b).abs().max()), scale)
    m = mask_of(on)
    for s, p in enumerate(on["params"]):
        assert torch.equal(bits(p.cpu()[~m]), bits(on["loaded"].cpu()[~m])), f"frozen parameters moved in step {s}"
    assert not torch.equal(on["params"][0].cpu()[m], on["loaded"].cpu()[m])


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_dropped_count_is_the_number_of_all_frozen_products(dev, kind):
    """Every product the launch-for-launch pass describes is recorded with the PARAMETERS its outputs (dW over npanels * N * C floats,
    dbias / dbias2 over N) overlap; those that overlap no trainable tensor are the all-frozen ones -- the fused q / k / v and k / v
    products count once, and only when all their tensors are frozen.  (Products that do not pass through WgradQueue.job -- the
    time-embedding linears' own launcher -- are in neither count.)"""
    on = run(kind, names_of(kind), skip=True)
    eng, st = stepper(kind, names_of(kind), skip=False)
    specs, total, base = eng.ps.specs, eng.ps.total, eng.ps.grads.data_ptr()
    order = sorted(specs.values(), key=lambda sp: sp.off)
    recs, inner = [], eng.wgrads.job

    def spy(*a, **k):
        j = inner(*a, **k)
        touched = set()
        for addr, n in ((j.dW, j.npanels * j.N * j.C), (j.dbias, j.N), (j.dbias2, j.N)):
            if addr:
                off = (addr - base) // 4 % total
                touched |= {sp.name for sp in order if sp.off < off + n and off < sp.off + sp.numel}
        recs.append(touched)
        return j
    eng.wgrads.job = spy
    st.step(*batch(kind, 0, dev))
    torch.cuda.synchronize()
    trainable = set(st.subset.names)
    assert all(recs), "a product whose outputs are outside the gradient buffer"
    frozen = sum(not (t & trainable) for t in recs)
    fused = [t for t in recs if sum(n.endswith(".weight") for n in t) > 1]
    print(f"[trainable] {kind}: {len(recs)} products, {frozen} all frozen, {len(fused)} fused")
    assert fused and len(recs) - on["issued"] == frozen > 0, (len(recs), on["issued"], frozen)
    if kind == "cond":                                   # the fused to_k / to_v product of a cross-attention: kept, and one job
        kv = [t for t in recs if any(".attn2.to_k." in n for n in t)]
        assert kv and all(any(".attn2.to_v." in n for n in t) for t in kv)


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_captured_step_equals_eager(dev, kind):
    eager = run(kind, names_of(kind), skip=True)
    eng, st = stepper(kind, names_of(kind), skip=True)
    args = batch(kind, 0, dev)
    loaded = eng.ps.flat.clone()

    def reset():
        eng.ps.flat.copy_(loaded)
        eng.refresh_weights(cast_shadow=True)
        st.opt.m.zero_(); st.opt.v.zero_(); st.opt.scalars.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.step(*args)                                   # settle allocations (and the sparse-fill plan) on the capture stream
        st.step(*args)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st.step(*args)
    torch.cuda.current_stream().wait_stream(side)
    reset()
    eng.ps.grads.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(eng.ps.flat), bits(eager["params"][0])), "replayed parameters differ from the eager step's"
    m = mask_of(eager)
    assert torch.equal(bits(eng.ps.grads.cpu()[:, m]), bits(eager["grads"].cpu()[:, m])), "replayed trainable gradients differ"
    assert np.array_equal(st.opt.scalars.cpu().numpy().view(np.int32), eager["blk"].view(np.int32)), "replayed scalars differ"


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_sparse_fill_stays_valid_under_a_selection(dev, kind):
    on = run(kind, names_of(kind), skip=True, sparse_fill=True)
    off = run(kind, names_of(kind), skip=True, sparse_fill=False)
    for s, (a, b) in enumerate(zip(on["params"], off["params"])):
        assert torch.equal(bits(a), bits(b)), f"step {s}: sparse_fill on / off differ"


def test_a_plan_recorded_under_one_selection_is_not_applied_under_another(dev):
    from siss_amd.trainable import Subset
    from siss_amd.unet import ALIGN
    eng = make_engine("plain")
    sig = eng._wgrad_sig()
    eng.set_trainable(Subset(eng.ps.specs, names_of("plain"), eng.ps.total, ALIGN))
    sig_a = eng._wgrad_sig()
    eng.set_trainable(Subset(eng.ps.specs, names_of("plain")[:2], eng.ps.total, ALIGN))
    sig_b = eng._wgrad_sig()
    eng.skip_frozen_wgrad = False
    assert len({sig, sig_a, sig_b}) == 3 and eng._wgrad_sig() == sig


# ================================================================ the class surface: requires_grad
def test_requires_grad_flags(dev):
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    m = UNet2DModel(UNet2DConfig(**KW), device=dev)
    m.load_state_dict(weights("plain"))
    m.engine.refresh_weights(cast_shadow=True)
    m.requires_grad_(False)
    for n, p in m.named_parameters():
        if "attentions" in n:
            p.requires_grad_(True)
    assert m.trainable_names() == names_of("plain")
    st = SISSStepper(m.engine, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2, mixed_precision="bf16",
                     trainable="requires_grad", **HPK)
    st.step(*batch("plain", 0, dev))
    torch.cuda.synchronize()
    by_names = run("plain", names_of("plain"), skip=True)
    assert torch.equal(bits(m.engine.ps.flat), bits(by_names["params"][0])), "flags and name list give different steps"
    # ... and through autograd on the class surface a frozen parameter's .grad stays None
    x0, _, _, t, _, _ = batch("plain", 0, dev)
    m(x0, t)[0].square().mean().backward()
    for n, p in m.named_parameters():
        assert (p.grad is not None) == ("attentions" in n), n
    # a flag changed AFTER the stepper was built: the class-surface backward follows the flags, not the stepper's selection
    late = dict(m.named_parameters())["mid_block.resnets.0.conv1.weight"]
    late.requires_grad_(True)
    m(x0, t)[0].square().mean().backward()
    assert late.grad is not None and float(late.grad.abs().max()) > 0, "a parameter unfrozen later received a dropped (zero) gradient"
    assert m.engine.wgrads.frozen is st.subset, "the stepper's selection must be back on the engine after the class-surface pass"
    with pytest.raises(ValueError, match="requires_grad"):
        SISSStepper(make_engine("plain"), S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, trainable="requires_grad", **HPK)


# ================================================================ the tasks
def _check_saved(out_dir, initial, pattern, lines):
    import re
    from safetensors.torch import load_file
    saved = load_file(os.path.join(out_dir, "unet", "diffusion_pytorch_model.safetensors"))
    assert set(saved) == set(initial)
    moved = 0
    for n, w in initial.items():
        if re.search(pattern, n):
            moved += not torch.equal(saved[n], w.float())
        else:
            assert torch.equal(bits(saved[n]), bits(w.float())), f"frozen tensor {n} changed"
    names = [n for n in initial if re.search(pattern, n)]
    assert moved >= len(names) // 2 and moved > 0, (moved, len(names))
    assert len(lines) == 2
    for st in lines:
        assert st["trainable_tensors"] == len(names)
        assert st["trainable_params"] == sum(initial[n].numel() for n in names)


def test_delete_celeb_with_trainable_attentions(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import main as entry
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    out = tmp_path / "out"
    small = ["unet.sample_size=16", "unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
             "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1", "unet.attention_head_dim=null"]
    ov = ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent",
          "allow_random_init=true", "allow_synthetic=true", f"data_dir={tmp_path}/nodata", "mixed_precision=bf16", *small]
    entry.main(["--config-name=delete_celeb", f"output_dir={out}", "+deletion.trainable=[attentions]", *ov])
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), ov)
    ucfg = {k: v for k, v in cfg.unet.items() if not k.startswith("_")}
    initial = UNet2DModel(UNet2DConfig.from_dict(ucfg), device=dev).engine.init_random(seed=int(cfg.random_seed))
    rundir = os.path.join(out, os.listdir(out)[0])
    lines = [json.loads(l) for l in open(os.path.join(rundir, "train_log_rank0.jsonl"))]
    _check_saved(rundir, initial, "attentions", lines)


def test_delete_sd_with_trainable_attn2(dev, tmp_path):
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConditionConfig
    from siss_amd.model import UNet2DConditionModel
    emb = tmp_path / "prompt.pt"
    torch.save(torch.randn(1, 77, 64), emb)
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"),
                    ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/out",
                     "pretrained_model_name_or_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true",
                     "+deletion.trainable=[attn2]"])
    cfg.validation_prompts = [str(emb)]
    cfg.unet = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=[64, 128],
                    down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"],
                    up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"], attention_head_dim=2, cross_attention_dim=64)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    initial = UNet2DConditionModel(UNet2DConditionConfig.from_dict(dict(cfg.unet)), device=dev).engine.init_random(seed=task.seed())
    task.run()
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"))]
    _check_saved(cfg.output_dir, initial, "attn2", lines)


# ================================================================ one rank, forced collectives
def test_pieces_exchange_on_one_rank_equals_the_step_without_a_group(dev):
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_trainable_worker.py"), ROOT], capture_output=True, text=True,
                       timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL_TRAINABLE ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line[-1][len("RCCL_TRAINABLE "):])
    assert out["ok"] and out["bitwise_params"] and out["bitwise_trainable_grads"] and out["collective_calls"]["all_reduce"] >= 1, out
    assert out["pieces"] <= 48 and not out["overlap"] and out["exchange"] == "allreduce", out
    # ONE grouped call over the trainable pieces of both gradient sets: 2 x pieces all-reduces inside the step, of exactly the pieces' floats
    assert out["step_all_reduces"] == 2 * out["pieces"] and out["exchanged_floats"] == 2 * out["piece_floats"] >= 2 * out["subset_floats"], out

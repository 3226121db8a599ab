"""csrc/saliency.hip and what stands on it (siss_amd/saliency.py, SISSStepper(saliency=...), deletion.saliency), on the GPU.  Every
comparison is EXACT: the select and the mask are integer work, the masked pair is the whole-buffer pair by construction.

* siss_absf_select / siss_saliency_mask against tests/saliency_ref.py (a sort of the uint32 magnitudes): n in {1, 3, 4, 255, 1025,
  2,097,152 + 5} (the last: one grid-stride round of 2048 x 256 x 4 floats plus a scalar tail), four kinds of input, k in {1, n // 2, n}
  and the number of non-zeros; one NaN / one inf is counted in `nonfinite` and from_gradient raises;
* the masked pair, buffers between sentinel guards (tests/test_hip_optimizer.py's Flat / Scal), n in {4, 36, 1025, 2,097,152 + 5},
  modes 0 / 1 / 2, step counts 1 and 2: an all-ones mask gives p, m, v, shadow, g_out and the scalar block of the whole-buffer pair
  bit for bit; any mask gives the scalar block of the whole-buffer pair on gradients multiplied by the mask, its values on the
  masked-in elements and the old bytes everywhere else; a NaN in a masked-out gradient reaches nothing;
* the stepper on the small UNet of tests/test_hip_surface.py (bf16): an all-ones mask is the plain stepper; a 50 % mask from
  forget_gradient + from_gradient freezes the masked-out floats, and its captured step equals the eager one; forget_gradient leaves the
  training state alone; the f32 engine runs a masked step; lora= / trainable= with saliency= raise;
* delete_celeb with +deletion.saliency: the two mask files, the log fields, the saved UNet, the reload from `path`, and the
  training-stream claim (a run without the key repeats itself, and the keyed run's first step logs its losses and importance weights).

Whole steps are compared bitwise between runs.  That holds on this UNet because every kernel of its step is repeatable: the one
order-dependent sum of the backward pass (csrc/timeemb.hip adds the column splits of the time-embedding cotangent atomically) has two
splits here (832 columns), and two float additions into a zeroed slot commute.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as O
import saliency_ref as R
from test_hip_optimizer import BF, F32, Flat, Scal, T, launch
from test_hip_small_kernels import same
from test_hip_surface import KW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HP = O.hyper(*O.HYPER["sd"])
HPK = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


# ================================================================ select and mask
class Select:
    """Work buffer and result block between guards, reused by every case of the module."""

    def __init__(self, dev):
        from siss_amd import lib
        self.work = Flat(lib.query("siss_absf_select_work_bytes") // 4, torch.int32, dev, fill=-7)
        self.words = lib.query("siss_absf_select_result_words")

    def run(self, dev, g, k):
        buf = Flat(len(g), F32, dev, body=g)
        res = Flat(self.words, torch.int64, dev, fill=-7)
        launch("siss_absf_select", buf.t, len(g), k, self.work.t, res.t)
        buf.check(T(g), "g after the select")
        res.guards("result block")
        self.work.guards("work buffer")
        r = res.t.cpu().tolist()
        assert r[6:] == [0, 0], "the spare words of the result block are not written"
        return dict(threshold_bits=r[0], count_gt=r[1], count_ge=r[2], nonfinite=r[3]), buf


@pytest.fixture(scope="module")
def sel(dev):
    return Select(dev)


@pytest.mark.parametrize("kind", list(R.INPUTS))
@pytest.mark.parametrize("n", R.SIZES)
def test_select_and_mask_equal_the_sorted_reference(dev, sel, n, kind):
    g = R.INPUTS[kind](n, 7 * n + 1)
    ks = R.ranks(g, n)
    assert ks
    for k in ks:
        want = R.select(g, k)
        got, buf = sel.run(dev, g, k)
        print(f"[saliency] {kind} n {n} k {k}: {got}")
        assert got == want, (kind, n, k, got, want)
        again, _ = sel.run(dev, g, k)
        assert again == got, "a second select differs: not repeatable"
        nwords = (n + 31) // 32
        words = Flat(nwords, torch.int32, dev, fill=-7)
        launch("siss_saliency_mask", buf.t, n, want["threshold_bits"], words.t)
        words.check(T(R.mask_words(g, want["threshold_bits"]).view(np.int32)), f"{kind} n {n} k {k}: packed mask (tail bits zero)")
        buf.check(T(g), "g after the mask")


@pytest.mark.parametrize("n", [255, R.SWEEP + 5])
@pytest.mark.parametrize("bad", [np.nan, -np.inf])
def test_one_nonfinite_value_is_counted(dev, sel, n, bad):
    g = R.scaled_normal(n, n)
    g[n // 3] = bad
    got, _ = sel.run(dev, g, max(1, n // 2))
    assert got == R.select(g, max(1, n // 2)) and got["nonfinite"] == 1


# ================================================================ the masked pair
MASKS = {"ones": lambda n: np.ones(n, bool), "half": lambda n: R.random_mask(n, 0.5, n), "sparse": lambda n: R.random_mask(n, 0.03, n + 1),
         "zero words": lambda n: R.zero_word_mask(n, n + 2), "one bit": lambda n: R.single_bit_mask(n, n + 3)}


def knob_of(mode):
    return 1e-2 if mode == 1 else 5.0


class State:
    """p, m, v, shadow, g_out in sentinel buffers (shadow and g_out start from recognisable old values, the same in every run)"""

    def __init__(self, dev, p, m, v, n):
        rng = np.random.default_rng(11)
        old_shadow, old_g = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
        self.p, self.m, self.v, self.g_out = (Flat(n, F32, dev, body=b) for b in (p, m, v, old_g))
        self.shadow = Flat(n, BF, dev, body=old_shadow)

    def args(self):
        return self.p.t, self.m.t, self.v.t, self.shadow.t, self.g_out.t

    def bufs(self):
        return dict(p=self.p, m=self.m, v=self.v, shadow=self.shadow, g_out=self.g_out)


def run_pair(dev, gx, ga, p, m, v, mode, step_before, words=None):
    """The whole-buffer pair (words None) or the masked pair on fresh copies: (scalar block, partial sums, State)."""
    n = len(gx)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    sc, st = Scal(dev, step_before=step_before), State(dev, p, m, v, n)
    hp = [float(h) for h in HP]
    if words is None:
        launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob_of(mode), 1.0, hp[1], hp[2], sc.partials.t, sc.blk.t)
        launch("siss_recombine_clip_adamw", bx.t, ba.t, *st.args(), n, *hp, sc.blk.t)
    else:
        launch("siss_grad_norms_scale_masked", bx.t, ba.t, n, words, mode, knob_of(mode), 1.0, hp[1], hp[2], sc.partials.t, sc.blk.t)
        launch("siss_recombine_clip_adamw_masked", bx.t, ba.t, *st.args(), n, words, *hp, sc.blk.t)
    bx.check(T(gx), "gx after the pair"); ba.check(T(ga), "ga after the pair")
    return sc, st


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [4, 36, 1025, R.SWEEP + 5])
def test_masked_pair_is_the_whole_buffer_pair_on_masked_gradients(dev, n, mode, step):
    rng = np.random.default_rng(n + 10 * mode + step)
    gx, ga = O.gauss_pair(n, n + mode)
    p = rng.standard_normal(n).astype(f32)
    m, v = O.warm_state(n, 3, HP, seed=5) if step == 2 else (np.zeros(n, f32), np.zeros(n, f32))
    for name, make in MASKS.items():
        flags = make(n)
        words = torch.from_numpy(R.pack(flags).view(np.int32)).to(dev)
        mx, ma = (gx, ga) if name == "ones" else (R.masked_gradient(gx, flags), R.masked_gradient(ga, flags))
        sc_w, st_w = run_pair(dev, mx, ma, p, m, v, mode, step - 1)
        sc_m, st_m = run_pair(dev, gx, ga, p, m, v, mode, step - 1, words)
        what = f"n {n} mode {mode} step {step} mask {name!r}"
        same(sc_m.blk.d.cpu(), sc_w.blk.d.cpu(), what + ": scalar block (pads and guards included)")
        assert sc_m.read(n)[6] == step
        if name == "ones":
            same(sc_m.partials.d.cpu(), sc_w.partials.d.cpu(), what + ": partial sums")
        fl = torch.from_numpy(flags)
        for key, buf in st_m.bufs().items():
            whole = st_w.bufs()[key]
            want = whole.flat.clone()                                # guards + the OLD body ...
            body = want[whole.g:whole.g + n]
            body[fl] = whole.d.cpu()[whole.g:whole.g + n][fl]        # ... with the whole-buffer run's values where the bit is set
            same(buf.d.cpu(), want, what + f": {key} (masked-in = the whole-buffer run on masked gradients, every other byte unchanged)")
        if flags.any():                                              # (3 % of 4 floats is an empty mask)
            assert not torch.equal(st_m.p.d.cpu(), st_m.p.flat), what + ": nothing moved"


def test_a_nan_in_a_masked_out_gradient_reaches_nothing(dev):
    n = 1025
    gx, ga = O.gauss_pair(n, 3)
    flags = R.random_mask(n, 0.5, 5)
    flags[[0, 1, 2, 3, 40, 1024]] = False, False, False, False, False, False      # a whole granule, a lane of a mixed one, the tail
    flags[41] = True
    words = torch.from_numpy(R.pack(flags).view(np.int32)).to(dev)
    rng = np.random.default_rng(0)
    p = rng.standard_normal(n).astype(f32)
    m, v = O.warm_state(n, 3, HP, seed=5)
    clean = run_pair(dev, gx, ga, p, m, v, 0, 1, words)
    bx, ba = gx.copy(), ga.copy()
    for i in (1, 40, 1024):
        bx[i] = np.nan
        ba[i] = np.inf
    dirty = run_pair(dev, bx, ba, p, m, v, 0, 1, words)
    same(dirty[0].blk.d.cpu(), clean[0].blk.d.cpu(), "scalar block with NaN / inf in masked-out gradients")
    assert np.isfinite(dirty[0].read(n)[list(O.NAMES.values())]).all()
    for key, buf in dirty[1].bufs().items():
        same(buf.d.cpu(), clean[1].bufs()[key].d.cpu(), f"{key} with NaN / inf in masked-out gradients")


# ================================================================ the stepper
def make_engine(dtype=torch.bfloat16):
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    return UNetEngine(UNet2DConfig(**KW), "cuda:0", dtype=dtype)


_W = {}


def weights():
    if "sd" not in _W:
        _W["sd"] = make_engine().init_random(seed=4)
    return _W["sd"]


def batch(step, dev):
    g = torch.Generator().manual_seed(100 + step)
    x0 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    a0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1).to(dev)
    noise = torch.randn(2, 3, 16, 16, generator=g).to(dev)
    return x0, a0, noise, torch.tensor([999, 300], device=dev), torch.tensor([0.9, 0.2], device=dev)


def stepper(saliency=None, dtype=torch.bfloat16, **kw):
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    eng = make_engine(dtype)
    eng.load_state_dict(weights())
    mask = saliency(eng) if callable(saliency) else saliency
    st = SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, lambd=0.5, train_batch_size=2,
                     mixed_precision="bf16" if dtype == torch.bfloat16 else None, saliency=mask, **HPK, **kw)
    return eng, st


def forget_batches(dev):
    g = torch.Generator().manual_seed(9)
    a0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1)
    while True:
        yield a0


def state_of(eng, st):
    return dict(p=eng.ps.flat.clone(), shadow=eng.ps.shadow.clone(), m=st.opt.m.clone(), v=st.opt.v.clone(), scalars=st.opt.scalars.clone())


def run_steps(eng, st, dev, steps=3):
    logged = []
    for s in range(steps):
        st.step(*batch(s, dev))
        logged.append(st.stats())
    torch.cuda.synchronize()
    return state_of(eng, st), logged


def test_all_ones_mask_is_the_plain_stepper(dev):
    from siss_amd.saliency import SaliencyMask
    plain, plain_log = run_steps(*stepper(), dev)
    ones, ones_log = run_steps(*stepper(SaliencyMask.ones), dev)
    for key in plain:
        assert torch.equal(ones[key].view(torch.uint8), plain[key].view(torch.uint8)), f"{key} after 3 steps under an all-ones mask"
    assert len(ones_log) == 3 and json.dumps(ones_log, sort_keys=True) == json.dumps(plain_log, sort_keys=True), "logged scalars differ"


def test_forget_gradient_leaves_the_training_state_alone(dev):
    from siss_amd.saliency import forget_gradient
    eng, st = stepper()
    st.step(*batch(0, dev))                                  # a warm state: non-zero moments, step count 1, a recorded fill plan
    before = state_of(eng, st)
    plans = dict(eng._fill_plans)
    gen = torch.Generator(device=dev).manual_seed(0)
    # a data-parallel stepper installs its exchange hook on the engine (SISSStepper._early_allreduce): it must be OFF inside every
    # backward pass of forget_gradient, back afterwards, and no collective may be left pending
    hook, seen, inner = (lambda: seen.append("called")), [], eng.backward
    eng.on_early_grads_final = hook

    def spy(*a, **k):
        seen.append(eng.on_early_grads_final)
        return inner(*a, **k)
    eng.backward = spy
    g = forget_gradient(st, forget_batches(dev), 2, generator=gen)
    del eng.backward
    assert seen == [None, None], f"the exchange hook was installed (or called) during forget_gradient: {seen}"
    assert eng.on_early_grads_final is hook and st._pending == []
    eng.on_early_grads_final = None
    torch.cuda.synchronize()
    assert g.shape == (eng.ps.total,) and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for key, t in state_of(eng, st).items():
        assert torch.equal(t.view(torch.uint8), before[key].view(torch.uint8)), f"forget_gradient changed {key}"
    assert int(eng.ps.grads.count_nonzero()) == 0, "the gradient buffers are not zero on return"
    assert st._micro == 0 and eng.wgrad_overwrite is False and dict(eng._fill_plans) == plans
    # the alignment padding holds exact zeros (what lets the select run over the whole buffer)
    real = torch.zeros(eng.ps.total, dtype=torch.bool, device=dev)
    for sp in eng.ps.specs.values():
        real[sp.off:sp.off + sp.numel] = True
    assert int(g[~real].count_nonzero()) == 0
    # one micro-batch twice = two micro-batches of the same images, noise apart: the scale is 1 / (B * n_batches), so magnitudes agree in size
    g1 = forget_gradient(st, forget_batches(dev), 1, generator=torch.Generator(device=dev).manual_seed(0))
    assert 0.25 < float(g.norm() / g1.norm()) < 4.0
    # ... and the step that follows is the step of a stepper that never computed it
    st.step(*batch(1, dev))
    eng2, st2 = stepper()
    st2.step(*batch(0, dev)); st2.step(*batch(1, dev))
    torch.cuda.synchronize()
    assert torch.equal(bits(eng.ps.flat), bits(eng2.ps.flat)), "the step after forget_gradient differs"


def half_mask(eng, st, dev):
    from siss_amd.saliency import SaliencyMask, forget_gradient
    g = forget_gradient(st, forget_batches(dev), 2, generator=torch.Generator(device=dev).manual_seed(0))
    return SaliencyMask.from_gradient(eng, g, 0.5, batches=2, seed=0), g


def test_half_mask_freezes_the_rest_and_captures(dev):
    eng, st = stepper()
    loaded = eng.ps.flat.clone()
    mask, g = half_mask(eng, st, dev)
    ref = R.select(g.cpu().numpy(), mask.k)
    assert mask.count == ref["count_ge"] >= mask.k == round(0.5 * mask.params) and mask.threshold > 0
    assert np.array_equal(mask.bits.cpu().numpy().view(np.uint32), R.mask_words(g.cpu().numpy(), ref["threshold_bits"]))
    st.set_saliency(mask)
    assert st.trainable_counts() == (mask.count, len(eng.ps.specs))
    flags = mask.to_bool()
    states = []
    for s in range(3):
        st.step(*batch(s, dev))
        torch.cuda.synchronize()
        states.append(eng.ps.flat.clone())
        assert torch.equal(bits(eng.ps.flat[~flags]), bits(loaded[~flags])), f"masked-out floats moved in step {s}"
    assert int((bits(eng.ps.flat[flags]) != bits(loaded[flags])).sum()) > 0, "no masked-in float moved"
    assert torch.equal(eng.ps.shadow.view(torch.int16), eng.ps.flat.to(torch.bfloat16).view(torch.int16)), "shadow is not the rounded master"
    # the same first step captured and replayed
    eng2, st2 = stepper()
    mask2, _ = half_mask(eng2, st2, dev)
    assert torch.equal(mask2.bits, mask.bits), "the mask is not repeatable"
    st2.set_saliency(mask2)
    args = batch(0, dev)

    def reset():
        eng2.ps.flat.copy_(loaded)
        eng2.refresh_weights(cast_shadow=True)
        st2.opt.m.zero_(); st2.opt.v.zero_(); st2.opt.scalars.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st2.step(*args)                                  # settle allocations (and the sparse-fill plan) on the capture stream
        st2.step(*args)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st2.step(*args)
    torch.cuda.current_stream().wait_stream(side)
    reset()
    eng2.ps.grads.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(eng2.ps.flat), bits(states[0])), "replayed parameters differ from the eager step's"


def test_from_gradient_refuses_nonfinite_and_too_few_nonzeros(dev):
    from siss_amd.saliency import SaliencyMask
    eng = make_engine()
    g = torch.zeros(eng.ps.total, device=dev)
    g[:1000] = torch.arange(1, 1001, device=dev, dtype=torch.float32)
    with pytest.raises(ValueError, match="fewer than k"):
        SaliencyMask.from_gradient(eng, g, 0.5)
    g[5] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        SaliencyMask.from_gradient(eng, g, 0.5)
    g[5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        SaliencyMask.from_gradient(eng, g, 0.5)
    for bad in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError, match="fraction"):
            SaliencyMask.from_gradient(eng, g, bad)


def test_f32_engine_runs_a_masked_step(dev):
    from siss_amd.saliency import SaliencyMask
    eng, st = stepper(dtype=torch.float32)
    loaded = eng.ps.flat.clone()
    flags = torch.from_numpy(R.random_mask(eng.ps.total, 0.5, 1)).to(dev)
    st.set_saliency(SaliencyMask.from_bool(eng, flags))
    st.step(*batch(0, dev))
    torch.cuda.synchronize()
    assert torch.equal(bits(eng.ps.flat[~flags]), bits(loaded[~flags])) and not torch.equal(eng.ps.flat[flags], loaded[flags])
    assert st.stats()["step"] == 1


def test_saliency_with_lora_or_trainable_raises(dev):
    from siss_amd.lora import LoRAState, parse_lora, select_targets
    from siss_amd.saliency import SaliencyMask
    eng = make_engine()
    eng.load_state_dict(weights())
    mask = SaliencyMask.ones(eng)
    names = [n for n in eng.ps.specs if "attentions" in n]
    with pytest.raises(ValueError, match=r"saliency.*trainable"):
        stepper(lambda e: SaliencyMask.ones(e), trainable=names)
    lcfg = parse_lora(dict(rank=2, targets=[r"attentions\.\d\.to_q\.weight"]))
    lora = LoRAState(eng, select_targets(eng.ps.specs, lcfg.patterns), lcfg.rank, lcfg.alpha, lcfg.seed)
    from siss_amd.step import SISSStepper
    from oracle import schedule as S
    with pytest.raises(ValueError, match=r"saliency.*lora"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, lora=lora, saliency=mask, **HPK)
    # a bring-your-own mask whose words are not 16-byte aligned (a slice) is refused by name, not by a bare launcher status
    eng3, st3 = stepper()
    odd = SaliencyMask.ones(eng3)
    odd.bits = torch.cat([odd.bits[:1], odd.bits])[1:]
    st3.set_saliency(odd)
    with pytest.raises(ValueError, match="16-byte"):
        st3.step(*batch(0, dev))
    other = make_engine()
    other.ps.total += 64
    with pytest.raises(ValueError, match="another engine"):
        SISSStepper(eng, S.alphas_cumprod(), scaling_norm=5.0, train_batch_size=2, saliency=SaliencyMask.ones(other), **HPK)


# ================================================================ the task
SMALL = ["unet.sample_size=16", "unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
         "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1", "unet.attention_head_dim=null"]


def run_task(tmp_path, name, *extra):
    sys.path.insert(0, ROOT)
    import main as entry
    out = tmp_path / name
    ov = ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent",
          "allow_random_init=true", "allow_synthetic=true", f"data_dir={tmp_path}/nodata", "mixed_precision=bf16", *SMALL]
    entry.main(["--config-name=delete_celeb", f"output_dir={out}", *extra, *ov])
    from safetensors.torch import load_file
    rundir = os.path.join(out, os.listdir(out)[0])
    lines = [json.loads(l) for l in open(os.path.join(rundir, "train_log_rank0.jsonl"))]
    return rundir, lines, load_file(os.path.join(rundir, "unet", "diffusion_pytorch_model.safetensors")), ov


def test_delete_celeb_with_a_saliency_mask(dev, tmp_path):
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConfig
    from siss_amd.model import UNet2DModel
    from siss_amd.saliency import CONFIG_FILE, MASK_FILE, SaliencyMask
    rundir, lines, saved, ov = run_task(tmp_path, "keyed", "+deletion.saliency={fraction:0.5,batches:2}")
    assert os.path.isfile(os.path.join(rundir, MASK_FILE)) and os.path.isfile(os.path.join(rundir, CONFIG_FILE))
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), ov)
    ucfg = {k: v for k, v in cfg.unet.items() if not k.startswith("_")}
    model = UNet2DModel(UNet2DConfig.from_dict(ucfg), device=dev)
    initial = model.engine.init_random(seed=int(cfg.random_seed))
    mask = SaliencyMask.load(rundir, model.engine)
    assert (c["fraction"], c["batches"], c["seed"]) == (0.5, 2, 0) and c["k"] == round(0.5 * c["real_params"]) <= c["count"] == mask.count
    assert int(mask.to_bool().sum()) == mask.count, "set bits on the alignment padding, or a wrong count"
    assert len(lines) == 2
    for st in lines:
        assert st["trainable_params"] == st["saliency_params"] == c["count"] and st["trainable_tensors"] == len(initial)
        assert st["saliency_fraction"] == c["count"] / c["real_params"] and st["saliency_threshold"] == c["threshold"] > 0
    # the saved UNet differs from the initial weights on a subset of the mask only
    ps = model.engine.ps
    model.engine.load_state_dict(saved)
    after = ps.flat.clone()
    model.engine.load_state_dict(initial)
    moved = bits(after) != bits(ps.flat)
    flags = mask.to_bool()
    assert int((moved & ~flags).sum()) == 0, "a masked-out weight changed"
    assert int(moved.sum()) > 0
    # a second run that loads the first run's files ends on the same weights, bit for bit
    _, lines2, saved2, _ = run_task(tmp_path, "reloaded", "+deletion.saliency={fraction:0.5,batches:2,path:'%s'}" % rundir)
    assert set(saved2) == set(saved)
    for n in saved:
        assert torch.equal(bits(saved2[n]), bits(saved[n])), f"{n}: the run from the saved mask differs"
    assert [l["saliency_params"] for l in lines2] == [c["count"]] * 2
    for k in ("norm_loss_x", "norm_loss_a", "scaling_factor", "pre_clip_norm"):       # the masked norms, pinned run against run
        assert [l[k] for l in lines2] == [l[k] for l in lines], k
    # the training stream: two runs without the key agree bit for bit, and the keyed run's first step -- the same batches, noise,
    # timesteps and uniforms on the same weights -- logs their losses and importance weights exactly.  (Its norm_loss_x is NOT the
    # plain run's: pass 1 under the mask sums the masked-in elements only, so it is the norm of the masked gradient -- smaller, and
    # bitwise what the masked-pair test holds it to.)
    _, plain1, w1, _ = run_task(tmp_path, "plain1")
    _, plain2, w2, _ = run_task(tmp_path, "plain2")
    for n in w1:
        assert torch.equal(bits(w1[n]), bits(w2[n])), f"{n}: two runs without the key differ"
    assert "saliency_params" not in plain1[0]
    assert plain1[0]["norm_loss_x"] == plain2[0]["norm_loss_x"]
    drawn = [k for k in plain1[0] if k.startswith(("loss", "importance_weight"))]
    assert len(drawn) >= 8
    for k in drawn:
        assert plain1[0][k] == lines[0][k] or (plain1[0][k] != plain1[0][k] and lines[0][k] != lines[0][k]), (k, plain1[0][k], lines[0][k])
    assert 0 < lines[0]["norm_loss_x"] < plain1[0]["norm_loss_x"] and 0 < lines[0]["norm_loss_a"] < plain1[0]["norm_loss_a"]

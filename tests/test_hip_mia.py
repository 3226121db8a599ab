"""The membership inference attacks on the GPU: the launchers of csrc/mia.hip (the transfer bitwise against torch between sentinel
guards, the two reductions exactly on integers and against math.fsum on Gaussian data, rows past the pool, refusals), MembershipAttack
end to end against the f64 chains of tests/mia_ref.py on the f64 oracle network (yardstick: the same chains in torch f32 / under
autocast(bf16) on this GPU), a negative control, graph against eager, batch independence, the training state, and the T-shirt task."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import mia_ref as R
from membership_ref import CELEB_TINY, seeded_oracle, state_checksum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777.25
GUARD = 64                      # floats either side of an output (a multiple of 4: the output stays 16-B aligned)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _guarded(n, dev):
    """(whole buffer, the n floats in its middle) with SENTINEL everywhere."""
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _expect(values):
    return torch.cat([torch.full((GUARD,), SENTINEL), values.reshape(-1).float(), torch.full((GUARD,), SENTINEL)])


# ---------------------------------------------------------------- 1. gather and transfer
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("chw", [1, 5, 1027, 768], ids=lambda c: f"chw{c}")
def test_transfer_is_bitwise_torchs_expression_between_guards(dev, chw, b):
    from siss_amd import lib
    from siss_amd.mia import transfer_coefficients
    from siss_amd.scheduler import DDPMScheduler
    g = torch.Generator().manual_seed(chw * 10 + b)
    n = 7                                                                  # pool rows: offsets 0 | 2 (the middle) | 5 (b = 3: one row past)
    pool, e, x = torch.rand(n, chw, generator=g) * 2 - 1, torch.randn(b, chw, generator=g), torch.randn(b, chw, generator=g)
    d_pool, d_e, d_x = pool.to(dev), e.to(dev), x.to(dev)
    offset = torch.zeros(1, dtype=torch.long, device=dev)
    ab = DDPMScheduler().alphas_cumprod
    for cx, ce in (transfer_coefficients(ab, "transfer", 100, 110), transfer_coefficients(ab, "transfer", 110, 100),
                   transfer_coefficients(ab, "noise", None, 200)):
        cxt, cet = torch.tensor(cx, dtype=torch.float32), torch.tensor(ce, dtype=torch.float32)
        # chain rows (offset NULL), no copy of e
        whole, y = _guarded(b * chw, dev)
        lib.call("siss_mia_transfer", d_x, d_e, None, b, b, chw, cx, ce, y, None)
        assert torch.equal(_bits(whole.cpu()), _bits(_expect(cxt * x + cet * e))), (cx, ce)
        # pool rows at an offset, with the copy of e
        for off in (0, 2, 5):
            offset.fill_(off)
            whole, y = _guarded(b * chw, dev)
            kwhole, keep = _guarded(b * chw, dev)
            lib.call("siss_mia_transfer", d_pool, d_e, offset, n, b, chw, cx, ce, y, keep)
            rows = [min(off + r, n - 1) for r in range(b)]                 # a row past the pool reads the last one
            assert torch.equal(_bits(whole.cpu()), _bits(_expect(cxt * pool[rows] + cet * e))), (cx, ce, off)
            assert torch.equal(_bits(kwhole.cpu()), _bits(_expect(e))), (cx, ce, off)
    for off in (0, 2, 5):                                                  # the gather
        offset.fill_(off)
        whole, y = _guarded(b * chw, dev)
        lib.call("siss_mia_gather", d_pool, offset, n, b, chw, y)
        assert torch.equal(_bits(whole.cpu()), _bits(_expect(pool[[min(off + r, n - 1) for r in range(b)]]))), off
    torch.cuda.synchronize()
    for d, h in ((d_pool, pool), (d_e, e), (d_x, x)):                      # the inputs are returned bit-identical
        assert torch.equal(_bits(d.cpu()), _bits(h))
    assert int(offset.item()) == 5


# ---------------------------------------------------------------- 2. the reductions
POISON = -12345.0


def _terms(kind, a, b_, c, cx, ce, p):
    """The f32 terms of one row as torch forms them on the CPU (each operation rounded on its own)."""
    if kind == "sqerr":
        d = (torch.tensor(cx) * a + torch.tensor(ce) * b_) - c
        return d * d
    d = a - b_
    return d * d if p == 2 else (d * d) * (d * d)


def _reduce(lib, kind, dev, a, b_, c, offset, n, cx, ce, p, sums, partials):
    b, chw = a.shape
    if kind == "sqerr":
        lib.call("siss_mia_transfer_sqerr", a, b_, c, offset, n, b, chw, cx, ce, sums, partials)
    else:
        lib.call("siss_mia_powdiff", a, b_, offset, n, b, chw, p, sums, partials)


@pytest.mark.parametrize("kind,p", [("sqerr", 2), ("powdiff", 2), ("powdiff", 4)])
@pytest.mark.parametrize("chw", [1, 5, 1027, 768, 8192], ids=lambda c: f"chw{c}")
def test_reductions_exact_on_integers_and_against_fsum(dev, chw, kind, p):
    from siss_amd import lib
    g = torch.Generator().manual_seed(chw + p)
    n, b = 8, 3                                                            # offsets 0, 3 (the middle), 6 (one row past the pool)
    offset = torch.zeros(1, dtype=torch.long, device=dev)
    partials = torch.zeros(int(lib.query("siss_mia_partials_words", b, chw)), dtype=torch.float64, device=dev)
    assert partials.numel() == b * max(1, min(64, chw // 1024))
    for data in ("integers", "gaussian"):
        if data == "integers":
            draw = lambda: torch.randint(-3, 4, (b, chw), generator=g).float()
            cx, ce = 2.0, -1.0
        else:
            draw = lambda: torch.randn(b, chw, generator=g)
            cx, ce = 0.9993206262588501, 0.012873172760009766             # (f32 values)
        sums = torch.full((n + b,), POISON, dtype=torch.float64, device=dev)
        inputs = {}
        for off in (0, 3, 6):
            a, b_, c = draw(), draw(), draw()
            inputs[off] = (a, b_, c)
            offset.fill_(off)
            _reduce(lib, kind, dev, a.to(dev), b_.to(dev), c.to(dev), offset, n, cx, ce, p, sums, partials)
        got = sums.cpu()
        assert bool((got[n:] == POISON).all()), "a row past the pool wrote its sum"
        worst = 0.0
        for off, (a, b_, c) in inputs.items():
            for r in range(b):
                if off + r >= n:
                    continue
                terms = _terms(kind, a[r], b_[r], c[r], cx, ce, p)
                if data == "integers":
                    assert float(got[off + r]) == float(terms.double().sum()) == float(int(terms.double().sum())), (off, r)
                else:
                    exact = math.fsum(terms.double().tolist())
                    worst = max(worst, abs(float(got[off + r]) - exact) / exact)
        if data == "gaussian":
            print(f"\n{kind} p={p} chw {chw}: worst relative error of the f64 sum {worst:.2e} (bound {chw * 2.0 ** -53:.2e})")
            assert worst <= chw * 2.0 ** -53
    # a batch in the middle touches its own entries only, and twice the same bits
    a, b_, c = (t.to(dev) for t in inputs[3])
    offset.fill_(3)
    runs = []
    for _ in range(2):
        sums = torch.full((n,), POISON, dtype=torch.float64, device=dev)
        _reduce(lib, kind, dev, a, b_, c, offset, n, cx, ce, p, sums, partials)
        runs.append(sums.cpu())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    assert bool((runs[0][:3] == POISON).all()) and bool((runs[0][6:] == POISON).all()) and bool((runs[0][3:6] != POISON).all())


def test_refusals_write_nothing(dev):
    from siss_amd import lib
    b, chw, n = 2, 64, 4
    x, e, ref = (torch.randn(b, chw, device=dev) for _ in range(3))
    offset = torch.zeros(1, dtype=torch.long, device=dev)
    sums = torch.full((n,), POISON, dtype=torch.float64, device=dev)
    partials = torch.full((int(lib.query("siss_mia_partials_words", b, chw)),), POISON, dtype=torch.float64, device=dev)
    whole, y = _guarded(b * chw, dev)
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 2)                       # not aligned to its element
    refused = [
        ("siss_mia_powdiff", (x, e, offset, n, b, chw, 3, sums, partials)),                         # p outside {2, 4}
        ("siss_mia_powdiff", (x, e, offset, n, b, chw, 0, sums, partials)),
        ("siss_mia_powdiff", (None, e, offset, n, b, chw, 2, sums, partials)),
        ("siss_mia_powdiff", (x, e, None, n, b, chw, 2, sums, partials)),
        ("siss_mia_powdiff", (x, e, offset, n, b, chw, 2, None, partials)),
        ("siss_mia_powdiff", (odd(x), e, offset, n, b, chw, 2, sums, partials)),
        ("siss_mia_powdiff", (x, e, offset, n, b, chw, 2, odd(sums), partials)),
        ("siss_mia_powdiff", (x, e, offset, 0, b, chw, 2, sums, partials)),
        ("siss_mia_transfer_sqerr", (x, e, None, offset, n, b, chw, 1.0, 0.5, sums, partials)),
        ("siss_mia_transfer_sqerr", (x, e, ref, offset, n, b, chw, 1.0, 0.5, sums, None)),
        ("siss_mia_transfer_sqerr", (x, odd(e), ref, offset, n, b, chw, 1.0, 0.5, sums, partials)),
        ("siss_mia_transfer_sqerr", (x, e, ref, offset, n, 0, chw, 1.0, 0.5, sums, partials)),
        ("siss_mia_transfer", (x, None, None, b, b, chw, 1.0, 0.5, y, None)),
        ("siss_mia_transfer", (x, e, None, b, b, chw, 1.0, 0.5, None, None)),
        ("siss_mia_transfer", (x, e, None, b, b, 0, 1.0, 0.5, y, None)),
        ("siss_mia_transfer", (odd(x), e, None, b, b, chw, 1.0, 0.5, y, None)),
        ("siss_mia_gather", (None, offset, n, b, chw, y)),
        ("siss_mia_gather", (x, None, n, b, chw, y)),
        ("siss_mia_gather", (x, offset, n, 70000, chw, y)),
    ]
    for name, args in refused:
        assert lib.call(name, *args, refusable=True) == 1, (name, args)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_mia_powdiff", x, e, offset, n, b, chw, 3, sums, partials)
    torch.cuda.synchronize()
    assert bool((sums == POISON).all()) and bool((partials == POISON).all()) and bool((whole == SENTINEL).all())


# ---------------------------------------------------------------- 3. end to end
SETTINGS = {"secmi": dict(t_sec=30, stride=10), "pia": dict(t=200, p=4), "loss": dict(t=100, noises=2)}
ATTACKS = ("secmi", "pia", "loss")
NOISE_SEED = 7


def _engine(dtype, sd, kw=CELEB_TINY):
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    eng = UNetEngine(UNet2DConfig(**kw), "cuda:0", dtype=dtype)
    eng.load_state_dict(sd)
    return eng


def _attack(eng, dev, batch_size=2, **kw):
    from siss_amd.mia import MembershipAttack
    from siss_amd.scheduler import DDPMScheduler
    return MembershipAttack(eng, DDPMScheduler(), dev, attacks=ATTACKS, batch_size=batch_size, **SETTINGS, **kw)


def _scores(attack, images, dev):
    """{attack: f64 [N] on the host} with the loss attack's noises from a generator seeded NOISE_SEED."""
    out = attack.scores(images, generator=torch.Generator(device=dev).manual_seed(NOISE_SEED))
    return {a: s.cpu() for a, s in out.items()}


def _rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


@pytest.fixture(scope="module")
def world(dev):
    """The fixture images (N = 5), the oracle network, the f64 reference scores, the torch f32 / bf16 yardsticks and the f32 engine."""
    from siss_amd.scheduler import DDPMScheduler
    fx = np.load(os.path.join(ROOT, "tests", "golden", "membership_ref.npz"))
    images = torch.from_numpy(fx["pool_all"])[:5].contiguous()
    assert images.shape == (5, 3, 16, 16)
    net = seeded_oracle(int(fx["net_seed"]))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert abs(state_checksum(sd) - float(fx["checksum"])) <= 1e-9 * abs(float(fx["checksum"])), "the seeded weights differ"
    ab = DDPMScheduler().alphas_cumprod.double().numpy()
    # the noises MembershipAttack.scores draws for the loss attack: [noises, C, H, W] from the seeded device generator
    noise = torch.randn((SETTINGS["loss"]["noises"], 3, 16, 16), device=dev, generator=torch.Generator(device=dev).manual_seed(NOISE_SEED)).cpu()
    net64 = seeded_oracle(int(fx["net_seed"])).double()
    ref = lambda x: R.all_scores(R.net_eps(net64), ab, x.double(), noise.double(), SETTINGS)
    gnet = seeded_oracle(int(fx["net_seed"])).to(dev)
    on_gpu = lambda autocast: {a: s.cpu() for a, s in R.all_scores(R.net_eps(gnet, autocast=autocast), ab, images.to(dev), noise.to(dev),
                                                                   SETTINGS).items()}
    w = dict(images=images, sd=sd, ref=ref(images), rolled=ref(torch.roll(images, 1, 0)), eng32=_engine(torch.float32, sd))
    w["e_each"] = {torch.float32: {a: _rel(s, w["ref"][a]) for a, s in on_gpu(None).items()},
                   torch.bfloat16: {a: _rel(s, w["ref"][a]) for a, s in on_gpu(torch.bfloat16).items()}}
    w["e_ref"] = {dt: max(each.values()) for dt, each in w["e_each"].items()}          # ONE number per dtype: the worst over the chains
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_engine_against_the_f64_chains_on_the_oracle_network(dev, world, dtype):
    """Yardstick: e_ref = the worst relative deviation from the f64 reference, over the three chains and the five images, of the same
    chains run on the oracle network with torch on this GPU (f32, or under autocast(bfloat16) for the bf16 engine).  The engine's worst
    relative deviation must stay within 2 * e_ref; both numbers are printed, and each attack's own pair beside them.  (An a-priori bound
    through the chains' network calls cannot be derived, so none is fixed.)

    Measured on an MI355X (worst relative deviation, torch | HIP engine): f32 secmi 3.23e-06 | 5.73e-06, pia 2.66e-06 | 2.94e-06, loss
    1.85e-08 | 4.05e-08, so e_ref = 3.23e-06 against 5.73e-06 (allowed 6.46e-06: SecMI's score is the squared difference of two nearby
    points of the chain, 1e-3 here, and carries the forwards' rounding amplified; the margin is small); bf16 secmi 4.71e-02 | 2.51e-02,
    pia 3.05e-02 | 1.84e-02, loss 7.18e-04 | 5.60e-04.  The per-attack pairs are printed, not asserted: in f32 the loss attack's
    deviations lie BELOW one f32 rounding (2^-24 = 5.96e-08) -- sums of 768 terms average the forwards' rounding out -- and the ratio
    of two such figures over five images says nothing about either network."""
    eng = world["eng32"] if dtype == torch.float32 else _engine(dtype, world["sd"])
    got = _scores(_attack(eng, dev), world["images"], dev)
    for a in ATTACKS:
        assert got[a].dtype == torch.float64 and got[a].shape == (5,)
        print(f"\n{a} ({dtype}): worst relative deviation from the f64 reference: torch {world['e_each'][dtype][a]:.3e}, HIP engine "
              f"{_rel(got[a], world['ref'][a]):.3e}; reference scores {world['ref'][a].tolist()}")
    e_hip, e_ref = max(_rel(got[a], world["ref"][a]) for a in ATTACKS), world["e_ref"][dtype]
    print(f"\n{dtype}: torch e_ref = {e_ref:.3e}, HIP engine {e_hip:.3e} (allowed {2 * e_ref:.3e})")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)


def test_negative_control_rolled_images_lie_far_outside_the_yardstick(dev, world):
    got = _scores(_attack(world["eng32"], dev), world["images"], dev)
    for a in ATTACKS:
        shift = ((world["rolled"][a] - got[a]).abs() / got[a].abs())
        print(f"\n{a}: smallest relative shift under rolled images {float(shift.min()):.3g}, 10 * e_ref {10 * world['e_ref'][torch.float32]:.3g}")
        assert bool((shift > 10 * world["e_ref"][torch.float32]).all()), a


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_graph_and_eager_give_the_same_bits_and_a_graph_repeats(dev, world, dtype):
    eng = world["eng32"] if dtype == torch.float32 else _engine(dtype, world["sd"])
    a = _attack(eng, dev, use_graph=True)
    first = _scores(a, world["images"], dev)
    again = _scores(a, world["images"], dev)                              # the captured graphs, replayed
    eager = _scores(_attack(eng, dev, use_graph=False), world["images"], dev)
    for k in ATTACKS:
        assert torch.equal(_bits(first[k]), _bits(again[k])), f"{k}: two evaluations on one graph differ"
        assert torch.equal(_bits(first[k]), _bits(eager[k])), f"{k}: graph and eager differ"
    assert a.forwards == {"secmi": 3 * 5, "pia": 3 * 2, "loss": 5}         # ceil(5 / 2) chains; ceil(10 / 2) pair forwards


def test_scores_do_not_depend_on_the_batch_size_nor_on_the_pools_other_images(dev, world):
    """The same image in another batch slot, another batch size or beside other images: its forwards see the same inputs, so every
    such score lies within the 2 * e_ref of the end-to-end test around the reference, and two of them within 4 * e_ref of each other."""
    imgs = world["images"]
    base = _scores(_attack(world["eng32"], dev, batch_size=2), imgs, dev)
    others = {"b1": _scores(_attack(world["eng32"], dev, batch_size=1), imgs, dev),
              "b5": _scores(_attack(world["eng32"], dev, batch_size=5), imgs, dev)}
    sub = _scores(_attack(world["eng32"], dev, batch_size=2), torch.cat([imgs[3:4], imgs[:2], -imgs[4:5]]), dev)
    others["pool"] = {a: torch.stack([sub[a][1], sub[a][2], base[a][2], sub[a][0], base[a][4]]) for a in ATTACKS}
    for name, got in others.items():
        for a in ATTACKS:
            d = _rel(got[a], base[a])
            print(f"\n{name} {a}: worst relative difference {d:.3e} (bound {4 * world['e_ref'][torch.float32]:.3e})")
            assert d <= 4 * world["e_ref"][torch.float32], (name, a)


# ---------------------------------------------------------------- 4. the training state is left alone
MNIST_SMALL = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=(64, 128),
                   down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), layers_per_block=1,
                   attention_head_dim=8, norm_num_groups=32, norm_eps=1e-5, downsample_padding=1, flip_sin_to_cos=True, freq_shift=0)


def test_an_evaluation_leaves_the_training_state_bitwise(dev):
    from siss_amd import lib
    from siss_amd.config import UNet2DConfig
    from siss_amd.mia import MembershipAttack
    from siss_amd.scheduler import DDPMScheduler
    from siss_amd.step import SISSStepper
    from siss_amd.unet import UNetEngine
    eng = UNetEngine(UNet2DConfig(**MNIST_SMALL), "cuda:0", dtype=torch.bfloat16)
    eng.init_random(seed=1)
    B = 2
    sched = DDPMScheduler()
    st = SISSStepper(eng, sched.alphas_cumprod, lr=1e-4, scaling_norm=5.0, train_batch_size=B, mixed_precision="bf16", inf_guard=True)
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (B, 1, 28, 28)
    for _ in range(2):                                   # two steps: AdamW moments, both gradient sets and a sparse-fill plan exist
        x0, a0, noise = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
        st.step(x0, a0, noise, torch.randint(0, 1000, (B,), device=dev, generator=g), torch.rand(B, device=dev, generator=g))
    torch.cuda.synchronize()
    lib.overwrite_log()
    ps = eng.ps
    snap = [ps.flat.clone(), ps.grads.clone(), ps.shadow.clone(), st.opt.m.clone(), st.opt.v.clone()]
    fill = (eng._fill_key, eng._fill_plan, dict(eng._fill_plans), eng.wgrad_overwrite)
    assert fill[2], "the steps recorded no sparse-fill plan"
    rng = (g.get_state().clone(), torch.cuda.get_rng_state(dev).clone(), torch.get_rng_state().clone(), random.getstate())
    m = MembershipAttack(eng, sched, dev, batch_size=2, secmi=dict(t_sec=20, stride=10), loss=dict(noises=2))
    images = torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(4)) * 2 - 1
    own = torch.Generator(device=dev).manual_seed(1)
    for _ in range(2):                                   # the capture, then a replay
        scores = m.scores(images, generator=own)
        assert all(bool(torch.isfinite(s).all()) and bool((s > 0).all()) for s in scores.values())
        torch.cuda.synchronize()
        for a, b in zip(snap, [ps.flat, ps.grads, ps.shadow, st.opt.m, st.opt.v]):
            assert torch.equal(_bits(a), _bits(b))
        assert (eng._fill_key, eng._fill_plan, eng.wgrad_overwrite) == (fill[0], fill[1], fill[3])
        assert eng._fill_plans.keys() == fill[2].keys() and all(eng._fill_plans[k] is v for k, v in fill[2].items())
        assert lib.overwrite_log() == []
        assert torch.equal(g.get_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(dev), rng[1])     # the loop's stream, the global one
        assert torch.equal(torch.get_rng_state(), rng[2]) and random.getstate() == rng[3]


def test_the_conditional_engine_is_refused_by_name(dev):
    from siss_amd.mia import MembershipAttack
    from siss_amd.scheduler import DDPMScheduler

    class UNetCondEngine:
        pass
    m = MembershipAttack(UNetCondEngine(), DDPMScheduler(), dev)
    with pytest.raises(NotImplementedError, match="UNetCondEngine"):
        m.scores(torch.zeros(1, 4, 8, 8))


# ---------------------------------------------------------------- 5. the task
TSHIRT_UNET = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
                   down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"], layers_per_block=1)
MIA_KEY = ("+metrics.mia={step_frequency: 1, num_members: 4, num_forget: 4, batch_size: 4, holdout: {limit: 6}, fpr: [0.2, 0.01], "
           "secmi: {t_sec: 20, stride: 10}, loss: {noises: 2}, seed: 3}")


def _run(tmp_path, name, extra, monkeypatch):
    """DeleteTShirt for three steps on synthetic data, with the inputs of every micro-batch and every launcher name recorded."""
    from siss_amd import hydra_lite as H
    from siss_amd import lib
    from siss_amd.step import SISSStepper
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    ["training_steps=3", "train_batch_size=2", "gradient_accumulation_steps=2", f"output_dir={tmp_path}/{name}",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "save_final=false",
                     "mixed_precision=bf16", "+dataloader_num_workers=1", *extra])
    cfg.unet = TSHIRT_UNET
    called, seen = set(), []
    real, real_micro = lib.call, SISSStepper.micro_step
    monkeypatch.setattr(lib, "call", lambda n, *a, **k: (called.add(n), real(n, *a, **k))[1])

    def micro(self, x0, a0, noise, t, u, *rest, **kw):
        seen.append([v.detach().clone() for v in (x0, a0, noise, t, u)])
        return real_micro(self, x0, a0, noise, t, u, *rest, **kw)
    monkeypatch.setattr(SISSStepper, "micro_step", micro)
    random.seed(5)
    try:
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).run()
    finally:
        monkeypatch.setattr(lib, "call", real)
        monkeypatch.setattr(SISSStepper, "micro_step", real_micro)
    torch.cuda.synchronize()
    return cfg, called, seen


def test_the_tshirt_task_records_the_attacks_without_touching_the_training_inputs(dev, tmp_path, monkeypatch):
    new = {"siss_mia_gather", "siss_mia_transfer", "siss_mia_transfer_sqerr", "siss_mia_powdiff"}
    cfg0, called, plain = _run(tmp_path, "plain", [], monkeypatch)
    assert not (new | {"siss_pair_noise", "siss_pair_sqerr"}) & called                   # the key absent: no launch is added,
    assert not [f for f in os.listdir(cfg0.output_dir) if f.startswith("mia")]           # no file is written
    cfg, called, with_key = _run(tmp_path, "mia", [MIA_KEY], monkeypatch)
    assert new | {"siss_pair_noise", "siss_pair_sqerr"} <= called
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "mia_rank0.jsonl"))]
    assert [r["global_step"] for r in lines] == [0, 1, 2, 3]
    fields = ["auc", "tpr_at_fpr_0.2", "tpr_at_fpr_0.01", "forget_auc", "forget_flagged_at_fpr_0.2", "forget_flagged_at_fpr_0.01",
              "forget_percentile", "member_mean", "forget_mean", "holdout_mean"]
    for r in lines:
        assert (r["members"], r["forget"], r["holdout"]) == (4, 1, 6) and r["seconds"] > 0     # (one synthetic forget image, scored once)
        assert set(r) == {"global_step", "seconds", "members", "forget", "holdout"} | {f"{a}_{f}" for a in ATTACKS for f in fields}
        assert all(isinstance(v, (int, float)) and math.isfinite(v) for v in r.values()), r
        for a in ATTACKS:
            assert 0 <= r[f"{a}_auc"] <= 1 and 0 <= r[f"{a}_forget_percentile"] <= 1 and r[f"{a}_member_mean"] > 0
    # the micro-batches: 3 steps x 2 accumulations, every input bitwise that of the run without the key
    assert len(plain) == len(with_key) == 6
    for a, b in zip(plain, with_key):
        for va, vb in zip(a, b):
            assert va.dtype == vb.dtype and torch.equal(_bits(va) if va.is_floating_point() else va, _bits(vb) if vb.is_floating_point() else vb)
    logs = [[json.loads(l) for l in open(os.path.join(c.output_dir, "train_log_rank0.jsonl"))] for c in (cfg0, cfg)]
    assert len(logs[0]) == len(logs[1]) == 3 and [set(r) for r in logs[0]] == [set(r) for r in logs[1]]
    # holdout: null -- score means only
    cfg, _, _ = _run(tmp_path, "means", ["+metrics.mia={step_frequency: 3, attacks: [pia], num_members: 2, batch_size: 2}"], monkeypatch)
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "mia_rank0.jsonl"))]
    assert [r["global_step"] for r in lines] == [0, 3]
    for r in lines:
        assert r["holdout"] == 0 and r["pia_auc"] is None and r["pia_forget_percentile"] is None and r["pia_holdout_mean"] is None
        assert r["pia_member_mean"] > 0 and r["pia_forget_mean"] > 0 and not [k for k in r if k.startswith(("secmi", "loss"))]


def test_the_tool_runs_one_evaluation_on_a_checkpoint_and_repeats_it(dev, tmp_path):
    """tools/mia.py: the loop's evaluation once, at the weights the configuration loads; the groups and the noises are seeded by
    metrics.mia.seed alone, so two invocations on one checkpoint write the same record (what makes two checkpoints comparable)."""
    from tools.mia import evaluate
    out = str(tmp_path / "mia.jsonl")
    overrides = ["checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "mixed_precision=bf16",
                 "+metrics.mia={num_members: 3, batch_size: 4, holdout: {limit: 5}, fpr: [0.2], secmi: {t_sec: 10, stride: 10}, loss: {noises: 1}}"]
    recs = [evaluate("delete_tshirt", os.path.join(ROOT, "config"), overrides, out, global_step=s) for s in (0, 7)]
    lines = [json.loads(l) for l in open(out)]
    assert [r["global_step"] for r in lines] == [0, 7] and lines == [json.loads(json.dumps(r)) for r in recs]
    drop = lambda r: {k: v for k, v in r.items() if k not in ("global_step", "seconds")}
    assert drop(lines[0]) == drop(lines[1])
    assert (lines[0]["members"], lines[0]["forget"], lines[0]["holdout"]) == (3, 1, 5)
    assert all(math.isfinite(v) for v in drop(lines[0]).values())
    with pytest.raises(ValueError, match="config-name"):
        evaluate("delete_sd", os.path.join(ROOT, "config"), [], out)
    with pytest.raises(ValueError, match="unknown field"):
        evaluate("delete_tshirt", os.path.join(ROOT, "config"), ["+metrics.mia={frequency: 1}"], out)

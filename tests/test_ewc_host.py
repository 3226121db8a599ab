"""Host side of the Fisher anchor (siss_amd/ewc.py, FlatAdamW.launch(ewc=...)), without a GPU:

* deletion.ewc: every refusal of parse_ewc names the offending entry; defaults and the round trip; the tasks read it in
  check_supported; the key is absent from the four YAMLs and the pre-training task refuses it;
* FisherAnchor: uniform, save / load, a fingerprint mismatch per field; the normalisation (mean over the real parameters 1 within
  1e-12 in f64, the padding stays 0; non-finite and all-zero F refused);
* tests/ewc_ref.py's f64 step against torch in f64 at 1e-12: the penalty gradient by autograd of (lambda / 2) sum F (theta - theta*)^2
  on top of given g_x, g_a, the recombination of oracle/step.py, clip_grad_norm_ and torch.optim.AdamW -- modes 0, 1, 2 and a single-set
  case; the f32 restatement of the fold against its f64 values;
* FlatAdamW.launch_sharded(ewc=...), launch(ranges=..., ewc=...) and launch(mask=..., ewc=...) refuse before any launch (an optimizer
  over CPU tensors with a recording launcher in place of the library's); the same recorder pins the entry points and every argument
  of launch's four paths (plain, ranges, mask, ewc), with and without want_grad;
* the variants' one table (siss_amd/variants.py): which (overlap, exchange) pairs set_overlap takes per variant, written out as a
  literal grid and checked on a SISSStepper built without its constructor (the constructor wants a device: what it resolves is set by
  hand; saliency and ewc go through set_saliency / set_ewc); what _fit_exchange switches off and says; exclusive()'s message;
* tasks._built_on_rank0 as rank 0 and as rank 1 of 2 over a recording stand-in for torch.distributed: the agreement comes before the
  tensor broadcast, an error string raises on every rank before any tensor moves.
"""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import ewc_ref as E
import optimizer_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ================================================================ the parsed key
def test_parse_ewc_defaults_and_round_trip():
    from siss_amd.ewc import FIELDS, parse_ewc
    assert parse_ewc(None) is None
    c = parse_ewc(dict(strength=10))
    assert c.as_dict() == dict(strength=10.0, batches=8, batch_size=None, seed=0, normalize=True, path=None)
    assert isinstance(c.strength, float) and tuple(c.as_dict()) == FIELDS
    full = dict(strength=0.5, batches=2, batch_size=1, seed=7, normalize=False, path="/somewhere")
    c = parse_ewc(full)
    assert c.as_dict() == full and parse_ewc(c.as_dict()).as_dict() == full
    c = parse_ewc(dict(strength=3, batches=None, batch_size=None, path=None))        # explicit nulls: the defaults
    assert (c.batches, c.batch_size, c.path) == (8, None, None)


def test_parse_ewc_refusals_name_the_entry():
    from siss_amd.ewc import parse_ewc
    ok = dict(strength=1.0)
    rows = [(3, "mapping"), ([1.0], "mapping"), ("10", "mapping"), (dict(ok, strenght=2), "strenght"), (dict(ok, rank=4), "rank"),
            ({}, "strength"), (dict(strength=None), "strength"), (dict(strength=0), "strength"), (dict(strength=-1.0), "strength"),
            (dict(strength="big"), "strength"), (dict(strength=True), "strength"), (dict(strength=float("nan")), "strength"),
            (dict(strength=float("inf")), "strength"),
            (dict(ok, batches=0), "batches"), (dict(ok, batches=1.5), "batches"), (dict(ok, batches=True), "batches"),
            (dict(ok, batch_size=0), "batch_size"), (dict(ok, batch_size=2.0), "batch_size"), (dict(ok, batch_size="4"), "batch_size"),
            (dict(ok, seed="x"), "seed"), (dict(ok, seed=1.5), "seed"), (dict(ok, normalize=1), "normalize"),
            (dict(ok, normalize="yes"), "normalize"), (dict(ok, path=3), "path")]
    for bad, word in rows:
        with pytest.raises(ValueError, match="deletion.ewc") as e:
            parse_ewc(bad)
        assert word in str(e.value), (bad, str(e.value))
    for kw, name in ((dict(trainable=["attn"]), "deletion.trainable"), (dict(lora=dict(rank=4)), "deletion.lora"),
                     (dict(saliency=dict(fraction=0.5)), "deletion.saliency")):
        with pytest.raises(ValueError, match=name) as e:
            parse_ewc(ok, **kw)
        assert "deletion.ewc" in str(e.value)


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config):
    from siss_amd import hydra_lite as H

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    assert task([]).ewc_config() is None and task(["+deletion.ewc=null"]).ewc_config() is None
    task([]).check_supported()
    t = task(["+deletion.ewc={strength:10,batches:2}"])
    assert t.ewc_config().as_dict() == dict(strength=10.0, batches=2, batch_size=None, seed=0, normalize=True, path=None)
    t.check_supported()
    for ov, word in (("10", "mapping"), ("{strength:1,rank:4}", "rank"), ("{batches:2}", "strength"), ("{strength:0}", "strength"),
                     ("{strength:1,batches:0}", "batches"), ("{strength:1,batch_size:0}", "batch_size"),
                     ("{strength:1,normalize:3}", "normalize")):
        with pytest.raises(ValueError, match="deletion.ewc") as e:
            task(["+deletion.ewc=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    for other, name in (("+deletion.trainable=[attn]", "deletion.trainable"), ("+deletion.lora={rank:4,targets:[attn]}", "deletion.lora"),
                        ("+deletion.saliency={fraction:0.5}", "deletion.saliency")):
        with pytest.raises(ValueError, match=name):
            task(["+deletion.ewc={strength:1}", other]).check_supported()


def test_the_yamls_lack_the_key_and_the_pretraining_task_refuses_it():
    from siss_amd import hydra_lite as H
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "ewc" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "ewc" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.ewc={strength:1}"])
    with pytest.raises(NotImplementedError, match="deletion.ewc"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [])
    H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


# ================================================================ the anchor object: files, fingerprint, normalisation
def fake_engine(numels=(70, 64, 5), align=64, seed=0):
    specs, off = {}, 0
    for i, n in enumerate(numels):
        specs[f"w{i}"] = types.SimpleNamespace(name=f"w{i}", off=off, numel=n)
        off += -(-n // align) * align
    flat = torch.randn(off, generator=torch.Generator().manual_seed(seed))
    return types.SimpleNamespace(ps=types.SimpleNamespace(specs=specs, total=off, flat=flat), device=torch.device("cpu"))


def real_of(eng):
    real = np.zeros(eng.ps.total, bool)
    for sp in eng.ps.specs.values():
        real[sp.off:sp.off + sp.numel] = True
    return real


def test_uniform_and_the_file_round_trip(tmp_path):
    from siss_amd.ewc import CONFIG_FILE, FISHER_FILE, FisherAnchor
    eng = fake_engine()
    total, real = eng.ps.total, real_of(eng)
    assert total == 256 and int(real.sum()) == 139
    u = FisherAnchor.uniform(eng, 2.5)
    assert np.array_equal(u.fisher.numpy(), real.astype(f32)), "uniform: 1 on the real parameters, 0 on the padding"
    assert torch.equal(u.pstar, eng.ps.flat) and u.pstar.data_ptr() != eng.ps.flat.data_ptr(), "pstar is a CLONE of the flat buffer"
    assert u.log_fields() == dict(ewc_strength=2.5) and (u.total, u.tensors, u.params) == (256, 3, 139)
    blk = np.arange(16, dtype=f32)
    assert u.stats_from(blk) == dict(ewc_penalty=12.0, ewc_grad_norm=13.0, ewc_strength=2.5)
    rng = np.random.default_rng(0)
    F = torch.from_numpy((rng.standard_normal(total) ** 2 * real).astype(f32))
    a = FisherAnchor(eng, F, eng.ps.flat.clone(), 10, batches=2, batch_size=4, seed=9, normalize=True, mean=0.25, max=3.0, zeros=1,
                     source="computed")
    a.save(str(tmp_path / "f"))
    assert sorted(os.listdir(tmp_path / "f")) == sorted([FISHER_FILE, CONFIG_FILE]) and FisherAnchor.present(str(tmp_path / "f"))
    assert not FisherAnchor.present(str(tmp_path)) and not FisherAnchor.present(None)
    c = json.load(open(tmp_path / "f" / CONFIG_FILE))
    assert c == dict(strength=10.0, batches=2, batch_size=4, seed=9, normalize=True, mean=0.25, max=3.0, zeros=1, source="computed",
                     total=total, tensors=3, real_params=139)
    eng.ps.flat.add_(1.0)                                # the anchor point of a loaded F is the engine's weights AT THE LOAD
    back = FisherAnchor.load(str(tmp_path / "f"), eng, 4.0)
    assert torch.equal(back.fisher, a.fisher) and torch.equal(back.pstar, eng.ps.flat) and back.strength == 4.0
    assert back.source == "loaded" and dict(back.config(), source=0, strength=0) == dict(a.config(), source=0, strength=0)
    for other, word in ((fake_engine((70, 64, 5, 1)), "total"), (fake_engine((70, 64, 4)), "real_params"), (fake_engine((70, 69)), "tensors")):
        with pytest.raises(ValueError, match=word):
            FisherAnchor.load(str(tmp_path / "f"), other, 4.0)
    for bad in (0, -1.0, None, "x"):
        with pytest.raises(ValueError, match="strength"):
            FisherAnchor.uniform(eng, bad)
    with pytest.raises(ValueError, match="fisher"):
        FisherAnchor(eng, F[:-1], eng.ps.flat.clone(), 1.0)
    with pytest.raises(ValueError, match="pstar"):
        FisherAnchor(eng, F, eng.ps.flat.double(), 1.0)


def test_normalisation_mean_one_and_zero_padding():
    from siss_amd.ewc import fisher_stats, normalize_fisher, real_mask
    eng = fake_engine((70, 64, 5, 1000))
    real = real_mask(eng.ps.specs, eng.ps.total)
    assert np.array_equal(real.numpy(), real_of(eng))
    rng = np.random.default_rng(3)
    F = torch.from_numpy(1e-6 * rng.standard_normal(eng.ps.total) ** 2 * real_of(eng))        # f64
    F[3] = 0
    before = F.clone()
    mean, mx, zeros = normalize_fisher(F, real)
    assert mean == float(before[real].mean()) and mx == float(before[real].max()) and zeros == 1
    assert abs(float(F[real].mean()) - 1.0) <= 1e-12
    assert int(F[~real].count_nonzero()) == 0, "the padding stays 0"
    assert fisher_stats(F, real)[2] == 1
    G = before.float()                                      # the same in f32: one rounding per element and one of the divisor
    normalize_fisher(G, real)
    assert abs(float(G[real].double().mean()) - 1.0) <= 2.0 ** -22 and int(G[~real].count_nonzero()) == 0
    for bad in (float("nan"), float("inf")):
        H = before.clone()
        H[5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            normalize_fisher(H, real)
    with pytest.raises(ValueError, match="zero on every parameter"):
        normalize_fisher(torch.zeros(eng.ps.total), real)


# ================================================================ the f64 restatement against torch in f64
HP = O.hyper(*O.HYPER["sd"])
KNOB = {0: 5.0, 1: 1e-2, 2: 5.0}


def torch_step(gx, ga, p0, pstar, F, lam, m, v, k, hp, mode, knob, max_norm):
    """autograd of the penalty on top of g_x, the recombination of oracle/step.py:114-126, clip_grad_norm_, torch.optim.AdamW -- f64"""
    lr, b1, b2, eps, wd = O.wide(hp)
    D = torch.float64
    gx, ga, pstar, F = (torch.from_numpy(np.asarray(t)).to(D) for t in (gx, ga, pstar, F))
    p = torch.from_numpy(np.asarray(p0)).to(D).clone().requires_grad_(True)
    penalty = 0.5 * float(f32(lam)) * (F * (p - pstar) ** 2).sum()
    gx2 = gx + torch.autograd.grad(penalty, p)[0]
    nx, na = float(torch.norm(gx2)), float(torch.norm(ga))
    if mode == 1:
        s = -max(float(f32(knob)) - float((gx2 * ga).sum()) / na ** 2, 0)
    else:
        s = float(f32(knob)) / na if na > 0 else float("inf")
        if mode == 2 and math.isinf(s):
            s = 0.0
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": torch.from_numpy(np.asarray(m)).to(D).clone(),
                    "exp_avg_sq": torch.from_numpy(np.asarray(v)).to(D).clone()}
    p.grad = gx2 - s * ga
    pre = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    opt.step()
    st = opt.state[p]
    return (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), dict(norm_x=nx, norm_a=na, scale=s, pre_clip_norm=pre,
                                                                                        penalty=float(penalty.detach()))


@pytest.mark.parametrize("case", ["mode 0", "mode 1", "mode 2", "single set"])
@pytest.mark.parametrize("k", [1, 3])
def test_f64_step_with_the_penalty_against_torch(case, k):
    n = 1027
    gx, ga, p, pstar, F = E.case(n, 5 + k, scale_d=1e-2)
    gx, ga = 40 * gx, 40 * ga                       # |g| > max_norm: the clip acts
    mode = 2 if case == "single set" else int(case[-1])
    if case == "single set":
        ga = np.zeros(n, f32)
    m, v = O.warm_state(n, k, HP, seed=2)
    lam = 3.0
    (p1, m1, v1, g1), sc, pen, tn, gx2 = E.step_f64(gx, ga, p, pstar, F, lam, m, v, k, HP, mode, KNOB[mode], 1.0)
    (pr, mr, vr), ref = torch_step(gx, ga, p, pstar, F, lam, m, v, k, HP, mode, KNOB[mode], 1.0)
    assert sc["clip_coef"] < 1 and pen > 0 and tn > 1e-3 * sc["norm_x"], "the case exercises neither the clip nor the penalty"
    if case == "single set":
        assert sc["scale"] == 0.0 and ref["scale"] == 0.0
    for key, want in (("norm_x", ref["norm_x"]), ("norm_a", ref["norm_a"]), ("scale", ref["scale"]), ("pre_clip_norm", ref["pre_clip_norm"])):
        assert abs(sc[key] - want) <= 1e-12 * abs(want), (key, sc[key], want)
    assert abs(pen - ref["penalty"]) <= 1e-12 * ref["penalty"]
    for name, got, want in (("p", p1, pr), ("m", m1, mr), ("v", v1, vr)):
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err <= 1e-12, (name, err)
    # ... and without the penalty the same step is a different one (the restatement's negative control)
    (p0, _, _, _), sc0, pen0, tn0, _ = E.step_f64(gx, ga, p, pstar, F, None, m, v, k, HP, mode, KNOB[mode], 1.0)
    assert pen0 == 0 and tn0 == 0 and abs(sc0["norm_x"] - sc["norm_x"]) > 1e-6 * sc["norm_x"] and float(np.abs(p0 - p1).max()) > 0


def test_f32_restatement_of_the_fold_against_f64():
    n = 1027
    gx, ga, p, pstar, F = E.case(n, 1)
    lam = 7.5
    gx2, d, t = E.fold_f32(gx, p, pstar, F, lam)
    assert np.array_equal(d, p - pstar) and gx2.dtype == f32
    want_t = lam * F.astype(f64) * d.astype(f64)                       # from the same f32 d: two roundings (strength * F, then * d)
    assert float(np.abs(t - want_t).max()) <= 2.01 * O.U * float(np.abs(want_t).max())
    assert float(np.abs(gx2 - (gx.astype(f64) + t.astype(f64))).max()) <= O.U * float(np.abs(gx2).max())
    pen, tn = E.penalty_f64(F, d, t, lam)
    assert abs(pen - 0.5 * lam * float((F.astype(f64) * d.astype(f64) ** 2).sum())) <= 1e-12 * pen
    assert abs(tn - float(np.linalg.norm(t.astype(f64)))) <= 1e-12 * tn
    # the accumulation: three roundings
    g = gx
    acc = E.fisher_accumulate_f32(g, F, 0.25)
    want = F.astype(f64) + g.astype(f64) ** 2 * 0.25
    assert acc.dtype == f32 and float(np.abs(acc - want).max()) <= 3 * O.U * float(np.abs(want).max())
    # integers: everything exact
    gx, ga, p, pstar, F = E.int_case(n, 2)
    gx2, d, t = E.fold_f32(gx, p, pstar, F, 1.0)
    assert np.array_equal(gx2, gx + F * (p - pstar))
    pen, tn = E.penalty_f64(F, d, t, 1.0)
    assert 2 * pen == int((F.astype(np.int64) * d.astype(np.int64) ** 2).sum()) and tn ** 2 == pytest.approx(int((t.astype(np.int64) ** 2).sum()), rel=1e-15)


# ================================================================ FlatAdamW's refusals
def cpu_optimizer(n=64):
    from siss_amd.optim import FlatAdamW
    opt = FlatAdamW.__new__(FlatAdamW)               # (the constructor wants a device buffer and the library's slab sizes)
    opt.p = torch.zeros(n)
    opt.m, opt.v, opt.shadow, opt.last_grad = torch.zeros(n), torch.zeros(n), None, None
    opt.lr, opt.betas, opt.eps, opt.wd, opt.max_grad_norm = 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0
    opt.partials, opt.scalars = torch.zeros(8, dtype=torch.float64), torch.zeros(16)
    return opt


def test_flat_adamw_refuses_the_anchor_with_ranges_mask_or_shards(monkeypatch):
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: calls.append(name) or 0)
    n = 64
    opt = cpu_optimizer(n)
    eng = fake_engine((n,))
    anchor = FisherAnchor.uniform(eng, 1.0)
    grads = torch.zeros(2, n)
    with pytest.raises(ValueError, match=r"ranges=.*ewc="):
        opt.launch(grads, scaling_norm=5.0, ranges=(torch.zeros(3, dtype=torch.int64), 1, 16), ewc=anchor)
    with pytest.raises(ValueError, match=r"mask=.*ewc="):
        opt.launch(grads, scaling_norm=5.0, mask=torch.zeros(2, dtype=torch.int32), ewc=anchor)
    with pytest.raises(NotImplementedError, match="Fisher anchor"):
        opt.launch_sharded(grads[0, :32], grads[1, :32], 0, 32, None, scaling_norm=5.0, ewc=anchor)
    assert calls == [], f"a refusal launched {calls}"
    # an anchor over another buffer is refused by name, before any launch
    other = FisherAnchor.uniform(fake_engine((n + 64,)), 1.0)
    with pytest.raises(ValueError, match="fisher"):
        opt.launch(grads, scaling_norm=5.0, ewc=other)
    assert calls == []
    # ... and the accepted call is pass 1 with the fold, then the plain pass 2, on the anchor's own tensors
    seen = []
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: seen.append((name, a)) or 0)
    monkeypatch.setattr(lib, "query", lambda name, *a: 4096)
    opt.launch(grads, scaling_norm=5.0, ewc=anchor)
    assert [s[0] for s in seen] == ["siss_grad_norms_scale_ewc", "siss_recombine_clip_adamw"]
    a = seen[0][1]
    assert a[2] is opt.p and a[3] is anchor.pstar and a[4] is anchor.fisher and a[5] == n and a[6] == 1.0 and a[13] is opt.ewc_partials


LAUNCH_PATHS = {"plain": ("siss_grad_norms_scale", "siss_recombine_clip_adamw"),
                "ranges": ("siss_grad_norms_scale_ranges", "siss_recombine_clip_adamw_ranges"),
                "mask": ("siss_grad_norms_scale_masked", "siss_recombine_clip_adamw_masked"),
                "ewc": ("siss_grad_norms_scale_ewc", "siss_recombine_clip_adamw")}


@pytest.mark.parametrize("want_grad", [False, True])
@pytest.mark.parametrize("path", list(LAUNCH_PATHS))
def test_flat_adamw_launch_sequence(monkeypatch, path, want_grad):
    """The two entry points of each of launch's four paths and every argument of both, by the header's parameter names; last_grad is
    allocated once, zero-filled where the path writes only part of it, and passed as g_out (None without want_grad)."""
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    from siss_amd.optim import MODE_NORM_FIX
    n = 64
    opt = cpu_optimizer(n)
    opt.shadow = torch.zeros(n, dtype=torch.bfloat16)
    grads = torch.zeros(2, n)
    tab, nr, granules = torch.tensor([4, 0, 8]), 1, 8                # one stretch: granules 4..11 of the 16
    words = torch.zeros(2, dtype=torch.int32)
    anchor = FisherAnchor.uniform(fake_engine((n,)), 2.0)
    kw = {"plain": {}, "ranges": dict(ranges=(tab, nr, granules)), "mask": dict(mask=words), "ewc": dict(ewc=anchor)}[path]
    seen = []
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: seen.append((name, a)) or 0)
    monkeypatch.setattr(lib, "query", lambda name, *a: 4096)
    monkeypatch.setattr(torch, "empty_like", lambda t: torch.full_like(t, float("nan")))     # (what `empty` leaves is told from zeros)
    opt.launch(grads, scaling_norm=5.0, want_grad=want_grad, **kw)
    first = opt.last_grad
    opt.launch(grads, scaling_norm=5.0, want_grad=want_grad, **kw)
    assert [s[0] for s in seen] == 2 * list(LAUNCH_PATHS[path])
    if want_grad:
        assert first is not None and opt.last_grad is first, "last_grad is allocated once"
        assert first.shape == opt.p.shape and first.dtype == torch.float32
        partial = path in ("ranges", "mask")
        assert bool((first == 0).all()) if partial else bool(first.isnan().all()), "zero-filled for ranges / mask, empty otherwise"
    else:
        assert opt.last_grad is None
    same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape
    for name, args in seen:
        assert len(args) == len(lib.PARAMS[name]) - 1, (name, len(args), lib.PARAMS[name])          # (the stream is lib.call's)
        a = dict(zip(lib.PARAMS[name], args))
        assert same(a.pop("gx"), grads[0]) and same(a.pop("ga"), grads[1]) and a.pop("n") == n and a.pop("scalars") is opt.scalars
        assert (a.pop("beta1"), a.pop("beta2")) == opt.betas
        if path == "ranges":
            assert a.pop("tab") is tab and (a.pop("nranges"), a.pop("total_granules")) == (nr, granules)
        if path == "mask":
            assert a.pop("bits") is words
        if name.startswith("siss_grad_norms_scale"):
            assert (a.pop("mode"), a.pop("knob"), a.pop("max_norm")) == (MODE_NORM_FIX, 5.0, 1.0) and a.pop("partials") is opt.partials
            if path == "ewc":
                assert a.pop("p") is opt.p and a.pop("pstar") is anchor.pstar and a.pop("F") is anchor.fisher
                assert a.pop("strength") == 2.0 and a.pop("ewc_partials") is opt.ewc_partials
        else:
            assert a.pop("p") is opt.p and a.pop("m") is opt.m and a.pop("v") is opt.v and a.pop("shadow") is opt.shadow
            assert a.pop("g_out") is (first if want_grad else None)
            assert (a.pop("lr"), a.pop("eps"), a.pop("wd")) == (opt.lr, opt.eps, opt.wd)
        assert a == {}, (name, sorted(a))
    # mode and knob of the other two recombinations
    del seen[:]
    opt.launch(grads, scaling_norm=5.0, inf_guard=True, **kw)
    opt.launch(grads, eta=1e-2, **kw)
    modes = [(dict(zip(lib.PARAMS[nm], a))["mode"], dict(zip(lib.PARAMS[nm], a))["knob"]) for nm, a in seen[::2]]
    assert modes == [(2, 5.0), (1, 1e-2)]


# ================================================================ which exchange each variant may use
def host_stepper(variant, monkeypatch):
    """A SISSStepper without its constructor (which wants a device, like FlatAdamW's): what the constructor resolves is set by hand for
    full / trainable / lora; saliency and ewc are reached the way a task reaches them, through set_saliency / set_ewc on a full stepper."""
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    from siss_amd.saliency import SaliencyMask
    from siss_amd.step import SISSStepper
    monkeypatch.setattr(lib, "query", lambda name, *a: 4096)
    eng = fake_engine((64,))
    eng.on_early_grads_final = None
    st = SISSStepper.__new__(SISSStepper)
    st.e, st.opt, st.pg, st.world, st.dp_on = eng, cpu_optimizer(64), object(), 1, True        # (dp.FORCE_COLLECTIVES on a stub group)
    st.lora = st.subset = st.saliency = st.ewc = None
    st.variant, st._launch_kw, st.overlap, st.exchange = "full", {}, False, "allreduce"
    st._ranges = st._mask = None
    if variant == "lora":
        st.lora = st.subset = types.SimpleNamespace(params=1, tensors=2)
    elif variant == "trainable":
        st.subset = types.SimpleNamespace(params=1, tensors=1)
    if variant in ("lora", "trainable"):
        st.variant = variant
    elif variant == "saliency":
        st.set_saliency(SaliencyMask.ones(eng))
    elif variant == "ewc":
        st.set_ewc(FisherAnchor.uniform(eng, 1.0))
    return st


# (overlap, exchange) -> accepted, per variant: written out, not computed from the table under test
ACCEPTS = {
    "full": {(True, "allreduce"): True, (True, "sharded"): True, (False, "allreduce"): True, (False, "sharded"): True},
    "trainable": {(True, "allreduce"): False, (True, "sharded"): False, (False, "allreduce"): True, (False, "sharded"): False},
    "lora": {(True, "allreduce"): False, (True, "sharded"): False, (False, "allreduce"): True, (False, "sharded"): False},
    "saliency": {(True, "allreduce"): True, (True, "sharded"): False, (False, "allreduce"): True, (False, "sharded"): False},
    "ewc": {(True, "allreduce"): True, (True, "sharded"): False, (False, "allreduce"): True, (False, "sharded"): False},
}


@pytest.mark.parametrize("variant", list(ACCEPTS))
def test_set_overlap_accepts_and_refuses_by_variant(monkeypatch, variant):
    st = host_stepper(variant, monkeypatch)
    for (on, exchange), ok in ACCEPTS[variant].items():
        if ok:
            st.set_overlap(on, exchange)
            assert (st.overlap, st.exchange) == (on, exchange)
            assert (st.e.on_early_grads_final is not None) == on
        else:
            with pytest.raises(NotImplementedError, match="allreduce"):
                st.set_overlap(on, exchange)
    # without collectives nothing is refused
    st.dp_on = False
    for on, exchange in ACCEPTS[variant]:
        st.set_overlap(on, exchange)


@pytest.mark.parametrize("variant,fitted,lines", [("full", (True, "sharded"), 0), ("trainable", (False, "allreduce"), 2),
                                                  ("lora", (False, "allreduce"), 2), ("saliency", (True, "allreduce"), 1),
                                                  ("ewc", (True, "allreduce"), 1)])
def test_the_exchange_asked_for_is_fitted_to_the_variant_and_said(monkeypatch, capsys, variant, fitted, lines):
    st = host_stepper(variant, monkeypatch)
    capsys.readouterr()
    st.exchange = "sharded"
    st._fit_exchange(True)
    assert (st.overlap, st.exchange) == fitted
    said = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[siss_amd] ")]
    assert len(said) == lines, said
    assert all("using the all-reduce" in l or "is off" in l for l in said)
    if variant in ("trainable", "lora"):            # one exchange mode: the autotune has nothing to time and runs no step
        st.e.ps.split = 0
        assert st.autotune_overlap(lambda: pytest.fail("a step was run")) is False


def test_log_fields_are_the_counts_and_the_active_variants_own(monkeypatch):
    counts = dict(trainable_params=64, trainable_tensors=1)
    assert host_stepper("full", monkeypatch).log_fields() == counts
    assert host_stepper("trainable", monkeypatch).log_fields() == dict(trainable_params=1, trainable_tensors=1)
    assert host_stepper("ewc", monkeypatch).log_fields() == dict(counts, ewc_strength=1.0)
    assert host_stepper("saliency", monkeypatch).log_fields() == dict(counts, saliency_params=64, saliency_fraction=1.0,
                                                                     saliency_threshold=None)


def test_exclusive_names_both_keys_and_the_reason():
    from siss_amd.variants import SHARD, VARIANTS, exclusive
    exclusive("here", {"ewc=": None, "lora=": 1, "trainable=": None})
    exclusive("here", {})
    with pytest.raises(ValueError, match=r"here: ewc= and lora= do not combine") as e:
        exclusive("here", {"ewc=": 0, "saliency=": None, "lora=": 1, "trainable=": 2})
    assert VARIANTS["ewc"].alone in str(e.value)
    with pytest.raises(NotImplementedError, match="mask=") as e:
        exclusive("there", {"ranges=": None, "mask=": 1, SHARD: True}, NotImplementedError)
    assert VARIANTS["saliency"].sharded in str(e.value) and SHARD in str(e.value)
    with pytest.raises(ValueError, match="deletion.lora.*deletion.trainable") as e:
        exclusive("config", {"deletion.lora": {}, "deletion.trainable": ["attn"]})
    assert VARIANTS["lora"].alone in str(e.value)


# ================================================================ the rank-0 build protocol of the tasks
class Built:
    def __init__(self, tensor, note):
        self.tensor, self.note, self.saved = tensor, note, None

    def save(self, directory):
        self.saved = directory


def rank0_protocol(monkeypatch, rank, sent, build, check=None):
    """_built_on_rank0 as `rank` of 2 over a recording stand-in for torch.distributed; sent: what rank 0's object list holds."""
    import torch.distributed as dist
    from siss_amd.tasks import _built_on_rank0
    calls = []

    def broadcast_object_list(word, src, group):
        calls.append(("broadcast_object_list", None if rank != 0 else word[0]))
        if rank != 0:
            word[0] = sent

    monkeypatch.setattr(dist, "broadcast_object_list", broadcast_object_list)
    monkeypatch.setattr(dist, "broadcast", lambda t, src, group: calls.append(("broadcast", t)))
    try:
        obj = _built_on_rank0("the.key: rank 0 could not build it", build, lambda o: dict(note=o.note),
                              lambda c: Built(torch.zeros(4), c["note"]), lambda o: o.tensor, "/out", rank, 2, "group",
                              check=check)
    except Exception as e:
        return e, calls
    return obj, calls


def test_rank0_builds_the_others_agree_first_then_receive(monkeypatch):
    mine = Built(torch.ones(4), "built here")
    checked = []
    # rank 0: builds, sends the description, then the tensor, checks, saves
    obj, calls = rank0_protocol(monkeypatch, 0, None, lambda: mine, check=lambda o, c: checked.append((o, c)))
    assert obj is mine and [c[0] for c in calls] == ["broadcast_object_list", "broadcast"]
    assert calls[0][1] == dict(note="built here") and calls[1][1] is mine.tensor
    assert checked == [(mine, dict(note="built here"))] and mine.saved == "/out"
    # rank 1: never builds; an empty object from the description receives the tensor; it does not save
    never = lambda: pytest.fail("a rank other than 0 built the object")
    obj, calls = rank0_protocol(monkeypatch, 1, dict(note="from rank 0"), never, check=lambda o, c: checked.append((o, c)))
    assert [c[0] for c in calls] == ["broadcast_object_list", "broadcast"]
    assert obj.note == "from rank 0" and calls[1][1] is obj.tensor and obj.saved is None and checked[-1] == (obj, dict(note="from rank 0"))
    # an error string: every rank raises BEFORE any tensor broadcast -- rank 0 its own exception, the others one that quotes it
    err, calls = rank0_protocol(monkeypatch, 1, "ValueError: F is zero", never)
    assert isinstance(err, RuntimeError) and "the.key: rank 0 could not build it (ValueError: F is zero)" in str(err)
    assert [c[0] for c in calls] == ["broadcast_object_list"]
    boom = ValueError("F is zero")

    def fails():
        raise boom
    err, calls = rank0_protocol(monkeypatch, 0, None, fails)
    assert err is boom and calls == [("broadcast_object_list", "ValueError: F is zero")]
    # a failing check raises after the broadcast, before the save
    def bad(o, c):
        raise RuntimeError("set bits differ")
    other = Built(torch.ones(4), "x")
    err, calls = rank0_protocol(monkeypatch, 0, None, lambda: other, check=bad)
    assert "set bits differ" in str(err) and len(calls) == 2 and other.saved is None


def test_one_rank_builds_and_saves_without_a_collective(monkeypatch):
    import torch.distributed as dist
    from siss_amd.tasks import _built_on_rank0
    monkeypatch.setattr(dist, "broadcast_object_list", lambda *a, **k: pytest.fail("a collective on one rank"))
    monkeypatch.setattr(dist, "broadcast", lambda *a, **k: pytest.fail("a collective on one rank"))
    mine = Built(torch.ones(4), "alone")
    assert _built_on_rank0("x", lambda: mine, None, None, None, "/out", 0, 1, None) is mine and mine.saved == "/out"


def test_the_entry_points_are_declared():
    from siss_amd import lib
    from siss_amd.ewc import ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert lib.has(name) and name in lib.PARAMS, name
    for name in ("siss_fisher_accumulate", "siss_grad_norms_scale_ewc"):
        assert lib.PARAMS[name][-1] == "stream" and name in lib.F32_SAME
    assert lib.query("siss_ewc_partials_words") == 2 * O.MAX_BLOCKS
    assert lib.PARAMS["siss_fisher_accumulate"] == ("g", "F", "n", "w", "stream")
    assert lib.PARAMS["siss_grad_norms_scale_ewc"] == ("gx", "ga", "p", "pstar", "F", "n", "strength", "mode", "knob", "max_norm", "beta1",
                                                      "beta2", "partials", "ewc_partials", "scalars", "stream")

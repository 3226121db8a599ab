"""Host side of gradient surgery (siss_amd/surgery.py, FlatAdamW.launch(surgery=...), SISSStepper.set_surgery), without a GPU:

* deletion.surgery: defaults and the round trip; every malformed mapping is refused by name; each pairing with another variant is
  refused; the three losses without a gradient pair under the norm fix are refused with their reason; the tasks read the key in
  check_supported; the key is absent from the four YAMLs and the pre-training task refuses it;
* the group table and the job plan of a small spec list (128 + 64 + 64 floats, 139 real parameters): offsets, the padding belongs to
  the tensor before it, the jobs tile [0, total) exactly once -- and siss_amd.surgery's plan equals tests/surgery_ref.py's restatement;
* properties of the f64 definition (tests/surgery_ref.py) on random data: <x', a> = 0 on every conflicting group under keep and
  mutual, <a', x> = 0 under forget and mutual, |a'| s = scaling_norm, a pair without conflict gives the plain step's s, clip and g,
  `global` on a buffer equals `tensor` on a one-tensor buffer; the coefficient form g = clip (cx x - ca a) equals clip (x' - s a');
* the kernel-order restatement against the definition (sums to 2^-40 relative, the block to f32 rounding), and against
  optimizer_ref's plain restatement bit for bit where nothing conflicts;
* FlatAdamW.launch(surgery=...): the two entry points and every argument by the header's names; refusals before any launch (with
  ranges / mask / ewc, EraseDiff's eta, a plan over another buffer, launch_sharded); SISSStepper.set_surgery on a stepper built without
  its constructor: the variant, the exchange table (overlap allowed, sharded refused and said), the refused losses, the log fields.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

import optimizer_ref as O
import surgery_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
HP = O.hyper(*O.HYPER["sd"])


# ================================================================ the parsed key
def test_parse_defaults_and_round_trip():
    from siss_amd.surgery import FIELDS, KEY, parse_surgery
    assert KEY == "deletion.surgery" and parse_surgery(None) is None
    assert parse_surgery({}).as_dict() == dict(mode="forget", granularity="tensor")
    assert parse_surgery(dict(mode=None, granularity=None)).as_dict() == dict(mode="forget", granularity="tensor")
    for mode in ("forget", "keep", "mutual"):
        for gran in ("global", "tensor"):
            c = parse_surgery(dict(mode=mode, granularity=gran))
            assert c.as_dict() == dict(mode=mode, granularity=gran) and tuple(c.as_dict()) == FIELDS
            assert parse_surgery(c.as_dict()).as_dict() == c.as_dict()


def test_parse_refusals_name_the_entry():
    from siss_amd.surgery import parse_surgery
    rows = [(3, "mapping"), (["mutual"], "mapping"), ("mutual", "mapping"), (dict(mod="keep"), "mod"), (dict(mode="keep", rank=4), "rank"),
            (dict(mode="pcgrad"), "mode"), (dict(mode=1), "mode"), (dict(mode=True), "mode"), (dict(mode=["keep"]), "mode"),
            (dict(granularity="layer"), "granularity"), (dict(granularity=2), "granularity"),
            (dict(mode="mutual", granularity="block"), "granularity")]
    for bad, word in rows:
        with pytest.raises(ValueError, match="deletion.surgery") as e:
            parse_surgery(bad)
        assert word in str(e.value), (bad, str(e.value))
    for kw, name in ((dict(trainable=["attn"]), "deletion.trainable"), (dict(lora=dict(rank=4)), "deletion.lora"),
                     (dict(saliency=dict(fraction=0.5)), "deletion.saliency"), (dict(ewc=dict(strength=1.0)), "deletion.ewc")):
        with pytest.raises(ValueError, match=name) as e:
            parse_surgery(dict(mode="mutual"), **kw)
        assert "deletion.surgery" in str(e.value) and "gradient pair" in str(e.value)


def test_the_losses_without_a_pair_under_the_norm_fix_are_refused_with_their_reason():
    from siss_amd.surgery import LOSSES, check_loss
    for loss in ("importance_sampling_with_mixture", "double_forward_with_neg_del", "subscore_bernoulli"):
        assert check_loss(loss) == loss and loss in LOSSES
    for loss, word in (("erasediff", "conflict rule"), ("simple_neg_del", "one gradient set"), ("naive_del", "one gradient set")):
        with pytest.raises(ValueError, match="deletion.surgery") as e:
            check_loss(loss)
        assert loss in str(e.value) and word in str(e.value)
    with pytest.raises(ValueError):
        check_loss("something_else")


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config):
    from siss_amd import hydra_lite as H

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    assert task([]).surgery_config() is None and task(["+deletion.surgery=null"]).surgery_config() is None
    task([]).check_supported()
    t = task(["+deletion.surgery={mode:mutual}"])
    assert t.surgery_config().as_dict() == dict(mode="mutual", granularity="tensor")
    t.check_supported()
    task(["+deletion.surgery={mode:keep,granularity:global}", "+deletion.ssd={alpha:10}"]).check_supported()      # ssd does combine
    for ov, word in (("mutual", "mapping"), ("{mode:pcgrad}", "mode"), ("{granularity:layer}", "granularity"), ("{rank:4}", "rank")):
        with pytest.raises(ValueError, match="deletion.surgery") as e:
            task(["+deletion.surgery=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    for other, name in (("+deletion.trainable=[attn]", "deletion.trainable"), ("+deletion.lora={rank:4,targets:[attn]}", "deletion.lora"),
                        ("+deletion.saliency={fraction:0.5}", "deletion.saliency"), ("+deletion.ewc={strength:1}", "deletion.ewc")):
        with pytest.raises(ValueError, match=name):
            task(["+deletion.surgery={mode:mutual}", other]).check_supported()
    for loss in ("erasediff", "simple_neg_del", "naive_del"):
        with pytest.raises(ValueError, match="deletion.surgery") as e:
            task(["+deletion.surgery={mode:mutual}", f"deletion.loss_fn={loss}"] + (["+deletion.eta=0.01"] if loss == "erasediff" else [])
                 ).check_supported()
        assert loss in str(e.value)


def test_the_yamls_lack_the_key_and_the_pretraining_task_refuses_it():
    from siss_amd import hydra_lite as H
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "surgery" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "surgery" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.surgery={mode:mutual}"])
    with pytest.raises(NotImplementedError, match="deletion.surgery"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [])
    H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


# ================================================================ the group table and the plan
def fake_engine(numels=(70, 64, 5), align=64, seed=0, order=None):
    specs, off = {}, 0
    for i in (order or range(len(numels))):
        specs[f"w{i}"] = types.SimpleNamespace(name=f"w{i}", off=off, numel=numels[i])
        off += -(-numels[i] // align) * align
    flat = torch.randn(off, generator=torch.Generator().manual_seed(seed))
    return types.SimpleNamespace(ps=types.SimpleNamespace(specs=specs, total=off, flat=flat), device=torch.device("cpu"))


def test_group_table_of_a_small_spec_list():
    from siss_amd.surgery import group_table, job_plan, plan_words
    eng = fake_engine()                                        # 128 + 64 + 64 floats, 139 real parameters
    assert eng.ps.total == 256 and sum(sp.numel for sp in eng.ps.specs.values()) == 139
    names, off = group_table(eng.ps.specs, eng.ps.total, "tensor")
    assert names == ["w0", "w1", "w2"] and off == [0, 128, 192, 256]
    for sp, lo, hi in zip(eng.ps.specs.values(), off, off[1:]):         # the padding belongs to the tensor before it
        assert lo == sp.off and hi - lo >= sp.numel and (hi == eng.ps.total or hi in [s.off for s in eng.ps.specs.values()])
    assert group_table(eng.ps.specs, eng.ps.total, "global") == (["*"], [0, 256])
    # buffer order is the offsets', not the dictionary's
    specs = dict(reversed(list(eng.ps.specs.items())))
    assert group_table(specs, eng.ps.total, "tensor") == (names, off)
    # a table whose first tensor does not start the buffer, or whose stretch cannot hold its tensor, is refused
    bad = {k: types.SimpleNamespace(name=k, off=sp.off + 64, numel=sp.numel) for k, sp in eng.ps.specs.items()}
    with pytest.raises(ValueError):
        group_table(bad, 320, "tensor")
    bad = dict(eng.ps.specs, w1=types.SimpleNamespace(name="w1", off=128, numel=65))
    with pytest.raises(ValueError, match="w1"):
        group_table(bad, 256, "tensor")
    for C in (64, 128, 1024):
        starts, groups, first = job_plan(off, C)
        assert (starts, groups, first) == R.plan(off, C)
        cover = np.zeros(256, int)
        for st, g in zip(starts, groups):
            ln = min(C, off[g + 1] - st)
            assert off[g] <= st and st + ln <= off[g + 1] and (st - off[g]) % C == 0
            cover[st:st + ln] += 1
        assert (cover == 1).all(), "the jobs tile [0, total) exactly once"
        assert first[0] == 0 and first[-1] == len(starts) and all(groups[j] == g for g in range(3) for j in range(first[g], first[g + 1]))
        words, jobs = plan_words(off, C)
        assert jobs == len(starts) and words == starts + groups + first + off
    assert job_plan(off, 64)[0] == [0, 64, 128, 192] and job_plan(off, 1024)[0] == [0, 128, 192]


# ================================================================ properties of the f64 definition
LENGTHS = (128, 64, 64, 260, 8, 1024, 36)


def dot(u, w):
    return math.fsum(np.asarray(u, f64) * np.asarray(w, f64))


@pytest.mark.parametrize("mode", R.MODES)
def test_projections_are_orthogonal_on_the_conflicting_groups_and_the_norm_fix_holds(mode):
    gx, ga, off = R.case(LENGTHS, 3)
    x2, a2, S, phi = R.project_f64(gx, ga, off, mode)
    assert phi == [True, False, False, True, False, False, True] or sum(phi) >= 2, phi
    assert not phi[1] and not phi[2] and not phi[4], "x = 0, a = 0 and xa = 0 must not conflict"
    assert S[1, 0] == 0 and S[2, 1] == 0 and S[4, 2] == 0 and S[4, 0] > 0 and S[4, 1] > 0
    for g, (lo, hi) in enumerate(zip(off, off[1:])):
        x, a = gx[lo:hi].astype(f64), ga[lo:hi].astype(f64)
        scale = math.sqrt(S[g, 0] * S[g, 1]) or 1.0
        if phi[g] and mode in ("keep", "mutual"):
            assert abs(dot(x2[lo:hi], a)) <= 1e-12 * scale
        if phi[g] and mode in ("forget", "mutual"):
            assert abs(dot(a2[lo:hi], x)) <= 1e-12 * scale
        if not phi[g] or mode == "forget":
            assert np.array_equal(x2[lo:hi], x)
        if not phi[g] or mode == "keep":
            assert np.array_equal(a2[lo:hi], a)
    sc = R.scalars_f64(S, mode, 0, 5.0, 1.0, 0.95, 0.999, 1)
    na2 = math.sqrt(dot(a2, a2))
    assert abs(na2 * sc["scale"] - 5.0) <= 1e-12 * 5.0, "|a'| s = scaling_norm"
    assert abs(sc["norm_a_projected"] - na2) <= 1e-12 * na2
    assert sc["conflicts"] == sum(phi) and -1 <= sc["cos"] <= 1
    assert abs(sc["removed_a"] - (1 - dot(a2, a2) / dot(ga, ga))) <= 1e-12
    assert abs(sc["removed_x"] - (1 - dot(x2, x2) / dot(gx, gx))) <= 1e-12
    assert (sc["removed_a"] > 0) == (mode != "keep") and (sc["removed_x"] > 0) == (mode != "forget")
    # the coefficient form IS the projected pair: cx x - ca a = x' - s a', and the pre-clip norm is its norm
    g_coef = R.per_element(sc["cx"], off) * gx.astype(f64) - R.per_element(sc["ca"], off) * ga.astype(f64)
    g_proj = x2 - sc["scale"] * a2
    assert np.abs(g_coef - g_proj).max() <= 1e-12 * np.abs(g_proj).max()
    assert abs(sc["pre_clip_norm"] - math.sqrt(dot(g_proj, g_proj))) <= 1e-10 * sc["pre_clip_norm"]


@pytest.mark.parametrize("nmode", [0, 2])
@pytest.mark.parametrize("mode", R.MODES)
def test_a_pair_without_conflict_gives_the_plain_step(mode, nmode):
    gx, ga, off = R.case(LENGTHS, 5, conflict="none")
    n = off[-1]
    rng = np.random.default_rng(1)
    p = rng.standard_normal(n).astype(f32)
    m, v = O.warm_state(n, 3, HP, seed=2)
    (p1, m1, v1, g1), sc = R.step_f64(gx, ga, p, m, v, 3, HP, off, mode, nmode, 5.0, 1.0)
    (p0, m0, v0, g0), sc0 = R.step_f64(gx, ga, p, m, v, 3, HP, off, None, nmode, 5.0, 1.0)
    assert sc["conflicts"] == 0 and sc["removed_a"] == 0 and sc["removed_x"] == 0 and sc["cos"] < 0
    for k in ("norm_x", "norm_a", "dot", "scale", "pre_clip_norm", "clip_coef"):
        assert abs(sc[k] - sc0[k]) <= 1e-12 * abs(sc0[k]), k
    assert (sc["cx"] == 1.0).all() and (sc["ca"] == sc["scale"]).all()
    for got, ref in ((p1, p0), (m1, m0), (v1, v0), (g1, g0)):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # all-zero forget set under the inf guard: s = 0, nothing conflicts, no NaN
    z = np.zeros(n, f32)
    (pz, _, _, gz), scz = R.step_f64(gx, z, p, m, v, 3, HP, off, mode, 2, 5.0, 1.0)
    assert scz["scale"] == 0.0 and scz["conflicts"] == 0 and np.isfinite(pz).all() and scz["cos"] == 0.0 and scz["removed_a"] == 0.0


@pytest.mark.parametrize("mode", R.MODES)
def test_global_equals_tensor_on_a_one_tensor_buffer(mode):
    gx, ga, off = R.case((1024 + 36,), 9, conflict={0})
    n = off[-1]
    p, m, v = np.ones(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    a = R.step_f64(gx, ga, p, m, v, 1, HP, [0, n], mode, 0, 5.0, 1.0)                # `global`
    b = R.step_f64(gx, ga, p, m, v, 1, HP, off, mode, 0, 5.0, 1.0)                   # `tensor`, one tensor
    assert a[1]["conflicts"] == 1 and all(np.array_equal(s, t) for s, t in zip(a[0], b[0]))
    # ... and on a buffer of several tensors the two differ (the negative control of this equality)
    gx, ga, off = R.case(LENGTHS, 3)
    n = off[-1]
    p, m, v = np.ones(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    a = R.step_f64(gx, ga, p, m, v, 1, HP, [0, n], mode, 0, 5.0, 1.0)
    b = R.step_f64(gx, ga, p, m, v, 1, HP, off, mode, 0, 5.0, 1.0)
    assert not np.array_equal(a[0][3], b[0][3])


# ================================================================ the kernel-order restatement against the definition
@pytest.mark.parametrize("C", [64, 1024])
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_of_the_kernels_against_the_definition(mode, C):
    lengths = (C - 4, C, C + 4, 2 * C + 8, 4, 64, 3 * C + 3)
    gx, ga, off = R.case(lengths, 11)
    rows = R.job_rows(gx, ga, off, C)
    _, _, first = R.plan(off, C)
    assert len(rows) == first[-1] == sum(-(-n // C) for n in lengths)
    S = R.group_sums(rows, first)
    S64 = R.sums_f64(gx, ga, off)
    # (four f32 operations per term, then f64: 4u per term -- optimizer_ref.scalar_bounds' argument, per group)
    ax = np.array([[dot(gx[lo:hi], gx[lo:hi]), dot(ga[lo:hi], ga[lo:hi]), math.fsum(np.abs(gx[lo:hi].astype(f64) * ga[lo:hi].astype(f64)))]
                   for lo, hi in zip(off, off[1:])])
    assert (np.abs(S - S64) <= 4 * R.U * ax + 1e-300).all()
    assert R.conflicts(S) == R.conflicts(S64)
    blk, coef = R.scalars_coef(S, mode, 0, 5.0, 1.0, 0.95, 0.999, 6)
    ref = R.scalars_f64(S, mode, 0, 5.0, 1.0, 0.95, 0.999, 7)          # from the SAME sums: only the fold orders and one rounding differ
    for k, i in O.NAMES.items():
        assert abs(float(blk[i]) - ref[k]) <= R.U * (1 + 2.0 ** -20) * abs(ref[k]), (k, blk[i], ref[k])
    for k, i in (("conflicts", 12), ("cos", 13), ("removed_a", 14), ("removed_x", 15)):
        assert abs(float(blk[i]) - ref[k]) <= R.U * (1 + 2.0 ** -20) * abs(ref[k]) + 1e-12, (k, blk[i], ref[k])
    assert (blk[[7, 10, 11]] == 0).all()
    assert np.array_equal(coef[:, 0], ref["cx"].astype(f32)) and np.array_equal(coef[:, 1], ref["ca"].astype(f32))
    quiet = [g for g, f in enumerate(R.conflicts(S)) if not f]
    assert quiet and (coef[quiet, 0] == f32(1)).all() and (coef[quiet, 1] == blk[3]).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_restated_update_without_conflict_is_the_plain_restatement_bit_for_bit(mode):
    gx, ga, off = R.case(LENGTHS, 5, conflict="none")
    n = off[-1]
    rng = np.random.default_rng(4)
    p = rng.standard_normal(n).astype(f32)
    m, v = O.warm_state(n, 3, HP, seed=2)
    _, _, first = R.plan(off, 64)
    blk, coef = R.scalars_coef(R.group_sums(R.job_rows(gx, ga, off, 64), first), mode, 0, 5.0, 1.0, HP[1], HP[2], 2)
    assert blk[12] == 0 and (coef[:, 0] == 1).all() and (coef[:, 1] == blk[3]).all()
    got = R.update_f32(gx, ga, p, m, v, blk, coef, off, HP)
    ref = O.adamw_f32(gx, ga, p, m, v, blk, HP)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, ref))
    # ... against the f64 definition: the precision of one f32 step (the update over its largest value)
    (p64, m64, v64, g64), _ = R.step_f64(gx, ga, p, m, v, 3, HP, off, mode, 0, 5.0, 1.0)
    assert np.abs(got[3] - g64).max() <= 8 * R.U * np.abs(g64).max()


# ================================================================ FlatAdamW.launch(surgery=...)
def cpu_optimizer(n=64):
    from siss_amd.optim import FlatAdamW
    opt = FlatAdamW.__new__(FlatAdamW)               # (the constructor wants a device buffer and the library's slab sizes)
    opt.p = torch.zeros(n)
    opt.m, opt.v, opt.shadow, opt.last_grad = torch.zeros(n), torch.zeros(n), None, None
    opt.lr, opt.betas, opt.eps, opt.wd, opt.max_grad_norm = 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0
    opt.partials, opt.scalars = torch.zeros(8, dtype=torch.float64), torch.zeros(16)
    return opt


CHUNK = 1024


def fake_query(name, *a):
    return {"siss_surgery_chunk": CHUNK, "siss_surgery_partials_words": 3 * (a[0] if a else 0),
            "siss_surgery_coef_words": 2 * (a[0] if a else 0)}.get(name, 4096)


def host_surgery(monkeypatch, eng, mode="mutual", granularity="tensor"):
    from siss_amd import lib
    from siss_amd.surgery import Surgery
    monkeypatch.setattr(lib, "has", lambda name: True)
    monkeypatch.setattr(lib, "query", fake_query)
    return Surgery(eng, mode, granularity)


def test_the_object_owns_the_plan_and_the_slabs(monkeypatch):
    eng = fake_engine((1100, 64, 5))                           # 1152 + 64 + 64 floats: the first tensor is two jobs of 1024
    sg = host_surgery(monkeypatch, eng)
    assert (sg.total, sg.tensors, sg.params) == (1280, 3, 1169) and sg.names == ["w0", "w1", "w2"]
    assert sg.offsets == [0, 1152, 1216, 1280] and sg.groups == 3 and sg.jobs == 4 and sg.chunk == CHUNK and sg.smode == 2
    assert sg.group_offsets.tolist() == sg.offsets and sg.group_offsets.dtype == torch.int64
    assert sg.plan.tolist() == [0, 1024, 1152, 1216, 0, 0, 1, 2, 0, 2, 3, 4, 0, 1152, 1216, 1280]
    assert sg.partials.numel() == 12 and sg.partials.dtype == torch.float64 and sg.group_sums.numel() == 9 and sg.coef.numel() == 6
    assert sg.log_fields() == dict(surgery_mode="mutual", surgery_granularity="tensor", surgery_groups=3)
    blk = torch.zeros(16)
    blk[12:] = torch.tensor([2.0, 0.25, 0.125, 0.5])
    assert sg.stats_from(blk) == dict(surgery_conflicts=2, surgery_cos=0.25, surgery_removed_a=0.125, surgery_removed_x=0.5,
                                      surgery_mode="mutual", surgery_granularity="tensor", surgery_groups=3)
    sg.group_sums.copy_(torch.tensor([4.0, 9.0, 3.0, 0.0, 1.0, 0.0, 1.0, 1.0, -0.5], dtype=torch.float64))
    assert sg.grams() == {"w0": (4.0, 9.0, 3.0, True), "w1": (0.0, 1.0, 0.0, False), "w2": (1.0, 1.0, -0.5, False)}
    g = host_surgery(monkeypatch, eng, "keep", "global")
    assert g.names == ["*"] and g.offsets == [0, 1280] and g.groups == 1 and g.jobs == 2 and g.smode == 1
    with pytest.raises(ValueError, match="mode"):
        host_surgery(monkeypatch, eng, "pcgrad")
    monkeypatch.setattr(__import__("siss_amd").lib, "has", lambda name: name != "siss_recombine_clip_adamw_surgery")
    with pytest.raises(RuntimeError, match="siss_recombine_clip_adamw_surgery"):
        from siss_amd.surgery import Surgery
        Surgery(eng)


@pytest.mark.parametrize("want_grad", [False, True])
def test_flat_adamw_launch_sequence_and_refusals(monkeypatch, want_grad):
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    n = 1280
    eng = fake_engine((1100, 64, 5))
    sg = host_surgery(monkeypatch, eng)
    opt = cpu_optimizer(n)
    opt.shadow = torch.zeros(n, dtype=torch.bfloat16)
    grads = torch.zeros(2, n)
    seen = []
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: seen.append((name, a)) or 0)
    with pytest.raises(ValueError, match=r"surgery=.*ranges="):
        opt.launch(grads, scaling_norm=5.0, ranges=(torch.zeros(3, dtype=torch.int64), 1, 16), surgery=sg)
    with pytest.raises(ValueError, match=r"surgery=.*mask="):
        opt.launch(grads, scaling_norm=5.0, mask=torch.zeros(40, dtype=torch.int32), surgery=sg)
    with pytest.raises(ValueError, match=r"surgery=.*ewc="):
        opt.launch(grads, scaling_norm=5.0, ewc=FisherAnchor.uniform(eng, 1.0), surgery=sg)
    with pytest.raises(NotImplementedError, match="gradient surgery"):
        opt.launch_sharded(grads[0, :32], grads[1, :32], 0, 32, None, scaling_norm=5.0, surgery=sg)
    with pytest.raises(ValueError, match="EraseDiff"):
        opt.launch(grads, eta=1e-2, surgery=sg)
    with pytest.raises(ValueError, match="plan"):
        opt.launch(grads, scaling_norm=5.0, surgery=host_surgery(monkeypatch, fake_engine((1100, 64, 5, 7))))
    assert seen == [], f"a refusal launched {[s[0] for s in seen]}"
    opt.launch(grads, scaling_norm=5.0, want_grad=want_grad, surgery=sg)
    first = opt.last_grad
    opt.launch(grads, scaling_norm=5.0, inf_guard=True, want_grad=want_grad, surgery=sg)
    assert [s[0] for s in seen] == 2 * ["siss_grad_norms_scale_surgery", "siss_recombine_clip_adamw_surgery"]
    assert (first is not None and opt.last_grad is first) if want_grad else opt.last_grad is None
    same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape
    modes = []
    for name, args in seen:
        assert len(args) == len(lib.PARAMS[name]) - 1, (name, len(args), lib.PARAMS[name])          # (the stream is lib.call's)
        a = dict(zip(lib.PARAMS[name], args))
        assert same(a.pop("gx"), grads[0]) and same(a.pop("ga"), grads[1]) and a.pop("n") == n and a.pop("scalars") is opt.scalars
        assert a.pop("groups") is sg.group_offsets and a.pop("T") == 3 and a.pop("plan") is sg.plan and a.pop("jobs") == 4
        assert a.pop("coef") is sg.coef and (a.pop("beta1"), a.pop("beta2")) == opt.betas
        if name == "siss_grad_norms_scale_surgery":
            modes.append((a.pop("smode"), a.pop("mode")))
            assert (a.pop("knob"), a.pop("max_norm")) == (5.0, 1.0)
            assert a.pop("partials") is sg.partials and a.pop("group_sums") is sg.group_sums
        else:
            assert a.pop("p") is opt.p and a.pop("m") is opt.m and a.pop("v") is opt.v and a.pop("shadow") is opt.shadow
            assert a.pop("g_out") is (first if want_grad else None)
            assert (a.pop("lr"), a.pop("eps"), a.pop("wd")) == (opt.lr, opt.eps, opt.wd)
        assert a == {}, (name, sorted(a))
    assert modes == [(2, 0), (2, 2)]


# ================================================================ the stepper's side
def host_stepper(monkeypatch, loss_fn="importance_sampling_with_mixture"):
    from siss_amd.step import SISSStepper
    eng = fake_engine((1100, 64, 5))
    eng.on_early_grads_final = None
    st = SISSStepper.__new__(SISSStepper)
    st.e, st.opt, st.pg, st.world, st.dp_on = eng, cpu_optimizer(1280), object(), 1, True
    st.lora = st.subset = st.saliency = st.ewc = st.surgery = None
    st.variant, st._launch_kw, st.overlap, st.exchange, st.loss_fn = "full", {}, False, "allreduce", loss_fn
    return st


def test_set_surgery_moves_a_full_stepper_and_fits_the_exchange(monkeypatch, capsys):
    from siss_amd.variants import VARIANTS, exchange_refusal
    v = VARIANTS["surgery"]
    assert v.overlap is None and v.sharded and "\n" not in v.sharded and v.alone
    assert exchange_refusal("surgery", True, "allreduce") is None and exchange_refusal("surgery", False, "sharded")
    st = host_stepper(monkeypatch)
    sg = host_surgery(monkeypatch, st.e)
    st.exchange = "sharded"
    st.overlap = True
    capsys.readouterr()
    st.set_surgery(sg)
    assert st.variant == "surgery" and st.surgery is sg and st._launch_kw == {"surgery": sg} and st._active() is sg
    assert (st.overlap, st.exchange) == (True, "allreduce") and st.e.on_early_grads_final is not None
    said = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[siss_amd] ")]
    assert len(said) == 1 and "gradient surgery" in said[0] and "using the all-reduce" in said[0]
    for (on, exchange), ok in {(True, "allreduce"): True, (True, "sharded"): False, (False, "allreduce"): True,
                               (False, "sharded"): False}.items():
        if ok:
            st.set_overlap(on, exchange)
            assert (st.overlap, st.exchange) == (on, exchange)
        else:
            with pytest.raises(NotImplementedError, match="allreduce"):
                st.set_overlap(on, exchange)
    assert st.log_fields() == dict(trainable_params=1169, trainable_tensors=3, surgery_mode="mutual", surgery_granularity="tensor",
                                   surgery_groups=3)
    # another variant on top, or surgery on top of another, is refused by name
    from siss_amd.saliency import SaliencyMask
    with pytest.raises(ValueError, match="set_saliency"):
        st.set_saliency(SaliencyMask.ones(st.e))
    st2 = host_stepper(monkeypatch)
    st2.set_saliency(SaliencyMask.ones(st2.e))
    with pytest.raises(ValueError, match="set_surgery"):
        st2.set_surgery(host_surgery(monkeypatch, st2.e))
    # a plan over another engine's layout
    st3 = host_stepper(monkeypatch)
    with pytest.raises(ValueError, match="layout"):
        st3.set_surgery(host_surgery(monkeypatch, fake_engine((1100, 64, 5, 7))))


@pytest.mark.parametrize("loss_fn,word", [("erasediff", "conflict rule"), ("simple_neg_del", "one gradient set"),
                                          ("naive_del", "one gradient set")])
def test_set_surgery_refuses_the_losses_without_a_pair(monkeypatch, loss_fn, word):
    st = host_stepper(monkeypatch, loss_fn)
    with pytest.raises(ValueError, match="surgery") as e:
        st.set_surgery(host_surgery(monkeypatch, st.e))
    assert loss_fn in str(e.value) and word in str(e.value) and st.variant == "full" and st.surgery is None


def test_the_entry_points_are_declared():
    from siss_amd import lib
    from siss_amd.build import EXACT
    from siss_amd.surgery import ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert lib.has(name) and name in lib.PARAMS, name
    for name in ("siss_grad_norms_scale_surgery", "siss_recombine_clip_adamw_surgery"):
        assert lib.PARAMS[name][-1] == "stream" and name in lib.F32_SAME
    assert "surgery.hip" in EXACT
    C = lib.query("siss_surgery_chunk")
    assert C > 0 and C % 1024 == 0
    assert lib.query("siss_surgery_partials_words", 7) == 21 and lib.query("siss_surgery_coef_words", 5) == 10

"""siss_amd/ssd.py and the restatement tests/ssd_ref.py without a GPU:

* parse_ssd: the defaults, the round trip, every refusal by message;
* the restatement: beta in [0, 1]; min(lambda / r, 1) and the branch form agree bit for bit, r = +inf and r == lambda included;
  0 / 0 gives 0 and a NaN never arises; the k-th largest by integer key is the k-th largest value;
* the tasks read the key and settle every refusal in check_supported (ssd + lora, ssd + trainable before any device work); the key
  is absent from the four YAMLs and the pre-training task refuses it;
* the entry points are declared, and the shared Fisher loop is the one FisherAnchor.from_batches runs.
"""
import os

import numpy as np
import pytest

import ssd_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
KEYED = "{fraction:0.01,keep_batches:4,forget_batches:4}"


# ================================================================ the parsed key
def test_parse_ssd_defaults_and_round_trip():
    from siss_amd.ssd import FIELDS, parse_ssd
    assert parse_ssd(None) is None
    c = parse_ssd(dict(fraction=0.01))
    assert c.as_dict() == {"alpha": None, "fraction": 0.01, "lambda": 1.0, "keep_batches": 64, "forget_batches": 64, "batch_size": 1,
                           "seed": 0, "targets": None, "path": None}
    assert set(c.as_dict()) == set(FIELDS) and isinstance(c.lam, float)
    # the issue's example, nulls spelled out
    c = parse_ssd({"alpha": None, "fraction": 0.01, "lambda": 1, "keep_batches": 64, "forget_batches": 64, "batch_size": 1, "seed": 0,
                   "targets": None, "path": None})
    assert (c.alpha, c.fraction, c.lam, c.targets, c.path) == (None, 0.01, 1.0, None, None)
    full = {"alpha": 10.0, "fraction": None, "lambda": 0.5, "keep_batches": 3, "forget_batches": 2, "batch_size": 2, "seed": 7,
            "targets": ["attn", r"conv_in\.weight"], "path": "/somewhere"}
    c = parse_ssd(full)
    assert c.as_dict() == full and parse_ssd(c.as_dict()).as_dict() == full
    assert parse_ssd(dict(alpha=0)).alpha == 0.0                    # alpha = 0 is legal: every weight the forget set touches


def test_parse_ssd_refusals_name_the_entry():
    from siss_amd.ssd import parse_ssd
    ok = dict(fraction=0.01)
    nan, inf = float("nan"), float("inf")
    rows = [(3, "mapping"), ([0.01], "mapping"), ("0.01", "mapping"), (dict(ok, fracton=2), "fracton"), (dict(ok, rank=4), "rank"),
            ({}, "exactly one of alpha and fraction"), (dict(alpha=None, fraction=None), "exactly one of alpha and fraction"),
            (dict(alpha=1.0, fraction=0.01), "exactly one of alpha and fraction"),
            (dict(alpha=-1), "alpha"), (dict(alpha=nan), "alpha"), (dict(alpha=inf), "alpha"), (dict(alpha="1"), "alpha"),
            (dict(alpha=True), "alpha"),
            (dict(fraction=0), "fraction"), (dict(fraction=1), "fraction"), (dict(fraction=1.5), "fraction"), (dict(fraction=-0.1), "fraction"),
            (dict(fraction="half"), "fraction"), (dict(fraction=nan), "fraction"),
            ({**ok, "lambda": 0}, "lambda"), ({**ok, "lambda": -1.0}, "lambda"), ({**ok, "lambda": nan}, "lambda"),
            ({**ok, "lambda": inf}, "lambda"), ({**ok, "lambda": "1"}, "lambda"),
            (dict(ok, keep_batches=0), "keep_batches"), (dict(ok, keep_batches=1.5), "keep_batches"), (dict(ok, keep_batches=True), "keep_batches"),
            (dict(ok, forget_batches=0), "forget_batches"), (dict(ok, forget_batches=-3), "forget_batches"),
            (dict(ok, batch_size=0), "batch_size"), (dict(ok, batch_size=2.0), "batch_size"),
            (dict(ok, seed="x"), "seed"), (dict(ok, seed=1.5), "seed"),
            (dict(ok, targets="attn"), "targets"), (dict(ok, targets=[]), "targets"), (dict(ok, targets=[3]), "targets"),
            (dict(ok, targets=["("]), "targets"), (dict(ok, path=3), "path")]
    for bad, word in rows:
        with pytest.raises(ValueError, match="deletion.ssd") as e:
            parse_ssd(bad)
        assert word in str(e.value), (bad, str(e.value))
    for kw, name in ((dict(trainable=["attn"]), "deletion.trainable"), (dict(lora=dict(rank=4)), "deletion.lora")):
        with pytest.raises(ValueError, match=name) as e:
            parse_ssd(ok, **kw)
        msg = str(e.value)
        assert "deletion.ssd" in msg and "weight-gradient products" in msg and "deletion.ssd.targets" in msg, msg
    with pytest.raises(ValueError, match="base copy taken before the dampening"):
        parse_ssd(ok, lora=dict(rank=4))


def test_targets_match_as_the_trainable_subset_does():
    from siss_amd.ssd import parse_ssd, select_targets
    names = ["conv_in.weight", "mid.attn.to_q.weight", "mid.attn.to_k.weight", "conv_out.bias"]
    assert select_targets(names, None) is None
    assert select_targets(names, parse_ssd(dict(fraction=0.1, targets=["attn"])).targets) == names[1:3]
    assert select_targets(names, parse_ssd(dict(fraction=0.1, targets=["."])).targets) is None        # everything: no restriction
    with pytest.raises(ValueError, match=r"deletion.ssd.targets.*matches no parameter"):
        select_targets(names, parse_ssd(dict(fraction=0.1, targets=["attn", "nothing_like_it"])).targets)


# ================================================================ the restatement
def test_ratio_has_no_nan_and_the_planted_cases():
    fk = np.array([0, 0, 2, 2, 1e-12, 1e2], f32)
    ff = np.array([0, 3, 0, 1, 1e2, 1e-12], f32)
    r = S.ratio_f32(fk, ff)
    assert r.dtype == f32 and not np.isnan(r).any()
    assert r[0] == 0 and np.isposinf(r[1]) and r[2] == 0 and r[3] == f32(0.5) and r[4] == f32(1e2) / f32(1e-12) and np.isfinite(r[4:]).all()
    p, fk, ff = S.case(100_003, 1)
    r = S.ratio_f32(fk, ff)
    both, only_keep, only_forget = (fk == 0) & (ff == 0), (fk == 0) & (ff != 0), (fk != 0) & (ff == 0)
    assert both.sum() > 100 and only_keep.sum() > 100 and only_forget.sum() > 100, "the case does not plant its zeros"
    assert not np.isnan(r).any() and (r >= 0).all()
    assert (r[both] == 0).all() and np.isposinf(r[only_keep]).all() and (r[only_forget] == 0).all()
    fin = (fk != 0) & (ff != 0)
    assert np.isfinite(r[fin]).all() and (r[fin] >= f32(2.0 ** -126)).all(), "a denormal or overflowing ratio in the test inputs"


@pytest.mark.parametrize("lam", [1.0, 0.1, 3.0, 1e-3])
def test_beta_forms_agree_bit_for_bit_and_lie_in_the_unit_interval(lam):
    p, fk, ff = S.case(100_003, 2)
    r = S.ratio_f32(fk, ff)
    r[:4] = [f32(lam), np.nextafter(f32(lam), f32(np.inf)), np.nextafter(f32(lam), f32(0)), f32(np.inf)]
    pos = r > 0                                              # (min(lambda / 0, 1) is 1 too, but by way of lambda / 0 = inf)
    a, b = S.beta_branch(r, lam), S.beta_min(r, lam)
    assert a.dtype == f32 and (a.view(np.uint32)[pos] == b.view(np.uint32)[pos]).all()
    assert (a >= 0).all() and (a <= 1).all() and not np.isnan(a).any()
    assert a[0] == 1 and a[1] < 1 and a[2] == 1 and a[3] == 0, a[:4]
    assert (a[r == 0] == 1).all() and (a[np.isposinf(r)] == 0).all()
    # the dampened weight never grows, never changes sign, and r = +inf zeroes it
    q, sel, beta = S.dampen_f32(p, r, 0.5, True, lam)
    assert (np.abs(q) <= np.abs(p)).all() and (np.signbit(q) == np.signbit(p)).all()
    assert (q[np.isposinf(r)] == 0).all() and (q.view(np.uint32)[~sel] == p.view(np.uint32)[~sel]).all()


def test_kth_largest_by_key_is_the_kth_largest_value_and_the_stats_count():
    p, fk, ff = S.case(20_011, 3)
    r = S.ratio_f32(fk, ff)
    order = np.sort(r)[::-1]
    for k in (1, 7, int((r == np.inf).sum()), int((r == np.inf).sum()) + 1, 5000):
        t, tb, gt, ge = S.kth_largest(r, k)
        assert t == order[k - 1] and gt == (r > t).sum() and ge == (r >= t).sum() and gt < k <= ge
    assert np.isposinf(S.kth_largest(r, 1)[0])
    q, sel, beta = S.dampen_f32(p, r, order[4999], False, 1.0)
    st = S.stats_f64(p, q, sel, beta)
    assert st["selected"] == sel.sum() >= 5000 and st["zeroed"] == (r == np.inf).sum() and st["dampened"] >= st["zeroed"]
    assert 0 < st["sum_p2_selected"] < st["sum_p2"] and 0 < st["sum_delta2"] <= st["sum_p2_selected"]
    pi, ri = S.int_case(4099, 4)
    qi, seli, bi = S.dampen_f32(pi, ri, 2.0, False, 1.0)
    sti = S.stats_f64(pi, qi, seli, bi)
    assert sti["selected"] == (ri >= 2).sum() == sti["dampened"] and sti["zeroed"] == 0
    assert sti["sum_beta"] * 8 == int(sti["sum_beta"] * 8) and sti["sum_delta2"] * 64 == int(sti["sum_delta2"] * 64)


# ================================================================ the tasks
@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config):
    from siss_amd import hydra_lite as H

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    assert task([]).ssd_config() is None and task(["+deletion.ssd=null"]).ssd_config() is None
    task([]).check_supported()
    t = task(["+deletion.ssd={alpha:null,fraction:0.01,lambda:1,keep_batches:64,forget_batches:64,batch_size:1,seed:0,targets:null,path:null}"])
    assert t.ssd_config().as_dict() == {"alpha": None, "fraction": 0.01, "lambda": 1.0, "keep_batches": 64, "forget_batches": 64,
                                        "batch_size": 1, "seed": 0, "targets": None, "path": None}
    t.check_supported()
    task(["+deletion.ssd={alpha:10,targets:[conv_in]}"]).check_supported()
    for ov, word in (("10", "mapping"), ("{fraction:0.1,rank:4}", "rank"), ("{lambda:1}", "exactly one"), ("{alpha:1,fraction:0.1}", "exactly one"),
                     ("{alpha:-1}", "alpha"), ("{fraction:1.5}", "fraction"), ("{fraction:0.1,lambda:0}", "lambda"),
                     ("{fraction:0.1,keep_batches:0}", "keep_batches"), ("{fraction:0.1,forget_batches:0}", "forget_batches"),
                     ("{fraction:0.1,batch_size:0}", "batch_size"), ("{fraction:0.1,targets:attn}", "targets"),
                     ("{fraction:0.1,targets:[no_such_parameter_anywhere]}", "matches no parameter")):
        with pytest.raises(ValueError, match="deletion.ssd") as e:
            task(["+deletion.ssd=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    # refused with the two keys that freeze weight gradients, before any device work (check_supported touches no device)
    for other, name in (("+deletion.trainable=[attn]", "deletion.trainable"), ("+deletion.lora={rank:4,targets:[attn]}", "deletion.lora")):
        with pytest.raises(ValueError, match=name) as e:
            task(["+deletion.ssd=" + KEYED, other]).check_supported()
        assert "deletion.ssd.targets" in str(e.value)
    # ... and it combines with the mask and with the anchor
    task(["+deletion.ssd=" + KEYED, "+deletion.saliency={fraction:0.5}"]).check_supported()
    task(["+deletion.ssd=" + KEYED, "+deletion.ewc={strength:10}"]).check_supported()


def test_the_yamls_lack_the_key_and_the_pretraining_task_refuses_it():
    from siss_amd import hydra_lite as H
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "ssd" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "ssd" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.ssd={fraction:0.01}"])
    with pytest.raises(NotImplementedError, match="deletion.ssd"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [])
    H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


def test_ssd_is_no_update_variant():
    from siss_amd import variants
    assert "ssd" not in variants.VARIANTS and "ssd" not in variants.ALIASES.values()


# ================================================================ the library's surface
def test_the_entry_points_are_declared():
    from siss_amd import lib
    from siss_amd.ssd import ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert lib.has(name) and name in lib.SIGNATURES, name
    for name in ("siss_ssd_ratio", "siss_ssd_dampen"):
        assert lib.PARAMS[name][-1] == "stream" and name in lib.F32_SAME
    assert lib.PARAMS["siss_ssd_partials_words"] == () and lib.RESTYPE["siss_ssd_partials_words"] is lib.L
    assert lib.PARAMS["siss_ssd_ratio"] == ("f_keep", "f_forget", "ratio", "n", "stream")
    assert lib.PARAMS["siss_ssd_dampen"] == ("p", "ratio", "n", "threshold", "strict", "lambda", "apply", "partials", "stats", "stream")
    assert lib.query("siss_ssd_partials_words") == 8 * 2048


def test_the_argument_checks_refuse_before_any_launch():
    """Status 1 comes from the host-side checks alone (no device is touched): null, misaligned and overlapping pointers, n <= 0, a
    lambda that is not finite or not positive, a threshold that is NaN or negative."""
    import ctypes as C
    from siss_amd import lib
    L = lib.load()
    A = 1 << 20                                              # (addresses are only compared, never dereferenced)
    n = 1027
    ok_ratio = (A, A + (1 << 16), A + (2 << 16), n)
    rows = [(0, ok_ratio[1], ok_ratio[2], n), (A, 0, ok_ratio[2], n), (A, ok_ratio[1], 0, n), (A + 4, *ok_ratio[1:]), (A, ok_ratio[1] + 8, *ok_ratio[2:]),
            (A, ok_ratio[1], ok_ratio[2] + 4, n), (A, ok_ratio[1], ok_ratio[2], 0), (A, ok_ratio[1], ok_ratio[2], -5),
            (A, ok_ratio[1], A, n), (A, ok_ratio[1], ok_ratio[1], n), (A, ok_ratio[1], A + 16, n), (A + 4096, ok_ratio[1], A, n)]
    for a in rows:
        assert L.siss_ssd_ratio(C.c_void_p(a[0]), C.c_void_p(a[1]), C.c_void_p(a[2]), a[3], None) == 1, a
    nan, inf = float("nan"), float("inf")
    good = dict(p=A, ratio=A + (1 << 16), n=n, threshold=1.0, strict=1, lam=1.0, apply=0, partials=A + (2 << 16), stats=A + (3 << 16))
    bad = [dict(p=0), dict(ratio=0), dict(partials=0), dict(stats=0), dict(p=A + 4), dict(ratio=good["ratio"] + 8), dict(n=0), dict(n=-1),
           dict(lam=0.0), dict(lam=-1.0), dict(lam=nan), dict(lam=inf), dict(threshold=nan), dict(threshold=-1.0), dict(threshold=-inf)]
    for change in bad:
        a = dict(good, **change)
        rc = L.siss_ssd_dampen(C.c_void_p(a["p"]), C.c_void_p(a["ratio"]), a["n"], a["threshold"], a["strict"], a["lam"], a["apply"],
                               C.c_void_p(a["partials"]), C.c_void_p(a["stats"]), None)
        assert rc == 1, change


def test_fisher_anchor_runs_the_shared_loop(monkeypatch):
    """FisherAnchor.from_batches and Importances.from_batches both go through variants.fisher_of_batches: one statement of zero /
    backward_batch(first=True) / siss_fisher_accumulate."""
    import inspect
    from siss_amd import ewc, ssd, variants
    src = inspect.getsource(variants.fisher_of_batches)
    assert "backward_batch(" in src and "first=True" in src and '"siss_fisher_accumulate"' in src and "quiet_backward(" in src
    for mod, fn in ((ewc, ewc.FisherAnchor.from_batches), (ssd, ssd.Importances.from_batches)):
        body = inspect.getsource(fn)
        assert "fisher_of_batches(" in body and "siss_fisher_accumulate\"" not in body and "backward_batch(" not in body, mod.__name__

"""siss_amd/uce.py and the restatement tests/uce_ref.py without a GPU:

* parse_uce: the defaults, the round trip, every refusal by the entry it names; targets match as deletion.trainable matches;
* the tasks: only delete_sd takes the key (delete_celeb, delete_tshirt and the pre-training task say "no cross-attention"), it is refused
  with deletion.lora, combines with the rest, is absent from the four YAMLs and is no row of variants.VARIANTS; the refused knobs of
  tests/test_host_logic.py stay refused beside it;
* the entry points are declared in the header, and their argument checks refuse before any launch (host job table, fake addresses);
* the method in f64 at X = 64, 2 edit prompts x 5 rows, 3 preserved prompts x 5 rows (25 rows < X), lambda in {0.1, 1}: the
  rearranged form W + W dT equals UCE's own form within 64 * cond(M) * 2^-52 relative (a backward-stability bound: both sides solve
  against the same M, each with a relative error of a modest multiple of cond(M) * 2^-53; 64 = X bounds the growth of a Frobenius norm
  over the rows -- not a measured figure); a vector orthogonal to all rows is mapped as before to the same bound; C_t = C_e gives
  E = 0 exactly; the edit residual shrinks strictly; on the f64 oracle UNet the edited output at the prompt moves towards the
  original's output at the destination;
* uce_ref.chain is sscd_search_ref.chain_sims on this file's data (module docstring of uce_ref); the files round trip and a foreign X
  is refused by field.

The edit residuals of the fixture below (seed 5; before the edit -> after it): lambda 0.1: 1.448 -> 3.314e-3, preserve drift 1.19e-3;
lambda 1: 1.448 -> 3.207e-2, preserve drift 1.12e-2 (printed by test_edit_residual_shrinks; a run files the same quantities under
"residuals" in its `uce.json`).
"""
import json
import os

import numpy as np
import pytest

import uce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
X, L = 64, 5
LAMBDAS = [0.1, 1.0]
KEYED = "{edit:[{prompt:a photo of a thing,target:null}],preserve:[a photo of a dog]}"


def fixture(seed=5):
    """(C_e [10, X], C_t [10, X], C_p [15, X], W [48, X]) f64: 2 edit prompts x 5 rows, 3 preserved prompts x 5 rows"""
    g = np.random.default_rng(seed)
    return g.standard_normal((2 * L, X)), g.standard_normal((2 * L, X)), g.standard_normal((3 * L, X)), g.standard_normal((48, X)) / 8


# ================================================================ the parsed key
def test_parse_uce_defaults_and_round_trip():
    from siss_amd.uce import DEFAULT_TARGETS, FIELDS, KEY, parse_uce
    assert KEY == "deletion.uce" and parse_uce(None) is None
    c = parse_uce(dict(edit=[dict(prompt="a cat", target=None)]))
    assert c.as_dict() == {"edit": [{"prompt": "a cat", "target": None}], "preserve": [], "preserve_file": None, "lambda": 0.1,
                           "edit_scale": 1.0, "preserve_scale": 1.0, "targets": DEFAULT_TARGETS, "path": None}
    assert set(c.as_dict()) == set(FIELDS) and DEFAULT_TARGETS == [r"attn2\.to_[kv]\.weight"]
    assert parse_uce(dict(edit=[dict(prompt="a cat")])).edit == [("a cat", None)]            # target left out: the empty prompt
    full = {"edit": [{"prompt": "a cat", "target": "a dog"}, {"prompt": "Van Gogh", "target": None}], "preserve": ["a tree", "a house"],
            "preserve_file": "/somewhere/keep.txt", "lambda": 1.0, "edit_scale": 2.0, "preserve_scale": 0.5,
            "targets": [r"attn2\.to_v\.weight"], "path": "/somewhere"}
    c = parse_uce(full)
    assert c.as_dict() == full and parse_uce(c.as_dict()).as_dict() == full
    assert isinstance(parse_uce(dict(full, **{"lambda": 1})).lam, float)


def test_parse_uce_refusals_name_the_entry():
    from siss_amd.uce import parse_uce
    ok = dict(edit=[dict(prompt="a cat", target=None)])
    nan, inf = float("nan"), float("inf")
    rows = [(3, "mapping"), (["a cat"], "mapping"), ("a cat", "mapping"), (dict(ok, edits=2), "edits"), (dict(ok, rank=4), "rank"),
            ({}, "edit"), (dict(edit=None), "edit"), (dict(edit=[]), "edit"), (dict(edit="a cat"), "edit"),
            (dict(edit=["a cat"]), "edit[0]"), (dict(edit=[dict(target="x")]), "edit[0]"), (dict(edit=[dict(prompt="a", to="b")]), "edit[0]"),
            (dict(edit=[dict(prompt="a"), dict(prompt="")]), "edit[1].prompt"), (dict(edit=[dict(prompt=3)]), "edit[0].prompt"),
            (dict(edit=[dict(prompt="a", target=4)]), "edit[0].target"), (dict(edit=[dict(prompt="a", target="")]), "edit[0].target"),
            (dict(ok, preserve="a dog"), "preserve"), (dict(ok, preserve=[3]), "preserve[0]"), (dict(ok, preserve=["a", ""]), "preserve[1]"),
            (dict(ok, preserve_file=3), "preserve_file"), (dict(ok, path=3), "path"),
            ({**ok, "lambda": 0}, "lambda"), ({**ok, "lambda": -1.0}, "lambda"), ({**ok, "lambda": nan}, "lambda"),
            ({**ok, "lambda": inf}, "lambda"), ({**ok, "lambda": "1"}, "lambda"), ({**ok, "lambda": True}, "lambda"),
            (dict(ok, edit_scale=0), "edit_scale"), (dict(ok, edit_scale=nan), "edit_scale"), (dict(ok, edit_scale="1"), "edit_scale"),
            (dict(ok, preserve_scale=-2), "preserve_scale"), (dict(ok, preserve_scale=inf), "preserve_scale"),
            (dict(ok, targets="attn2"), "targets"), (dict(ok, targets=[]), "targets"), (dict(ok, targets=[3]), "targets"),
            (dict(ok, targets=["("]), "targets")]
    for bad, word in rows:
        with pytest.raises(ValueError, match="deletion.uce") as e:
            parse_uce(bad)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError, match="deletion.lora") as e:
        parse_uce(ok, lora=dict(rank=4))
    assert "deletion.uce" in str(e.value) and "base copy" in str(e.value) and "before the edit" in str(e.value)


def test_preserve_file_holds_one_prompt_per_line(tmp_path):
    from siss_amd.uce import parse_uce
    f = tmp_path / "keep.txt"
    f.write_text("a tree\n\n  a house  \n")
    c = parse_uce(dict(edit=[dict(prompt="a cat")], preserve=["a dog"], preserve_file=str(f)))
    assert c.preserved_prompts() == ["a dog", "a tree", "a house"]
    with pytest.raises(FileNotFoundError, match="deletion.uce.preserve_file"):
        parse_uce(dict(edit=[dict(prompt="a cat")], preserve_file=str(tmp_path / "none.txt"))).preserved_prompts()


def test_targets_match_as_the_trainable_subset_does_and_must_be_matrices_over_the_text():
    from types import SimpleNamespace as NS
    from siss_amd.uce import check_targets, parse_uce, select_targets
    names = ["conv_in.weight", "mid.attn2.to_q.weight", "mid.attn2.to_k.weight", "mid.attn2.to_v.weight", "mid.attn1.to_k.weight"]
    pats = parse_uce(dict(edit=[dict(prompt="a")])).targets
    assert select_targets(names, pats) == names[2:4]
    assert select_targets(names, parse_uce(dict(edit=[dict(prompt="a")], targets=["."])).targets) == names
    with pytest.raises(ValueError, match=r"deletion.uce.targets.*matches no parameter"):
        select_targets(names, parse_uce(dict(edit=[dict(prompt="a")], targets=["attn2", "nothing_like_it"])).targets)
    specs = {"mid.attn2.to_k.weight": NS(kind="mat", native_shape=(128, 64)), "mid.attn1.to_k.weight": NS(kind="mat", native_shape=(128, 128)),
             "conv_in.weight": NS(kind="conv_in", native_shape=(64, 64)), "b": NS(kind="vec", native_shape=(64,))}
    assert check_targets(specs, ["mid.attn2.to_k.weight"], 64) == ["mid.attn2.to_k.weight"]
    for bad in ("mid.attn1.to_k.weight", "conv_in.weight", "b"):
        with pytest.raises(ValueError, match="deletion.uce.*not a matrix") as e:
            check_targets(specs, [bad], 64)
        assert bad in str(e.value)
    with pytest.raises(KeyError, match="nope"):
        check_targets(specs, ["nope"], 64)


# ================================================================ the tasks
def task(config, ov):
    from siss_amd import hydra_lite as H
    cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


def test_delete_sd_reads_the_key_and_settles_its_refusals_in_check_supported(tmp_path):
    syn = "allow_synthetic=true"
    assert task("delete_sd", []).uce_config() is None and task("delete_sd", ["+deletion.uce=null"]).uce_config() is None
    task("delete_sd", []).check_supported()
    t = task("delete_sd", ["+deletion.uce=" + KEYED, syn])
    assert t.uce_config().as_dict()["edit"] == [{"prompt": "a photo of a thing", "target": None}]
    t.check_supported()
    for ov, word in (("10", "mapping"), ("{edit:[{prompt:a}],rank:4}", "rank"), ("{preserve:[a]}", "edit"), ("{edit:[]}", "edit"),
                     ("{edit:[{prompt:a}],lambda:0}", "lambda"), ("{edit:[{prompt:a}],edit_scale:-1}", "edit_scale"),
                     ("{edit:[{prompt:a}],targets:attn2}", "targets"), ("{edit:[{prompt:a}],targets:[no_such_parameter_anywhere]}", "matches no parameter"),
                     ("{edit:[{prompt:a}],targets:[attn1.to_k.weight]}", "not a matrix"), ("{edit:[{prompt:a}],targets:[conv_in.weight]}", "not a matrix")):
        with pytest.raises(ValueError, match="deletion.uce") as e:
            task("delete_sd", ["+deletion.uce=" + ov, syn]).check_supported()
        assert word in str(e.value), str(e.value)
    # a prompt that cannot be embedded (no text encoder on disk, no allow_synthetic) is named
    for ov, word in (("{edit:[{prompt:a cat,target:a dog}]}", "edit[0].prompt"), ("{edit:[{prompt:a cat}],preserve:[a dog]}", "edit[0].prompt")):
        with pytest.raises(FileNotFoundError, match="deletion.uce") as e:
            task("delete_sd", ["+deletion.uce=" + ov, "pretrained_model_name_or_path=/nonexistent"]).check_supported()
        assert word in str(e.value), str(e.value)
    # refused with deletion.lora before any device work; combines with everything else
    with pytest.raises(ValueError, match="deletion.lora") as e:
        task("delete_sd", ["+deletion.uce=" + KEYED, syn, "+deletion.lora={rank:4,targets:[attn2.to_q]}"]).check_supported()
    assert "deletion.uce" in str(e.value)
    for other in ("+deletion.trainable=[attn2]", "+deletion.saliency={fraction:0.5}", "+deletion.ewc={strength:10}",
                  "+deletion.ssd={fraction:0.01}", "+deletion.surgery={mode:forget}"):
        task("delete_sd", ["+deletion.uce=" + KEYED, syn, other]).check_supported()
    task("delete_sd", ["+deletion.uce=" + KEYED, syn, "deletion.loss_fn=teacher_target", "+deletion.teacher={forget:esd,keep:teacher}"]).check_supported()
    # the knobs tests/test_host_logic.py pins stay refused beside the key
    for knob in ("snr_gamma=5.0", "input_perturbation=0.1", "prediction_type=v_prediction", "use_8bit_adam=true"):
        with pytest.raises(NotImplementedError, match=knob.split("=")[0]):
            task("delete_sd", ["+deletion.uce=" + KEYED, syn, knob]).check_supported()


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "train_tshirt_mnist"])
def test_the_tasks_without_cross_attention_refuse_the_key(config):
    task(config, []).check_supported()
    with pytest.raises(NotImplementedError, match="deletion.uce") as e:
        task(config, ["+deletion.uce=" + KEYED]).check_supported()
    assert "no cross-attention" in str(e.value)


def test_the_yamls_lack_the_key_and_uce_is_no_update_variant():
    from siss_amd import hydra_lite as H
    from siss_amd import variants
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "uce" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "uce" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    assert "uce" not in variants.VARIANTS and "uce" not in variants.ALIASES.values() and "uce" not in variants.ALIASES


# ================================================================ the library's surface
def test_the_entry_points_are_declared():
    from siss_amd import lib
    from siss_amd.uce import ENTRY_POINTS
    header = open(lib.HEADER).read()
    for name in ENTRY_POINTS:
        assert lib.has(name) and name in lib.SIGNATURES and f" {name}(" in header, name
    for name in ("siss_uce_delta", "siss_uce_apply"):
        assert lib.PARAMS[name][-1] == "stream" and name in lib.F32_SAME
    assert lib.PARAMS["siss_uce_delta"] == ("p", "jobs", "njobs", "E", "X", "delta", "stream")
    assert lib.PARAMS["siss_uce_apply"] == ("p", "jobs", "njobs", "X", "delta", "apply", "partials", "stats", "stream")
    assert lib.PARAMS["siss_uce_partials_words"] == ("floats", "njobs") and lib.RESTYPE["siss_uce_partials_words"] is lib.L
    for floats, njobs, jobs in ((4096, 1, [(0, 0, 64)]), (3 * 4100, 3, [(0, 0, 64), (8192, 64, 65), (16384, 129, 1)])):
        assert lib.query("siss_uce_partials_words", floats, njobs) == 4 * (floats // 4096 + njobs) >= 4 * R.chunks(jobs, 64)
    assert "uce.hip" in open(os.path.join(ROOT, "siss_amd", "build.py")).read().split("EXACT = {")[1].split("}")[0]


def test_the_argument_checks_refuse_before_any_launch():
    """Status 1 comes from the host-side checks alone (no device is touched; the job table is a HOST array, the other addresses are
    only compared, never dereferenced): null and misaligned pointers, X % 4 != 0, njobs <= 0, a job with rows <= 0 or a bad offset, two
    jobs sharing rows of delta, delta or E overlapping a target's floats."""
    import ctypes as C
    from siss_amd import lib
    Lb = lib.load()
    A = 1 << 24
    Xd = 64
    P, E, Dl, PT, ST = A, A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (4 << 20)
    good_jobs = [(0, 0, 33), (4096, 33, 16)]

    def table(jobs):
        b = R.job_bytes(jobs)
        return (C.c_char * len(b)).from_buffer_copy(b)

    def delta(p=P, jobs=good_jobs, njobs=None, e=E, x=Xd, d=Dl):
        t = table(jobs) if jobs is not None else None
        return Lb.siss_uce_delta(C.c_void_p(p), t, len(jobs) if njobs is None else njobs, C.c_void_p(e), x, C.c_void_p(d), None)

    def apply(p=P, jobs=good_jobs, njobs=None, x=Xd, d=Dl, pt=PT, st=ST):
        t = table(jobs) if jobs is not None else None
        return Lb.siss_uce_apply(C.c_void_p(p), t, len(jobs) if njobs is None else njobs, x, C.c_void_p(d), 0, C.c_void_p(pt), C.c_void_p(st), None)
    floats = 4096 + 16 * Xd                                  # the targets' extent of p
    bad_tables = [[(0, 0, 0)], [(0, 0, -3)], [(0, 0, 33), (4096, 33, 0)], [(2, 0, 33)], [(-64, 0, 33)], [(0, -1, 33)],
                  [(0, 0, 33), (4096, 32, 16)], [(0, 0, 33), (4096, 0, 16)]]
    for fn, extra in ((delta, [dict(e=0), dict(e=E + 4), dict(e=P), dict(e=P + 4 * (floats - 16)), dict(e=P - 4 * Xd * Xd + 16),
                               dict(e=Dl), dict(e=Dl + 4 * 48 * Xd)]),
                      (apply, [dict(pt=0), dict(st=0), dict(pt=PT + 4), dict(st=ST + 4)])):
        bad = [dict(p=0), dict(d=0), dict(p=P + 4), dict(d=Dl + 8), dict(x=0), dict(x=-4), dict(x=66), dict(x=63), dict(njobs=0),
               dict(njobs=-1), dict(d=P), dict(d=P + 4 * (floats - 16)), dict(d=P - 4 * 49 * Xd + 16)] + [dict(jobs=t) for t in bad_tables] + extra
        for change in bad:
            assert fn(**change) == 1, (fn.__name__, change)
    assert Lb.siss_uce_delta(C.c_void_p(P), None, 2, C.c_void_p(E), Xd, C.c_void_p(Dl), None) == 1
    assert Lb.siss_uce_apply(C.c_void_p(P), None, 2, Xd, C.c_void_p(Dl), 0, C.c_void_p(PT), C.c_void_p(ST), None) == 1


# ================================================================ the method, in f64
def test_edit_matrix_is_the_restatement_and_refuses_what_it_cannot_use():
    from siss_amd.uce import edit_matrix
    Ce, Ct, Cp, W = fixture()
    for lam in LAMBDAS:
        ed = edit_matrix(Ce, Ct, Cp, lam, 1.0, 1.0)
        E, M, D, dT = R.edit_matrix(Ce, Ct, Cp, lam)
        assert ed.E.dtype == f32 and ed.E.shape == (X, X) and ed.M.dtype == f64 and ed.D.dtype == f64 and ed.E.flags["C_CONTIGUOUS"]
        assert np.allclose(ed.M, M, rtol=1e-14, atol=0) and np.allclose(ed.D, D, rtol=1e-14, atol=1e-14)
        cond = np.linalg.cond(M)
        assert abs(ed.cond - cond) <= 1e-9 * cond and (ed.n_edit, ed.n_preserve, ed.X) == (10, 15, X)
        # Cholesky solve against numpy's LU solve: both backward stable, cond(M) * 2^-52 * X relative in the Frobenius norm
        assert np.linalg.norm(ed.E.astype(f64) - dT.T) <= (X * cond * 2.0 ** -52 + 2.0 ** -24) * np.linalg.norm(dT)
    import torch
    ed_t = edit_matrix(torch.from_numpy(Ce).reshape(2, L, X), torch.from_numpy(Ct).reshape(2, L, X), None, 0.1)
    assert np.array_equal(ed_t.E, edit_matrix(Ce, Ct, np.zeros((0, X)), 0.1).E) and ed_t.n_preserve == 0
    bad = Ce.copy()
    bad[3, 7] = np.nan
    for args, word in (((bad, Ct, Cp, 0.1), "C_e"), ((Ce, bad, Cp, 0.1), "C_t"), ((Ce, Ct, bad, 0.1), "C_p")):
        with pytest.raises(ValueError, match="non-finite") as e:
            edit_matrix(*args)
        assert word in str(e.value)
    bad[3, 7] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        edit_matrix(bad, Ct, Cp, 0.1)
    for lam in (0, -0.1, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="lambda"):
            edit_matrix(Ce, Ct, Cp, lam)
    with pytest.raises(ValueError, match="edit_scale"):
        edit_matrix(Ce, Ct, Cp, 0.1, 0.0)
    with pytest.raises(ValueError, match="preserve_scale"):
        edit_matrix(Ce, Ct, Cp, 0.1, 1.0, -1.0)
    for Ct_bad in (Ct[:-1], Ct[:, :-4], np.concatenate([Ct, Ct])):
        with pytest.raises(ValueError, match="C_t"):
            edit_matrix(Ce, Ct_bad, Cp, 0.1)
    with pytest.raises(ValueError, match="C_p"):
        edit_matrix(Ce, Ct, Cp[:, :-4], 0.1)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("scales", [(1.0, 1.0), (2.0, 0.5)])
def test_rearranged_form_equals_uces_own_form_within_the_stability_bound(lam, scales):
    Ce, Ct, Cp, W = fixture()
    s_e, s_p = scales
    E, M, D, dT = R.edit_matrix(Ce, Ct, Cp, lam, s_e, s_p)
    bound = 64 * np.linalg.cond(M) * 2.0 ** -52
    ours, theirs = W + W @ dT, R.uce_form(W, Ce, Ct, Cp, lam, s_e, s_p)
    rel = np.linalg.norm(ours - theirs) / np.linalg.norm(theirs)
    print(f"\n[uce] lambda {lam}, scales {scales}: cond(M) {np.linalg.cond(M):.4g}, |rearranged - UCE's form| / |UCE's form| {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound
    assert np.linalg.norm(ours - W) > 1e-3 * np.linalg.norm(W), "the edit is too small to tell the two forms from the identity"
    # a vector orthogonal to every row (edited and preserved) is mapped as before: D v = 0 and M v = lambda v, so dT v = 0
    g = np.random.default_rng(11)
    v = g.standard_normal(X)
    Q, _ = np.linalg.qr(np.concatenate([Ce, Cp]).T)
    v -= Q @ (Q.T @ v)
    v -= Q @ (Q.T @ v)
    assert np.abs(np.concatenate([Ce, Cp]) @ v).max() <= 1e-13 * np.linalg.norm(v)
    for Wn in (ours, theirs):
        assert np.linalg.norm(Wn @ v - W @ v) <= bound * np.linalg.norm(W) * np.linalg.norm(v)
    # ... and the package's E (f32) agrees with dT to its one rounding
    from siss_amd.uce import edit_matrix
    ed = edit_matrix(Ce, Ct, Cp, lam, s_e, s_p)
    assert np.abs(ed.E.astype(f64) - dT.T).max() <= 2.0 ** -24 * np.abs(dT).max() + bound * np.linalg.norm(dT)


def test_equal_destinations_give_a_zero_edit_exactly():
    from siss_amd.uce import edit_matrix
    Ce, Ct, Cp, W = fixture()
    for lam in LAMBDAS:
        ed = edit_matrix(Ce, Ce.copy(), Cp, lam)
        assert not ed.D.any() and not ed.E.any()
        assert np.array_equal(R.edit_matrix(Ce, Ce, Cp, lam)[0], np.zeros((X, X), f32))


@pytest.mark.parametrize("lam", LAMBDAS)
def test_edit_residual_shrinks(lam):
    from siss_amd import uce
    Ce, Ct, Cp, W = fixture()
    names = ["a.attn2.to_k.weight", "a.attn2.to_v.weight"]
    Ws = {names[0]: W, names[1]: W[::-1] * 0.5}
    ed = uce.edit_matrix(Ce, Ct, Cp, lam)
    before = uce.values_before(Ws, names, Ct, Cp)
    r0 = uce.residuals(Ws, names, before, Ce, Cp)
    after = {n: w + w @ ed.E.astype(f64).T for n, w in Ws.items()}
    r1 = uce.residuals(after, names, before, Ce, Cp)
    print(f"\n[uce] lambda {lam}: edit residual {r0['edit_residual']:.5g} -> {r1['edit_residual']:.4g}, preserve drift {r1['preserve_drift']:.3g}")
    assert r0["preserve_drift"] == 0.0 and 0 < r1["edit_residual"] < r0["edit_residual"]
    for n in names:
        assert 0 < r1["per_tensor"][n]["edit_residual"] < r0["per_tensor"][n]["edit_residual"]
        assert 0 < r1["per_tensor"][n]["preserve_drift"] < r1["per_tensor"][n]["edit_residual"] + 1
    e_ref, p_ref = R.residuals([after[n] for n in names], [Ws[n] for n in names], Ce, Ct, Cp)
    assert abs(r1["edit_residual"] - e_ref) <= 1e-12 and abs(r1["preserve_drift"] - p_ref) <= 1e-12
    assert r1["edit_residual"] < 0.1 and r1["preserve_drift"] < 0.1, "25 rows in 64 dimensions: the edit should nearly reach its destination"


def test_edited_oracle_unet_moves_towards_the_destinations_output():
    import torch
    from oracle.unet_cond import OracleUNet2DCondition, UNetCondConfig
    from siss_amd import uce
    torch.manual_seed(0)
    oc = UNetCondConfig.tiny(ch=(32, 64), heads=2, cross_dim=X, sample_size=8, in_channels=4)
    oc.layers_per_block = 1
    net = OracleUNet2DCondition(oc).double()
    g = torch.Generator().manual_seed(2)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    names = [n for n in sd0 if n.endswith("attn2.to_k.weight") or n.endswith("attn2.to_v.weight")]
    assert names and all(sd0[n].shape[1] == X for n in names)
    c, cstar, keep = torch.randn(1, L, X, generator=g).double(), torch.randn(1, L, X, generator=g).double(), torch.randn(3, L, X, generator=g).double()
    ed = uce.edit_matrix(c, cstar, keep, 0.1)
    x, t = torch.randn(1, 4, 8, 8, generator=g).double(), torch.tensor([500])
    with torch.no_grad():
        out_c, out_star = net(x, t, c)[0], net(x, t, cstar)[0]
        out_keep = net(x, t, keep[:1])[0]
        E = torch.from_numpy(ed.E).double()
        net.load_state_dict({k: (v + v @ E.T if k in names else v) for k, v in sd0.items()})
        new_c, new_keep = net(x, t, c)[0], net(x, t, keep[:1])[0]
    d0, d1 = float((out_c - out_star).norm()), float((new_c - out_star).norm())
    print(f"\n[uce] oracle UNet: |out(c) - out(c*)| {d0:.4g} -> |out'(c) - out(c*)| {d1:.4g}; a preserved prompt moved by {float((new_keep - out_keep).norm()):.3g}")
    assert d0 > 0 and d1 < d0
    assert float((new_keep - out_keep).norm()) < d0


# ================================================================ the restatement and the files
def test_chain_is_chain_sims_on_this_data_and_resolves_the_tie_it_cannot():
    g = np.random.default_rng(3)
    q, e = g.standard_normal((7, 20)).astype(f32), g.standard_normal((20, 20)).astype(f32)
    assert np.array_equal(R.chain(q, e).view(np.uint32), R.chain_sims(q, e).view(np.uint32))
    # s = 1 + 2^-23 after two steps, then a product of 2^-24 - 2^-70: ONE rounding stays below the midpoint of 1 + 2^-23 and 1 + 2^-22
    # and gives 1 + 2^-23; the f64 sum lands ON the midpoint and rounds to even, 1 + 2^-22
    u = 2.0 ** -23
    qq = np.array([[1.0, 2.0 ** -12, (1 + u) * 2.0 ** -12]], f32)
    ee = np.array([[1.0, 2.0 ** -11, (1 - u) * 2.0 ** -12]], f32)
    assert float(qq[0, 2]) * float(ee[0, 2]) == 2.0 ** -24 * (1 - u * u) and float(qq[0, 1]) * float(ee[0, 1]) == u
    assert R.chain(qq, ee)[0, 0] == f32(1 + u) and R.chain_sims(qq, ee)[0, 0] == f32(1 + 2 * u)
    assert R.chain(qq, -ee)[0, 0] == -f32(1 + u)
    # apply_ref and the statistics on small integers are exact
    p = np.arange(-64, 192, dtype=f32)
    jobs = [(0, 1, 2), (128, 0, 1)]
    d = np.arange(3 * 4, dtype=f32)
    qn = R.apply_ref(p, jobs, d, 4)
    assert np.array_equal(qn[:8], p[:8] + d[4:12]) and np.array_equal(qn[128:132], p[128:132] + d[:4]) and np.array_equal(qn[8:128], p[8:128])
    st = R.stats_f64(p, jobs, d, 4)
    assert st == dict(sum_delta2=float((d.astype(f64) ** 2).sum()), sum_p2=float((p[:8].astype(f64) ** 2).sum() + (p[128:132].astype(f64) ** 2).sum()),
                      max_delta=11.0, floats=12)


def test_files_round_trip_and_a_foreign_x_is_refused_by_field(tmp_path):
    from siss_amd import uce
    Ce, Ct, Cp, W = fixture()
    ed = uce.edit_matrix(Ce, Ct, Cp, 0.1, 2.0, 0.5)
    assert not uce.present(str(tmp_path))
    uce.save(str(tmp_path), ed, dict(config={"lambda": 0.1}, stats={"floats": 12}, residuals={"edit_residual": 0.5, "per_tensor": {}}))
    assert uce.present(str(tmp_path)) and sorted(os.listdir(tmp_path)) == [uce.CONFIG_FILE, uce.EDIT_FILE]
    c = json.load(open(tmp_path / uce.CONFIG_FILE))
    assert (c["X"], c["edit_rows"], c["preserve_rows"], c["lambda"], c["edit_scale"], c["preserve_scale"], c["source"]) == (X, 10, 15, 0.1, 2.0, 0.5, "computed")
    assert c["cond"] == ed.cond and c["stats"] == {"floats": 12} and c["residuals"]["edit_residual"] == 0.5
    assert c["embeddings"] == uce.embeddings_digest(X, Ce, Ct, Cp) != uce.embeddings_digest(X, Ce, Ct, Cp * 2)
    back = uce.load(str(tmp_path), X)
    for k in ("E", "M", "D"):
        a, b = getattr(back, k), getattr(ed, k)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert (back.source, back.cond, back.lam, back.n_edit, back.n_preserve, back.digest) == ("loaded", ed.cond, 0.1, 10, 15, ed.digest)
    with pytest.raises(ValueError, match=r"X = 64, this UNet's cross_attention_dim is 768"):
        uce.load(str(tmp_path), 768)

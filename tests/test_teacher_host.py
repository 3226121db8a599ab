"""The host side of the teacher-target objective (siss_amd/teacher.py, `deletion.loss_fn=teacher_target` + `deletion.teacher`), no GPU:

* parse_teacher: the documented mapping, its defaults, and every malformed one refused by name;
* the row layout of the two forwards for the six combinations of keep and forget, against tests/teacher_ref.py's own statement of it;
* the exclusivity messages: FlatAdamW.launch(fixed_weight=...) with ranges / mask / ewc / surgery / eta, launch_sharded, the stepper's
  loss_fn / teacher= pair and the four variants without a weighted pass 1;
* the three delete tasks and the pre-training task through main.main([...]) up to the point where a GPU is needed: delete_sd accepts
  the key (and reaches the loading of the UNet), the others refuse it with their reason, and every refusal of delete_sd is settled in
  check_supported; the key is absent from the YAMLs;
* the restatement against itself: on a two-layer toy network in f64 the autograd gradient of the restated objective equals the one
  formed from the restated cotangent (J^T cot), for every keep x forget combination;
* the entry points are declared in the header with the documented argument lists, and teacher.hip is built without contraction.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

import optimizer_ref as O
import teacher_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
COMBOS = [(k, f) for k in R.KEEPS for f in R.FORGETS]


# ================================================================ the parsed key
def test_parse_defaults_and_round_trip():
    from siss_amd.teacher import FIELDS, KEY, LOSS, parse_teacher
    assert KEY == "deletion.teacher" and LOSS == "teacher_target" and parse_teacher(None) is None
    d = parse_teacher({}).as_dict()
    assert d == dict(forget="esd", keep="noise", guidance=1.0, weight=1.0, anchor_prompt=None, path=None) and tuple(d) == FIELDS
    c = parse_teacher(dict(forget="anchor", keep="teacher", guidance=0, weight=2, anchor_prompt="a photo", path=None))
    assert c.as_dict() == dict(forget="anchor", keep="teacher", guidance=0.0, weight=2.0, anchor_prompt="a photo", path=None)
    assert parse_teacher(c.as_dict()).as_dict() == c.as_dict()
    for keep in ("noise", "teacher", "none"):
        assert parse_teacher(dict(forget="esd", keep=keep, guidance=2.5)).as_dict()["keep"] == keep
    # deletion.lora and deletion.ssd are not among the keys it refuses
    import inspect
    assert set(inspect.signature(parse_teacher).parameters) == {"value", "trainable", "saliency", "ewc", "surgery"}


def test_parse_refusals_name_the_entry():
    from siss_amd.teacher import parse_teacher
    rows = [(3, "mapping"), (["esd"], "mapping"), ("esd", "mapping"), (dict(forgot="esd"), "forgot"), (dict(forget="esd", rank=4), "rank"),
            (dict(forget="sd"), "forget"), (dict(forget=1), "forget"), (dict(keep="all"), "keep"), (dict(keep=True), "keep"),
            (dict(guidance=-0.5), "guidance"), (dict(guidance="1"), "guidance"), (dict(guidance=float("nan")), "guidance"),
            (dict(guidance=True), "guidance"), (dict(weight=0), "weight"), (dict(weight=-1.0), "weight"), (dict(weight=float("inf")), "weight"),
            (dict(weight="2"), "weight"), (dict(forget="anchor"), "anchor_prompt"), (dict(forget="anchor", anchor_prompt=""), "anchor_prompt"),
            (dict(forget="esd", anchor_prompt="a dog"), "anchor_prompt"), (dict(forget="anchor", anchor_prompt=3), "anchor_prompt"),
            (dict(path=3), "path")]
    for bad, word in rows:
        with pytest.raises(ValueError, match="deletion.teacher") as e:
            parse_teacher(bad)
        assert word in str(e.value), (bad, str(e.value))
    for kw, name in ((dict(trainable=["attn"]), "deletion.trainable"), (dict(saliency=dict(fraction=0.5)), "deletion.saliency"),
                     (dict(ewc=dict(strength=1.0)), "deletion.ewc"), (dict(surgery=dict(mode="mutual")), "deletion.surgery")):
        with pytest.raises(ValueError, match=name) as e:
            parse_teacher(dict(forget="esd"), **kw)
        assert "deletion.teacher" in str(e.value) and "no weighted form" in str(e.value)


def test_a_path_without_unet_is_refused(tmp_path):
    from siss_amd.teacher import check_path
    with pytest.raises(FileNotFoundError, match="deletion.teacher.path") as e:
        check_path(tmp_path)
    assert "unet/" in str(e.value)
    os.makedirs(tmp_path / "unet")
    open(tmp_path / "unet" / "config.json", "w").write("{}")
    with pytest.raises(FileNotFoundError, match="diffusion_pytorch_model.safetensors"):
        check_path(tmp_path)
    open(tmp_path / "unet" / "diffusion_pytorch_model.safetensors", "w").write("")
    assert check_path(tmp_path) == os.path.join(str(tmp_path), "unet")


# ================================================================ the rows
@pytest.mark.parametrize("keep,forget", COMBOS)
def test_row_layout(keep, forget):
    from siss_amd.teacher import row_layout
    B = 3
    lay = row_layout(keep, forget, B)
    student = ([] if keep == "none" else [("keep", "c", B)]) + [("forget", "c", B)]
    teacher = ([("keep", "c", B)] if keep == "teacher" else []) + [("forget", "c" if forget == "esd" else "anchor", B)] \
        + ([("forget", "empty", B)] if forget == "esd" else [])
    assert lay["student"] == student and lay["teacher"] == teacher
    R_, Rt, k, u = R.rows(keep, forget, B)
    assert (lay["R"], lay["Rt"], lay["k"], lay["u"]) == (R_, Rt, k, u)
    assert lay["R"] == sum(n for *_, n in student) and lay["Rt"] == sum(n for *_, n in teacher)
    # the restated targets read exactly those rows: a teacher output whose row r holds the value r
    teach = np.repeat(np.arange(Rt, dtype=f32)[:, None], 5, 1)
    y = R.targets(np.full((B, 5), -1, f32), teach, B, keep, forget, 0.0)       # eta = 0: the esd target is u
    want = ([] if keep == "none" else ([-1.0] * B if keep == "noise" else list(range(B)))) \
        + [float((u if forget == "esd" else k) + i) for i in range(B)]
    assert y[:, 0].tolist() == want
    with pytest.raises(ValueError):
        row_layout("all", forget, B)


# ================================================================ exclusivity
def test_fixed_weight_is_exclusive_with_the_passes_that_have_no_weighted_form():
    from siss_amd.optim import FlatAdamW
    opt = FlatAdamW.__new__(FlatAdamW)
    opt.p = torch.zeros(8)
    g = torch.zeros(2, 8)
    for kw, name in ((dict(ranges=(None, 1, 2)), "ranges="), (dict(mask=torch.zeros(1, dtype=torch.int32)), "mask="),
                     (dict(ewc=object()), "ewc="), (dict(surgery=object()), "surgery="), (dict(eta=0.1), "eta=")):
        with pytest.raises(ValueError, match="fixed_weight=") as e:
            opt.launch(g, fixed_weight=1.0, **kw)
        assert name in str(e.value) and "no weighted form" in str(e.value), str(e.value)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="fixed_weight"):
            opt.launch(g, fixed_weight=bad)
    with pytest.raises(NotImplementedError, match="fixed_weight=") as e:
        opt.launch_sharded(g[0], g[1], 0, 8, None, fixed_weight=1.0)
    assert "shard" in str(e.value)


def test_the_stepper_wants_the_loss_and_the_teacher_together():
    from siss_amd.step import TEACHER, SISSStepper
    assert TEACHER == "teacher_target"
    eng = types.SimpleNamespace()
    kw = dict(lr=1e-4, train_batch_size=2)
    with pytest.raises(ValueError, match="teacher=") as e:
        SISSStepper(eng, torch.ones(4), loss_fn="teacher_target", **kw)
    assert "teacher_target" in str(e.value)
    with pytest.raises(ValueError, match="teacher=") as e:
        SISSStepper(eng, torch.ones(4), loss_fn="double_forward_with_neg_del", teacher=object(), **kw)
    assert "double_forward_with_neg_del" in str(e.value) and "teacher_target" in str(e.value)
    with pytest.raises(ValueError, match="teacher_cfg="):
        SISSStepper(eng, torch.ones(4), teacher_cfg=object(), **kw)
    for name in ("trainable", "saliency", "ewc", "surgery"):
        with pytest.raises(ValueError, match=f"teacher=.*{name}=") as e:
            SISSStepper(eng, torch.ones(4), loss_fn="teacher_target", teacher=object(), **{name: object()}, **kw)
        assert "no weighted form" in str(e.value)


# ================================================================ the tasks, through main.main
class _NeedsGPU(Exception):
    pass


SD = ["--config-name=delete_sd", "pretrained_model_name_or_path=/nonexistent", "allow_random_init=true"]


def run_main(monkeypatch, tmp_path, argv):
    """main.main(argv) with the device selection a no-op and the loading of the UNet -- the first thing that needs a GPU, and what
    follows check_supported / check_metrics -- replaced by a marker."""
    sys.path.insert(0, ROOT)
    import main as entry
    from siss_amd import tasks
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)

    def load_unet(self, device):
        raise _NeedsGPU()
    for cls in (tasks.DeleteSD, tasks._DeleteBase):
        monkeypatch.setattr(cls, "load_unet", load_unet)
    entry.main([*argv, f"output_dir={tmp_path}/out"])


def test_delete_sd_accepts_the_key(monkeypatch, tmp_path):
    for key in ("{forget:esd,keep:teacher}", "{forget:esd,keep:none,guidance:2.5,weight:0.5}", "{forget:anchor,keep:noise,anchor_prompt:a photo}"):
        with pytest.raises(_NeedsGPU):
            run_main(monkeypatch, tmp_path, [*SD, "allow_synthetic=true", "deletion.loss_fn=teacher_target", "+deletion.teacher=" + key])
    # the teacher combines with deletion.lora and deletion.ssd
    with pytest.raises(_NeedsGPU):
        run_main(monkeypatch, tmp_path, [*SD, "allow_synthetic=true", "deletion.loss_fn=teacher_target", "+deletion.teacher={forget:esd}",
                                         "+deletion.lora={rank:4,targets:[attn1.to_q]}"])
    with pytest.raises(_NeedsGPU):                   # without the key: today's run
        run_main(monkeypatch, tmp_path, [*SD, "allow_synthetic=true"])


def test_delete_sd_settles_every_refusal_before_the_first_step(monkeypatch, tmp_path):
    T = "deletion.loss_fn=teacher_target"
    rows = [([T], ValueError, "deletion.teacher"),                                               # the loss name without the key
            (["+deletion.teacher={forget:esd}"], ValueError, "teacher_target"),                  # the key without the loss name
            ([T, "+deletion.teacher={forget:sd}"], ValueError, "forget"),
            ([T, "+deletion.teacher={forget:esd,rank:2}"], ValueError, "rank"),
            ([T, "+deletion.teacher={forget:anchor}"], ValueError, "anchor_prompt"),
            ([T, "+deletion.teacher={forget:esd,weight:0}"], ValueError, "weight"),
            ([T, "+deletion.teacher={forget:esd}", "+deletion.trainable=[attn]"], ValueError, "deletion.trainable"),
            ([T, "+deletion.teacher={forget:esd}", "+deletion.saliency={fraction:0.5}"], ValueError, "deletion.saliency"),
            ([T, "+deletion.teacher={forget:esd}", "+deletion.ewc={strength:1}"], ValueError, "deletion.ewc"),
            ([T, "+deletion.teacher={forget:esd}", "+deletion.surgery={mode:mutual}"], ValueError, "deletion.surgery"),
            ([T, "+deletion.teacher={forget:esd,path:" + str(tmp_path / "nowhere") + "}"], FileNotFoundError, "unet/")]
    for ov, exc, word in rows:
        with pytest.raises(exc, match="teacher") as e:
            run_main(monkeypatch, tmp_path, [*SD, "allow_synthetic=true", *ov])
        assert word in str(e.value), (ov, str(e.value))
    # prompts that cannot be embedded: no text_encoder/ on disk and no allow_synthetic
    with pytest.raises(FileNotFoundError, match="anchor_prompt") as e:
        run_main(monkeypatch, tmp_path, [*SD, T, "+deletion.teacher={forget:anchor,anchor_prompt:a photo}"])
    assert "allow_synthetic" in str(e.value)
    with pytest.raises(FileNotFoundError, match="empty prompt"):
        run_main(monkeypatch, tmp_path, [*SD, T, "+deletion.teacher={forget:esd}"])
    emb = tmp_path / "anchor.pt"
    torch.save(torch.zeros(1, 77, 768), emb)
    with pytest.raises(_NeedsGPU):                   # a .pt embedding on disk is embeddable without either
        run_main(monkeypatch, tmp_path, [*SD, T, "+deletion.teacher={forget:anchor,anchor_prompt:" + str(emb) + "}"])


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt"])
def test_the_pixel_space_tasks_refuse_the_key_with_their_reason(monkeypatch, tmp_path, config):
    base = ["--config-name=" + config, "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true"]
    for ov in (["+deletion.teacher={forget:esd}"], ["deletion.loss_fn=teacher_target"],
               ["deletion.loss_fn=teacher_target", "+deletion.teacher={forget:esd}"]):
        with pytest.raises(NotImplementedError, match="deletion.teacher") as e:
            run_main(monkeypatch, tmp_path, [*base, *ov])
        assert "defined through prompts" in str(e.value) and "delete_sd" in str(e.value)
    with pytest.raises(_NeedsGPU):
        run_main(monkeypatch, tmp_path, base)


def test_the_yamls_lack_the_key_and_the_pretraining_task_refuses_it():
    from siss_amd import hydra_lite as H
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "teacher" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "teacher" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.teacher={forget:esd}"])
    with pytest.raises(NotImplementedError, match="deletion.teacher"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"), [])
    assert H.instantiate(cfg.task, cfg=cfg, _recursive_=False).teacher_config() is None


def test_the_synthetic_anchor_is_an_embedding_of_its_own():
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"), ["allow_synthetic=true", "pretrained_model_name_or_path=/nonexistent"])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    prompt = task._prompt_embedding("a prompt", "cpu")
    anchor = task._prompt_embedding("an anchor", "cpu", synthetic_seed=2)
    empty = task._empty_prompt_embedding("cpu", "test")
    assert prompt.shape == anchor.shape == empty.shape == (1, 77, 768)
    assert not torch.equal(prompt, anchor) and not torch.equal(prompt, empty) and not torch.equal(anchor, empty)
    assert torch.equal(prompt, task._prompt_embedding("a prompt", "cpu")), "the prompt's synthetic embedding is today's"


# ================================================================ the restatement against itself
@pytest.mark.parametrize("keep,forget", COMBOS)
def test_autograd_of_the_objective_equals_the_cotangent_pulled_back(keep, forget):
    """f64, a two-layer toy network: grad L = J^T cot with cot = 2 / B * (pred - y) per row set, g = g_x + weight g_a."""
    B, shape, L, X = 3, (2, 3, 3), 5, 4
    chw = int(np.prod(shape))
    g = torch.Generator().manual_seed(3)
    student, teacher = R.ToyNet(chw, X, seed=1), R.ToyNet(chw, X, seed=2)
    for p in teacher.parameters():
        p.requires_grad_(False)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x_t, a_t, noise, cond, empty, anchor = rnd(B, *shape), rnd(B, *shape), rnd(B, *shape), rnd(B, L, X), rnd(1, L, X), rnd(1, L, X)
    t = torch.tensor([999, 400, 50])
    eta, weight = 2.5, 0.75
    params = list(student.parameters())
    args = (x_t, a_t, t, cond, noise)
    kw = dict(keep=keep, forget=forget, eta=eta, weight=weight, batch=B, empty=empty, anchor=anchor)
    total, lx, la = R.objective(student, teacher, *args, **kw)
    auto = torch.autograd.grad(total, params)
    # the same from the restated targets and cotangent: rows stacked as the kernel sees them
    with torch.no_grad():
        tk = lambda x, c: teacher(x, t, c)
        rows_t = ([tk(x_t, cond)] if keep == "teacher" else []) + [tk(a_t, cond if forget == "esd" else anchor.expand(B, L, X))] \
            + ([tk(a_t, empty.expand(B, L, X))] if forget == "esd" else [])
        teach = torch.cat(rows_t).flatten(1)
    Rn, Rt, k0, u0 = R.rows(keep, forget, B)
    assert teach.shape[0] == Rt
    kk = teach[k0:k0 + B]
    yf = teach[u0:u0 + B] - eta * (kk - teach[u0:u0 + B]) if forget == "esd" else kk
    pred_a = student(a_t, t, cond)
    cot_a = 2.0 / B * (pred_a - yf.view_as(pred_a)).detach()
    ga = torch.autograd.grad(pred_a, params, grad_outputs=cot_a)
    if keep == "none":
        gx = [torch.zeros_like(p) for p in params]
        assert float(lx) == 0.0
    else:
        yk = noise if keep == "noise" else teach[:B].view_as(noise)
        pred_x = student(x_t, t, cond)
        gx = torch.autograd.grad(pred_x, params, grad_outputs=2.0 / B * (pred_x - yk).detach())
        assert abs(float(lx) - float(((pred_x - yk) ** 2).sum() / B)) <= 1e-12 * float(lx)
    assert abs(float(la) - float(((pred_a - yf.view_as(pred_a)) ** 2).sum() / B)) <= 1e-12 * float(la)
    for a, x, f in zip(auto, gx, ga):
        want = x + weight * f
        assert float((a - want).abs().max()) <= 1e-12 * float(want.abs().max()), (keep, forget)
    # and gradient_pair splits the same total
    px, pa, _, _ = R.gradient_pair(student, params, teacher, *args, **kw)
    for a, x, f in zip(auto, px, pa):
        assert float((a - (x + weight * f)).abs().max()) <= 1e-12 * float(a.abs().max())
    # with eta = 0 the esd target is the unconditional prediction; the teacher takes no gradient
    assert all(p.grad is None for p in teacher.parameters())


def test_the_restated_kernel_arithmetic():
    """targets / cotangent / sums on values whose results are known: eta = 0 gives u bit for bit, integers give exact sums, the f32
    order of u - eta (k - u) is three roundings."""
    B, chw = 2, 7
    rng = np.random.default_rng(0)
    teach = rng.standard_normal((3 * B, chw)).astype(f32)
    noise = rng.standard_normal((B, chw)).astype(f32)
    pred = rng.standard_normal((2 * B, chw)).astype(f32)
    y0 = R.targets(noise, teach, B, "teacher", "esd", 0.0)
    assert np.array_equal(y0[B:].view(np.uint32), teach[2 * B:3 * B].view(np.uint32)) and np.array_equal(y0[:B], teach[:B])
    k, u, eta = teach[B:2 * B], teach[2 * B:], f32(2.5)
    y = R.targets(noise, teach, B, "teacher", "esd", 2.5)
    assert np.array_equal(y[B:], (u - (eta * (k - u)).astype(f32)).astype(f32))
    ip, it = rng.integers(-8, 9, (2 * B, chw)).astype(f32), rng.integers(-8, 9, (3 * B, chw)).astype(f32)
    cot, sums, yy = R.seed(ip, noise, it, B, "teacher", "esd", 1.0, 0.25)
    assert np.array_equal(sums, ((ip.astype(f64) - yy.astype(f64)) ** 2).sum(1)) and np.array_equal(cot, f32(0.5) * (ip - yy))
    assert R.partials_words(4, 1) == 4 and R.partials_words(4, 4096) == 4 and R.partials_words(3, 4097) == 6


def test_the_weighted_block_is_the_plain_block_with_the_scale_given():
    gx, ga = O.gauss_pair(1027, 1)
    hp = O.hyper(*O.HYPER["sd"])
    sums = O.norm_sums_f32(gx, ga)
    blk = R.weighted_scalars_f32(*sums, 0.75, 1.0, hp[1], hp[2], 4)
    plain = O.scalars_f32(*sums, 0, 5.0, 1.0, hp[1], hp[2], 4)
    same = [O.NAMES[k] for k in ("norm_x", "norm_a", "dot", "step", "bc1", "bc2_sqrt")]
    assert np.array_equal(blk[same], plain[same]) and blk[3] == f32(-0.75)
    xx, aa, xa = (float(v) for v in sums)
    assert abs(float(blk[4]) - np.sqrt(xx + 1.5 * xa + 0.5625 * aa)) <= 2 * O.U * float(blk[4])
    # g = g_x + w g_a through the f64 update equals optimizer_ref's own update at scale -w
    p, m, v = (np.zeros(1027) for _ in range(3))
    (p1, *_), sc = R.weighted_step_f64(gx, ga, p, m, v, 1, hp, 0.75, 1.0)
    g = (np.asarray(gx, f64) + 0.75 * np.asarray(ga, f64)) * sc["clip_coef"]
    (p2, *_), = (O.adamw_f64(g, np.zeros(1027), p, m, v, dict(sc, scale=0.0, clip_coef=1.0), hp),)
    assert np.allclose(p1, p2, rtol=1e-13, atol=0)


# ================================================================ the C ABI
def test_the_entry_points_are_declared():
    from siss_amd import build
    from siss_amd.lib import PARAMS, RESTYPE, F32_SAME
    import ctypes
    assert PARAMS["siss_teacher_seed"] == ("pred", "noise", "noise_bf16", "teach", "teach_rows", "B", "chw", "keep_mode", "forget_mode",
                                           "eta", "scale", "cot", "sums", "partials", "stream")
    assert PARAMS["siss_grad_norms_weighted"] == ("gx", "ga", "n", "weight", "max_norm", "beta1", "beta2", "partials", "scalars", "stream")
    assert PARAMS["siss_teacher_partials_words"] == ("R", "chw") and RESTYPE["siss_teacher_partials_words"] is ctypes.c_long
    assert {"siss_teacher_seed", "siss_grad_norms_weighted"} <= F32_SAME
    assert "teacher.hip" in build.EXACT and "teacher.hip" in build.sources()

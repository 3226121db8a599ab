"""Host side of the trainable-subset update (siss_amd/trainable.py, the drop rule of siss_amd/wgrad.py, `deletion.trainable` in
siss_amd/tasks.py), no GPU:

* names -> merged granule table against tests/optimizer_ref.py zero_table / zero_mask;
* the "all outputs frozen" rule of the weight-gradient queue on a fake engine (CPU tensors), the fused to_k / to_v product included;
* every refusal of `deletion.trainable`, and null / an absent key / today's composed config being identical;
* an f64 restatement of the subset step -- optimizer_ref.step_f64 on the gathered trainable elements, scattered back -- against
  torch.optim.AdamW + clip_grad_norm_ over ONLY the trainable tensors of a small parameter list, modes 0, 1 and 2.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

import optimizer_ref as R
from siss_amd import trainable as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 64


def specs_of(shapes):
    """name -> spec (off, numel) laid out like ParamStore: every start rounded up to ALIGN floats; and the total"""
    out, off = {}, 0
    for name, numel in shapes:
        out[name] = types.SimpleNamespace(name=name, off=off, numel=numel)
        off += -(-numel // ALIGN) * ALIGN
    return out, off


SHAPES = [("conv_in.weight", 1728), ("conv_in.bias", 64), ("down.attn2.to_q.weight", 4096), ("down.attn2.to_k.weight", 4100),
          ("down.attn2.to_v.weight", 4096), ("down.attn2.to_out.0.weight", 4096), ("down.attn2.to_out.0.bias", 64),
          ("mid.resnets.0.conv1.weight", 36864), ("mid.resnets.0.conv1.bias", 7), ("up.attn2.to_k.weight", 1000),
          ("up.attn2.to_v.weight", 1000), ("conv_out.weight", 1729), ("conv_out.bias", 3)]


# ================================================================ selection -> table
@pytest.mark.parametrize("pick", [["attn2"], [r"attn2\.to_[kv]\."], [r"^conv_out\."], [r"\.bias$"], ["conv_in", "conv_out.bias"]])
def test_table_is_the_zero_ranges_table_of_the_selected_tensors(pick):
    specs, total = specs_of(SHAPES)
    names = TR.select(list(specs), TR.parse_patterns(pick))
    import re
    assert names == [n for n in specs if any(re.search(p, n) for p in pick)]
    sub = TR.Subset(specs, names, total, ALIGN)
    # the expected cover: [off, off + roundup(numel, ALIGN)) of every selected tensor, as a float mask
    want = np.zeros(total, bool)
    for n in names:
        want[specs[n].off:specs[n].off + -(-specs[n].numel // ALIGN) * ALIGN] = True
    tab, n, granules = sub.host_table()
    starts, pre = tab[:n], tab[n:]
    lens = [b - a for a, b in zip(pre, pre[1:])]
    ref_tab, ref_total = R.zero_table(starts, lens)
    assert list(ref_tab) == tab and ref_total == granules == int(want.sum()) // 4
    assert np.array_equal(R.zero_mask(total, starts, lens), want)
    # merged: no two stretches touch, ascending
    assert all(a1 + l1 < a2 for a1, l1, a2 in zip(starts, lens, starts[1:]))
    assert sub.tensors == len(names) and sub.params == sum(specs[n].numel for n in names)
    for nm, sp in specs.items():                                         # the frozen test the queue asks, tensor by tensor
        assert sub.is_frozen(sp.off, sp.numel) == (nm not in names), nm
    assert sub.is_frozen(0, total) is False


def test_adjacent_tensors_merge_and_pieces_merge_across_the_smallest_gaps():
    specs, total = specs_of([(f"t{i}", 64) for i in range(200)])
    sub = TR.Subset(specs, [f"t{i}" for i in range(200) if i % 4 != 3], total, ALIGN)
    assert sub.stretches == tuple((256 * k, 256 * k + 192) for k in range(50))
    assert len(sub.pieces(48)) == 1 and len(sub.pieces(50)) == 50          # equal gaps: merged all at once
    specs, total = specs_of([(f"t{i}", 64) for i in range(400)])
    keep = [i for i in range(400) if i % 4 == 0 or i in (1, 9)]            # two gaps of 2 tensors instead of 3
    sub = TR.Subset(specs, [f"t{i}" for i in keep], total, ALIGN)
    assert len(sub.stretches) == 100
    pieces = sub.pieces(99)
    assert len(pieces) == 98 and pieces[0] == (0, 64 * 5) and all(any(a <= s and e <= b for a, b in pieces) for s, e in sub.stretches)
    assert TR.Subset(specs, ["t3", "t4", "t5"], total, ALIGN).stretches == ((192, 384),)
    with pytest.raises(KeyError, match="nope"):
        TR.Subset(specs, ["t1", "nope"], total, ALIGN)
    with pytest.raises(ValueError, match="empty"):
        TR.Subset(specs, [], total, ALIGN)


# ================================================================ refusals
@pytest.mark.parametrize("value,word", [([], "empty"), (["attn2", "to_[k"], "to_[k"), (["("], "'('"), ("attn2", "LIST"), ([3], "3"),
                                        ([""], "''"), ({"a": 1}, "LIST")])
def test_malformed_entries_are_refused_by_name(value, word):
    with pytest.raises(ValueError) as e:
        TR.parse_patterns(value)
    assert word in str(e.value) and "deletion.trainable" in str(e.value)


def test_an_expression_that_matches_nothing_is_refused_and_everything_is_said(capsys):
    specs, _ = specs_of(SHAPES)
    with pytest.raises(ValueError, match="attn3") as e:
        TR.select(list(specs), TR.parse_patterns(["attn2", "attn3"]))
    assert "matches no parameter" in str(e.value)
    assert TR.select(list(specs), TR.parse_patterns(["."])) is None
    assert "matches every parameter" in capsys.readouterr().out
    assert TR.select(list(specs), None) is None and TR.parse_patterns(None) is None


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config, capsys):
    from siss_amd import hydra_lite as H
    base = H.compose(config, os.path.join(ROOT, "config"), [])
    assert "trainable" not in (base.get("deletion") or {}), "the YAMLs do not list the key"
    task = lambda ov: H.instantiate(H.compose(config, os.path.join(ROOT, "config"), ov).task, cfg=H.compose(config, os.path.join(ROOT, "config"), ov),
                                    _recursive_=False)
    for ov in ([], ["+deletion.trainable=null"]):
        t = task(ov)
        assert t.trainable_patterns() is None
        fake = types.SimpleNamespace(named_parameters=lambda: iter([("a.attn2.to_k.weight", None), ("b.conv.weight", None)]))
        assert t.trainable_names(fake) is None
    null = H.compose(config, os.path.join(ROOT, "config"), ["+deletion.trainable=null"])
    assert {k: v for k, v in dict(null.deletion).items() if k != "trainable"} == dict(base.deletion) and null.deletion.get("trainable") is None
    t = task(["+deletion.trainable=['attn2\\.to_[kv]\\.', '^b\\.']"])
    assert [p.pattern for p in t.trainable_patterns()] == [r"attn2\.to_[kv]\.", r"^b\."]
    fake = types.SimpleNamespace(named_parameters=lambda: iter([("a.attn2.to_k.weight", None), ("b.conv.weight", None), ("c.w", None)]))
    assert t.trainable_names(fake) == ["a.attn2.to_k.weight", "b.conv.weight"]
    for ov, word in ((["+deletion.trainable=[]"], "empty"), (["+deletion.trainable=['to_[k']"], "to_[k"), (["+deletion.trainable=attn2"], "LIST")):
        with pytest.raises(ValueError, match="deletion.trainable") as e:
            task(ov).check_supported()
        assert word in str(e.value)
    # ... and so do an entry that matches no parameter of the CONFIGURED UNet and a selection of everything (said, then the full update):
    # check_supported knows the parameter names from the configuration alone
    task([]).check_supported()
    some = "attn2" if config == "delete_sd" else "attentions"
    task([f"+deletion.trainable=[{some}]"]).check_supported()
    with pytest.raises(ValueError, match="zzz") as e:
        task([f"+deletion.trainable=[{some},zzz]"]).check_supported()
    assert "matches no parameter" in str(e.value)
    capsys.readouterr()
    task(["+deletion.trainable=['.']"]).check_supported()
    assert "matches every parameter" in capsys.readouterr().out
    names = task([]).unet_param_names()
    assert len(names) == {"delete_celeb": 450, "delete_sd": 686}.get(config, len(names)) and len(set(names)) == len(names)
    with pytest.raises(ValueError, match="zzz"):
        task(["+deletion.trainable=[attn2,zzz]"]).trainable_names(fake)


# ================================================================ the queue's drop rule
class _FakeEngine:
    f32, wgrad_overwrite, skip_frozen_wgrad = False, False, True

    def __init__(self, specs, total):
        self.device = torch.device("cpu")
        self.ps = types.SimpleNamespace(specs=specs, total=total, grads=torch.zeros(2, total))

    def window(self, name):
        return self.ps.grads[0:, self.ps.specs[name].off:]


def test_a_product_is_dropped_only_when_every_output_is_frozen():
    from siss_amd.wgrad import WgradQueue
    specs, total = specs_of([("a.to_k.weight", 64 * 32), ("a.to_v.weight", 64 * 32), ("a.to_out.weight", 64 * 64), ("a.to_out.bias", 64),
                             ("b.to_k.weight", 64 * 32), ("b.to_v.weight", 64 * 32), ("c.conv.weight", 9 * 64 * 64), ("c.conv.bias", 64)])
    eng = _FakeEngine(specs, total)
    q = WgradQueue(eng)
    Y, X = torch.zeros(8, 128, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16)
    kw = dict(nsets=2, rows_per_set=4, row_begin=0, row_end=4, x_set_rows=0)

    def kv(site):                                            # the fused to_k / to_v product: ONE job, N = 2 x 64 over C = 32
        return q.job(Y, 128, X, 32, eng.window(site + ".to_k.weight"), 128, 32, **kw)

    def out(site="a", bias=True):
        return q.job(Y, 64, X, 64, eng.window(site + ".to_out.weight"), 64, 64, dbias=eng.ps.grads[0, specs[site + ".to_out.bias"].off:] if bias else None, **kw)

    def conv():
        return q.job(Y, 64, X, 64, eng.window("c.conv.weight"), 64, 64, list(range(9)), [0] * 9, dbias=eng.ps.grads[0, specs["c.conv.bias"].off:], **kw)
    assert all(j is not None for j in (kv("a"), kv("b"), out(), conv())) and (q.issued, q.dropped) == (4, 0)     # no selection: nothing dropped
    sel = lambda names: q.set_frozen(TR.Subset(specs, names, total, ALIGN))
    sel(["a.to_v.weight"])                                   # one half of the fused product trainable: it runs
    assert kv("a") is not None and kv("b") is None and out() is None and conv() is None
    sel(["a.to_k.weight"])
    assert kv("a") is not None and kv("b") is None
    sel(["a.to_out.bias"])                                   # the bias alone keeps the product
    assert out() is not None and out(bias=False) is None and kv("a") is None
    sel(["c.conv.bias"])
    assert conv() is not None and out() is None
    sel(["a.to_out.weight"])
    assert conv() is None and out() is not None
    issued, dropped = q.issued, q.dropped
    assert dropped == 8
    eng.skip_frozen_wgrad = False                            # launch for launch the full update's pass
    assert all(j is not None for j in (kv("a"), kv("b"), out(), conv())) and (q.issued, q.dropped) == (issued + 4, dropped)
    eng.skip_frozen_wgrad = True
    scratch = torch.zeros(2, 9 * 64 * 64)                    # an output that is no window of the gradient buffer is read by somebody
    assert q.job(Y, 64, X, 64, scratch, 64, 64, set_stride=scratch[0].numel(), **kw) is not None
    assert q.all_frozen((eng.window("c.conv.weight"), 9 * 64 * 64, total, 2), (eng.ps.grads[0, specs["c.conv.bias"].off:], 64, total, 2))
    assert not q.all_frozen((eng.window("a.to_out.weight"), 64 * 64, total, 2))
    q.set_frozen(None)
    assert out() is not None and conv() is not None


# ================================================================ the subset step in f64 against torch
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_subset_step_in_f64_is_torch_adamw_and_clip_over_the_trainable_tensors(mode):
    """optimizer_ref.step_f64 on the gathered trainable elements, scattered back, against the reference's own sequence restricted to
    the trainable tensors: norms over them, s (delete_celeb.py:740-746, delete_tshirt.py:688-690), g = g_x - s g_a,
    clip_grad_norm_(trainable, 1.0), torch.optim.AdamW(trainable).step() -- all in f64.  Two steps, the state carried; frozen tensors
    hold NaN gradients.  Bound: both sides are f64 evaluations of the same expressions in different association orders: 1e-12 relative
    to the largest update (2^-53 times a few hundred operations)."""
    rng = np.random.default_rng(mode)
    shapes = [("a.w", 300), ("a.b", 5), ("attn2.k", 129), ("c.w", 64), ("attn2.v", 1000), ("d.b", 3)]
    specs, total = specs_of(shapes)
    names = [n for n, _ in shapes if "attn2" in n or n == "d.b"]
    sub = TR.Subset(specs, names, total, ALIGN)
    mask = np.zeros(total, bool)
    for a, b in sub.stretches:
        mask[a:b] = True
    hp = R.hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    lr, b1, b2, eps, wd = R.wide(hp)
    knob = 1e-2 if mode == 1 else 5.0
    p = np.zeros(total)
    for n, numel in shapes:
        p[specs[n].off:specs[n].off + numel] = rng.standard_normal(numel)
    p0 = p.copy()
    m, v = np.zeros(total), np.zeros(total)
    tp = {n: torch.tensor(p[specs[n].off:specs[n].off + specs[n].numel], dtype=torch.float64, requires_grad=True) for n in names}
    opt = torch.optim.AdamW(list(tp.values()), lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for step in (1, 2):
        gx, ga = np.full(total, np.nan), np.full(total, np.nan)
        gx[mask] = ga[mask] = 0.0                                           # the alignment padding: zero gradients
        for n in names:
            sl = slice(specs[n].off, specs[n].off + specs[n].numel)
            gx[sl], ga[sl] = 0.3 * rng.standard_normal(specs[n].numel), 0.5 * rng.standard_normal(specs[n].numel)
        if mode == 2 and step == 2:
            ga[mask] = 0.0                                                  # |g_a| = 0: the inf guard makes s = 0
        (pn, mn, vn, _), sc = R.step_f64(gx[mask], ga[mask], p[mask], m[mask], v[mask], step, hp, mode, knob, 1.0)
        p[mask], m[mask], v[mask] = pn, mn, vn
        # the reference's sequence on the trainable tensors
        tx = {n: torch.tensor(gx[specs[n].off:specs[n].off + specs[n].numel]) for n in names}
        ta = {n: torch.tensor(ga[specs[n].off:specs[n].off + specs[n].numel]) for n in names}
        na = math.sqrt(sum(float((t ** 2).sum()) for t in ta.values()))
        if mode == 1:
            dot = sum(float((tx[n] * ta[n]).sum()) for n in names)
            s = -max(float(np.float32(knob)) - dot / na ** 2, 0.0)
        else:
            s = float(np.float32(knob)) / na if na else math.inf
            if mode == 2 and math.isinf(s):
                s = 0.0
        for n in names:
            tp[n].grad = tx[n] - s * ta[n]
        total_norm = torch.nn.utils.clip_grad_norm_(list(tp.values()), 1.0)
        opt.step()
        assert abs(float(total_norm) - sc["pre_clip_norm"]) <= 1e-12 * max(float(total_norm), 1.0)
        assert abs(s - sc["scale"]) <= 1e-12 * max(abs(s), 1.0)
        scale = max(float((tp[n].detach() - torch.tensor(p0[specs[n].off:specs[n].off + specs[n].numel])).abs().max()) for n in names)
        for n in names:
            got = p[specs[n].off:specs[n].off + specs[n].numel]
            assert float(np.abs(got - tp[n].detach().numpy()).max()) <= 1e-12 * scale, (step, n)
    frozen = ~mask
    assert np.array_equal(p[frozen], p0[frozen]) and not m[frozen].any() and not v[frozen].any()
    assert not np.isnan(p).any()


def test_parameter_names_come_from_the_checkpoint_config_when_it_is_on_disk(tmp_path):
    """check_supported judges the selection on the UNet load_unet() will build: the checkpoint's config.json, where load_unet reads it."""
    import json
    from siss_amd import hydra_lite as H
    from siss_amd.config import UNet2DConditionConfig, UNet2DConfig
    from siss_amd.unet import UNetEngine
    from siss_amd.unet_cond import UNetCondEngine
    small = UNet2DConfig(sample_size=16, block_out_channels=(64, 128), down_block_types=("DownBlock2D", "AttnDownBlock2D"),
                         up_block_types=("AttnUpBlock2D", "UpBlock2D"), layers_per_block=1)
    cond = UNet2DConditionConfig(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(64, 128),
                                 down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
                                 attention_head_dim=2, cross_attention_dim=64)
    for config, key, ucfg, eng in (("delete_celeb", "checkpoint_path", small, UNetEngine), ("delete_sd", "pretrained_model_name_or_path", cond, UNetCondEngine)):
        d = tmp_path / config / "unet"
        d.mkdir(parents=True)
        raw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(ucfg).items()}
        (d / "config.json").write_text(json.dumps({**raw, "_class_name": "x"}))
        cfg = H.compose(config, os.path.join(ROOT, "config"), [f"{key}={tmp_path / config}", "+deletion.trainable=[down_blocks.1.attentions]"])
        task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
        names = task.unet_param_names()
        assert names == eng.param_names(ucfg) and len(names) < 450             # (not the default architecture: 450 / 686 tensors)
        if config == "delete_celeb":
            task.check_supported()                               # the small UNet has attention in down block 1 ...
        else:
            with pytest.raises(ValueError, match="matches no parameter"):    # ... the small conditional one has it in block 0 only
                task.check_supported()

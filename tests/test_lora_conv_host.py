"""Host side of LoRA on the 3x3 convolutions (`deletion.lora.conv_targets`, siss_amd/lora.py), no GPU:

* parsing with conv_targets alone and with both lists, and every refusal by name;
* select_conv_targets on the tiny UNet: what it takes, what it passes over, what it refuses;
* the layout: the linear rows of a state with conv targets are those of the same state without, the conv block lies behind them,
  aligned and disjoint, the padding is zero; params; the linear init bit-equal with and without conv targets; the conv init;
* the conv job table's bytes against the documented 64-byte record;
* the adapter file: peft's Conv2d shapes, a bit-equal round trip, native <-> reference against ops.conv_w_to_native; a linear-only
  state writes the files it wrote before;
* the f64 restatement (tests/lora_conv_ref.py) against torch.autograd.grad through F.conv2d with W0 + s (B @ A.flatten(1)).
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import lora_conv_ref as CR
import lora_ref as LR
from siss_amd import lora as LO
from test_lora_host import ALIGN, PROJ, ROOT, host_engine, tiny_specs

CONV = r"resnets\.\d+\.conv[12]\.weight"


# ================================================================ parsing and refusals
def test_parse_reads_conv_targets_alone_and_beside_targets():
    c = LO.parse_lora({"rank": 4, "conv_targets": [CONV]})
    assert c.patterns is None and [p.pattern for p in c.conv_patterns] == [CONV] and (c.rank, c.alpha, c.seed, c.scale) == (4, 4.0, 0, 1.0)
    c = LO.parse_lora({"rank": 16, "alpha": 8, "seed": 7, "targets": ["attn"], "conv_targets": [CONV, "conv_out"]})
    assert [p.pattern for p in c.patterns] == ["attn"] and [p.pattern for p in c.conv_patterns] == [CONV, "conv_out"]
    assert (c.rank, c.alpha, c.seed, c.scale) == (16, 8.0, 7, 0.5), "rank, alpha and seed are shared by both kinds"
    c = LO.parse_lora({"rank": 4, "targets": ["attn"]})
    assert c.conv_patterns is None and [p.pattern for p in c.patterns] == ["attn"]
    c = LO.parse_lora({"rank": 4, "targets": None, "conv_targets": [CONV]})
    assert c.patterns is None and len(c.conv_patterns) == 1


@pytest.mark.parametrize("value,words", [
    ({"rank": 4}, ("targets",)),
    ({"rank": 4, "targets": None, "conv_targets": None}, ("targets",)),
    ({"rank": 4, "targets": []}, ("empty", "deletion.lora.targets")),
    ({"rank": 4, "targets": [], "conv_targets": [CONV]}, ("empty", "deletion.lora.targets")),
    ({"rank": 4, "conv_targets": []}, ("empty", "deletion.lora.conv_targets")),
    ({"rank": 4, "targets": ["attn"], "conv_targets": []}, ("empty", "deletion.lora.conv_targets")),
    ({"rank": 4, "conv_targets": "conv1"}, ("LIST", "deletion.lora.conv_targets")),
    ({"rank": 4, "conv_targets": ["conv[1"]}, ("conv[1", "deletion.lora.conv_targets")),
    ({"rank": 4, "conv_targets": [""]}, ("deletion.lora.conv_targets",)),
    ({"rank": 4, "conv_targets": [3]}, ("deletion.lora.conv_targets",)),
    ({"rank": 0, "conv_targets": [CONV]}, ("rank=0",)),
    ({"rank": 65, "conv_targets": [CONV]}, ("rank=65",)),
    ({"rank": 4, "conv_targets": [CONV], "alpha": 0}, ("alpha",)),
    ({"rank": 4, "conv_targets": [CONV], "seed": 1.5}, ("seed",)),
    ({"rank": 4, "conv_targets": [CONV], "conv_rank": 2}, ("conv_rank",)),
    ({"rank": 4, "conv_targets": [CONV], "dropout": 0.1}, ("dropout",)),
])
def test_malformed_values_are_refused_by_name(value, words):
    with pytest.raises(ValueError) as e:
        LO.parse_lora(value)
    assert all(w in str(e.value) for w in words) and "deletion.lora" in str(e.value), str(e.value)


def test_conv_targets_with_trainable_is_refused():
    with pytest.raises(ValueError, match="deletion.trainable"):
        LO.parse_lora({"rank": 4, "conv_targets": [CONV]}, trainable=["attn"])


# ================================================================ select_conv_targets
def test_conv_targets_are_3x3_weights_and_everything_else_is_refused_by_name():
    specs = tiny_specs()
    pats = lambda *p: LO.parse_lora({"rank": 4, "conv_targets": list(p)}).conv_patterns
    conv3 = [n for n in specs if specs[n].kind == "conv3"]
    assert "conv_out.weight" in conv3 and any("downsamplers" in n for n in conv3) and any("upsamplers" in n for n in conv3)
    names = LO.select_conv_targets(specs, pats(CONV))
    assert names == [n for n in specs if re.search(CONV, n)] and len(names) >= 8
    assert all(specs[n].kind == "conv3" and specs[n].native_shape[0] == 9 for n in names)
    # the downsampler's, the upsampler's and conv_out's convolutions
    assert LO.select_conv_targets(specs, pats(r"samplers\.0\.conv\.weight", r"^conv_out\.weight")) == \
        [n for n in conv3 if "samplers" in n or n == "conv_out.weight"]
    # written for MODULES: the biases an expression also matches are passed over; with the norms of a whole resnet too
    assert LO.select_conv_targets(specs, pats(r"resnets\.\d+\.conv[12]")) == names
    assert LO.select_conv_targets(specs, pats(r"samplers|conv_out|resnets\.\d+\.(conv[12]|norm[12])\.")) == conv3
    for bad, word in ((r"to_q\.weight", "deletion.lora.targets"), (r"conv_shortcut\.weight", "deletion.lora.targets"),
                      (r"^conv_in\.weight", "input convolution"), (r"^conv_in", "input convolution"), (r"conv", "deletion.lora.targets"),
                      (r"time_emb_proj", "deletion.lora.targets"), (r"conv1\.bias", "bias / norm"), (r"norm1\.weight", "bias / norm")):
        with pytest.raises(ValueError, match="deletion.lora.conv_targets") as e:
            LO.select_conv_targets(specs, pats(CONV, bad))
        assert word in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="zzz") as e:
        LO.select_conv_targets(specs, pats(CONV, "zzz"))
    assert "matches no parameter" in str(e.value) and "deletion.lora.conv_targets" in str(e.value)
    # `targets` keeps refusing the convolutions, with the words it had, and now points to conv_targets
    with pytest.raises(ValueError, match="deletion.lora.targets") as e:
        LO.select_targets(specs, LO.parse_lora({"rank": 4, "targets": [CONV]}).patterns)
    assert "3x3 convolution" in str(e.value) and repr(CONV) in str(e.value) and "conv_targets" in str(e.value)
    cfg = LO.parse_lora({"rank": 4, "targets": [PROJ], "conv_targets": [CONV]})
    assert LO.resolve_targets(specs, cfg) == (LO.select_targets(specs, cfg.patterns), names)
    assert LO.resolve_targets(specs, LO.parse_lora({"rank": 4, "conv_targets": [CONV]})) == ([], names)


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_resolve_conv_targets_in_check_supported(config):
    from siss_amd import hydra_lite as H

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    t = task(["+deletion.lora={rank:4,conv_targets:['resnets\\.\\d+\\.conv[12]\\.weight']}"])
    c = t.lora_config()
    assert c.patterns is None and [p.pattern for p in c.conv_patterns] == [CONV]
    t.check_supported()
    task(["+deletion.lora={rank:4,targets:[to_q],conv_targets:[conv_out,'samplers\\.0\\.conv\\.weight']}"]).check_supported()
    for ov, word in (("{rank:4,conv_targets:[zzz]}", "zzz"), ("{rank:4,conv_targets:[to_q]}", "deletion.lora.targets"),
                     ("{rank:4,conv_targets:['^conv_in']}", "input convolution"), ("{rank:4,conv_targets:[]}", "empty"),
                     ("{rank:4,targets:['conv1\\.weight'],conv_targets:[conv_out]}", "3x3 convolution")):
        with pytest.raises(ValueError, match="deletion.lora") as e:
            task(["+deletion.lora=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="deletion.trainable"):
        task(["+deletion.lora={rank:4,conv_targets:[conv_out]}", "+deletion.trainable=[attn]"]).check_supported()


def test_the_pretraining_task_refuses_conv_targets_too():
    from siss_amd import hydra_lite as H
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.lora={rank:4,conv_targets:[conv_out]}"])
    with pytest.raises(NotImplementedError, match="deletion.lora"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


# ================================================================ layout, init and the job table
def both_states(rank=4, seed=3):
    eng = host_engine()
    specs = eng.ps.specs
    lin = LO.select_targets(specs, LO.parse_lora({"rank": rank, "targets": [PROJ]}).patterns)
    conv = [n for n in specs if specs[n].kind == "conv3"]                       # resnets, both samplers, conv_out
    return eng, lin, conv, LO.LoRAState(eng, lin, rank, alpha=8.0, seed=seed), \
        LO.LoRAState(eng, lin, rank, alpha=8.0, seed=seed, conv_names=list(reversed(conv)))


@pytest.mark.parametrize("rank", [1, 3, 4, 64])
def test_the_conv_block_lies_behind_the_linear_block(rank):
    eng, lin, conv, plain, st = both_states(rank)
    specs = eng.ps.specs
    assert st.names == plain.names and st.rows == plain.rows and st.shapes == plain.shapes, "the linear rows changed"
    assert (st.project_tiles, st.merge_tiles) == (plain.project_tiles, plain.merge_tiles)
    assert np.array_equal(st.jobs.numpy(), plain.jobs.numpy())
    assert plain.conv_names == () and plain.conv_rows == [] and plain.L == max(r[2] + -(-r[4] * rank // ALIGN) * ALIGN for r in plain.rows)
    assert st.conv_names == tuple(sorted(conv, key=lambda n: specs[n].off))
    for n, row in zip(st.conv_names, st.conv_rows):
        sp = specs[n]
        assert (row[0], (row[8], row[4], row[5])) == (sp.off, sp.native_shape) and row[8] * row[4] * row[5] == sp.numel and row[8] == 9
    a_offs, b_offs = [r[1] for r in st.conv_rows], [r[2] for r in st.conv_rows]
    assert all(o % ALIGN == 0 for o in a_offs + b_offs + [r[3] for r in st.conv_rows]) and st.L % ALIGN == 0
    assert min(a_offs) == plain.L, "the conv block starts where the linear block ends"
    assert max(a_offs) < min(b_offs), "every A lies before every B"
    spans = sorted([(r[1], r[1] + 9 * rank * r[5]) for r in st.conv_rows] + [(r[2], r[2] + r[4] * rank) for r in st.conv_rows])
    assert all(e <= s2 and s2 - e < ALIGN for (_, e), (s2, _) in zip(spans, spans[1:])) and 0 <= st.L - spans[-1][1] < ALIGN
    # W0 of the conv targets is packed behind the linear targets' W0
    w0 = [(r[3], r[3] + 9 * r[4] * r[5]) for r in st.conv_rows]
    assert w0[0][0] == plain.w0.numel() and all(e <= s2 for (_, e), (s2, _) in zip(w0, w0[1:])) and w0[-1][1] <= st.w0.numel()
    assert torch.equal(st.w0[:plain.w0.numel()], plain.w0)
    for row in st.conv_rows:
        n = 9 * row[4] * row[5]
        assert torch.equal(st.w0[row[3]:row[3] + n], eng.ps.flat[row[0]:row[0] + n])
    # tile prefix sums: ceil(O / 64) + 9 ceil(I / 64) in the projection, 9 ceil(O / 64) ceil(I / 64) in the merge
    pt = [-(-r[4] // 64) + 9 * -(-r[5] // 64) for r in st.conv_rows]
    mt = [9 * -(-r[4] // 64) * -(-r[5] // 64) for r in st.conv_rows]
    assert [r[6] for r in st.conv_rows] == list(np.cumsum([0] + pt[:-1])) and st.conv_project_tiles == sum(pt)
    assert [r[7] for r in st.conv_rows] == list(np.cumsum([0] + mt[:-1])) and st.conv_merge_tiles == sum(mt)
    # params / tensors / state bytes count both kinds
    want = sum(rank * sum(specs[n].native_shape) for n in lin) + sum(rank * (specs[n].native_shape[1] + 9 * specs[n].native_shape[2]) for n in conv)
    assert st.params == want and st.tensors == 2 * (len(lin) + len(conv)) and st.optimizer_state_bytes() == 8 * st.L
    assert st.p.numel() == st.L and tuple(st.g.shape) == (2, st.L) and not st.g.any()
    used = LR.used_mask(st.L, st.rows, rank) | CR.used_mask(st.L, st.conv_rows, rank)
    assert int(used.sum()) == st.params and not (LR.used_mask(st.L, st.rows, rank) & CR.used_mask(st.L, st.conv_rows, rank)).any()
    assert not st.p[torch.from_numpy(~used)].any(), "the padding is not zero"


def test_init_linear_draws_first_then_peft_conv_init():
    eng, lin, conv, plain, st = both_states(4, seed=3)
    assert torch.equal(st.p[:plain.L].view(torch.int32), plain.p.view(torch.int32)), "the linear init changed with conv targets beside it"
    for i, row in enumerate(st.conv_rows):
        A, B = st.conv_A(i), st.conv_B(i)
        fan = 9 * row[5]
        assert tuple(A.shape) == (9, 4, row[5]) and tuple(B.shape) == (row[4], 4) and not B.any()
        assert float(A.abs().max()) <= fan ** -0.5 and float(A.std()) > 0.4 * fan ** -0.5
    # the draws, restated: the linear targets' [r, I], then each conv target's [r, I, 3, 3] in the reference layout, converted
    from siss_amd import ops
    gen = torch.Generator().manual_seed(3)
    for row in st.rows:
        torch.rand(4, row[5], generator=gen)
    for i, row in enumerate(st.conv_rows):
        a_ref = (torch.rand(4, row[5], 3, 3, generator=gen) * 2 - 1) * (1.0 / (9 * row[5]) ** 0.5)
        assert torch.equal(st.conv_A(i), ops.conv_w_to_native(a_ref))
    again = LO.LoRAState(eng, lin, 4, alpha=8.0, seed=3, conv_names=conv)
    assert torch.equal(again.p, st.p) and not torch.equal(LO.LoRAState(eng, lin, 4, seed=4, conv_names=conv).p, st.p)
    # conv targets alone: names = [] is allowed then, and only then
    only = LO.LoRAState(eng, [], 4, conv_names=conv)
    assert only.names == () and only.rows == [] and only.conv_rows[0][1] == 0 and only.params == sum(4 * (r[4] + 9 * r[5]) for r in only.conv_rows)
    for names, cn, exc in (([], [], KeyError), (lin, ["conv_in.weight"], ValueError), (lin, [lin[0]], KeyError), (lin, [conv[0], conv[0]], KeyError),
                           (lin, ["nope.weight"], KeyError), (lin, [conv[0][:-len("weight")] + "bias"], ValueError), ([conv[0]], [], ValueError)):
        with pytest.raises(exc):
            LO.LoRAState(eng, names, 4, conv_names=cn)


def test_conv_job_table_bytes_are_the_documented_record():
    shapes = [(192, 48, 40), (20480, 17, 130), (8192 * 9, 3, 64)]
    rows, L, w0_floats, pt, mt = LO.conv_layout(shapes, 3, ALIGN, base=1024, w0_base=4096)
    assert rows[0][1] == 1024 and rows[0][3] == 4096 and all(r[8] == 9 for r in rows)
    rec = LO.conv_job_table(rows)
    assert rec.dtype.itemsize == 64
    # {long w_off, a_off, b_off, w0_off; int O, I, ptile0, mtile0, taps, pad[3] = 0}
    want = b"".join(np.array(r[:4], "<i8").tobytes() + np.array(r[4:9], "<i4").tobytes() + bytes(12) for r in rows)
    assert rec.tobytes() == want and len(want) == 64 * len(rows)
    assert LO.conv_job_table([]).tobytes() == b""
    # the linear record is untouched
    lrows = LO.layout(shapes, 3, ALIGN)[0]
    assert LO.job_table(lrows).dtype.itemsize == 48


# ================================================================ the adapter file
def test_conv_save_load_round_trip_is_bit_equal_in_pefts_shapes(tmp_path):
    from safetensors.torch import load_file
    from siss_amd import ops
    eng, lin, conv, plain, st = both_states(3, seed=1)
    g = torch.Generator().manual_seed(9)
    for i in range(len(st.rows)):
        st.B(i).copy_(torch.randn(st.B(i).shape, generator=g))
    for i in range(len(st.conv_rows)):
        st.conv_B(i).copy_(torch.randn(st.conv_B(i).shape, generator=g))
    st.steps, st.base = 12, "/some/checkpoint"
    st.save(str(tmp_path / "lora"))
    assert sorted(os.listdir(tmp_path / "lora")) == ["lora_config.json", "pytorch_lora_weights.safetensors"]
    sd = load_file(str(tmp_path / "lora" / "pytorch_lora_weights.safetensors"))
    assert len(sd) == 2 * (len(lin) + len(conv))
    for i, n in enumerate(st.conv_names):
        mod = n[:-len(".weight")]
        co, ci = eng.ps.specs[n].ref_shape[:2]
        a, b = sd[f"unet.{mod}.lora_A.weight"], sd[f"unet.{mod}.lora_B.weight"]
        assert tuple(a.shape) == (3, ci, 3, 3) and tuple(b.shape) == (co, 3, 1, 1)
        # native <-> reference: A's file form is what ops.conv_w_to_native maps onto the native [9, r, Ci]
        assert torch.equal(ops.conv_w_to_native(a), st.conv_A(i)) and torch.equal(a, ops.conv_w_from_native(st.conv_A(i)))
        assert torch.equal(b[:, :, 0, 0], st.conv_B(i))
        # ... and peft's merge of the file's tensors is the native one: (B.flatten(1) @ A.flatten(1)).reshape(W.shape)
        delta = (b.flatten(1).double() @ a.flatten(1).double()).reshape(co, ci, 3, 3)
        native = torch.einsum("ok,tki->toi", st.conv_B(i).double(), st.conv_A(i).double())
        assert float((ops.conv_w_to_native(delta) - native).abs().max()) <= 1e-14 * float(native.abs().max())
    c = json.load(open(tmp_path / "lora" / "lora_config.json"))
    assert c["targets"] == list(st.names) and c["conv_targets"] == list(st.conv_names) and c["lora_params"] == st.params
    back = LO.LoRAState.load(eng, str(tmp_path / "lora"))
    assert torch.equal(back.p.view(torch.int32), st.p.view(torch.int32)) and (back.names, back.conv_names) == (st.names, st.conv_names)
    assert (back.rank, back.alpha, back.steps, back.base) == (3, 8.0, 12, "/some/checkpoint")
    for k, v in st.state_dict().items():
        assert torch.equal(sd[k].view(torch.int32), v.view(torch.int32)), k
    # strict: a wrong shape, a missing and an unexpected key
    k = f"unet.{st.conv_names[0][:-len('.weight')]}.lora_A.weight"
    good = st.state_dict()
    with pytest.raises(ValueError, match="shape") as e:
        st.load_state_dict(dict(good, **{k: good[k].flatten(1)}))
    assert k in str(e.value)
    with pytest.raises(ValueError, match="shape"):
        st.load_state_dict(dict(good, **{k.replace("lora_A", "lora_B"): good[k.replace("lora_A", "lora_B")][:, :, 0, 0]}))
    with pytest.raises(KeyError, match="missing"):
        st.load_state_dict({kk: v for kk, v in good.items() if kk != k})
    with pytest.raises(KeyError, match="unexpected"):
        plain.load_state_dict(good)
    st.load_state_dict(good)


def test_a_linear_only_state_writes_the_files_it_wrote_before(tmp_path):
    from safetensors.torch import load_file
    eng, lin, conv, plain, st = both_states(3, seed=1)
    plain.steps, plain.base = 5, "/b"
    plain.save(str(tmp_path / "a"))
    text = open(tmp_path / "a" / "lora_config.json").read()
    # the file of the linear-only mode, restated: these keys in this order, indent 1, no conv_targets
    want = json.dumps(dict(rank=3, alpha=8.0, targets=list(plain.names), seed=1, base_checkpoint="/b", steps=5, lora_params=plain.params), indent=1)
    assert text == want and "conv_targets" not in text
    sd = load_file(str(tmp_path / "a" / "pytorch_lora_weights.safetensors"))
    assert list(sd) == sorted(k for n in plain.names for k in LO.adapter_keys(n)) and all(v.dim() == 2 for v in sd.values())
    assert "lora_conv_tensors" not in plain.log_fields() and set(plain.log_fields()) == {"lora_rank", "lora_alpha", "lora_params", "lora_tensors"}
    assert st.log_fields()["lora_conv_tensors"] == 2 * len(conv) and st.log_fields()["lora_params"] == st.params
    assert LO.LoRAState.load(eng, str(tmp_path / "a")).conv_names == ()


# ================================================================ the f64 restatement is the chain rule of peft's Conv2d adapter
@pytest.mark.parametrize("r,s", [(1, 1.0), (4, 2.0), (16, 0.25)])
def test_reference_conv_projection_is_autograd_through_the_parametrisation(r, s):
    from siss_amd import ops
    g = torch.Generator().manual_seed(r)
    shapes = [(64, 6, 5), (1024, 3, 8)]
    rows, L, w0_floats, _, _ = LO.conv_layout(shapes, r, ALIGN)
    P = 1024 + 9 * 3 * 8
    used = CR.used_mask(L, rows, r)
    p = torch.zeros(L, dtype=torch.float64)
    p[torch.from_numpy(used)] = torch.randn(int(used.sum()), generator=g, dtype=torch.float64)
    w0 = torch.randn(w0_floats, generator=g, dtype=torch.float64)
    merged, _ = CR.merge(np.zeros(P), rows, w0.numpy(), p.numpy(), r, s)
    for row in rows:
        w_off, a, b, w0_off, O, I, _, _, T = row
        A_nat, B_nat = CR.views(p.numpy(), row, r)
        A = torch.from_numpy(CR.a_native_to_ref(A_nat)).requires_grad_(True)            # lora_A.weight [r, I, 3, 3]
        B = torch.from_numpy(B_nat.copy()).reshape(O, r, 1, 1).requires_grad_(True)     # lora_B.weight [O, r, 1, 1]
        base = ops.conv_w_from_native(w0[w0_off:w0_off + T * O * I].reshape(T, O, I))
        W = base + s * (B.flatten(1) @ A.flatten(1)).reshape(base.shape)                # peft's get_delta_weight
        assert np.abs(ops.conv_w_to_native(W.detach()).numpy().reshape(-1) - merged[w_off:w_off + T * O * I]).max() <= 1e-12
        x = torch.randn(2, I, 7, 6, generator=g, dtype=torch.float64)
        cot = torch.randn(2, O, 7, 6, generator=g, dtype=torch.float64)
        y = torch.nn.functional.conv2d(x, W, padding=1)
        dW, dA, dB = torch.autograd.grad((y * cot).sum(), (W, A, B))
        got, _ = CR.project(ops.conv_w_to_native(dW).reshape(1, -1).numpy(), [(0, a, b, w0_off, O, I, 0, 0, T)], p.numpy(), r, s, nsets=1)
        scale = max(float(dA.abs().max()), float(dB.abs().max()))
        assert np.abs(got[0, a:a + T * r * I] - ops.conv_w_to_native(dA).numpy().reshape(-1)).max() <= 1e-12 * scale
        assert np.abs(got[0, b:b + O * r] - dB.numpy().reshape(-1)).max() <= 1e-12 * scale
        assert not got[1].any() and not got[0][~used].any()

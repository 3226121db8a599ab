"""Host side of the LoRA unlearning mode (siss_amd/lora.py, `deletion.lora` in siss_amd/tasks.py), no GPU:

* parsing and every refusal of `deletion.lora` (a conv3 target, both keys set, rank 0 / 65, an entry that matches nothing, ...);
* the flat buffer's layout (every A, then every B, each padded to ALIGN) and the job table against the specs of a tiny UNet;
* the adapter file: key names, a bit-equal save / load round trip, a strict load that refuses a wrong shape;
* the f64 reference's dA, dB (tests/lora_ref.py) against torch.autograd.grad through W0 + s B A on a random linear, to 1e-12.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

import lora_ref as LR
from siss_amd import lora as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 64
KW = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
          down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)
PROJ = r"attentions\.\d+\.to_(q|k|v|out\.0)\.weight"


def tiny_specs():
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    return UNetEngine.param_specs(UNet2DConfig(**KW))


def host_engine(seed=0):
    """What LoRAState reads of an engine, on the CPU: the specs of the tiny UNet and a random flat master."""
    specs = tiny_specs()
    total = max(sp.off + -(-sp.numel // ALIGN) * ALIGN for sp in specs.values())
    flat = torch.randn(total, generator=torch.Generator().manual_seed(seed))
    return types.SimpleNamespace(device=torch.device("cpu"), ps=types.SimpleNamespace(specs=specs, flat=flat, total=total))


# ================================================================ parsing and refusals
def test_parse_reads_the_mapping_and_defaults():
    assert LO.parse_lora(None) is None
    c = LO.parse_lora({"rank": 4, "targets": ["attn"]})
    assert (c.rank, c.alpha, c.seed, c.scale, [p.pattern for p in c.patterns]) == (4, 4.0, 0, 1.0, ["attn"])
    c = LO.parse_lora({"rank": 16, "alpha": 8, "targets": ["to_q", "to_v"], "seed": 7})
    assert (c.rank, c.alpha, c.seed, c.scale) == (16, 8.0, 7, 0.5)


@pytest.mark.parametrize("value,word", [({"rank": 0, "targets": ["attn"]}, "rank=0"), ({"rank": 65, "targets": ["attn"]}, "rank=65"),
                                        ({"rank": 4.0, "targets": ["attn"]}, "rank=4.0"), ({"rank": True, "targets": ["attn"]}, "rank"),
                                        ({"targets": ["attn"]}, "rank=None"), ({"rank": 4}, "targets"), ({"rank": 4, "targets": []}, "empty"),
                                        ({"rank": 4, "targets": "attn"}, "LIST"), ({"rank": 4, "targets": ["to_[k"]}, "to_[k"),
                                        ({"rank": 4, "targets": ["attn"], "alpha": 0}, "alpha"), ({"rank": 4, "targets": ["attn"], "alpha": "x"}, "alpha"),
                                        ({"rank": 4, "targets": ["attn"], "dropout": 0.1}, "dropout"), ([4, "attn"], "mapping"),
                                        ({"rank": 4, "targets": ["attn"], "seed": 1.5}, "seed")])
def test_malformed_values_are_refused_by_name(value, word):
    with pytest.raises(ValueError) as e:
        LO.parse_lora(value)
    assert word in str(e.value) and "deletion.lora" in str(e.value)


def test_both_keys_set_is_refused():
    with pytest.raises(ValueError, match="deletion.trainable"):
        LO.parse_lora({"rank": 4, "targets": ["attn"]}, trainable=["attn"])
    assert LO.parse_lora(None, trainable=["attn"]) is None


def test_targets_are_linear_weights_and_everything_else_is_refused_by_name():
    specs = tiny_specs()
    pats = lambda *p: LO.parse_lora({"rank": 4, "targets": list(p)}).patterns
    names = LO.select_targets(specs, pats(PROJ))
    assert names and all(n.endswith(".weight") and specs[n].kind == "mat" and len(specs[n].native_shape) == 2 for n in names)
    assert names == [n for n in specs if __import__("re").search(PROJ, n)]
    # the 1x1 shortcut is a plain [O, I] matrix too
    sc = LO.select_targets(specs, pats(r"conv_shortcut\.weight"))
    assert sc and all(specs[n].kind == "conv1" for n in sc)
    for bad, word in ((r"resnets\.0\.conv1\.weight", "3x3 convolution"), (r"^conv_in\.weight", "input convolution"),
                      (r"to_q\.bias", "bias / norm"), (r"group_norm\.weight", "bias / norm"), (r"resnets\.0\.conv", "3x3 convolution")):
        with pytest.raises(ValueError, match="deletion.lora.targets") as e:
            LO.select_targets(specs, pats(PROJ, bad))
        assert word in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="zzz") as e:
        LO.select_targets(specs, pats(PROJ, "zzz"))
    assert "matches no parameter" in str(e.value)
    # an expression written for the attention MODULES: their projections' weights; the biases and the norm it also matches carry no adapter
    assert LO.select_targets(specs, pats("attentions")) == names


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config):
    from siss_amd import hydra_lite as H
    base = H.compose(config, os.path.join(ROOT, "config"), [])
    assert "lora" not in (base.get("deletion") or {}), "the YAMLs do not list the key"

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    assert task([]).lora_config() is None and task(["+deletion.lora=null"]).lora_config() is None
    task([]).check_supported()
    proj = r"attn[12]\.to_q\.weight" if config == "delete_sd" else r"attentions\.\d\.to_q\.weight"
    t = task(["+deletion.lora={rank:4,targets:['%s'],alpha:8}" % proj])
    c = t.lora_config()
    assert (c.rank, c.alpha, [p.pattern for p in c.patterns]) == (4, 8.0, [proj])
    t.check_supported()
    mods = "attn" if config == "delete_sd" else "attentions"       # written for the attention MODULES (the SD names say attn1 / attn2)
    task(["+deletion.lora={rank:4,targets:[%s]}" % mods]).check_supported()
    for ov, word in (("{rank:0,targets:[attn]}", "rank=0"), ("{rank:65,targets:[attn]}", "rank=65"), ("{rank:4,targets:[zzz]}", "zzz"),
                     ("{rank:4,targets:['conv1\\.weight']}", "3x3 convolution"), ("{rank:4,targets:[]}", "empty"), ("attn", "mapping")):
        with pytest.raises(ValueError, match="deletion.lora") as e:
            task(["+deletion.lora=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="deletion.trainable"):
        task(["+deletion.lora={rank:4,targets:[attn]}", "+deletion.trainable=[attn]"]).check_supported()


def test_the_pretraining_task_refuses_the_key():
    from siss_amd import hydra_lite as H
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.lora={rank:4,targets:[attn]}"])
    with pytest.raises(NotImplementedError, match="deletion.lora"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [])
    H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


# ================================================================ layout and job table
@pytest.mark.parametrize("rank", [1, 3, 16, 64])
def test_layout_every_a_then_every_b_aligned_and_disjoint(rank):
    shapes = [(128, 48, 40), (4096, 17, 130), (8192, 320, 768), (300032, 64, 64)]
    rows, L, w0_floats, pt, mt = LO.layout(shapes, rank, ALIGN)
    assert [r[0] for r in rows] == [s[0] for s in shapes] and [(r[4], r[5]) for r in rows] == [(s[1], s[2]) for s in shapes]
    a_offs, b_offs = [r[1] for r in rows], [r[2] for r in rows]
    assert all(o % ALIGN == 0 for o in a_offs + b_offs + [r[3] for r in rows]) and L % ALIGN == 0 and w0_floats % ALIGN == 0
    assert max(a_offs) < min(b_offs), "every A lies before every B"
    spans = sorted([(r[1], r[1] + rank * r[5]) for r in rows] + [(r[2], r[2] + r[4] * rank) for r in rows])
    assert spans[0][0] == 0 and all(e <= s2 and s2 - e < ALIGN for (_, e), (s2, _) in zip(spans, spans[1:])) and 0 <= L - spans[-1][1] < ALIGN
    assert int(LR.used_mask(L, rows, rank).sum()) == sum(rank * (O + I) for _, O, I in shapes)
    w0 = [(r[3], r[3] + r[4] * r[5]) for r in rows]
    assert w0[0][0] == 0 and all(e <= s2 for (_, e), (s2, _) in zip(w0, w0[1:])) and w0[-1][1] <= w0_floats
    # tile prefix sums: ceil(O / 64) row tiles + ceil(I / 64) column tiles in the projection, their product in the merge
    ptiles = [-(-O // 64) + -(-I // 64) for _, O, I in shapes]
    mtiles = [-(-O // 64) * -(-I // 64) for _, O, I in shapes]
    assert [r[6] for r in rows] == list(np.cumsum([0] + ptiles[:-1])) and pt == sum(ptiles)
    assert [r[7] for r in rows] == list(np.cumsum([0] + mtiles[:-1])) and mt == sum(mtiles)
    rec = LO.job_table(rows)
    assert rec.dtype.itemsize == 48 and rec.tobytes() == b"".join(np.array(r[:4], "<i8").tobytes() + np.array(r[4:], "<i4").tobytes() for r in rows)


def test_job_table_against_the_specs_of_a_tiny_unet():
    eng = host_engine()
    specs = eng.ps.specs
    names = LO.select_targets(specs, LO.parse_lora({"rank": 4, "targets": [PROJ]}).patterns)
    st = LO.LoRAState(eng, list(reversed(names)), 4, alpha=8.0, seed=3)
    assert st.names == tuple(sorted(names, key=lambda n: specs[n].off)) and st.scale == 2.0
    for n, row in zip(st.names, st.rows):
        sp = specs[n]
        assert (row[0], row[4], row[5]) == (sp.off, *sp.native_shape) and row[4] * row[5] == sp.numel
    assert st.params == sum(4 * sum(specs[n].native_shape) for n in names) and st.tensors == 2 * len(names)
    assert st.p.numel() == st.L and tuple(st.g.shape) == (2, st.L) and st.optimizer_state_bytes() == 8 * st.L
    used = torch.from_numpy(LR.used_mask(st.L, st.rows, 4))
    assert not st.p[~used].any() and not st.g.any()
    for i, row in enumerate(st.rows):                       # peft's init: A ~ U(-1/sqrt(I), 1/sqrt(I)), B = 0; W0 is the master's copy
        A, B = st.A(i), st.B(i)
        assert tuple(A.shape) == (4, row[5]) and tuple(B.shape) == (row[4], 4)
        assert not B.any() and float(A.abs().max()) <= row[5] ** -0.5 and float(A.std()) > 0.4 * row[5] ** -0.5
        assert torch.equal(st.w0[row[3]:row[3] + row[4] * row[5]], eng.ps.flat[row[0]:row[0] + row[4] * row[5]])
    again = LO.LoRAState(eng, names, 4, alpha=8.0, seed=3)
    assert torch.equal(again.p, st.p) and not torch.equal(LO.LoRAState(eng, names, 4, seed=4).p, st.p)
    for bad, exc in ((["conv_in.weight"], ValueError), ([names[0], names[0]], KeyError), (["nope.weight"], KeyError), ([], KeyError)):
        with pytest.raises(exc):
            LO.LoRAState(eng, bad, 4)
    for rank in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            LO.LoRAState(eng, names, rank)


# ================================================================ the adapter file
def test_save_load_round_trip_is_bit_equal_with_peft_style_keys(tmp_path):
    from safetensors.torch import load_file
    eng = host_engine()
    names = LO.select_targets(eng.ps.specs, LO.parse_lora({"rank": 3, "targets": [PROJ]}).patterns)
    st = LO.LoRAState(eng, names, 3, alpha=6.0, seed=1)
    g = torch.Generator().manual_seed(9)
    for i in range(len(st.rows)):
        st.B(i).copy_(torch.randn(st.B(i).shape, generator=g))
    st.steps, st.base = 12, "/some/checkpoint"
    st.save(str(tmp_path / "lora"))
    assert sorted(os.listdir(tmp_path / "lora")) == ["lora_config.json", "pytorch_lora_weights.safetensors"]
    sd = load_file(str(tmp_path / "lora" / "pytorch_lora_weights.safetensors"))
    n0 = st.names[0]
    assert n0.endswith(".to_q.weight")
    mod = n0[:-len(".weight")]
    assert f"unet.{mod}.lora_A.weight" in sd and f"unet.{mod}.lora_B.weight" in sd and len(sd) == 2 * len(names)
    O, I = eng.ps.specs[n0].native_shape
    assert tuple(sd[f"unet.{mod}.lora_A.weight"].shape) == (3, I) and tuple(sd[f"unet.{mod}.lora_B.weight"].shape) == (O, 3)
    c = json.load(open(tmp_path / "lora" / "lora_config.json"))
    assert (c["rank"], c["alpha"], c["targets"], c["base_checkpoint"], c["steps"]) == (3, 6.0, list(st.names), "/some/checkpoint", 12)
    back = LO.LoRAState.load(eng, str(tmp_path / "lora"))
    assert torch.equal(back.p.view(torch.int32), st.p.view(torch.int32)) and back.names == st.names
    assert (back.rank, back.alpha, back.steps, back.base) == (3, 6.0, 12, "/some/checkpoint")
    for k, v in st.state_dict().items():
        assert torch.equal(sd[k].view(torch.int32), v.view(torch.int32)), k


def test_strict_load_refuses_wrong_shapes_and_names():
    eng = host_engine()
    names = LO.select_targets(eng.ps.specs, LO.parse_lora({"rank": 4, "targets": [PROJ]}).patterns)
    st = LO.LoRAState(eng, names, 4)
    sd = st.state_dict()
    k = next(iter(sd))
    with pytest.raises(ValueError, match="shape") as e:
        st.load_state_dict(dict(sd, **{k: sd[k][:, :-1].clone()}))
    assert k in str(e.value)
    with pytest.raises(ValueError, match="shape"):
        LO.LoRAState(eng, names, 8).load_state_dict(sd)              # an adapter of another rank
    with pytest.raises(KeyError, match="missing"):
        st.load_state_dict({kk: v for kk, v in sd.items() if kk != k})
    with pytest.raises(KeyError, match="unexpected"):
        st.load_state_dict(dict(sd, **{"unet.mid_block.nope.lora_A.weight": sd[k]}))
    st.load_state_dict(sd)


# ================================================================ the f64 reference is the chain rule
@pytest.mark.parametrize("r,s", [(1, 1.0), (4, 2.0), (16, 0.25)])
def test_reference_projection_is_autograd_through_the_parametrisation(r, s):
    g = torch.Generator().manual_seed(r)
    shapes = [(64, 48, 40), (2048, 17, 130)]
    rows, L, w0_floats, _, _ = LO.layout(shapes, r, ALIGN)
    P = 2048 + 17 * 130
    p = torch.zeros(L, dtype=torch.float64)
    p[torch.from_numpy(LR.used_mask(L, rows, r))] = torch.randn(int(LR.used_mask(L, rows, r).sum()), generator=g, dtype=torch.float64)
    w0 = torch.randn(w0_floats, generator=g, dtype=torch.float64)
    cot = torch.randn(2, P, generator=g, dtype=torch.float64)          # dL_k / dW: any two cotangents of the merged weights
    ref, _ = LR.project(cot.numpy(), rows, p.numpy(), r, s, nsets=2)
    merged, _ = LR.merge(np.zeros(P), rows, w0.numpy(), p.numpy(), r, s)
    for row in rows:
        w_off, a, b, w0_off, O, I, _, _ = row
        A = p[a:a + r * I].reshape(r, I).clone().requires_grad_(True)
        B = p[b:b + O * r].reshape(O, r).clone().requires_grad_(True)
        W = w0[w0_off:w0_off + O * I].reshape(O, I) + s * B @ A
        assert np.abs(W.detach().numpy().reshape(-1) - merged[w_off:w_off + O * I]).max() <= 1e-12
        x = torch.randn(5, I, generator=g, dtype=torch.float64)
        for k in range(2):
            # a linear layer y = x W^T with the loss <y, c>: dL/dW = c^T x -- the cotangent handed to the reference is that product
            c = torch.randn(5, O, generator=g, dtype=torch.float64)
            dW = (c.t() @ x).detach()
            dA, dB = torch.autograd.grad(((x @ W.t()) * c).sum(), (A, B), retain_graph=True)
            got, _ = LR.project(dW.reshape(1, -1).numpy(), [(0, a, b, w0_off, O, I, 0, 0)], p.numpy(), r, s, nsets=1)
            scale = max(float(dA.abs().max()), float(dB.abs().max()))
            assert np.abs(got[0, a:a + r * I] - dA.numpy().reshape(-1)).max() <= 1e-12 * scale
            assert np.abs(got[0, b:b + O * r] - dB.numpy().reshape(-1)).max() <= 1e-12 * scale
            assert not got[1].any()
    assert not ref[:, ~LR.used_mask(L, rows, r)].any()


def test_adapter_step_is_adamw_on_the_adapter_buffer():
    """lora_ref.adapter_step against torch.optim.AdamW + clip_grad_norm_ over the adapter tensors (mode 0: s = scaling_norm / |g_a|)."""
    import optimizer_ref as R
    rng = np.random.default_rng(0)
    n, knob = 1000, 5.0
    hp = R.hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2)
    gx, ga, p0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    (p, m, v, g), sc = LR.adapter_step(gx, ga, p0, np.zeros(n), np.zeros(n), 1, hp, 0, knob, 1.0)
    t = torch.from_numpy(p0.copy()).requires_grad_(True)
    lr, b1, b2, eps, wd = R.wide(hp)
    opt = torch.optim.AdamW([t], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    t.grad = torch.from_numpy(gx - knob / np.linalg.norm(ga) * ga)
    pre = float(torch.nn.utils.clip_grad_norm_([t], 1.0))
    opt.step()
    assert abs(pre - sc["pre_clip_norm"]) <= 1e-12 * pre and np.abs(t.detach().numpy() - p).max() <= 1e-12

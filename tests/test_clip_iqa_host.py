"""Host side of the SD CLIP-IQA score (siss_amd/clip_iqa.py, DeleteSD's opt-in metric): the parameter surface against the restatement
tests/clip_iqa_ref.py, strict loading, the checkpoint loader on a TorchScript file / a state dict / a safetensors file / a foreign
key set, the network's wiring with the launchers emulated by torch in f64, the restatement's anchors against transformers' CLIP text
model, the padding rule of the pooling position, the prompt table, the tracker's records and the task's refusals.  No GPU."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clip_iqa_ref as R  # noqa: E402
import metric_net_emul  # noqa: E402
from siss_amd import metric_net  # noqa: E402

SMALL_KW = dict(layers=(1, 1, 1, 1), width=64, output_dim=64, text_width=128, text_heads=2, text_layers=2, vocab_size=96, context_length=16)
SOT, EOT = 94, 95                                   # the two last ids of the small vocabulary, as in CLIP's
IDS = torch.tensor([[SOT, 3, 4, EOT] + [0] * 12, [SOT, 7, EOT] + [0] * 13, [SOT, 9, 9, 5, EOT] + [0] * 11, [SOT, EOT] + [0] * 14])


@pytest.fixture(scope="module")
def net():
    return R.make(0)


@pytest.fixture(scope="module")
def small():
    return R.make(1, **R.SMALL)


def _small_model(small, **kw):
    from siss_amd.clip_iqa import CLIPIQAModel
    m = CLIPIQAModel(**{**SMALL_KW, **kw})
    m.load_state_dict(small.state_dict())
    return m


def test_keys_order_and_shapes_against_the_restatement(net, small):
    from siss_amd.clip_iqa import CLIPIQAModel
    for ref, m in ((net.state_dict(), CLIPIQAModel()), (small.state_dict(), CLIPIQAModel(**SMALL_KW))):
        sd = m.state_dict()
        assert list(sd) == list(ref)                                  # the OpenAI module's state-dict order
        assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ref.values()]
    sd = CLIPIQAModel().state_dict()
    assert {"visual.conv1.weight", "visual.bn3.running_var", "visual.layer3.5.bn2.running_var", "visual.layer1.0.downsample.0.weight",
            "visual.layer4.0.downsample.1.bias", "visual.attnpool.positional_embedding", "visual.attnpool.c_proj.bias",
            "transformer.resblocks.11.attn.in_proj_weight", "transformer.resblocks.0.mlp.c_fc.bias", "token_embedding.weight",
            "ln_final.bias", "text_projection", "positional_embedding", "logit_scale"} <= set(sd)
    assert "visual.layer1.1.downsample.0.weight" not in sd and "visual.layer2.0.downsample.-1.weight" not in sd
    assert sd["visual.conv1.weight"].shape == (32, 3, 3, 3) and sd["visual.attnpool.positional_embedding"].shape == (50, 2048)
    assert sd["visual.attnpool.c_proj.weight"].shape == (1024, 2048) and sd["text_projection"].shape == (512, 1024)
    assert sd["token_embedding.weight"].shape == (49408, 512) and sd["positional_embedding"].shape == (77, 512)
    learned = [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert sum(sd[k].numel() for k in learned) == sum(p.numel() for p in net.parameters()) == 102_007_137    # OpenAI's RN50
    torch.manual_seed(5)                              # building the model leaves the global random stream where it was
    a = torch.rand(3)
    torch.manual_seed(5)
    CLIPIQAModel(**SMALL_KW)
    assert torch.equal(torch.rand(3), a)
    for bad in (dict(width=32), dict(width=96), dict(layers=(1, 1, 1)), dict(heads=7), dict(batch_size=0), dict(text_width=96)):
        with pytest.raises(ValueError):
            CLIPIQAModel(**{**SMALL_KW, **bad})


def test_strict_load_refusals_and_eval_only(small):
    from siss_amd.clip_iqa import CLIPIQAModel
    good = small.state_dict()
    m = CLIPIQAModel(**SMALL_KW)
    assert m.load_state_dict(good) is None
    assert all(torch.equal(v, good[k]) for k, v in m.state_dict().items())
    # what may be absent, and what an OpenAI archive carries besides
    m.load_state_dict({k: v for k, v in good.items() if not k.endswith("num_batches_tracked") and k != "logit_scale"})
    m.load_state_dict({**good, "input_resolution": torch.tensor(224), "context_length": torch.tensor(16), "vocab_size": torch.tensor(96)})
    with pytest.raises(RuntimeError, match=r"missing keys \['visual.layer2.0.downsample.0.weight'\]"):
        m.load_state_dict({k: v for k, v in good.items() if k != "visual.layer2.0.downsample.0.weight"})
    with pytest.raises(RuntimeError, match=r"missing keys \['visual.attnpool.positional_embedding'\]"):   # loaded, though not used
        m.load_state_dict({k: v for k, v in good.items() if k != "visual.attnpool.positional_embedding"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['visual.layer1.1.conv1.weight'\]"):
        m.load_state_dict({**good, "visual.layer1.1.conv1.weight": torch.zeros(64, 256, 1, 1)})
    with pytest.raises(RuntimeError, match="visual.attnpool.c_proj.weight has shape"):
        m.load_state_dict({**good, "visual.attnpool.c_proj.weight": torch.zeros(1024, 2048)})
    with pytest.raises(RuntimeError, match="transformer.resblocks.0.attn.in_proj_weight has shape"):
        m.load_state_dict({**good, "transformer.resblocks.0.attn.in_proj_weight": torch.zeros(128, 128)})
    with pytest.raises(NotImplementedError, match="eval mode"):
        m.train()
    assert m.train(False) is m and m.eval() is m
    with pytest.raises(RuntimeError, match="cuda"):                # no CPU path
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="cuda"):
        m.embed_u8(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="cuda"):
        m.anchors(IDS[:2])
    with pytest.raises(ValueError, match="uint8"):
        m.embed_u8(torch.zeros(1, 32, 32, 3))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        m(torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError, match="vocabulary of 96"):      # refused on the host: a bad id would fault the gather
        m.anchors(torch.tensor([[SOT, 96, EOT], [SOT, 1, EOT]]))
    with pytest.raises(ValueError, match="16 positions"):
        m.anchors(torch.zeros(2, 17, dtype=torch.long))
    with pytest.raises(ValueError, match=r"\[2 P, L\]"):
        m.anchors(IDS[:3])


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_loader_on_torchscript_state_dict_safetensors_and_a_foreign_key_set(small, tmp_path):
    from safetensors.torch import save_file
    from siss_amd.clip_iqa import CLIPIQAModel
    good = small.state_dict()
    want = _small_model(small).state_dict()
    torch.jit.script(small).save(str(tmp_path / "clip.torchscript.pt"))
    torch.save(good, str(tmp_path / "state.pt"))
    save_file({k: v.contiguous() for k, v in good.items()}, str(tmp_path / "clip.safetensors"))
    for name in ("clip.torchscript.pt", "state.pt", "clip.safetensors"):
        m = CLIPIQAModel.load(tmp_path / name, batch_size=4)
        assert not m.training and m.batch_size == 4 and _same(m.state_dict(), want), name
        assert (m.layers, m.width, m.heads, m.output_dim) == ((1, 1, 1, 1), 64, 32, 64)       # the sizes follow the file
        assert (m.text_width, m.text_heads, m.text_layers, m.vocab_size, m.context_length, m.input_resolution) == (128, 2, 2, 96, 16, 224)
    # a foreign key set: a transformers-style CLIP, named in the message with what is missing
    foreign = {("vision_model." + k[len("visual."):] if k.startswith("visual.") else k): v for k, v in good.items()}
    torch.save(foreign, str(tmp_path / "foreign.pt"))
    with pytest.raises(RuntimeError) as e:
        CLIPIQAModel.load(tmp_path / "foreign.pt")
    assert "not an OpenAI-format CLIP ResNet" in str(e.value) and "'visual.conv1.weight'" in str(e.value)
    assert "unexpected keys ['vision_model.conv1.weight'" in str(e.value)
    (tmp_path / "junk.bin").write_bytes(b"not a checkpoint at all")
    with pytest.raises(RuntimeError, match="neither"):
        CLIPIQAModel.load(tmp_path / "junk.bin")
    with pytest.raises(FileNotFoundError, match="not a file"):
        CLIPIQAModel.load(tmp_path / "missing.pt")


# ---------------------------------------------------------------- the wiring, launchers emulated in f64
def _pack_conv64(w, b, stride, pad, device, _pack=metric_net.pack_conv):
    """metric_net.pack_conv's layer with the weights and the bias kept in f64 (its layout restated: [Cout][Kp] in (kh, kw, ci) order)."""
    L = _pack(w, b, stride, pad, "cpu")
    cout, cin, kh, kw = w.shape
    assert L["cin_p"] == cin and (cin <= 4 or cin % 32 == 0)
    L["w"] = torch.zeros(cout, L["Kp"], dtype=torch.float64)
    L["w"][:, :kh * kw * cin] = w.permute(0, 2, 3, 1).reshape(cout, -1).double()
    L["b"] = b.double()
    return L


def _tokens(x, m, N, HW, E):
    return torch.cat([m.view(N, 1, E), x.reshape(N, HW, E)], 1)


def _emulated_call(name, *a):
    """What the launchers compute, by torch's f64 operations on host tensors (the arguments as lib.call gets them): the shared
    convolution in tests/metric_net_emul.py (in f64 here: the buffers are), csrc/clip_iqa.hip's own here."""
    import torch.nn.functional as F
    if metric_net_emul.call(name, *a) == 0:
        return 0
    if name == "siss_clipiqa_avgpool":
        x, y, N, H, W, C, k = a
        assert tuple(x.shape) == (N, H, W, C) and tuple(y.shape) == (N, H // k, W // k, C) and C % 4 == 0
        y.copy_(F.avg_pool2d(x.permute(0, 3, 1, 2), k).permute(0, 2, 3, 1))
    elif name == "siss_clipiqa_token_mean":
        x, m, N, HW, C = a
        assert x.numel() == N * HW * C and tuple(m.shape) == (N, C)
        m.copy_(x.reshape(N, HW, C).mean(1))
    elif name == "siss_clipiqa_fold_query":
        q, wk, bk, qt, c, N, E, heads, scale = a
        D = E // heads
        assert q.numel() == N * E and tuple(wk.shape) == (E, E) and tuple(qt.shape) == (N, heads, E) and tuple(c.shape) == (N, heads)
        qh = q.reshape(N, heads, D).double() * scale
        qt.copy_(torch.einsum("nhd,hde->nhe", qh, wk.double().view(heads, D, E)))
        c.copy_(torch.einsum("nhd,hd->nh", qh, bk.double().view(heads, D)))
    elif name == "siss_clipiqa_scores":
        x, m, qt, c, s, N, HW, E, heads = a
        assert tuple(s.shape) == (N, heads, HW + 1) and E % 64 == 0
        s.copy_(torch.einsum("nhe,nte->nht", qt, _tokens(x, m, N, HW, E)) + c[:, :, None])
    elif name == "siss_clipiqa_pool":
        x, m, s, xbar, N, HW, E, heads = a
        assert tuple(xbar.shape) == (N, heads, E) and heads <= 256
        xbar.copy_(torch.einsum("nht,nte->nhe", s.softmax(-1), _tokens(x, m, N, HW, E)))
    elif name == "siss_clipiqa_head_value":
        xbar, wv, bv, o, N, E, heads = a
        D = E // heads
        o.copy_((torch.einsum("hde,nhe->nhd", wv.double().view(heads, D, E), xbar) + bv.double().view(heads, D)).reshape(N, E))
    elif name == "siss_clipiqa_score":
        f, anchors, N, D, P, out = a
        assert tuple(f.shape) == (N, D) and tuple(anchors.shape) == (2 * P, D) and tuple(out.shape) == (N, P)
        out.copy_(R.score(f.double(), anchors.double()))
    else:
        raise KeyError(name)
    return 0


@pytest.mark.parametrize("h, w", [(32, 32), (72, 40)])
def test_network_wiring_with_emulated_launchers(small, monkeypatch, h, w):
    """siss_amd/clip_iqa.py's side of the network -- BN folding, which layer reads what, where the pools sit on the main path and
    on the shortcut, the floors, the attention pool's folded form, c_proj, the score, the chunking -- against the f64 restatement,
    no GPU: the launchers are replaced by torch's f64 operations and the activations are kept in f64, so the agreement is held to
    1e-10 of the reference's scale (f64 rounding through ~20 layers is orders below that; any wiring error is orders above)."""
    from siss_amd import clip_iqa, lib
    monkeypatch.setattr(lib, "call", _emulated_call)
    monkeypatch.setattr(clip_iqa, "ACT", torch.float64)
    monkeypatch.setattr(metric_net, "pack_conv", _pack_conv64)
    monkeypatch.setattr(clip_iqa, "pack_linear", lambda w_, b_, d: (w_.double(), b_.double()))
    u8 = torch.randint(0, 256, (3, h, w, 3), generator=torch.Generator().manual_seed(h), dtype=torch.uint8)
    x = R.normalise(u8).double()
    ref = R.embed(small, x)
    anc = R.anchors(small, IDS)
    m = _small_model(small, batch_size=2)                           # two chunks
    m.device = torch.device("cuda")                                # packing is refused on a CPU model; the tensors stay on the host
    m._pack()
    m.device = torch.device("cpu")
    got, scores, _ = m._run(x, None, anc)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    serr = float((scores - R.score(ref, anc)).abs().max())
    print(f"\nwiring {h}x{w}: rows {err:.2e} of scale {scale:.2f}, scores {serr:.2e}")
    assert got.shape == (3, 64) and scores.shape == (3, 2) and got.dtype == torch.float64
    assert err <= 1e-10 and serr <= 1e-10
    assert m._shapes(1, h, w)[0] == (h // 32, w // 32)
    # (the stride on conv2 is a network only where every map is even: a strided 3 x 3 rounds an odd size up, the pool beside it down)
    even = h % 32 == 0 and w % 32 == 0
    for ctl in (R.variant(small, maxpool=True), R.reset_bn(small)) + ((R.variant(small, stride_on_conv2=True),) if even else ()):
        assert float((R.embed(ctl, x) - got).abs().max()) / scale >= 1e-4
    # token 1 as the query: another network wherever the map has more than one position (on a 1 x 1 map the mean IS that token)
    away = float((R.embed(R.variant(small, query_token=1), x) - got).abs().max()) / scale
    assert away >= 1e-4 if (h // 32) * (w // 32) > 1 else away <= 1e-10
    # a chunk whose largest tensor would reach 2^31 elements is refused before anything runs; an image too small for the pools too
    assert m.max_elements(1, 512, 512) == 256 * 256 * 64
    with pytest.raises(ValueError, match="2\\^31"):
        m._features(torch.empty(1024, 3, 512, 512, device="meta"))
    with pytest.raises(ValueError, match="too small"):
        m._features(torch.empty(1, 3, 16, 64, device="meta"))


# ---------------------------------------------------------------- anchors
def test_restated_anchors_match_transformers_clip_text_model(small):
    """The restatement's text tower against transformers' CLIPTextModelWithProjection on the same weights (remapped by
    clip_iqa.text_encoder_state, the very remapping the HIP encoder is fed through), in f64: 1e-10."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    from siss_amd.clip_iqa import text_encoder_state
    cfg = CLIPTextConfig(vocab_size=96, hidden_size=128, intermediate_size=512, projection_dim=64, num_hidden_layers=2,
                         num_attention_heads=2, max_position_embeddings=16, hidden_act="quick_gelu", eos_token_id=EOT,
                         bos_token_id=SOT, pad_token_id=0)
    hf = CLIPTextModelWithProjection(cfg).double().eval()
    sd = small.state_dict()
    st = {"text_model." + k: v.double() for k, v in text_encoder_state(sd, 2).items()}
    st["text_projection.weight"] = sd["text_projection"].t().double()
    res = hf.load_state_dict(st, strict=False)
    assert not res.unexpected_keys and all("position_ids" in k for k in res.missing_keys)
    with torch.no_grad():
        e = hf(input_ids=IDS).text_embeds
    e = e / e.norm(dim=-1, keepdim=True)
    a = R.anchors(small, IDS)
    err = float((a - e).abs().max())
    print(f"\nanchors against transformers: {err:.2e}")
    assert a.shape == (4, 64) and err <= 1e-10
    assert float((a[0] - a[1]).abs().max()) > 1e-3                 # (the prompts are told apart)


def test_zero_padded_and_eot_padded_ids_give_the_same_anchors(small):
    from siss_amd.clip_iqa import eot_positions
    padded = IDS.clone()
    padded[padded == 0] = EOT                                      # a CLIP tokenizer pads with the end-of-text id
    assert eot_positions(IDS) == eot_positions(padded) == [3, 2, 4, 1] == R.first_largest(padded).tolist()
    assert padded.argmax(-1).tolist() == [3, 2, 4, 1]              # (torch's argmax takes the first too; the code does not lean on it)
    a, b = R.anchors(small, IDS), R.anchors(small, padded)
    assert float((a - b).abs().max()) <= 1e-14
    # pooling at the LAST occurrence would not: the row there has seen the padding
    last = [15, 15, 15, 15]
    x = R._as(small, torch.float64, "cpu")
    with torch.no_grad():
        h = x.ln_final(x.transformer((x.token_embedding(padded) + x.positional_embedding).permute(1, 0, 2)).permute(1, 0, 2))
        wrong = h[torch.arange(4), torch.tensor(last)] @ x.text_projection
    wrong = wrong / wrong.norm(dim=-1, keepdim=True)
    assert float((wrong - a).abs().max()) > 1e-3


# ---------------------------------------------------------------- the metric's surface
def test_prompt_table_and_metric_arguments(small):
    from siss_amd.clip_iqa import PROMPTS, CLIPImageQualityAssessment, format_prompts
    assert list(PROMPTS) == ["quality", "brightness", "noisiness", "colorfullness", "sharpness", "contrast", "complexity", "natural",
                             "happy", "scary", "new", "warm", "real", "beautiful", "lonely", "relaxing"]
    assert PROMPTS["quality"] == ("Good photo.", "Bad photo.") and PROMPTS["noisiness"] == ("Clean photo.", "Noisy photo.")
    assert all(len(v) == 2 and all(t.endswith(" photo.") for t in v) for v in PROMPTS.values())
    assert format_prompts(("quality",)) == (["Good photo.", "Bad photo."], ["quality"])
    texts, names = format_prompts(("sharpness", ("a", "b"), "real", ("c", "d")))
    assert names == ["sharpness", "user_defined_0", "real", "user_defined_1"]
    assert texts == ["Sharp photo.", "Blurry photo.", "a", "b", "Real photo.", "Abstract photo.", "c", "d"]
    for bad in (["quality"], ("nice",), (("a",),), (("a", "b", "c"),), (3,), ()):
        with pytest.raises(ValueError):
            format_prompts(bad)
    m = _small_model(small)
    q = CLIPImageQualityAssessment(model=m, prompt_ids=IDS[:2])
    assert q.prompts_names == ["quality"] and q.data_range == 1.0 and torch.equal(q.prompt_ids, IDS[:2])
    assert CLIPImageQualityAssessment(model=m, prompts=("quality", ("x", "y")), prompt_ids=IDS).prompts_names == ["quality", "user_defined_0"]
    with pytest.raises(ValueError, match="clip_iqa"):
        CLIPImageQualityAssessment(model=m, prompt_ids=IDS[:2], model_name_or_path="openai/clip-vit-base-patch16")
    with pytest.raises(ValueError, match="CLIPIQAModel is needed"):
        CLIPImageQualityAssessment(prompt_ids=IDS[:2])
    with pytest.raises(ValueError, match="prompt_ids .*or tokenizer"):
        CLIPImageQualityAssessment(model=m)                         # no token ids are hard-coded
    with pytest.raises(ValueError, match=r"\[2, L\]"):
        CLIPImageQualityAssessment(model=m, prompt_ids=IDS)
    with pytest.raises(ValueError, match="data_range"):
        CLIPImageQualityAssessment(model=m, prompt_ids=IDS[:2], data_range=0)
    with pytest.raises(FileNotFoundError, match="tokenizer"):
        CLIPImageQualityAssessment(model=m, tokenizer="/nowhere/tokenizer")
    with pytest.raises(ValueError, match="No samples"):
        q.compute()
    with pytest.raises(RuntimeError, match="cuda"):
        q.update(torch.zeros(1, 3, 32, 32))


def test_tracker_records(tmp_path):
    from siss_amd.clip_iqa import CLIPIQAScore
    out = tmp_path / "metrics_rank0.jsonl"
    tr = CLIPIQAScore(None, IDS[:2], str(out))
    vals = torch.tensor([[0.25], [0.5], [1.0], [0.1]], dtype=torch.float32)
    assert tr.record(0, vals, 3) == {"global_step": 3, "clip_iqa_0": float(vals.double().mean())}
    tr.record(1, torch.tensor([[1.0]]), 3)
    tr.record(0, torch.tensor([[float("nan")], [0.5]]), 4)
    lines = [json.loads(l) for l in open(out)]
    assert lines == [{"global_step": 3, "clip_iqa_0": float(vals.double().mean())}, {"global_step": 3, "clip_iqa_1": 1.0},
                     {"global_step": 4, "clip_iqa_0": None}]
    with pytest.raises(ValueError, match=r"\[2 P, L\]"):
        CLIPIQAScore(None, IDS[:3], str(out))


def _cfg(tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    return H.compose("delete_sd", os.path.join(ROOT, "config"), [f"base_dir={tmp_path}", f"output_dir={tmp_path}/out", *overrides])


def test_check_clip_iqa_refusals_fire_before_any_step(small, tmp_path, capsys):
    from siss_amd.clip_iqa import CLIPIQAScore
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    (ckpt / "vae").mkdir(parents=True)
    torch.save(small.state_dict(), str(tmp_path / "clip.pt"))
    torch.save({"trunk." + k: v for k, v in small.state_dict().items()}, str(tmp_path / "foreign.pt"))
    torch.save(IDS[:2], str(tmp_path / "ids.pt"))
    torch.save(IDS, str(tmp_path / "four.pt"))
    torch.save(torch.tensor([[SOT, 200, EOT], [SOT, 1, EOT]]), str(tmp_path / "big.pt"))
    base = [f"pretrained_model_name_or_path={ckpt}"]
    model, ids = f"metrics.clip_iqa.model_path={tmp_path}/clip.pt", f"metrics.clip_iqa.prompt_ids_path={tmp_path}/ids.pt"

    def check(*ov):                                  # what run() does before it loads anything onto the device
        task = DeleteSD(_cfg(tmp_path, *ov))
        task.fill_cfg()
        task.check_supported()
        task.check_metrics()
        return task.clip_iqa

    assert check(*base) is None                                                       # key null (the shipped default)
    assert _cfg(tmp_path, *base).metrics.clip_iqa is None
    assert check(*base, "metrics.clip_iqa=false") is None
    cfg = _cfg(tmp_path, *base)
    del cfg["metrics"]
    assert DeleteSD(cfg).check_clip_iqa() is None                                     # no metrics block at all
    tr = check(*base, model, ids, "metrics.clip_iqa.batch_size=4")
    assert isinstance(tr, CLIPIQAScore) and torch.equal(tr.prompt_ids, IDS[:2]) and tr.out_path == f"{tmp_path}/out/metrics_rank0.jsonl"
    assert tr.model.batch_size == 4 and tr.model.output_dim == 64 and tr.model.layers == (1, 1, 1, 1)
    assert check(*base, model, ids).model.batch_size == 16
    with pytest.raises(ValueError, match="model_path"):
        check(*base, "metrics.clip_iqa=true")                                         # bare true: the mapping with no keys
    with pytest.raises(ValueError, match="model_path"):
        check(*base, ids)
    with pytest.raises(FileNotFoundError, match="model_path.*not a file"):
        check(*base, f"metrics.clip_iqa.model_path={tmp_path}/missing.pt", ids)
    with pytest.raises(RuntimeError, match="not an OpenAI-format CLIP ResNet.*missing keys"):
        check(*base, f"metrics.clip_iqa.model_path={tmp_path}/foreign.pt", ids)
    with pytest.raises(FileNotFoundError, match="vae"):
        check(f"pretrained_model_name_or_path={tmp_path}/nowhere", model, ids)
    with pytest.raises(FileNotFoundError, match="prompt_ids_path.*tokenizer_path"):
        check(*base, model)                                                           # no tokenizer/ beside the checkpoint either
    with pytest.raises(FileNotFoundError, match="tokenizer_path"):
        check(*base, model, f"metrics.clip_iqa.tokenizer_path={tmp_path}/no_tokenizer")
    with pytest.raises(FileNotFoundError, match="prompt_ids_path.*not a file"):
        check(*base, model, f"metrics.clip_iqa.prompt_ids_path={tmp_path}/gone.pt")
    with pytest.raises(ValueError, match=r"prompt_ids_path.*\[2, L\]"):
        check(*base, model, f"metrics.clip_iqa.prompt_ids_path={tmp_path}/four.pt")
    with pytest.raises(ValueError, match="vocabulary 96"):
        check(*base, model, f"metrics.clip_iqa.prompt_ids_path={tmp_path}/big.pt")
    # a missing checkpoint with allow_random_init: a random-init network, loudly
    capsys.readouterr()
    tr = check(*base, f"metrics.clip_iqa.model_path={tmp_path}/missing.pt", ids, "allow_random_init=true")
    said = capsys.readouterr().out
    assert isinstance(tr, CLIPIQAScore) and "RANDOM-INIT" in said and "NOT comparable" in said and tr.model.output_dim == 1024
    assert not os.path.exists(tmp_path / "out" / "train_log_rank0.jsonl")


def test_text_encoder_keyword_and_remapping(small):
    """CLIPTextEncoder's dtype keyword defaults to bf16 and refuses anything but bf16 / f32; the remapping splits in_proj into q / k / v."""
    import inspect
    from siss_amd.clip_iqa import text_encoder_state
    from siss_amd.text_encoder import CLIPTextEncoder
    assert inspect.signature(CLIPTextEncoder.__init__).parameters["dtype"].default is torch.bfloat16
    sd = small.state_dict()
    st = text_encoder_state(sd, 2)
    w = sd["transformer.resblocks.1.attn.in_proj_weight"]
    assert torch.equal(st["encoder.layers.1.self_attn.q_proj.weight"], w[:128]) and torch.equal(st["encoder.layers.1.self_attn.v_proj.weight"], w[256:])
    assert torch.equal(st["encoder.layers.0.mlp.fc1.weight"], sd["transformer.resblocks.0.mlp.c_fc.weight"])
    assert torch.equal(st["final_layer_norm.bias"], sd["ln_final.bias"]) and len(st) == 4 + 2 * 16


def test_new_entry_points_are_declared_and_bound():
    from siss_amd import lib
    for n in ("siss_clipiqa_avgpool", "siss_clipiqa_token_mean", "siss_clipiqa_fold_query", "siss_clipiqa_scores", "siss_clipiqa_pool",
              "siss_clipiqa_head_value", "siss_clipiqa_score"):
        assert n in lib.SIGNATURES and lib.PARAMS[n][-1] == "stream" and n in lib.F32_SAME, n
    assert "siss_quick_gelu_f32" in lib.SIGNATURES and "siss_quick_gelu_f32" in lib.F32_SAME      # reachable inside lib.f32_mode(True)
    assert lib.SIGNATURES["siss_quick_gelu_f32"] == lib.SIGNATURES["siss_quick_gelu"]
    assert lib.PARAMS["siss_clipiqa_scores"][:5] == ("x", "m", "qt", "c", "s")

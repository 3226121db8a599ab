"""The SD CLIP-IQA score on the GPU (csrc/clip_iqa.hip behind siss_amd/clip_iqa.py): the average pool, the folded attention pool
and the score kernel against f64, the whole image tower and the score against the f64 restatement (tests/clip_iqa_ref.py) with
negative controls and determinism, the anchors of the f32 text tower, two full-size images from both source forms, the checkpoint
loader's round trip, and the metric in the delete_sd task loop.

The bound of a network output is the project's convention for metric networks: 8 x the deviation of the same restatement run in torch
f32 from its f64 run, measured in the test and printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clip_iqa_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL_KW = dict(layers=(1, 1, 1, 1), width=64, output_dim=64, text_width=128, text_heads=2, text_layers=2, vocab_size=96, context_length=16)
SOT, EOT = 94, 95
IDS = torch.tensor([[SOT, 3, 4, EOT] + [0] * 12, [SOT, 7, EOT] + [0] * 13, [SOT, 9, 9, 5, EOT] + [0] * 11, [SOT, EOT] + [0] * 14])
# "Good photo." / "Bad photo." shaped rows in the full vocabulary (start, two words, a full stop, end; zero padding as torchmetrics')
FULL_IDS = torch.tensor([[49406, 886, 1125, 269, 49407] + [0] * 72, [49406, 2103, 1125, 269, 49407] + [0] * 72])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def net():
    return R.make(0)


@pytest.fixture(scope="module")
def small():
    return R.make(1, **R.SMALL)


def _model(ref_net, dev, **kw):
    from siss_amd.clip_iqa import CLIPIQAModel
    m = CLIPIQAModel(**kw)
    m.load_state_dict(ref_net.state_dict())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model(net, dev):
    return _model(net, dev)


@pytest.fixture(scope="module")
def small_model(small, dev):
    return _model(small, dev, **SMALL_KW)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- average pool
@pytest.mark.parametrize("N, H, W, C", [(2, 4, 4, 32), (1, 9, 5, 64), (3, 2, 2, 2048)])
def test_avgpool_against_f64(dev, N, H, W, C):
    from siss_amd import lib
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(H * W + C))
    ref = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2).double(), 2).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (N, H // 2, W // 2, C)                           # floor: an odd last row / column is dropped
    y = torch.full((N, H // 2, W // 2, C), float("nan"), device=dev)
    lib.call("siss_clipiqa_avgpool", x.to(dev), y, N, H, W, C, 2)
    err = float((y.cpu().double() - ref).abs().max()) / float(x.abs().max())
    print(f"\navgpool [{N}, {H}, {W}, {C}]: {err:.2e} of scale (bound 2^-22 = {2.0 ** -22:.2e})")
    assert err <= 2.0 ** -22
    y2 = torch.full_like(y, float("nan"))
    lib.call("siss_clipiqa_avgpool", x.to(dev), y2, N, H, W, C, 2)
    assert torch.equal(_bits(y), _bits(y2))
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_clipiqa_avgpool", x.to(dev), y, N, H, W, C, max(H, W) + 1)      # a window larger than the map
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_clipiqa_avgpool", x.to(dev), y, N, H, W * C // 6, 6, 2)         # C % 4 != 0


# ---------------------------------------------------------------- attention pooling
E, HEADS, OUT = 2048, 32, 64


def _pool_model(pool, dev):
    """A CLIPIQAModel whose attention pool holds `pool`'s parameters (the trunk is not run)."""
    from siss_amd.clip_iqa import CLIPIQAModel
    m = CLIPIQAModel(**SMALL_KW)
    sd = m.state_dict()
    for k, v in pool.state_dict().items():
        if k != "positional_embedding":
            sd["visual.attnpool." + k] = v
    m.load_state_dict(sd)
    m.to(dev)
    m._pack()
    return m


@pytest.mark.parametrize("biases", [False, True], ids=["zero-biases", "biases"])
@pytest.mark.parametrize("N, H, W", [(1, 1, 1), (2, 2, 2), (3, 3, 2), (2, 16, 16)], ids=["1x1", "2x4", "3x6", "2x256"])
def test_attention_pool_against_the_unfolded_f64_form(dev, N, H, W, biases):
    """The folded form on the kernels against F.multi_head_attention_forward with every token projected through k_proj and v_proj,
    in f64.  q . b_k is the same for every token of a head, so the softmax hides it from the output: the LOGITS are held against
    f64 as well (same convention: 8 x torch's f32 deviation), where a dropped q . b_k is far away.  b_v and b_q show in the output."""
    g = torch.Generator().manual_seed(N * 100 + H * W + int(biases))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        pool = R.AttentionPool2d(7, E, HEADS, OUT)
    with torch.no_grad():
        pool.positional_embedding = torch.nn.Parameter(torch.randn(H * W + 1, E, generator=g) * 0.5)
        for lin in (pool.q_proj, pool.k_proj, pool.v_proj, pool.c_proj):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * E ** -0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.5 if biases else torch.zeros(lin.bias.shape))
    x = torch.relu(torch.randn(N, E, H, W, generator=g) + 0.3)                 # a layer4 map: after a ReLU
    ref = R.attention_pool(pool, x)
    e32 = float((R.attention_pool(pool, x, torch.float32) - ref).abs().max())
    bound = 8 * e32
    m = _pool_model(pool, dev)
    h = x.permute(0, 2, 3, 1).contiguous().to(dev)
    got, logits = m.attention_pool(h, N, H * W, return_logits=True)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"\nattention pool N = {N}, HW = {H * W}, biases {biases}: max|d| {err:.3e}, bound {bound:.3e} (f32 unfolded form {e32:.3e}), "
          f"max|f64| {float(ref.abs().max()):.3e}")
    assert got.shape == (N, OUT) and e32 > 0 and err <= bound
    assert torch.equal(_bits(m.attention_pool(h, N, H * W)), _bits(got))        # the same call, the same bits
    # controls: the positional embedding added; token 1 as the query (on a 1 x 1 map token 1 IS the mean token: no control there)
    away = float((R.attention_pool(_ctl(pool, pos_embedding=True), x) - got.cpu().double()).abs().max())
    print(f"  control positional embedding: {away / bound:.0f} bounds")
    assert away >= 100 * bound
    if H * W > 1:
        away = float((R.attention_pool(_ctl(pool, query_token=1), x) - got.cpu().double()).abs().max())
        print(f"  control query token 1: {away / bound:.0f} bounds")
        assert away >= 100 * bound
    # the logits s[n, h, t] = q_h . k_t / 8 of the unfolded form
    lref, l32 = _logits(pool, x, torch.float64), _logits(pool, x, torch.float32)
    lbound = 8 * float((l32 - lref).abs().max())
    lerr = float((logits.cpu().double() - lref).abs().max())
    print(f"  logits: max|d| {lerr:.3e}, bound {lbound:.3e}, max|f64| {float(lref.abs().max()):.3e}")
    assert logits.shape == (N, HEADS, H * W + 1) and lerr <= lbound
    if biases:                                                                  # what dropping a bias term would give
        for name in ("q_proj", "v_proj") if H * W > 1 else ("v_proj",):         # (one position: both tokens are equal, q is moot)
            away = float((R.attention_pool(_ctl(pool, zero_bias=name), x) - got.cpu().double()).abs().max())
            print(f"  control {name}.bias dropped: {away / bound:.0f} bounds")
            assert away >= 100 * bound
        away = float((_logits(_ctl(pool, zero_bias="k_proj"), x, torch.float64) - logits.cpu().double()).abs().max())
        print(f"  control q . b_k dropped from the logits: {away / lbound:.0f} bounds")
        assert away >= 100 * lbound


def _logits(pool, x, dtype):
    """[N, heads, HW + 1]: the unfolded form's q_h . k_t / sqrt(D), every token through k_proj."""
    import copy
    p = copy.deepcopy(pool).to(dtype)
    with torch.no_grad():
        tok = x.to(dtype).flatten(2).permute(0, 2, 1)
        tok = torch.cat([tok.mean(1, keepdim=True), tok], 1)                    # [N, T, E]
        N, T, _ = tok.shape
        q = p.q_proj(tok[:, :1]).view(N, HEADS, E // HEADS) * (E // HEADS) ** -0.5
        k = p.k_proj(tok).view(N, T, HEADS, E // HEADS)
        return torch.einsum("nhd,nthd->nht", q, k)


def _ctl(pool, pos_embedding=False, query_token=0, zero_bias=None):
    import copy
    p = copy.deepcopy(pool)
    p.pos_embedding, p.query_token = pos_embedding, query_token
    if zero_bias:
        with torch.no_grad():
            getattr(p, zero_bias).bias.zero_()
    return p


# ---------------------------------------------------------------- score kernel
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("D", [64, 1024])
def test_score_kernel_against_f64(dev, D, P):
    from siss_amd import lib
    g = torch.Generator().manual_seed(D + P)
    a = torch.nn.functional.normalize(torch.randn(2 * P, D, generator=g).double(), dim=1).float()
    f = torch.randn(6, D, generator=g) * torch.tensor([1.0, 30.0, 1e-3, 1.0, 1.0, 1.0]).view(6, 1)
    f[3] = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0) * 1e-20        # a row of norm 1e-20
    d = a[0].double() - a[1].double()
    f[4], f[5] = (d / d.norm() * 5).float(), (-d / d.norm() * 5).float()                    # the first pair's logit gap: far out
    ref = R.score(f.double(), a.double())
    gap = 100 * (f[4:6].double() / f[4:6].double().norm(dim=1, keepdim=True)) @ d
    assert float(gap[0]) >= 100 and float(gap[1]) <= -100 and float(f[3].double().norm()) == pytest.approx(1e-20, rel=1e-3)
    out = torch.full((6, P), float("nan"), device=dev)
    lib.call("siss_clipiqa_score", f.to(dev), a.to(dev), 6, D, P, out)
    got = out.cpu().double()
    err = float((got - ref).abs().max())
    print(f"\nscore D = {D}, P = {P}: max|d| {err:.2e} (bound 2^-23 = {2.0 ** -23:.2e}); saturated {got[4, 0]:.3e} / {got[5, 0]:.3e}")
    assert torch.isfinite(got).all() and err <= 2.0 ** -23
    assert float(got[4, 0]) == 1.0 and 0.0 <= float(got[5, 0]) <= 1e-40 and float(got.min()) >= 0 and float(got.max()) <= 1
    out2 = torch.full((6, P), float("nan"), device=dev)
    lib.call("siss_clipiqa_score", f.to(dev), a.to(dev), 6, D, P, out2)
    assert torch.equal(_bits(out), _bits(out2))
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_clipiqa_score", f.to(dev), a.to(dev), 6, D, 0, out)


# ---------------------------------------------------------------- the whole image tower and the score
def _images(shape, seed):
    n, _, h, w = shape
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, R.normalise(u8)


def _against_f64(ref_net, m, dev, shape, seed, anc, f64_device="cpu"):
    u8, x = _images(shape, seed)
    ref = R.embed(ref_net, x, torch.float64, f64_device).cpu()
    r32 = R.embed(ref_net, x, torch.float32)
    e32 = float((r32 - ref).abs().max())
    sref = R.score(ref, anc)
    s32 = float((R.score(r32.double(), anc) - sref).abs().max())
    bound, sbound = 8 * e32, 8 * s32
    got, scores = m(x.to(dev), anchors=anc.float().to(dev))
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda and scores.shape == sref.shape
    err, serr = float((got.cpu().double() - ref).abs().max()), float((scores.cpu().double() - sref).abs().max())
    print(f"\nCLIP image tower {shape}: rows max|d| {err:.3e}, bound {bound:.3e} (f32 restatement {e32:.3e}), max|f64| "
          f"{float(ref.abs().max()):.3e}; scores max|d| {serr:.3e}, bound {sbound:.3e} (f32 restatement {s32:.3e})")
    assert e32 > 0 and err <= bound
    assert serr <= sbound
    again = m(x.to(dev), anchors=anc.float().to(dev))
    assert torch.equal(_bits(again[0]), _bits(got)) and torch.equal(_bits(again[1]), _bits(scores))
    return u8, x, ref, got, scores, bound


def _controls(ref_net, x, ref, got, bound, even):
    ctls = [("max pools", R.variant(ref_net, maxpool=True)), ("BN statistics reset", R.reset_bn(ref_net))]
    if even:             # (a strided 3 x 3 rounds an odd map up, the pool of the shortcut down: a network only where every map is even)
        ctls.append(("stride on conv2", R.variant(ref_net, stride_on_conv2=True)))
    for name, ctl in ctls:
        c = R.embed(ctl, x)
        away, away_gpu = float((c - ref).abs().max()), float((c - got.cpu().double()).abs().max())
        print(f"  control {name}: {away / bound:.0f} bounds from the restatement, {away_gpu / bound:.0f} from the GPU")
        assert away >= 100 * bound and away_gpu >= 100 * bound


@pytest.mark.parametrize("shape", [(3, 3, 32, 32), (2, 3, 64, 64), (2, 3, 72, 40)], ids=["3x32x32", "2x64x64", "2x72x40"])
def test_small_network_against_the_f64_restatement(dev, small, small_model, shape):
    """Layers (1, 1, 1, 1), width 64, output 64: a 1 x 1 final map, a 2 x 2 one, and 72 x 40 whose maps 9 x 5 and 4 x 2 floor."""
    anc = R.anchors(small, IDS)
    u8, x, ref, got, scores, bound = _against_f64(small, small_model, dev, shape, shape[2], anc)
    _controls(small, x, ref, got, bound, even=shape[2] % 32 == 0 and shape[3] % 32 == 0)
    assert small_model._shapes(1, shape[2], shape[3])[0] == (shape[2] // 32, shape[3] // 32)
    # chunks of one image give the same bits; so do the bytes through the fused preprocessing
    one = _model(small, dev, **{**SMALL_KW, "batch_size": 1})
    rows1, scores1 = one(x.to(dev), anchors=anc.float().to(dev))
    assert torch.equal(_bits(rows1), _bits(got)) and torch.equal(_bits(scores1), _bits(scores))
    assert torch.equal(_bits(small_model.embed_u8(u8.to(dev))), _bits(got))
    assert torch.equal(_bits(small_model.scores_u8(u8.to(dev), anc.float().to(dev))), _bits(scores))


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 96, 64)], ids=["2x64x64", "1x96x64"])
def test_rn50_against_the_f64_restatement(dev, net, model, shape):
    anc = torch.nn.functional.normalize(torch.randn(2, 1024, generator=torch.Generator().manual_seed(3)).double(), dim=1)
    u8, x, ref, got, scores, bound = _against_f64(net, model, dev, shape, shape[2], anc)
    _controls(net, x, ref, got, bound, even=True)
    one = _model(net, dev, batch_size=1)
    rows1, scores1 = one(x.to(dev), anchors=anc.float().to(dev))
    assert torch.equal(_bits(rows1), _bits(got)) and torch.equal(_bits(scores1), _bits(scores))


# ---------------------------------------------------------------- anchors on the device
def _anchors_against_f64(ref_net, m, ids):
    ref = R.anchors(ref_net, ids)
    got = m.anchors(ids)
    err = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print(f"\nanchors {tuple(ids.shape)}: {err:.2e} of scale (the f32 instrument's bound 1e-4)")
    assert got.shape == ref.shape and got.dtype == torch.float32 and err <= 1e-4
    assert float((got.cpu().double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert m.anchors(ids) is got                                                # computed once per set of ids
    return got


def test_anchors_of_the_f32_text_tower(dev, net, small, model, small_model):
    from siss_amd import lib
    got = _anchors_against_f64(small, small_model, IDS)
    padded = IDS.clone()
    padded[padded == 0] = EOT                                                   # a CLIP tokenizer's padding: the same anchors
    assert float((small_model.anchors(padded) - got).abs().max()) <= 1e-6
    _anchors_against_f64(net, model, FULL_IDS)                                  # the full 12 x 512 tower, 77 positions
    assert not lib.in_f32_mode()
    # the image scores of the metric's own surface: one prompt a vector, several a dict by name
    from siss_amd.clip_iqa import CLIPImageQualityAssessment
    u8, x = _images((2, 3, 32, 32), 5)
    imgs = (u8.permute(0, 3, 1, 2).float() / 255).to(dev)
    q = CLIPImageQualityAssessment(model=small_model, prompt_ids=IDS[:2])
    want = R.score(R.embed(small, x), R.anchors(small, IDS))
    v = q(imgs)
    assert v.shape == (2,) and float((v.cpu().double() - want[:, 0]).abs().max()) <= 1e-4
    assert torch.equal(_bits(v), _bits(small_model.scores_u8(u8.to(dev), small_model.anchors(IDS[:2]))[:, 0]))
    q.update(imgs * 1.0)
    assert q.compute().shape == (4,)
    q.reset()
    q2 = CLIPImageQualityAssessment(model=small_model, prompts=("quality", ("a", "b")), prompt_ids=IDS, data_range=255.0)
    d = q2(imgs * 255)
    assert set(d) == {"quality", "user_defined_0"} and float((d["user_defined_0"].cpu().double() - want[:, 1]).abs().max()) <= 1e-4


def _forward_as_it_was(enc, input_ids):
    """CLIPTextEncoder.__call__ before it had a dtype: the bf16 launch sequence, written out on the encoder's own operands."""
    from siss_amd import lib, ops
    up = lambda n, m: -(-n // m) * m
    ids = input_ids.to(enc.device)
    B, S = ids.shape
    C, Hh = enc.C, enc.heads
    D = C // Hh
    Dp, Sp = up(D, 64), up(S, 64)
    rows, BH = B * S, B * Hh
    bb = lambda shape, dt=torch.bfloat16: torch.zeros(shape, dtype=dt, device=enc.device)
    x, y, h = bb((rows, C)), bb((rows, C)), bb((rows, C))
    x.copy_((enc.tok[ids] + enc.pos[:S]).reshape(rows, C))
    q, k, v = bb((rows, C)), bb((rows, C)), bb((rows, C))
    qh, kh, vh = bb((BH, Sp, Dp)), bb((BH, Sp, Dp)), bb((BH, Sp, Dp))
    vT, sc, p = bb((BH, Dp, Sp)), bb((BH, Sp, Sp)), bb((BH, Sp, Sp))
    oh, o, f1 = bb((BH, Sp, Dp)), bb((rows, C)), bb((rows, enc.inner))
    mean, rstd = bb((rows,), torch.float32), bb((rows,), torch.float32)

    def linear(a, name, out, n_out, k_in, residual=None):
        ops.gemm_nt(lib.ptr(a), k_in, enc.w[name + ".weight"], lib.ptr(out), n_out, rows, n_out, k_in, [0], [0],
                    bias=enc.f[name + ".bias"], res_ptr=lib.ptr(residual) if residual is not None else None, ldr=n_out)

    def ln(a, name, out):
        lib.call("siss_layernorm_fwd", a, enc.f[name + ".weight"], enc.f[name + ".bias"], out, mean, rstd, rows, C, enc.eps)
    for i in range(enc.n_layers):
        pre = f"encoder.layers.{i}"
        ln(x, pre + ".layer_norm1", h)
        for nm, dst, hd in (("q_proj", q, qh), ("k_proj", k, kh), ("v_proj", v, vh)):
            linear(h, f"{pre}.self_attn.{nm}", dst, C, C)
            lib.call("siss_head_split", dst, hd, B, S, Hh, D, Sp, Dp)
        lib.call("siss_transpose_bf16", vh, vT, BH, Sp, Dp)
        ops.gemm_nt(lib.ptr(qh), Dp, kh, lib.ptr(sc), Sp, Sp, Sp, Dp, [0], [0], alpha=D ** -0.5, batch=BH,
                    stride_a=Sp * Dp, stride_w=Sp * Dp, stride_c=Sp * Sp)
        lib.call("siss_softmax_rows_fwd", sc, p, BH * Sp, S, Sp, Sp)
        ops.gemm_nt(lib.ptr(p), Sp, vT, lib.ptr(oh), Dp, Sp, Dp, Sp, [0], [0], batch=BH,
                    stride_a=Sp * Sp, stride_w=Dp * Sp, stride_c=Sp * Dp)
        lib.call("siss_head_merge", oh, o, B, S, Hh, D, Sp, Dp)
        linear(o, pre + ".self_attn.out_proj", y, C, C, residual=x)
        ln(y, pre + ".layer_norm2", h)
        linear(h, pre + ".mlp.fc1", f1, enc.inner, C)
        lib.call("siss_quick_gelu", f1, f1, f1.numel())
        linear(f1, pre + ".mlp.fc2", x, C, enc.inner, residual=y)
    ln(x, "final_layer_norm", h)
    return h.float().view(B, S, C).clone()


def test_default_text_encoder_is_bitwise_what_it_was(dev, small):
    from siss_amd.clip_iqa import text_encoder_state
    from siss_amd.text_encoder import CLIPTextEncoder
    enc = CLIPTextEncoder(text_encoder_state(small.state_dict(), 2), 2, 1e-5, dev)
    assert enc.dtype == torch.bfloat16 and all(w.dtype == torch.bfloat16 for w in enc.w.values())
    got = enc(IDS)[0]
    want = _forward_as_it_was(enc, IDS)
    assert got.dtype == torch.float32 and torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    f32 = CLIPTextEncoder(text_encoder_state(small.state_dict(), 2), 2, 1e-5, dev, dtype=torch.float32)
    assert all(w.dtype == torch.float32 for w in f32.w.values())
    d = float((f32(IDS)[0] - got).abs().max())
    assert 0 < d <= 0.25                                                         # (bf16 against f32: close, and not the same path)
    with pytest.raises(TypeError, match="bfloat16 or torch.float32"):
        CLIPTextEncoder(text_encoder_state(small.state_dict(), 2), 2, 1e-5, dev, dtype=torch.float16)


# ---------------------------------------------------------------- full size
def test_full_size_images_from_both_source_forms(dev, net, model):
    """n = 2 at 3 x 512 x 512, the size the reference feeds (T = 257 tokens): from uint8, and from a bf16 decoder output."""
    from siss_amd.kmeans import KMeansClassifier
    shape = (2, 3, 512, 512)
    anc = torch.nn.functional.normalize(torch.randn(2, 1024, generator=torch.Generator().manual_seed(4)).double(), dim=1)
    u8, x, ref, got, scores, bound = _against_f64(net, model, dev, shape, 512, anc, f64_device=dev)
    a = anc.float().to(dev)
    assert torch.equal(_bits(model.scores_u8(u8.to(dev), a)), _bits(scores))
    dec = (torch.rand(shape, generator=torch.Generator().manual_seed(6)) * 2.4 - 1.2).to(dev).to(torch.bfloat16)
    s_dec, bytes_ = model.scores_decoded(dec, a)
    km = KMeansClassifier(np.zeros((2, 3 * 512 * 512), np.float32))
    assert torch.equal(bytes_, km.from_decoded(dec)[0])                          # the k-means classifier's bytes, bit for bit
    assert int(bytes_.min()) == 0 and int(bytes_.max()) == 255
    assert torch.equal(_bits(s_dec), _bits(model.scores_u8(bytes_, a)))          # the two source forms: the same scores
    rows_dec, bytes2 = model.embed_decoded(dec)
    assert torch.equal(bytes2, bytes_) and torch.equal(_bits(rows_dec), _bits(model.embed_u8(bytes_)))
    assert model.max_elements(1, 512, 512) == 256 * 256 * 64 and model.max_elements(16, 512, 512) < 1 << 31
    with pytest.raises(ValueError, match="2\\^31"):
        model._features(torch.empty(1024, 3, 512, 512, device="meta"))


def test_loader_round_trip(dev, small, small_model, tmp_path):
    from siss_amd.clip_iqa import CLIPIQAModel
    torch.jit.script(small).save(str(tmp_path / "clip.torchscript.pt"))
    loaded = CLIPIQAModel.load(tmp_path / "clip.torchscript.pt").to(dev)
    _, x = _images((2, 3, 64, 48), seed=3)
    assert torch.equal(_bits(loaded(x.to(dev))), _bits(small_model(x.to(dev))))
    assert torch.equal(_bits(loaded.anchors(IDS)), _bits(small_model.anchors(IDS)))


# ---------------------------------------------------------------- DeleteSD
def _crop(path, k, size=32, cols=1, pad=2):
    from PIL import Image
    a = np.asarray(Image.open(path))
    r, q = divmod(k, cols)
    return a[r * (size + pad) + pad:r * (size + pad) + pad + size, q * (size + pad) + pad:q * (size + pad) + pad + size]


def test_delete_sd_clip_iqa_end_to_end(dev, tmp_path):
    from PIL import Image
    from test_hip_sd_sampling import _run, _tiny_checkpoint
    from siss_amd import lib
    from siss_amd.clip_iqa import CLIPImageQualityAssessment
    from siss_amd.kmeans import KMeansClassifier
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    torch.save(FULL_IDS, tmp_path / "iqa_ids.pt")
    prompt = str(tmp_path / "prompt_ids.pt")
    evals = ["training_steps=1", "eval_every=1", "+eval_batches=2", "+eval_batch_size=1", "+pipeline.num_inference_steps=2", "resolution=32"]
    iqa = [f"metrics.clip_iqa.model_path={tmp_path}/RN50.pt", "metrics.clip_iqa.allow_random_init=true",
           f"metrics.clip_iqa.prompt_ids_path={tmp_path}/iqa_ids.pt"]

    def hook(task):
        inner = task.evaluate

        def evaluate(unet, sched, forget_image, step, device):
            e = unet.engine
            torch.cuda.synchronize()
            flat, shadow = e.ps.flat.clone(), e.ps.shadow.clone()
            inner(unet, sched, forget_image, step, device)
            torch.cuda.synchronize()
            assert torch.equal(e.ps.flat, flat) and torch.equal(e.ps.shadow, shadow)      # evaluation only reads the weights
        task.evaluate = evaluate

    task, _, cfg = _run(tmp_path, "iqa", ckpt, evals + iqa, prompt, hook)
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))]
    print("\nclip_iqa", lines)
    assert [r["global_step"] for r in lines] == [1] and all(set(r) == {"global_step", "clip_iqa_0"} for r in lines)
    # the recorded value is the metric's own value on the tiles of the written grid
    metric = CLIPImageQualityAssessment(model=task.clip_iqa.model, prompt_ids=FULL_IDS)
    for r in lines:
        v = r["clip_iqa_0"]
        assert isinstance(v, float) and 0.0 <= v <= 1.0
        path = os.path.join(cfg.output_dir, f"validation_p0_step{r['global_step']}.png")
        tiles = torch.from_numpy(np.stack([_crop(path, k) for k in (0, 1)]).copy())
        imgs = tiles.permute(0, 3, 1, 2).float() / 255                           # ToTensor on the host: a true division
        again = float(torch.cat([metric(imgs[k:k + 1].to(dev)) for k in (0, 1)]).cpu().double().mean())
        print(f"  step {r['global_step']}: recorded {v:.9f}, the metric on the grid's images {again:.9f}")
        assert abs(v - again) <= 1e-6
    # with the k-means fraction and SSCD on as well: three records per step, and the three metrics see the same bytes
    Image.fromarray(torch.randint(0, 256, (32, 32, 3), generator=g, dtype=torch.uint8).numpy()).save(str(tmp_path / "mem.png"))
    own = _crop(os.path.join(cfg.output_dir, "validation_p0_step1.png"), 0).reshape(-1).astype(np.float32)
    KMeansClassifier(np.stack([np.where(own < 128, 255.0, 0.0).astype(np.float32), own])).save(str(tmp_path / "km.npz"))
    others = [f"metrics.fraction_deletion.classifier_path={tmp_path}/km.npz", f"metrics.sscd.model_path={tmp_path}/sscd.pt",
              "metrics.sscd.allow_random_init=true", f"data_files.mem_img_path={tmp_path}/mem.png"]
    seen = {"kmeans": [], "sscd": [], "clip_iqa": []}

    def spy(task):
        hook(task)
        inner = task.evaluate

        def evaluate(*a):                            # (the trackers are built by run(), after this hook: wrap them at the evaluation)
            fused, s_u8, c_u8 = task.kmeans.from_decoded, task.sscd.score_u8, task.clip_iqa.score_u8

            def from_decoded(img):
                out = fused(img)
                seen["kmeans"].append(out[0].clone())
                return out
            task.kmeans.from_decoded = from_decoded
            task.sscd.score_u8 = lambda u8: (seen["sscd"].append(u8.clone()), s_u8(u8))[1]
            task.clip_iqa.score_u8 = lambda u8: (seen["clip_iqa"].append(u8.clone()), c_u8(u8))[1]
            try:
                inner(*a)
            finally:
                task.kmeans.from_decoded, task.sscd.score_u8, task.clip_iqa.score_u8 = fused, s_u8, c_u8
        task.evaluate = evaluate

    _, _, cfg_b = _run(tmp_path, "all", ckpt, evals + iqa + others, prompt, spy)
    both = [json.loads(l) for l in open(os.path.join(cfg_b.output_dir, "metrics_rank0.jsonl"))]
    print("  all three", both)
    assert len(seen["kmeans"]) == len(seen["sscd"]) == len(seen["clip_iqa"]) == 2
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(seen["kmeans"], seen["sscd"], seen["clip_iqa"]))
    for key in ("deletion_fraction_0", "sscd_0", "clip_iqa_0"):
        assert [r["global_step"] for r in both if key in r] == [1], key
    assert all(0.0 <= r["clip_iqa_0"] <= 1.0 for r in both if "clip_iqa_0" in r)
    # refused before the first step, with what is missing in the message
    with pytest.raises(FileNotFoundError, match="prompt_ids_path.*tokenizer_path"):
        _run(tmp_path, "bad", ckpt, ["training_steps=1"] + iqa[:2], prompt)
    assert not os.path.exists(os.path.join(str(tmp_path), "bad", "train_log_rank0.jsonl"))
    assert lib.PROF is None

"""siss_groupnorm_bwd_sc: the backward of a width-changing resnet's norm1 with the 1x1 conv_shortcut's dgrad (dout . W_sc) formed in the
same launch as the apply pass (the product's epilogue), against the composition it replaces -- siss_gemm_nt (one panel, halo mask) writing the [rows x C]
cotangent, then siss_groupnorm_bwd_ld / _s2d (two-pass kernels) reading it back as `accum`.  Reference provider: diffusers'
ResnetBlock2D (norm1 + conv_shortcut) differentiated at delete_celeb.py:691,:702.

The fused K loop accumulates in the generic NT kernel's order, rounds the product to bf16 where the stored tensor was rounded and adds
in the apply kernel's order, so wherever the reference product does not split K the two dx are THE SAME BITS.  The generic kernel
splits K only for K loops of at least 12 steps (K >= 768); every case here has K <= 128, so every case asserts that the split-K
counter stayed 0 and that dx is bitwise equal.  dgamma / dbeta come from the same statistics kernel through float atomics: compared at
the tolerance tests/test_hip_groupnorm.py uses for them (5e-3 of scale).
"""
import pytest
import torch

from test_hip_groupnorm import G, _bf, _close, _run_fwd, dev  # noqa: F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu

CASES = {
    # rows_per_image 64: a 128-row tile spans images (three when it starts inside one); cpg 3: a 16-B chunk spans groups; ragged column tile
    "a_6x6_c96": dict(B=2, H=6, W=6, C=96, K=64),
    # ... and with three saved samples the rows of a set (192) are no multiple of the tile
    "a2_6x6_c96_b3": dict(B=3, H=6, W=6, C=96, K=64),
    "b_40x48_c384_s2d": dict(B=1, H=40, W=48, C=384, K=128, split=256, s2d=True),
    "c_64x64_c256_split_acc": dict(B=2, H=64, W=64, C=256, K=128, split=128, accb=True, acc2=True, ld_extra=64),
    "d_90x90_c256": dict(B=2, H=90, W=90, C=256, K=128),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_fused_shortcut_dgrad_equals_product_then_groupnorm_backward(dev, case):
    from siss_amd import lib, ops
    from siss_amd.layout import Act
    c = CASES[case]
    B, H, W, C, K = c["B"], c["H"], c["W"], c["C"], c["K"]
    split, s2d, accb, acc2, ld_extra = c.get("split", 0), c.get("s2d", False), c.get("accb", False), c.get("acc2", False), c.get("ld_extra", 0)
    sets, nsets, eps, silu = 2, 2, 1e-6, True
    n2 = sets * B
    g = torch.Generator().manual_seed(C + H + K + B)
    x = _bf(torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = _bf(torch.randn(n2, C, H, W, generator=g))
    dout = _bf(torch.randn(n2, K, H, W, generator=g))
    wT = (torch.randn(1, C, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)          # the dgrad copy: [1][Cin][Cout]
    r2 = _bf(torch.randn(n2, C, H, W, generator=g)) if acc2 else None
    r3 = _bf(torch.randn(n2, C - split, H, W, generator=g)) if split else None
    part = torch.zeros(lib.query("siss_gn_partial_words", n2, H, W, C, G), device=dev)
    gconst = torch.zeros(n2 * G * 4, device=dev)
    xa, ldxv, _, _, _, (mean, rstd) = _run_fwd(lib, dev, x, gamma, beta, eps, silu, False, ld_extra, part)
    assert ldxv == (C + ld_extra if ld_extra else 0)
    dya, douta = Act.from_nchw(dy, dev), Act.from_nchw(dout, dev)
    a2 = Act.from_nchw(r2, dev) if acc2 else None
    gm, bt = gamma.to(dev), beta.to(dev)
    P = 4096

    def targets(junk):
        if split:
            da = Act(n2, H // 2, W // 2, 4 * split, dev) if s2d else Act(n2, H, W, split, dev)
            db = Act.from_nchw(r3, dev) if accb else Act(n2, H, W, C - split, dev)
            fill = [] if not junk else ([da] if not s2d else []) + ([] if accb else [db])
        else:
            da, db = Act(n2, H, W, C, dev), None
            fill = [da] if junk else []
        for a in fill:                     # the fused launch must write every row of its targets, the halo rows as zeros
            a.data.fill_(3.0)
        return da, db

    assert lib.query("siss_groupnorm_set_slab", 0) == 0
    try:
        # ---- the composition that exists
        lib.dispatch_counts(reset=True)
        acc = Act(n2, H, W, C, dev)
        ops.conv_dgrad(douta, wT, acc, ksize=1)
        counts = lib.dispatch_counts()
        assert counts["gemm_nt_kernel"] == 1 and counts["gemm_nt_kernel/splitk"] == 0
        da0, db0 = targets(False)
        g0 = torch.zeros(nsets, P, device=dev)
        lib.call("siss_groupnorm_bwd_ld_s2d" if s2d else "siss_groupnorm_bwd_ld", dya.data, xa.data, gm, bt, mean, rstd, da0.data,
                 acc.data, a2.data if acc2 else None, db0.data if split else None, split, int(accb), g0[0, 64:], g0[0, 2048:],
                 None, 0, part, n2, B, n2 // nsets, P, H, W, C, G, int(silu), 0, ldxv)
        torch.cuda.synchronize()
        # ---- the fused launch
        lib.dispatch_counts(reset=True)
        da1, db1 = targets(True)
        g1 = torch.zeros(nsets, P, device=dev)
        lib.call("siss_groupnorm_bwd_sc", dya.data, xa.data, gm, bt, mean, rstd, da1.data, douta.data, K, wT[0], K,
                 a2.data if acc2 else None, db1.data if split else None, split, int(accb), g1[0, 64:], g1[0, 2048:], None, part,
                 gconst, n2, B, n2 // nsets, P, H, W, C, G, int(silu), int(s2d), ldxv)
        torch.cuda.synchronize()
        counts = lib.dispatch_counts()
        assert counts["gn_bwd_sc_kernel"] == 1 and counts["gemm_nt_kernel"] == 0 and counts["gn_slab"] == 0
    finally:
        lib.query("siss_groupnorm_set_slab", -1)
    assert da1.halo_is_zero() and (db1 is None or db1.halo_is_zero())
    assert float(da0.buf.float().abs().max()) > 0
    assert torch.equal(da0.buf, da1.buf), "dx (first part)"
    if split:
        assert torch.equal(db0.buf, db1.buf), "dx2"
    for k in range(nsets):
        _close(g1[k, 64:64 + C].cpu(), g0[k, 64:64 + C].cpu(), 5e-3, f"dgamma set {k}")
        _close(g1[k, 2048:2048 + C].cpu(), g0[k, 2048:2048 + C].cpu(), 5e-3, f"dbeta set {k}")


def test_fused_launcher_refuses_column_sums_and_bad_shapes(dev):
    """colsum is not supported (norm1 never asks for it): SISS_ERR_ARG, nothing launched; so is a K that is no multiple of 64."""
    from siss_amd import lib
    from siss_amd.layout import Act
    B, H, W, C, K = 1, 6, 6, 64, 64
    x, dy, dout, dx = (Act(n, H, W, ch, dev) for n, ch in ((B, C), (2 * B, C), (2 * B, K), (2 * B, C)))
    f = lambda n: torch.zeros(n, device=dev)
    wT = torch.zeros(C, K, dtype=torch.bfloat16, device=dev)
    part = f(lib.query("siss_gn_partial_words", 2 * B, H, W, C, G))
    args = lambda colsum, k: (dy.data, x.data, f(C), f(C), f(B * G), f(B * G), dx.data, dout.data, K, wT, k, None, None, 0, 0, f(2 * C), f(2 * C),
                              colsum, part, f(2 * B * G * 4), 2 * B, B, B, C, H, W, C, G, 1, 0, 0)
    lib.dispatch_counts(reset=True)
    assert lib.call("siss_groupnorm_bwd_sc", *args(f(2 * B * C), K), refusable=True) == 1
    assert lib.call("siss_groupnorm_bwd_sc", *args(None, 32), refusable=True) == 1
    assert lib.dispatch_counts()["gn_bwd_sc_kernel"] == 0
    assert lib.call("siss_groupnorm_bwd_sc", *args(None, K)) == 0
    torch.cuda.synchronize()
    assert lib.dispatch_counts()["gn_bwd_sc_kernel"] == 1


# ---------------------------------------------------------------- the engine
KW = dict(sample_size=128, in_channels=3, out_channels=3, block_out_channels=(128, 128, 256),
          down_block_types=("DownBlock2D", "DownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "UpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)


def _grads_agree(ga, gb, what):
    for s in range(2):
        a, b = ga[s].double(), gb[s].double()
        assert float((a * b).sum() / (a.norm() * b.norm())) >= 0.999, (what, s)
        assert abs(float(a.norm() / b.norm()) - 1) < 1e-2, (what, s)


@pytest.fixture(scope="module")
def engine_runs():
    """The 128 x 128 network of test_folded_shortcut_equals_the_separate_1x1_product with sc_in_gn_min_px lowered to its top
    resolution, nsets 2: one eager forward + backward with the switch off and one with it on, the `on` engine kept for the replay."""
    from siss_amd import lib
    from siss_amd.config import UNet2DConfig
    from siss_amd.unet import UNetEngine
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 3, 128, 128, generator=g).cuda()
    t = torch.tensor([999, 400]).cuda()
    cot = (torch.randn(4, 3, 128, 128, generator=g) * 1e-2).cuda()
    outs = {}
    for on in (False, True):
        eng = UNetEngine(UNet2DConfig(**KW), "cuda:0")
        eng.init_random(seed=4)
        assert eng.sc_in_gn_min_px == 65536
        eng.sc_in_gn, eng.sc_in_gn_min_px = on, 16384
        calls = []
        orig = lib.call
        lib.call = lambda name, *a, _o=orig, _c=calls, **k: (_c.append(name), _o(name, *a, **k))[1]
        try:
            pred = eng.forward(x, t).clone()
            eng.zero_grad()
            eng.backward(cot, nsets=2)
            torch.cuda.synchronize()
        finally:
            lib.call = orig
        outs[on] = (pred, eng.ps.grads.clone(), calls, eng)
    return outs, (x, t, cot)


def test_engine_takes_the_fused_launcher_at_the_sites_over_the_threshold(engine_runs):
    outs, _ = engine_runs
    on, off = outs[True][2], outs[False][2]
    # the two 128 x 128 up resnets (256 -> 128 channels): the fused launcher instead of the fold into conv2's dgrad
    assert on.count("siss_groupnorm_bwd_sc") == 2 and on.count("siss_conv3x3_dgrad_sc") == 0
    assert off.count("siss_groupnorm_bwd_sc") == 0 and off.count("siss_conv3x3_dgrad_sc") == 2
    assert on.count("siss_conv3x3_sc") == 2                     # the forward fold stays
    assert torch.equal(outs[True][0], outs[False][0]), "prediction"
    _grads_agree(outs[True][1], outs[False][1], "on / off")


def test_engine_backward_with_the_fused_launcher_replays_from_a_graph(engine_runs):
    """A pass (forward, gradient fill, backward) with the switch on captured into a hipGraph on the default queues and replayed
    twice: the eager gradients at the same bounds both times.  Nothing in the captured path synchronises with the host (a capture
    that did would fail)."""
    outs, (x, t, cot) = engine_runs
    eng, eager = outs[True][3], outs[True][1]

    def run():
        eng.forward(x, t)
        eng.zero_grad()
        eng.backward(cot, nsets=2)
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        run()                                                   # warm-up on the capture stream: every buffer of the pass exists
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            run()
    torch.cuda.current_stream().wait_stream(cap)
    for _ in range(2):
        eng.ps.grads.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        _grads_agree(eng.ps.grads, eager, "replay / eager")

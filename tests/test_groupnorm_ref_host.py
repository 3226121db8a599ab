"""tests/groupnorm_ref.py against torch (no GPU): the reference equals torch's f64 group_norm (+ silu) and its autograd; the restated
launch shapes equal the library's; the budget ACCEPTS an honest f32 evaluation (torch's f32 group_norm / autograd, outputs rounded to
bf16) on every case of the GPU tables of tests/test_hip_groupnorm_exact.py and REJECTS mutants of the reference -- the mistakes a
GroupNorm kernel of this layout can make -- on the cases where each applies.  Reference against reference: no GPU result sets anything.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as R

F64, G = torch.float64, R.G32
ALL_FWD = R.FWD_CASES + R.QS_CASES
ids = lambda cases: [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# the reference is torch's operation
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("B,C,H,W", [(2, 320, 5, 7), (3, 128, 6, 6), (2, 1920, 3, 2)])
def test_forward_equals_torch_f64(B, C, H, W, silu):
    g = torch.Generator().manual_seed(C + H)
    x = R.bf(torch.randn(B, C, H, W, generator=g, dtype=F64) * 1.5 + 0.3)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g, dtype=F64), 0.1 * torch.randn(C, generator=g, dtype=F64)
    f = R.forward(x, gamma, beta, 1e-5, G, silu)
    ref = F.group_norm(x, G, gamma, beta, 1e-5)
    ref = F.silu(ref) if silu else ref
    xg = x.view(B, G, -1)
    assert _rel(f["y"], ref) <= 1e-12
    assert _rel(f["mean"], xg.mean(-1)) <= 1e-12 and _rel(f["rstd"], (xg.var(-1, unbiased=False) + 1e-5).rsqrt()) <= 1e-12
    assert (f["S"] >= f["z"].abs() * (1 - 1e-12)).all(), "S bounds |z|: it is the sum of the absolute values of z's terms"


def _torch_backward(x, gamma, beta, eps, silu, dy, nx, set_images, dtype=F64):
    """dx per cotangent sample (x index n2 % nx), dgamma / dbeta per set (n2 // set_images), from torch's autograd."""
    xr, gr, br = (v.to(dtype).clone().requires_grad_(True) for v in (x, gamma, beta))
    y = F.group_norm(xr, G, gr, br, eps)
    y = F.silu(y) if silu else y
    n2, C = dy.shape[0], dy.shape[1]
    nsets = n2 // set_images
    dx = torch.zeros(dy.shape, dtype=dtype)
    dg, db = torch.zeros(nsets, C, dtype=dtype), torch.zeros(nsets, C, dtype=dtype)
    for i in range(n2):
        cot = torch.zeros_like(y)
        cot[i % nx] = dy[i].to(dtype)
        gx, gg, gb = torch.autograd.grad(y, (xr, gr, br), cot, retain_graph=True)
        dx[i] = gx[i % nx]
        dg[i // set_images] += gg; db[i // set_images] += gb
    return dx, dg, db


@pytest.mark.parametrize("name,B,sets,set_images,C,H,W,silu,split", [
    ("two sets", 2, 2, 2, 320, 5, 7, True, 0), ("one set", 3, 1, 3, 128, 4, 4, False, 0),
    ("No-IS: 2B saved samples, the set from the sample index", 4, 1, 2, 128, 4, 4, True, 0),
    ("split, accumulating", 2, 2, 2, 1920, 2, 3, True, 1280)])
def test_backward_equals_torch_f64_autograd(name, B, sets, set_images, C, H, W, silu, split):
    g = torch.Generator().manual_seed(C + H)
    rnd = lambda *s: R.bf(torch.randn(*s, generator=g, dtype=F64))
    x = rnd(B, C, H, W) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g, dtype=F64), 0.1 * torch.randn(C, generator=g, dtype=F64)
    n2 = sets * B
    dy, a1, a2 = rnd(n2, C, H, W), rnd(n2, C, H, W), rnd(n2, C, H, W)
    old2 = rnd(n2, C - split, H, W) if split else None
    b = R.backward(x, gamma, beta, 1e-5, G, silu, dy, B, set_images, a1, a2, old2, split)
    dx, dg, db = _torch_backward(x, gamma, beta, 1e-5, silu, dy, B, set_images)
    assert _rel(b["t"], dx) <= 1e-12 and _rel(b["dgamma"], dg) <= 1e-12 and _rel(b["dbeta"], db) <= 1e-12
    assert _rel(b["colsum"], dx.sum((2, 3))) <= 1e-10          # (sums of cancelling terms: relative to the largest entry)
    tot = dx + a1 + a2
    if split:
        tot[:, split:] += old2
        assert torch.equal(b["first"], b["total"][:, :split]) and torch.equal(b["second"], b["total"][:, split:])
    assert _rel(b["total"], tot) <= 1e-12
    assert (b["Stot"] >= b["total"].abs() * (1 - 1e-12)).all() and (b["A_colsum"] >= b["colsum"].abs() * (1 - 1e-12)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the restated launch shapes
def test_partial_words_equal_the_library():
    from siss_amd import lib
    from siss_amd.build import build
    build(verbose=False)                      # hipcc cross-compiles without a GPU, and the query is host code (tests/test_host_logic.py does the same)
    lib.load()
    shapes ={(c.H, c.W, c.C) for c in ALL_FWD + R.BWD_CASES}
    shapes |= {(h, w, c) for h in (1, 3, 16, 33, 64, 100, 256) for w in (1, 7, 64, 256) for c in range(32, 2561, 32) if c % 8 == 0}
    for (h, w, c) in sorted(shapes):
        for n in (1, 3, 8):
            assert R.partial_words(n, h, w, c, G) == lib.query("siss_gn_partial_words", n, h, w, c, G), (n, h, w, c)
    for bad in ((4, 4, 100, 32), (4, 4, 36, 4), (4, 4, 64, 64)):          # C % G, C % 8, G > 32
        assert R.partial_words(1, *bad) == -1 == lib.query("siss_gn_partial_words", 1, *bad)


def test_the_sd_widths_slice_and_dispatch_as_the_issue_says():
    cut = lambda c: (R.shape(4, 4, c, G).nslices, R.shape(4, 4, c, G).C)
    assert [cut(c) for c in (320, 640, 960, 1280, 1920, 2560)] == [(1, 320), (1, 640), (1, 960), (2, 640), (2, 960), (4, 640)]
    # (the narrowest slice of whole groups that is a multiple of 8 channels: two images never make the 128 blocks that stop the search)
    assert [R.slab_slice(8, 8, c, G, 2).Cs for c in (320, 640, 960)] == [40, 40, 120]
    assert [R.slab_slice(8, 8, c, G, 64).Cs for c in (320, 640, 960)] == [80, 80, 120]
    assert R.slab_slice(36, 36, 128, G, 2) is None and R.slab_slice(32, 32, 128, G, 2) is not None
    assert R.slab_slice(36, 36, 320, G, 2) is None and R.slab_slice(28, 28, 320, G, 2) is not None    # (5 lanes per pixel: 102 x 8 pixels at most)
    assert R.plan_fwd(64, 64, 128, G, 3, 0).nchunks == 16 and R.plan_fwd(20, 20, 1024, G, 2, 0).nchunks == 13
    assert R.plan_bwd(8, 8, 320, G, 2, 4, 2, 1).kernel == "slab" and R.plan_bwd(20, 20, 320, G, 2, 4, 2, 1).kernel == "two_pass"
    assert R.plan_bwd(4, 4, 1920, G, 2, 4, 2, 1).kernel == "two_pass"           # sliced widths never take the slab kernels
    assert R.plan_fwd(15, 15, 128, G, 3, 0, qs=(128,)).kernel == "qstats" and R.plan_fwd(15, 15, 320, G, 3, 0, qs=(320,)).kernel == "two_pass"


def _nchunks(px, C, N, blocks):
    """shape().nchunks for an array of pixel counts (one slice: C <= 1024)."""
    ppi = R.K_THREADS // (C // 8)
    cd = lambda a, b: -(-a // b)
    nch = np.minimum(cd(blocks, N), cd(px, 16 * ppi))
    by32 = cd(px, 32 * ppi)
    nch = np.where((nch > by32) & (by32 * N >= 256), by32, nch)
    nch = np.clip(nch, 1, 256)
    return cd(px, cd(px, nch))


def test_no_small_shape_has_a_statistics_launch_cut_differently():
    """gn_bwd_apply_kernel folds `pchunks` slab entries, the block count of the STATISTICS launch (kBlocksBwdStats = 767), which differs
    from its own (kBlocksBwd = 512) only at large sites: under 10 M elements (32 groups, up to 128 saved samples, one slice or more)
    there is none, so the backward table of the GPU suite has no such case.  The smallest found is 53 x 58 x 320 with 32 saved samples
    (31 M elements: 16 against 17 blocks per sample)."""
    limit = 10_000_000
    for C in range(32, 1025, 32):
        for N in range(1, 129):
            px = np.arange(1, limit // (C * N) + 1)
            if px.size == 0:
                continue
            a, s = _nchunks(px, C, N, R.BLOCKS_BWD), _nchunks(px, C, N, R.BLOCKS_BWD_STATS)
            assert (a == s).all(), (C, N, int(px[(a != s).argmax()]))
    for (h, w, c, n) in ((13, 17, 320, 3), (64, 64, 128, 16), (160, 160, 128, 2), (272, 272, 256, 1), (53, 58, 320, 32)):   # _nchunks is shape()
        for blocks in (R.BLOCKS_BWD, R.BLOCKS_BWD_STATS):
            assert _nchunks(np.array([h * w]), c, n, blocks)[0] == R.shape(h, w, c, G, n, blocks).nchunks
    s, ss = R.shape(53, 58, 320, G, 32, R.BLOCKS_BWD), R.shape(53, 58, 320, G, 32, R.BLOCKS_BWD_STATS)
    assert (s.nchunks, ss.nchunks) == (16, 17)
    for c in R.BWD_CASES:
        p = R.plan_bwd(c.H, c.W, c.C, G, c.B, c.n2, c.simg, 0)
        assert p.nchunks == p.pchunks


# ---------------------------------------------------------------------------------------------------------------------
# the budget accepts an honest f32 evaluation
def _to_bf16(v):
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


def _worst(got, ref, budget):
    return float(((got - ref).abs() / budget).max())


@pytest.mark.parametrize("c", ALL_FWD, ids=ids(ALL_FWD))
def test_forward_budget_accepts_torch_f32(c):
    x, gamma, beta = R.fwd_inputs(c)
    f = R.forward(x, gamma, beta, c.eps, G, c.silu)
    y, mean, rstd = torch.native_group_norm(x.float(), gamma.float(), beta.float(), c.B, c.C, c.H * c.W, G, c.eps)
    y = _to_bf16(F.silu(y) if c.silu else y)
    for slab_on in (0, 1):
        p = R.plan_fwd(c.H, c.W, c.C, G, c.B, slab_on, qs=c.qs)
        by, bm, br = R.fwd_budget(f, gamma, beta, c.silu, p.L_stats, c.eps)
        assert _worst(y, f["y"], by) <= 1 and _worst(mean.to(F64), f["mean"], bm) <= 1 and _worst(rstd.to(F64), f["rstd"], br) <= 1
        if c.dist == "std":
            assert float((by / R.half_ulp_bf16(f["y"])).median()) < 1.1, "the bf16 rounding makes up almost all of the budget"


@pytest.mark.parametrize("c", R.BWD_CASES, ids=ids(R.BWD_CASES))
def test_backward_budget_accepts_torch_f32_autograd(c):
    x, gamma, beta, dy, a1, a2, old2 = R.bwd_inputs(c)
    b = R.backward(x, gamma, beta, c.eps, G, c.silu, dy, c.B, c.simg, a1, a2, old2, c.split, c.acc_dx2)
    dx, dg, db = _torch_backward(x, gamma, beta, c.eps, c.silu, dy, c.B, c.simg, torch.float32)
    tot = dx.clone()
    for r in (a1, a2):
        tot = tot + r.float() if r is not None else tot
    if c.split and c.acc_dx2:
        tot[:, c.split:] += old2.float()
    for slab_on in (0, 1):
        p = R.plan_bwd(c.H, c.W, c.C, G, c.B, c.n2, c.simg, slab_on)
        bud = R.bwd_budget(b, gamma, beta, c.silu, p)
        assert _worst(_to_bf16(tot), b["total"], bud["dx"]) <= 1
        assert _worst(dg.to(F64), b["dgamma"], bud["dgamma"]) <= 1 and _worst(db.to(F64), b["dbeta"], bud["dbeta"]) <= 1
        assert _worst(dx.sum((2, 3)).to(F64), b["colsum"], bud["colsum"]) <= 1


def test_f32_budget_accepts_an_f32_evaluation_on_f64_statistics():
    """The f32 forms sum in f64 and round once: f64 statistics rounded to f32, then the element chain in f32."""
    for c in (R.FWD_CASES[0], R.FWD_CASES[8], R.FWD_CASES[-4]):
        x, gamma, beta = R.fwd_inputs(c)
        f = R.forward(x, gamma, beta, c.eps, G, c.silu)
        cg = torch.arange(c.C) // (c.C // G)
        m, r = f["mean"].float()[:, cg, None, None], f["rstd"].float()[:, cg, None, None]
        sc = r * gamma.float()[None, :, None, None]
        z = x.float() * sc + (beta.float()[None, :, None, None] - m * sc)
        y = (F.silu(z) if c.silu else z).to(F64)
        by, bm, br = R.fwd_budget(f, gamma, beta, c.silu, 0, c.eps, bf16=False)
        assert _worst(y, f["y"], by) <= 1 and _worst(f["rstd"].float().to(F64), f["rstd"], br) <= 1


# ---------------------------------------------------------------------------------------------------------------------
# the budget rejects mutants
def _share(mut, ref, budget):
    return float(((mut - ref).abs() > budget).double().mean())


def _fwd(c, **mut):
    x, gamma, beta = R.fwd_inputs(c)
    eps = mut.pop("eps", c.eps)
    f = R.forward(x, gamma, beta, c.eps, G, c.silu)
    m = R._forward(x, gamma, beta, eps, G, c.silu, **mut)
    p = R.plan_fwd(c.H, c.W, c.C, G, c.B, 0, qs=c.qs)
    by, bm, br = R.fwd_budget(f, gamma, beta, c.silu, p.L_stats, c.eps)
    return dict(y=_share(_to_bf16(m["y"]), f["y"], by), mean=_share(m["mean"], f["mean"], bm), rstd=_share(m["rstd"], f["rstd"], br))


def _bwd(c, **mut):
    x, gamma, beta, dy, a1, a2, old2 = R.bwd_inputs(c)
    b = R.backward(x, gamma, beta, c.eps, G, c.silu, dy, c.B, c.simg, a1, a2, old2, c.split, c.acc_dx2)
    m = R._backward(x, gamma, beta, c.eps, G, c.silu, dy, c.B, c.simg, a1, a2, old2, c.split, c.acc_dx2, **mut)
    bud = R.bwd_budget(b, gamma, beta, c.silu, R.plan_bwd(c.H, c.W, c.C, G, c.B, c.n2, c.simg, 0))
    out = dict(dx=_share(_to_bf16(m["total"]), b["total"], bud["dx"]))
    for k in ("dgamma", "dbeta", "colsum"):
        out[k] = _share(m[k], b[k], bud[k])
    if c.split:
        out["second"] = _share(_to_bf16(m["second"]), b["second"], bud["dx"][:, c.split:])
    return out


def _case(table, name):
    return next(c for c in table if c.name == name)


STD_FWD = [c for c in R.FWD_CASES if c.dist == "std" and c.H * c.W > 1]


@pytest.mark.parametrize("c", STD_FWD, ids=ids(STD_FWD))
def test_mutant_count_includes_the_halo(c):
    """cnt = (H + 2)(W + 2) cpg: mean and var shrink by at least (1 - HW / (H + 2)(W + 2)) >= 11 % at the largest site of the table --
    every statistic violates its budget (of the order of 1e-6 relative), and y moves by far more than a bf16 half-ulp (2^-9
    relative) wherever |xhat gamma| is not small: at least 80 % of the elements."""
    s = _fwd(c, cnt=(c.H + 2) * (c.W + 2) * (c.C // G))
    assert s["rstd"] == 1.0 and s["mean"] == 1.0 and s["y"] >= 0.8, s


@pytest.mark.parametrize("name", ["sd320_20x20", "sd960_8x8", "ex_acc_20x20"])
def test_mutant_count_includes_the_halo_backward(name):
    """The backward's S1 / cnt and S2 / cnt with the padded count (mean / rstd are inputs there: the hook also moves them, as a kernel
    that recomputed them would)."""
    c = _case(R.BWD_CASES, name)
    assert _bwd(c, cnt=(c.H + 2) * (c.W + 2) * (c.C // G))["dx"] >= 0.8


@pytest.mark.parametrize("c", STD_FWD, ids=ids(STD_FWD))
def test_mutant_count_off_by_one_pixel_fails_through_rstd(c):
    """cnt + cpg: at 36 x 36 and 64 x 64 no output element need move by a bf16 half-ulp (the count is off by 1 / 1296 and 1 / 4096); rstd
    moves by about half of that relative, three orders above its budget: EVERY (sample, group) must violate."""
    s = _fwd(c, cnt=c.H * c.W * (c.C // G) + c.C // G)
    assert s["rstd"] == 1.0, s


@pytest.mark.parametrize("name", ["sd320_8x8", "sd960_8x8", "sd320_5x7", "sd960_5x7", "sd320_36x36"])
def test_mutant_lane_takes_its_first_channels_group(name):
    """cpg = 10 / 30: a lane's 8 channels straddle two groups at offsets that are no multiples of 4.  With the first channel's group
    for all 8, 6 + 4 + 2 of every 40 channels at cpg = 10 (30 %) and 2 + 4 + 6 of every 120 at cpg = 30 (10 %) are normalised with
    the neighbouring group's statistics, which differ by O(1 / sqrt(cnt)) relative: at least a third of THOSE elements must violate at
    the 8 x 8 sites, where the groups' statistics differ most; the rest of the tensor is untouched."""
    c = _case(R.FWD_CASES, name)
    cpg = c.C // G
    grp = ((torch.arange(c.C) // 8) * 8) // cpg
    wrong = float((grp != torch.arange(c.C) // cpg).double().mean())
    assert abs(wrong - (0.3 if cpg == 10 else 0.1)) < 1e-9
    s = _fwd(c, chan_group=grp)
    assert s["y"] >= wrong / 3 and s["y"] <= wrong, (s, wrong)


@pytest.mark.parametrize("name", ["small_c320_8x8", "small_c128_36x36"])
def test_mutant_eps_omitted(name):
    """std 2^-7: var = 6.1e-5 against eps = 1e-5 -- without eps rstd is 8 % larger; every statistic and nearly every element violate.  (At
    unit variance the same mutant moves rstd by 5e-6 relative and no output at all.)"""
    s = _fwd(_case(R.FWD_CASES, name), eps=0.0)
    assert s["rstd"] == 1.0 and s["y"] >= 0.9, s


@pytest.mark.parametrize("name", ["sl1280_4x4", "sl1920_4x4", "sl2560_6x5", "sl1920_6x5_view"])
def test_mutant_slice_uses_its_local_group_index(name):
    """Slice z of a wide tensor reading mean / rstd at g instead of g0 + g: every channel outside slice 0 (1/2, 1/2, 3/4 of them) is
    normalised with another group's statistics."""
    c = _case(R.FWD_CASES, name)
    s = R.shape(c.H, c.W, c.C, G, c.B)
    grp = (torch.arange(c.C) % s.C) // s.cpg
    outside = 1 - 1 / s.nslices
    assert _fwd(c, chan_group=grp)["y"] >= 0.5 * outside
    b = _case(R.BWD_CASES, "sl1920_split1280_4x4")
    assert _bwd(b, chan_group=(torch.arange(b.C) % 960) // 60)["dx"] >= 0.25


TWO_SETS = [c for c in R.BWD_CASES if c.sets == 2]


@pytest.mark.parametrize("c", TWO_SETS, ids=ids(TWO_SETS))
def test_mutants_of_the_cotangent_sets(c):
    """Set 1 normalised with set 0's S1 / S2: half of the samples get a wrong mean-subtraction, of the size of S1 / cnt ~ 1 / sqrt(cnt) of
    |dy| -- above a half-ulp for most elements at small sites, for fewer at large ones: at least 10 % of all elements, and every column
    sum of set 1 (the term does not cancel in a sum over pixels).
    x index n2 // sets instead of n2 % nx: with nx >= 2 at least one cotangent sample in four meets another saved sample; its dx is
    unrelated: at least 20 % of all elements.
    dgamma / dbeta of both sets landing in set 0: every entry of both sets is off by the other set's sum."""
    nx = c.B
    s = _bwd(c, s12_src=lambda i: i % nx)
    assert s["dx"] >= 0.1 and s["colsum"] >= 0.45, s
    s = _bwd(c, xindex=lambda i: i // c.sets)
    moved = sum((i // c.sets) != (i % nx) for i in range(c.n2)) / c.n2
    assert moved >= 0.25 and s["dx"] >= 0.8 * moved, (s, moved)
    s = _bwd(c, set_of=lambda i: 0)
    assert s["dgamma"] >= 0.99 and s["dbeta"] >= 0.99, s


@pytest.mark.parametrize("name", ["sl1920_split1280_4x4"])
def test_mutant_split_taken_per_slice(name):
    """1920 = 2 x 960 split at 1280: slice 1 comparing its LOCAL channel index with split_c sends none of its channels to the second
    part -- channels [1280, 1920) never reach dx2, which keeps its old contents: every element of the second part is off by t + accum."""
    c = _case(R.BWD_CASES, name)
    ch = torch.arange(c.C)
    assert _bwd(c, second_of=(ch % 960) >= c.split)["second"] >= 0.95

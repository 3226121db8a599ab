"""The GroupNorm (+ SiLU) kernels through their C entry points against the f64 reference of tests/groupnorm_ref.py, variant by variant:
two-pass and one-launch slab forms, the statistics hand-over (siss_quad_stats -> siss_groupnorm_fwd_qs), channel slices of tensors wider
than 1024 channels, one and two cotangent sets, the No-IS layout, split targets, every running cotangent of the EXTRA forms, and the f32
forms of csrc/f32_path.hip on the same tables.

Every output is held to the BUDGET derived in groupnorm_ref.py (bf16 half-ulp of the f64 result + the f32 operation chain + the
statistics' summation error for the launch shape in use), not to a fraction of the tensor's scale; mean and rstd are outputs and are held
to theirs.  Every launch's dispatch counters must match the plan computed from the restated launch shapes, and every buffer is compared
WHOLE: halo and guard rows zero, the neighbouring columns of a wider input buffer untouched, sentinels intact behind mean / rstd, behind
`partial`, around the gradient rows and behind the column sums.  The backward gets the f64 statistics rounded to f32 as its mean / rstd
inputs, so that its budget does not inherit the forward's.  tests/test_groupnorm_ref_host.py runs the same budget over the same cases
against torch and against mutants of the reference on the CPU.

The restated launch shapes are compared with the one number of them the library exposes (siss_gn_partial_words: slices x chunks x groups at
N = 1); lpp, ppi, chunk_px at a case's own N and slab_slice are pinned only through the dispatch counters (groupnorm_ref.py says so).
When the module is done, the `dev` fixture prints the worst error-to-budget ratio per kernel family over the cases that ran (pytest -s;
docs/kernels.md records them): a report, not a check.
"""
import functools

import pytest
import torch

import groupnorm_ref as R

pytestmark = pytest.mark.gpu
G, F64, BF16, F32 = R.G32, torch.float64, torch.bfloat16, torch.float32
SENT = 5.0                    # sentinel of the f32 side buffers
JUNK = 768.0                  # (bf16-exact) what an output's interior holds before the launch: every element must be written
P, OFF_G, OFF_B = 8192, 64, 4096          # floats per gradient set; where dgamma / dbeta start inside a set's row
RATIOS, NOTES = {}, {}
ids = lambda cases: [c.name for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    yield torch.device("cuda:0")
    # a REPORT, not a check (hold() has asserted every figure): what docs/kernels.md records, over whichever cases ran (pytest -s shows it)
    for k in sorted(RATIOS):
        print(f"\nMEASURED {k:14s} worst error / budget {RATIOS[k]:.3f}", end="")
    for (fam, name), rel in sorted(NOTES.items()):
        print(f"\nMEASURED rstd relative error {fam:14s} {name:22s} {rel:.3g}", end="")
    print()


@functools.lru_cache(maxsize=None)
def ref_fwd(c):
    x, gamma, beta = R.fwd_inputs(c)
    return x, gamma, beta, R.forward(x, gamma, beta, c.eps, G, c.silu)


@functools.lru_cache(maxsize=None)
def ref_bwd(c):
    x, gamma, beta, dy, a1, a2, old2 = R.bwd_inputs(c)
    return x, gamma, beta, dy, a1, a2, old2, R.backward(x, gamma, beta, c.eps, G, c.silu, dy, c.B, c.simg, a1, a2, old2, c.split, c.acc_dx2)


def hold(family, what, got, ref, budget):
    """|got - ref| <= budget at EVERY element of the buffer (budget 0: the element must equal ref); records the worst ratio."""
    got, ref, budget = got.detach().to("cpu", F64).reshape(-1), ref.to(F64).reshape(-1), budget.to(F64).reshape(-1)
    assert got.shape == ref.shape == budget.shape, (what, got.shape, ref.shape, budget.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs()
    live = budget > 0
    ratio = float((err[live] / budget[live]).max()) if live.any() else 0.0
    print(f"{family:14s} {what:10s} worst error / budget = {ratio:.3f}")
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    bad = err > budget
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the budget (worst ratio {ratio:.3g}; first at flat index "
                           f"{int(bad.nonzero()[0])}: got {float(got[bad][0])!r}, ref {float(ref[bad][0])!r}, budget {float(budget[bad][0]):.3g})")


def padded_ref(v):
    """A reference or budget tensor in NCHW -> the WHOLE flat buffer of a padded activation: zeros (budget 0) outside the interior."""
    from siss_amd.layout import Act
    return Act.from_nchw(v, "cpu", dtype=F64).buf


def to_act(v, dev, dtype, ld_extra=0):
    """A padded activation holding v; with ld_extra, as a column window [ld_extra, ld_extra + C) of a wider buffer full of junk."""
    from siss_amd.layout import Act, ActView
    if not ld_extra:
        return Act.from_nchw(v, dev, dtype=dtype), None, 0
    n, c, h, w = v.shape
    base = Act(n, h, w, c + ld_extra, dev, dtype=dtype)
    base.interior().normal_()
    base.interior()[..., ld_extra:] = v.permute(0, 2, 3, 1).to(dtype).to(dev)
    return ActView(base, ld_extra, c), base, base.c


def sentinel(n, tail=64):
    return torch.full((n + tail,), SENT, dtype=F32)


def counts_delta(lib, fn):
    before = lib.dispatch_counts()
    fn()
    torch.cuda.synchronize()
    after = lib.dispatch_counts()
    return {k: after[k] - before[k] for k in ("gn_slab", "gn_qstats", "gn_bwd_sc_kernel")}


class slab_mode:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from siss_amd import lib
        assert lib.query("siss_groupnorm_set_slab", self.on) == self.on

    def __exit__(self, *exc):
        from siss_amd import lib
        lib.query("siss_groupnorm_set_slab", -1)
        return False


def test_restated_launch_shapes_equal_the_library(dev):
    from siss_amd import lib
    for c in R.FWD_CASES + R.QS_CASES + R.BWD_CASES:
        for n in (1, c.B, 2 * c.B):
            assert R.partial_words(n, c.H, c.W, c.C, G) == lib.query("siss_gn_partial_words", n, c.H, c.W, c.C, G), c.name


# ---------------------------------------------------------------------------------------------------------------------
# forward
def run_forward(dev, c, slab_on, f32):
    from siss_amd import lib
    from siss_amd.layout import Act
    x, gamma, beta, f = ref_fwd(c)
    dtype = F32 if f32 else BF16
    plan = R.plan_fwd(c.H, c.W, c.C, G, c.B, slab_on, qs=c.qs, f32=f32)
    family = "f32 fwd" if f32 else {"two_pass": "fwd two-pass", "slab": "fwd slab", "qstats": "hand-over"}[plan.kernel]
    xa, base, ldx = to_act(x, dev, dtype, c.ld_extra)
    base_before = base.buf.clone() if base is not None else None
    words = lib.query("siss_gn_partial_words", c.B, c.H, c.W, c.C, G)
    mean, rstd, part = sentinel(c.B * G).to(dev), sentinel(c.B * G).to(dev), sentinel(words).to(dev)
    npix = c.B * c.H * c.W
    if c.compact:
        ybuf = torch.full((npix * c.C + 64,), JUNK, dtype=dtype, device=dev)
        yp = ybuf
    else:
        ya = Act(c.B, c.H, c.W, c.C, dev, dtype=dtype)
        ya.interior().fill_(JUNK)
        ybuf, yp = ya.buf, ya.data
    g32, b32 = gamma.to(F32).to(dev), beta.to(F32).to(dev)
    qbufs = []
    if c.qs:
        from siss_amd.layout import ActView
        assert base is None and not f32
        c0 = 0
        for w in c.qs:
            v = ActView(xa, c0, w) if len(c.qs) > 1 else xa
            q = torch.full((lib.query("siss_conv_qstats_words", xa.rows, w),), float("nan"), device=dev)
            lib.call("siss_quad_stats", v.data, xa.c, xa.rows, w, xa.rows_per_image, q)
            qbufs.append(q)
            c0 += w
        qbufs.append(None)

    def launch():
        if c.qs:
            lib.call("siss_groupnorm_fwd_qs", xa.data, g32, b32, yp, mean, rstd, part, qbufs[0], c.qs[0], qbufs[1], c.B, c.H, c.W, c.C, G,
                     c.eps, int(c.silu), int(c.compact), ldx)
        else:
            lib.call("siss_groupnorm_fwd_ld", xa.data, g32, b32, yp, mean, rstd, part, c.B, c.H, c.W, c.C, G, c.eps, int(c.silu),
                     int(c.compact), ldx)

    with slab_mode(slab_on), lib.f32_mode(f32):
        assert counts_delta(lib, launch) == plan.counts, f"{c.name}: the launch did not take the planned kernels ({plan.kernel})"
    by, bm, br = R.fwd_budget(f, gamma, beta, c.silu, plan.L_stats, c.eps, bf16=not f32)
    tail = torch.full((64,), SENT, dtype=F64)
    hold(family, "mean", mean, torch.cat([f["mean"].reshape(-1), tail]), torch.cat([bm.reshape(-1), 0 * tail]))
    hold(family, "rstd", rstd, torch.cat([f["rstd"].reshape(-1), tail]), torch.cat([br.reshape(-1), 0 * tail]))
    assert (part[words:] == SENT).all(), "the launch wrote past siss_gn_partial_words"
    if c.compact:
        junk = torch.full((64,), JUNK, dtype=F64)
        nhwc = lambda v: v.permute(0, 2, 3, 1).reshape(-1)
        hold(family, "y", ybuf, torch.cat([nhwc(f["y"]), junk]), torch.cat([nhwc(by), 0 * junk]))
    else:
        hold(family, "y", ybuf, padded_ref(f["y"]), padded_ref(by))
    if base is not None:
        assert torch.equal(base.buf, base_before), "the input buffer (its neighbouring columns included) must be left alone"
    if c.dist in ("offset", "small"):
        rel = float(((rstd[:c.B * G].cpu().to(F64) - f["rstd"].reshape(-1)).abs() / f["rstd"].reshape(-1)).max())
        NOTES[(family, c.name)] = rel
        print(f"{family} {c.name}: rstd relative error {rel:.3g} = 2^{torch.log2(torch.tensor(rel + 1e-300)).item():.1f}")
        if c.dist == "offset":
            assert rel < 2.0 ** -11, "the one-pass statistics show in an output: sums about a pivot, or f64 one level earlier"
    if c.dist == "ones":
        cpg = c.C // G
        yg = (ybuf[:npix * c.C].view(c.B, c.H * c.W, c.C) if c.compact else ya.interior().reshape(c.B, c.H * c.W, c.C))[..., 5 * cpg:6 * cpg]
        bt = beta[5 * cpg:6 * cpg].to(F32)
        want = (torch.nn.functional.silu(bt) if c.silu else bt).to(BF16).to(F64)
        # (the f32 form's unrounded y lies within half a bf16 ulp of bf16(act(beta)) plus z's own rounding, 316 gamma u: the same line holds it)
        assert ((yg.cpu().to(F64) - want).abs() <= 2 * R.half_ulp_bf16(want)).all(), "a constant group: y = bf16(act(beta)) to one bf16 ulp"
        r5 = rstd[:c.B * G].view(c.B, G)[:, 5].cpu().to(F64)
        assert ((r5 - c.eps ** -0.5).abs() <= 1.01 * R.U * c.eps ** -0.5).all(), "a constant group: the sums are exact, rstd = 1 / sqrt(eps)"


@pytest.mark.parametrize("slab_on", [0, 1], ids=["two_pass", "slab"])
@pytest.mark.parametrize("c", R.FWD_CASES, ids=ids(R.FWD_CASES))
def test_forward(dev, c, slab_on):
    run_forward(dev, c, slab_on, False)


@pytest.mark.parametrize("c", R.FWD_CASES, ids=ids(R.FWD_CASES))
def test_forward_f32_form(dev, c):
    run_forward(dev, c, 1, True)


@pytest.mark.parametrize("c", R.QS_CASES, ids=ids(R.QS_CASES))
def test_forward_on_handed_over_statistics(dev, c):
    """siss_quad_stats leaves the (half tile, image slot, quad) entries, siss_groupnorm_fwd_qs folds them in f64 and runs no statistics
    pass -- or, where a group is not whole quads (C = 320), ignores them and runs it.  mean / rstd against f64 under the budget."""
    run_forward(dev, c, 0, False)


# ---------------------------------------------------------------------------------------------------------------------
# backward
def run_backward(dev, c, slab_on, f32):
    from siss_amd import lib
    from siss_amd.layout import Act
    x, gamma, beta, dy, a1, a2, old2, b = ref_bwd(c)
    dtype = F32 if f32 else BF16
    n2, nsets = c.n2, c.n2 // c.simg
    plan = R.plan_bwd(c.H, c.W, c.C, G, c.B, n2, c.simg, slab_on, f32=f32)
    family = "f32 bwd" if f32 else {"two_pass": "bwd two-pass", "slab": "bwd slab"}[plan.kernel]
    xa, base, ldx = to_act(x, dev, dtype, c.ld_extra)
    base_before = base.buf.clone() if base is not None else None
    nhwc = lambda v: v.permute(0, 2, 3, 1).reshape(-1, v.shape[1])
    dyp = nhwc(dy).to(dtype).to(dev).contiguous() if c.cdy else Act.from_nchw(dy, dev, dtype=dtype).data
    acc = Act.from_nchw(a1, dev, dtype=dtype) if c.acc else None
    acc2 = Act.from_nchw(a2, dev, dtype=dtype) if c.acc2 else None
    g32, b32 = gamma.to(F32).to(dev), beta.to(F32).to(dev)
    mean, rstd = b["fwd"]["mean"].to(F32).to(dev).contiguous(), b["fwd"]["rstd"].to(F32).to(dev).contiguous()
    words = lib.query("siss_gn_partial_words", n2, c.H, c.W, c.C, G)
    bud = R.bwd_budget(b, gamma, beta, c.silu, plan, bf16=not f32)
    grads0 = torch.full((nsets, P), SENT, dtype=F32)
    grads0[:, OFF_G:OFF_G + c.C] = 0; grads0[:, OFF_B:OFF_B + c.C] = 0
    runs = []
    for rep in range(2 if plan.kernel == "slab" else 1):
        part, grads = sentinel(words).to(dev), grads0.clone().to(dev)
        cs = None
        if c.colsum:
            cs = torch.full((n2, c.C + 8), SENT, dtype=F32)
            cs[:, :c.C] = 0
            cs = cs.to(dev)
        if c.split:
            da = Act(n2, c.H, c.W, c.split, dev, dtype=dtype)
            da.interior().fill_(JUNK)
            db = Act.from_nchw(old2, dev, dtype=dtype)                 # (a target that does not accumulate must lose these)
        else:
            da, db = Act(n2, c.H, c.W, c.C, dev, dtype=dtype), None
            da.interior().fill_(JUNK)

        def launch():
            lib.call("siss_groupnorm_bwd_ld", dyp, xa.data, g32, b32, mean, rstd, da.data, acc.data if acc else None,
                     acc2.data if acc2 else None, db.data if db else None, c.split, int(c.acc_dx2), grads[0, OFF_G:], grads[0, OFF_B:],
                     cs, c.C + 8 if c.colsum else 0, part, n2, c.B, c.simg, P, c.H, c.W, c.C, G, int(c.silu), int(c.cdy), ldx)

        with slab_mode(slab_on), lib.f32_mode(f32):
            assert counts_delta(lib, launch) == plan.counts, f"{c.name}: the launch did not take the planned kernels ({plan.kernel})"
        runs.append((da.buf.clone(), None if db is None else db.buf.clone(), None if cs is None else cs.clone()))
    if c.split:
        hold(family, "dx", da.buf, padded_ref(b["first"]), padded_ref(bud["dx"][:, :c.split]))
        hold(family, "dx2", db.buf, padded_ref(b["second"]), padded_ref(bud["dx"][:, c.split:]))
    else:
        hold(family, "dx", da.buf, padded_ref(b["total"]), padded_ref(bud["dx"]))
    want, wb = grads0.to(F64), torch.zeros(nsets, P, dtype=F64)
    want[:, OFF_G:OFF_G + c.C] = b["dgamma"]; wb[:, OFF_G:OFF_G + c.C] = bud["dgamma"]
    want[:, OFF_B:OFF_B + c.C] = b["dbeta"]; wb[:, OFF_B:OFF_B + c.C] = bud["dbeta"]
    hold(family, "dgamma/dbeta", grads, want, wb)
    if c.colsum:
        want, wb = torch.full((n2, c.C + 8), SENT, dtype=F64), torch.zeros(n2, c.C + 8, dtype=F64)
        want[:, :c.C] = b["colsum"]; wb[:, :c.C] = bud["colsum"]
        hold(family, "colsum", cs, want, wb)
    assert (part[words:] == SENT).all(), "the launch wrote past siss_gn_partial_words"
    if base is not None:
        assert torch.equal(base.buf, base_before), "the saved input (its neighbouring columns included) must be left alone"
    if len(runs) == 2:
        (d0, e0, c0), (d1, e1, c1) = runs
        assert torch.equal(d0, d1) and (e0 is None or torch.equal(e0, e1)), "slab kernel: dx must be bitwise repeatable"
        assert c0 is None or torch.equal(c0, c1), "slab kernel: the block owns its column sums -- bitwise repeatable"


@pytest.mark.parametrize("slab_on", [0, 1], ids=["two_pass", "slab"])
@pytest.mark.parametrize("c", R.BWD_CASES, ids=ids(R.BWD_CASES))
def test_backward(dev, c, slab_on):
    run_backward(dev, c, slab_on, False)


@pytest.mark.parametrize("c", R.BWD_CASES, ids=ids(R.BWD_CASES))
def test_backward_f32_form(dev, c):
    run_backward(dev, c, 1, True)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def test_launchers_refuse_bad_shapes_and_pointers_without_launching(dev):
    from siss_amd import lib
    from siss_amd.layout import Act
    H = W = 4
    f = lambda n: torch.zeros(n, device=dev)

    def fwd(C, Gq, x=None):
        a, y = Act(2, H, W, C, dev), Act(2, H, W, C, dev)
        return lib.call("siss_groupnorm_fwd_ld", a.data if x is None else x, f(C), f(C), y.data, f(2 * 32), f(2 * 32), f(4096), 2, H, W, C, Gq,
                        1e-6, 1, 0, 0, refusable=True)

    def bwd(C, Gq, split=0, x=None):
        a, d, o = Act(2, H, W, C, dev), Act(2, H, W, C, dev), Act(2, H, W, C, dev)
        o2 = Act(2, H, W, C, dev) if split else None
        return lib.call("siss_groupnorm_bwd_ld", d.data, a.data if x is None else x, f(C), f(C), f(2 * 32), f(2 * 32), o.data, None, None,
                        o2.data if split else None, split, 0, f(C), f(C), None, 0, f(4096), 2, 2, 2, C, H, W, C, Gq, 1, 0, 0, refusable=True)

    odd = Act(2, H, W, 64, dev).buf[1:]                              # 2 bytes past a 16-B boundary
    assert odd.data_ptr() % 16 == 2
    before = lib.dispatch_counts()
    for what, rc in (("C % G", fwd(40, 32)), ("C % 8", fwd(36, 4)), ("G > 32", fwd(512, 64)), ("misaligned x", fwd(64, 32, odd)),
                     ("C % G (bwd)", bwd(40, 32)), ("C % 8 (bwd)", bwd(36, 4)), ("G > 32 (bwd)", bwd(512, 64)),
                     ("misaligned x (bwd)", bwd(64, 32, x=odd)), ("split_c % 8", bwd(64, 32, split=20))):
        assert rc == 1, f"{what}: expected the argument error"
    torch.cuda.synchronize()
    assert lib.dispatch_counts() == before
    assert fwd(64, 32) == 0 and bwd(64, 32) == 0 and bwd(64, 32, split=24) == 0      # the same calls with nothing wrong are taken
    torch.cuda.synchronize()

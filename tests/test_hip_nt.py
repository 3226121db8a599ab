"""The NT product family of csrc/gemm_nt.hip, csrc/gemm_nt_c3p.hip and the shared epilogue of csrc/nt_common.h called DIRECTLY at their
C entry points, variant by variant, BITWISE against tests/nt_ref.py (which tests/test_nt_ref_host.py pins to torch on the CPU).

csrc/gemm_nt.hip      siss_gemm_nt, siss_gemm_nt_alpha_cols, siss_gemm_nt_mulsub, siss_gemm_nt_qstats, siss_gemm_nt_d2s,
                      siss_gemm_nt_d2s_bias, siss_gemm_nt_d2s_phases on gemm_nt_kernel<128,4,1>, <128,4,2>, <128,4,4>, <128,4,1,160>,
                      their split-K forms (S = 2, 3, 5, 7, 8; 2 on the double-buffered form) and gemm_nt_reduce_kernel
csrc/gemm_nt_c3p.hip  the persistent 3x3 kernel: siss_gemm_nt on large grids, siss_conv3x3_sc, siss_conv3x3_dgrad_sc, statistics
csrc/f32_path.hip     the f32 forms of all of these (through lib.f32_mode)

Why bitwise: A, W, A2, W2, Wx and R hold integers that bf16 represents exactly, bias / bias2 / rowbias / rowsub hold integers and
alpha is a power of two.  Every product and every partial sum -- in any K order, in any split, in the split-K slab -- is then an
integer below 2^24 (nt_ref asserts it on the CPU before it rounds anything): exact in the MFMA's f32 accumulators and in f32 memory.
The value in front of each of the two roundings to bf16 is therefore known exactly, each rounding is round-to-nearest-even of it,
and the result must equal the reference bit for bit.  "narrow" operands lie in [-4, 4]; "wide" ones in [-31, 31], where most
outputs need rounding, ties and non-ties.  There is no tolerance in this module.

What lies around the operands: every entry of A and A2 outside nt_ref.needed_masks (the columns outside the panels' windows, the rows
no panel reaches), R at halo rows and in the columns [N, ldr), rowbias in [N, ldrb) and behind the last image is NaN.  Halo rows and
guard rows of A hold VALUES, so a wrong shift shows.  C and Cx are flat buffers filled with a sentinel, with ldc > N and spare rows in
front of row 0 and behind row M, and the WHOLE buffer is compared: nothing lands past N or outside [0, M), halo rows hold zeros, and
the depth-to-space forms leave C's halo alone.  lib.dispatch_counts is asserted for every launch against plan(), which restates the
dispatch rule of gemm_nt_dispatch: no case can silently move to another kernel.
"""
import dataclasses

import numpy as np
import pytest
import torch

import nt_ref as R
from siss_amd.layout import conv3x3_panels

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENT = -12288.0                       # exact in bf16
AMP = {"unit": 1, "narrow": 4, "wide": 31}
NT, SPLITK, WIDE, C3P = "gemm_nt_kernel", "gemm_nt_kernel/splitk", "gemm_nt_kernel/wide", "gemm_nt_c3p_kernel"
KEYS = (NT, SPLITK, WIDE, C3P)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    d = torch.device("cuda:0")
    lib.ensure_workspace(d)
    return d


def cdiv(a, b):
    return -(-a // b)


def is_triples(shifts, coffs):
    return len(shifts) == 9 and all(shifts[g + 1] == shifts[g] + 1 and shifts[g + 2] == shifts[g] + 2 and
                                    coffs[g] == coffs[g + 1] == coffs[g + 2] for g in (0, 3, 6))


def plan(c, workspace=True, rowsub=False):
    """The dispatch rule of gemm_nt_dispatch (csrc/gemm_nt.hip) restated: (counter that moves, stage depth, split count S).
    The stage depth has no counter of its own; it follows from the number of 128 x 128 tiles (times batch, times the four phases):
    more than 512 tiles run gemm_nt_kernel<128,4,1> (<128,4,1,160>, counted as /wide too, when N is a multiple of 160 but not of
    128), 257..512 tiles <128,4,2>, at most 256 tiles the 4-deep ring <128,4,4> -- unless 129..256 tiles meet 24 or more K steps
    and a workspace: then <128,4,2> with two splits.  At most 128 tiles with 12 or more steps split K by
    S = min(256 / tiles, 8, steps / 6) on the ring when S >= 2.  Nine 3x3 panels on 256 or more 128-row tiles with N % 128 == 0 and
    rows_per_image >= 256 go to the persistent kernel."""
    phases = 4 if c.phase_p0 is not None else 1
    conv3 = is_triples(c.shifts, c.coffs) and c.batch == 1 and not rowsub and not c.mul and not c.d2s
    if conv3 and c.N % 128 == 0 and c.rows_per_image >= 256 and (c.Wp == 0 or c.Wp >= 8) and cdiv(c.M, 128) * (c.N // 128) >= 256 \
            and (not c.Nx or c.Kp >= 128):
        return C3P, 0, 1
    assert not c.K2 and not c.Nx
    tiles = cdiv(c.M, 128) * cdiv(c.N, 128) * c.batch * phases
    steps = c.npanels * (c.Kp // 64)
    if tiles > 512:
        return (WIDE if c.N % 160 == 0 and c.N % 128 else NT), 1, 1
    if tiles > 256:
        return NT, 2, 1
    splittable = c.batch == 1 and phases == 1 and workspace
    if splittable and tiles <= 128 and steps >= 12:
        S = min(256 // tiles, 8, steps // 6)
        if S >= 2:
            return SPLITK, 4, S
    if splittable and tiles > 128 and steps >= 24:
        return SPLITK, 2, 2
    return NT, 4, 1


def counts(kernel, launches=1):
    out = dict.fromkeys(KEYS, 0)
    if kernel is not None:
        out[NT if kernel == WIDE else kernel] = launches
        if kernel == WIDE:
            out[WIDE] = launches
    return out


def launch(fn, expect):
    """Run fn() and assert the dispatch counters it moved."""
    from siss_amd import lib
    lib.dispatch_counts(reset=True)
    fn()
    torch.cuda.synchronize()
    got = lib.dispatch_counts()
    assert {k: got[k] for k in KEYS} == expect


def same(got, want, dt, what):
    """Bitwise: a device tensor against the reference's f64 buffer (whose values are exact in dt)."""
    w = torch.from_numpy(np.asarray(want, dtype=np.float64))
    wt = w.to(dt)
    assert bool(((wt.to(torch.float64) == w) | torch.isnan(w)).all()), what + ": the reference is not exact in the output type"
    it = torch.int16 if dt == BF else torch.int32
    g = got.detach().cpu().contiguous()
    assert g.dtype == dt and g.shape == wt.shape, (what, g.dtype, g.shape, wt.shape)
    ne = g.view(it) != wt.view(it)
    if bool(ne.any()):
        i = ne.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, the first at flat index {i}: "
                             f"got {g.flatten()[i].item()!r}, want {wt.flatten()[i].item()!r}")


def conv_case(n, hp, wp, N, Kp, coff=0, **kw):
    """3x3 panels over n images of hp x wp PADDED pixels; coff: the channel window's offset in a wider A (the concat view)."""
    shifts, _ = conv3x3_panels(wp, Kp)
    return R.Case(M=n * hp * wp, N=N, Kp=Kp, shifts=tuple(shifts), coffs=(coff,) * 9, lda=coff + Kp + 8, ldc=N + 8,
                  rows_per_image=hp * wp, Hp=hp, Wp=wp, **kw)


class Prob:
    """One product: integer host operands with their guard rows, the reference result (computed once), NaN-masked device operands
    and sentinel-filled outputs.  res: None | "sep" (R a buffer of its own, row stride c.ldr) | "c" (R is C itself)."""

    def __init__(self, c, dev, seed, amp="narrow", bias=False, bias2=False, rowbias=False, rowsub=False, res=None, f32=False,
                 ramp=256, bamp=64):
        rng = np.random.default_rng(seed)
        a = AMP[amp]
        self.c, self.dev, self.f32, self.res = c, dev, f32, res
        self.dt = F32 if f32 else BF
        ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
        g = c.Wp + 2 if c.Hp else 2
        self.a0 = max(g, 1 - min(c.shifts))
        sa = c.strideA // c.lda if c.batch > 1 else 0
        assert c.batch == 1 or (c.strideA % c.lda == 0 and sa >= c.M)
        arows = self.a0 + (c.batch - 1) * sa + c.M + max(max(c.shifts), 0) + g
        self.A = ints(-a, a, (arows, c.lda))
        self.W = ints(-a, a, (c.batch, c.npanels, c.N, c.Kp))
        self.strideW = c.npanels * c.N * c.Kp + 64 if c.batch > 1 else 0
        self.A2 = ints(-a, a, (arows, c.lda2)) if c.K2 else None
        self.W2 = ints(-a, a, (c.N, c.K2)) if c.K2 else None
        self.Wx = ints(-a, a, (c.Nx, c.Kp)) if c.Nx else None
        self.bias = ints(-bamp, bamp, c.N) if bias else None
        self.bias2 = ints(-bamp, bamp, c.N) if bias2 else None
        self.rowbias = ints(-bamp, bamp, (c.nimages + 1, c.ldrb)) if rowbias else None
        self.rowsub = ints(-32, 32, c.batch * c.M) if rowsub else None
        # outputs: spare rows in front and behind, sentinels everywhere
        orows = c.nimages * (2 * c.Hp - 2) * (2 * c.Wp - 2) if c.d2s else c.M
        span = (c.batch - 1) * c.strideC
        self.c0 = 3 * c.ldc
        self.Cprior = np.full(self.c0 + span + orows * c.ldc + 3 * c.ldc, SENT)
        self.r0, self.Rh = 0, None
        if res == "sep":
            self.r0 = 2 * c.ldr
            self.Rh = ints(-ramp, ramp, self.r0 + span + orows * c.ldr + 2 * c.ldr)
        m = R.needed_masks(c, self.A.shape, self.a0, self.A2.shape if c.K2 else None, self.a0,
                           self.Rh.size if res == "sep" else 0, self.r0, self.rowbias.shape if rowbias else None)
        assert not m["A"].all() and m["A"][self.a0 + min(c.shifts)].any()
        self.mA, self.mA2 = m["A"], m["A2"]
        if res == "sep":
            assert not m["R"].all()
            self.Rh = np.where(m["R"], self.Rh, np.nan)
        if res == "c":                                   # the residual lives in C: values where it is read, sentinels elsewhere
            mc = R.needed_masks(dataclasses.replace(c, ldr=c.ldc), self.A.shape, self.a0, r_size=self.Cprior.size, r0=self.c0)["R"]
            self.Cprior = np.where(mc, ints(-ramp, ramp, self.Cprior.size), self.Cprior)
        if rowbias:
            self.rowbias = np.where(m["rowbias"], self.rowbias, np.nan)
        self.Xprior = np.full(2 * c.ldcx + c.M * c.ldcx + 2 * c.ldcx, SENT) if c.Nx else None
        # the reference, once
        acc = R.accumulate(c, self.A, self.a0, self.W, self.A2, self.a0, self.W2)
        self.want = R.store(c, acc, self.Cprior, self.c0, bias=self.bias, bias2=self.bias2, rowbias=self.rowbias, rowsub=self.rowsub,
                            R=self.Rh, r0=self.r0, r_is_c=res == "c", f32=f32)
        self.wantx = R.store_x(c, R.accumulate_x(c, self.A, self.a0, self.Wx), self.Xprior, 2 * c.ldcx, f32=f32) if c.Nx else None
        # device operands
        t = lambda x, dt=self.dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
        self.Ad = t(np.where(self.mA, self.A, np.nan))
        self.A2d = t(np.where(self.mA2, self.A2, np.nan)) if c.K2 else None
        if c.batch > 1:
            wh = np.full((c.batch, self.strideW), np.nan)
            wh[:, :c.npanels * c.N * c.Kp] = self.W.reshape(c.batch, -1)
            self.Wd = t(wh)
        else:
            self.Wd = t(self.W)
        self.W2d, self.Wxd, self.Rd = t(self.W2), t(self.Wx), t(self.Rh)
        self.biasd, self.bias2d, self.rowbiasd, self.rowsubd = (t(x, F32) for x in (self.bias, self.bias2, self.rowbias, self.rowsub))
        self.fresh()

    def fresh(self):
        """New sentinel-filled outputs (a Prob may be launched several ways against its one reference)."""
        self.Cd = torch.from_numpy(self.Cprior).to(self.dt).to(self.dev)
        self.Xd = torch.from_numpy(self.Xprior).to(self.dt).to(self.dev) if self.c.Nx else None
        return self

    # pointers
    @property
    def a(self):
        return self.Ad[self.a0:]

    @property
    def cptr(self):
        return self.Cd[self.c0:]

    @property
    def r(self):
        return self.cptr if self.res == "c" else (self.Rd[self.r0:] if self.res == "sep" else None)

    @property
    def ldr(self):
        return self.c.ldc if self.res == "c" else self.c.ldr

    def panels(self):
        from siss_amd import lib
        return lib.int_array(list(self.c.shifts)), lib.int_array(list(self.c.coffs))

    def stored(self):
        """[M][N] of the reference's stored values (plain row layout)."""
        c = self.c
        return self.want[self.c0:self.c0 + c.M * c.ldc].reshape(c.M, c.ldc)[:, :c.N]

    def check(self, what):
        same(self.Cd, self.want, self.dt, what + ": C")
        if self.c.Nx:
            same(self.Xd, self.wantx, self.dt, what + ": Cx")

    # launches
    def gemm_nt(self):
        from siss_amd import lib
        c = self.c
        s, co = self.panels()
        lib.call("siss_gemm_nt", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, self.rowbiasd, c.ldrb, self.r, self.ldr,
                 c.M, c.N, c.Kp, c.npanels, s, co, c.rows_per_image, c.Hp, c.Wp, float(c.alpha), c.batch, c.strideA, self.strideW,
                 c.strideC)

    def qstats(self, q):
        from siss_amd import lib
        c = self.c
        s, co = self.panels()
        written = lib.C.c_int(0)
        lib.call("siss_gemm_nt_qstats", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, self.rowbiasd, c.ldrb, self.r, self.ldr,
                 c.M, c.N, c.Kp, c.npanels, s, co, c.rows_per_image, c.Hp, c.Wp, float(c.alpha), q, lib.C.byref(written))
        return written.value

    def alpha_cols(self):
        from siss_amd import lib
        c = self.c
        lib.call("siss_gemm_nt_alpha_cols", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, self.r, self.ldr, c.M, c.N, c.Kp,
                 float(c.alpha), c.alpha_cols)

    def mulsub(self):
        from siss_amd import lib
        c = self.c
        lib.call("siss_gemm_nt_mulsub", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.r, self.ldr, self.rowsubd, c.M, c.N, c.Kp,
                 float(c.alpha), c.batch, c.strideA, self.strideW, c.strideC)

    def d2s(self):
        from siss_amd import lib
        c = self.c
        s, co = self.panels()
        if c.phase_p0 is not None:
            lib.call("siss_gemm_nt_d2s_phases", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, self.r, self.ldr, c.M, c.N, c.Kp,
                     lib.int_array(list(c.phase_p0)), s, co, c.rows_per_image, c.Hp, c.Wp)
        elif self.bias is not None:
            lib.call("siss_gemm_nt_d2s_bias", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, c.M, c.N, c.Kp, c.npanels, s, co,
                     c.rows_per_image, c.Hp, c.Wp, c.d2s - 1)
        else:
            lib.call("siss_gemm_nt_d2s", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.r, self.ldr, c.M, c.N, c.Kp, c.npanels, s, co,
                     c.rows_per_image, c.Hp, c.Wp, c.d2s - 1)

    def sc(self, q=None):
        from siss_amd import lib
        c = self.c
        s, co = self.panels()
        if not self.f32:
            assert lib.query("siss_conv3x3_sc_takes", c.M, c.N, c.Kp, c.K2, c.rows_per_image, c.Wp, c.lda, c.ldc, c.lda2) == 1
        written = lib.C.c_int(0)
        lib.call("siss_conv3x3_sc", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.biasd, self.rowbiasd, c.ldrb, self.A2d[self.a0:],
                 c.lda2, self.W2d, c.K2, self.bias2d, c.M, c.N, c.Kp, s, co, c.rows_per_image, c.Hp, c.Wp, q,
                 lib.C.byref(written) if q is not None else None)
        return written.value

    def dgrad_sc(self):
        from siss_amd import lib
        c = self.c
        s, co = self.panels()
        if not self.f32:
            assert lib.query("siss_conv3x3_dgrad_sc_takes", c.M, c.N, c.Kp, c.Nx, c.rows_per_image, c.Wp, c.lda, c.ldc, c.ldcx,
                             self.ldr if self.res else 0) == 1
        lib.call("siss_conv3x3_dgrad_sc", self.a, c.lda, self.Wd, self.cptr, c.ldc, self.r, self.ldr if self.res else 0, self.Wxd,
                 self.Xd[2 * c.ldcx:], c.ldcx, c.Nx, c.M, c.N, c.Kp, s, co, c.rows_per_image, c.Hp, c.Wp)


def workspace_counters_are_zero(dev):
    from siss_amd import lib
    assert not bool(lib.ensure_workspace(dev)[-4096:].any()), "a split-K launch left an arrival counter set"


def go(p, fn, kernel, what, launches=1):
    launch(fn, counts(kernel, launches))
    p.check(what)


# ================================================================ generic kernel, one panel, rows without a pixel structure
ONE_PANEL = [
    # M, N, Kp, bias, res, amp      (K loops of 1, 2, 3, 5 and 7 steps on the 4-deep ring; M % 128 in {1, 127}; N % 128 != 0)
    (1, 8, 64, False, None, "wide"),
    (1, 136, 448, True, "sep", "narrow"),
    (127, 72, 128, True, None, "narrow"),
    (127, 128, 320, False, "sep", "wide"),
    (129, 8, 192, True, "sep", "narrow"),
    (129, 136, 64, True, None, "wide"),
    (129, 128, 448, False, None, "narrow"),
    (257, 72, 320, False, "sep", "narrow"),
    (257, 136, 128, True, "sep", "wide"),
    (257, 128, 192, True, None, "narrow"),
    (257, 8, 64, False, "sep", "narrow"),
    (127, 136, 192, False, None, "narrow"),
]


@pytest.mark.parametrize("M,N,Kp,bias,res,amp", ONE_PANEL)
def test_one_panel_ring(dev, M, N, Kp, bias, res, amp):
    """lda > Kp with a non-zero column offset, ldc > N, ldr != ldc, alpha = 0.5."""
    c = R.Case(M=M, N=N, Kp=Kp, coffs=(16,), lda=16 + Kp + 8, ldc=N + 8, ldr=N + 24, alpha=0.5)
    assert plan(c) == (NT, 4, 1)
    p = Prob(c, dev, seed=M + N + Kp, amp=amp, bias=bias, res=res)
    go(p, p.gemm_nt, NT, f"{M}x{N}x{Kp}")


@pytest.mark.parametrize("cols", [4, 64, 132])
def test_alpha_cols(dev, cols):
    c = R.Case(M=129, N=192, Kp=128, lda=136, ldc=200, ldr=208, alpha=0.25, alpha_cols=cols)
    p = Prob(c, dev, seed=cols, amp="wide", bias=True, res="sep" if cols == 64 else None)
    go(p, p.alpha_cols, NT, f"alpha_cols {cols}")


def test_batched_with_strides_larger_than_the_operands(dev):
    M, N, Kp = 127, 72, 192
    c = R.Case(M=M, N=N, Kp=Kp, lda=Kp + 8, ldc=N + 8, ldr=N + 16, batch=3, strideA=(M + 3) * (Kp + 8), strideC=(M + 2) * (N + 16), alpha=2.0)
    p = Prob(c, dev, seed=7, amp="wide", bias=True, res="sep")
    go(p, p.gemm_nt, NT, "batch 3")


@pytest.mark.parametrize("amp", ["narrow", "wide"])
def test_mulsub(dev, amp):
    M, N, Kp = 77, 72, 64
    c = R.Case(M=M, N=N, Kp=Kp, lda=Kp + 8, ldc=N + 8, ldr=N + 16, batch=2, strideA=(M + 1) * (Kp + 8), strideC=(M + 2) * (N + 16),
               alpha=0.5, mul=True)
    p = Prob(c, dev, seed=8, amp=amp, rowsub=True, res="sep", ramp=16)
    go(p, p.mulsub, NT, "mulsub")


# ================================================================ panelled, with pixels
@pytest.mark.parametrize("n,hp,wp,N,Kp,coff,amp", [
    (5, 8, 8, 136, 64, 0, "wide"),          # 6 x 6 interiors, rows_per_image = 64: two images per tile, the last tile half empty
    (5, 8, 9, 72, 64, 64, "narrow"),        # 6 x 7: rows_per_image = 72, tile 1 spans THREE images; the concat view (coff = 64)
    (3, 16, 16, 72, 128, 0, "narrow"),      # 14 x 14; 18 steps on 6 tiles: split-K by 3, the reduce kernel with halo and row bias
    (2, 32, 32, 128, 64, 32, "wide"),       # 30 x 30
])
def test_conv3x3_small_grids(dev, n, hp, wp, N, Kp, coff, amp):
    """Row bias different per image, residual with a row stride of its own, a last tile that overhangs the last image."""
    c = conv_case(n, hp, wp, N, Kp, coff, ldr=N + 16, ldrb=N + 4)
    p = Prob(c, dev, seed=n + hp + wp, amp=amp, bias=True, rowbias=True, res="sep")
    go(p, p.gemm_nt, plan(c)[0], f"3x3 {n}x{hp}x{wp}")
    workspace_counters_are_zero(dev)


@pytest.mark.parametrize("n,hp,wp", [(1, 258, 258), (2, 5, 67), (2, 4, 131)])
def test_reciprocal_halo_test(dev, n, hp, wp):
    """(int)((rem + 0.5f) * inv_wp) must be the exact quotient at the largest grid and at widths that are no powers of two: one
    wrong row would turn a halo row into a value or a value into zero."""
    c = R.Case(M=n * hp * wp, N=8, Kp=64, lda=72, ldc=16, ldr=24, rows_per_image=hp * wp, Hp=hp, Wp=wp)
    assert plan(c)[1] == (1 if hp == 258 else 4)
    p = Prob(c, dev, seed=wp, res="sep")
    go(p, p.gemm_nt, NT, f"halo {hp}x{wp}")


# ================================================================ stage depths
@pytest.mark.parametrize("M,N,npanels,Kp,want,amp", [
    (16640, 512, 1, 64, (NT, 1, 1), "wide"),           # 520 tiles: four single-buffered blocks per CU
    (21889, 320, 1, 64, (WIDE, 1, 1), "wide"),         # 516 tiles of 128 x 128 -> 128 x 160 tiles
    (16640, 960, 1, 64, (WIDE, 1, 1), "narrow"),
    (8321, 512, 1, 64, (NT, 2, 1), "wide"),            # 264 tiles: the double-buffered form
    (8300, 136, 4, 384, (SPLITK, 2, 2), "wide"),       # 130 tiles, 24 steps: two splits on the double-buffered form
    (8300, 136, 1, 64, (NT, 4, 1), "narrow"),          # 130 tiles, one step: the unsplit ring
])
def test_stage_depths(dev, M, N, npanels, Kp, want, amp):
    shifts = (0,) if npanels == 1 else (-1, 0, 1, 2)
    c = R.Case(M=M, N=N, Kp=Kp, shifts=shifts, coffs=(8,) * npanels, lda=Kp + 16, ldc=N + 8, ldr=N + 8)
    assert plan(c) == want
    p = Prob(c, dev, seed=N, amp=amp, bias=True, res="sep")
    go(p, p.gemm_nt, want[0], f"{M}x{N} {want}")
    workspace_counters_are_zero(dev)


# ================================================================ split-K
def splitk_case(kind):
    if kind == "S2":
        return R.Case(M=300, N=136, Kp=256, shifts=(-1, 0, 1), coffs=(0,) * 3, lda=264, ldc=144, ldr=152), 2
    if kind == "S3":
        return R.Case(M=129, N=128, Kp=384, shifts=(-2, 0, 5), coffs=(8,) * 3, lda=400, ldc=136, ldr=136), 3
    if kind == "S5":                                   # 50 tiles, 36 steps: 256 / 50 = 5; 36 % 5 != 0
        return conv_case(1, 25, 127, 136, 256, ldr=152, ldrb=140), 5
    if kind == "S7":                                   # nine panels of five steps: 45 % 7 != 0, every split begins inside a panel
        return conv_case(5, 7, 11, 72, 320, ldr=88, ldrb=76), 7          # M = 385: M % 128 = 1
    if kind == "S8":
        return conv_case(3, 5, 47, 136, 384, ldr=152, ldrb=140), 8       # M = 705: M % 128 = 65; 54 % 8 != 0
    raise KeyError(kind)


@pytest.mark.parametrize("kind,amp", [("S2", "wide"), ("S3", "narrow"), ("S5", "narrow"), ("S7", "wide"), ("S8", "narrow")])
def test_split_k(dev, kind, amp):
    """Row bias + residual + halo through the reduce kernel's four row quarters; then the same product with the workspace withdrawn:
    it must run unsplit and give the same bits."""
    from siss_amd import lib
    c, S = splitk_case(kind)
    assert plan(c) == (SPLITK, 4, S) and plan(c, workspace=False) == (NT, 4, 1)
    p = Prob(c, dev, seed=S, amp=amp, bias=True, rowbias=c.Hp > 0, res="sep")
    go(p, p.gemm_nt, SPLITK, kind)
    workspace_counters_are_zero(dev)
    ws = lib.ensure_workspace(dev)
    try:
        assert lib.load().siss_gemm_nt_set_workspace(None, 0) == 0
        p.fresh()
        go(p, p.gemm_nt, NT, kind + " without a workspace")
    finally:
        assert lib.load().siss_gemm_nt_set_workspace(lib.C.c_void_p(ws.data_ptr()), ws.numel()) == 0
    workspace_counters_are_zero(dev)


# ================================================================ depth-to-space
def s2d_dgrad_panels(wp):
    """Per plane (0..3) the shifts of a stride-2, pad-1 3x3 convolution's dgrad over its space-to-depth planes: 1 / 2 / 2 / 4 taps."""
    planes = {}
    for ky in range(3):
        for kx in range(3):
            dy_, py, dx_, px = (ky - 1) >> 1, (ky - 1) & 1, (kx - 1) >> 1, (kx - 1) & 1
            planes.setdefault(py * 2 + px, []).append(-(dy_ * wp + dx_))
    return [tuple(planes[pl]) for pl in range(4)]


def phase_panels(wp):
    """Per phase the 2 x 2 taps of a sub-pixel upsample convolution (UNetEngine._upsample_subpixel)."""
    return [tuple((a + (pl >> 1) - 1) * wp + (b + (pl & 1) - 1) for a in range(2) for b in range(2)) for pl in range(4)]


def d2s_case(n, hp, wp, N, Kp, shifts, **kw):
    return R.Case(M=n * hp * wp, N=N, Kp=Kp, shifts=tuple(shifts), coffs=(0,) * len(shifts), lda=Kp + 8, ldc=N + 8, ldr=N + 16,
                  rows_per_image=hp * wp, Hp=hp, Wp=wp, **kw)


@pytest.mark.parametrize("plane", range(4))
@pytest.mark.parametrize("res", ["sep", "c"])
def test_d2s_planes(dev, plane, res):
    c = d2s_case(2, 7, 11, 72, 64, s2d_dgrad_panels(11)[plane], d2s=1 + plane)
    p = Prob(c, dev, seed=plane, amp="wide" if plane & 1 else "narrow", res=res)
    go(p, p.d2s, NT, f"d2s plane {plane} R {res}")


@pytest.mark.parametrize("plane", range(4))
def test_d2s_bias_phases_one_by_one(dev, plane):
    c = d2s_case(2, 7, 11, 72, 128, phase_panels(11)[plane], d2s=1 + plane)
    p = Prob(c, dev, seed=10 + plane, amp="narrow" if plane & 1 else "wide", bias=True)
    go(p, p.d2s, NT, f"d2s_bias phase {plane}")


@pytest.mark.parametrize("n,hp,wp,N,taps,res,want", [
    (2, 7, 11, 72, "1224", "c", (NT, 4, 1)),
    (2, 7, 11, 72, "4444", None, (NT, 4, 1)),
    (2, 7, 11, 72, "1224", "sep", (NT, 4, 1)),
    (1, 129, 129, 8, "1224", "c", (NT, 1, 1)),         # 131 row tiles x 4 phases = 524 blocks: the single-buffered form
    (1, 129, 131, 8, "4444", None, (NT, 1, 1)),
])
def test_d2s_four_planes_in_one_launch(dev, n, hp, wp, N, taps, res, want):
    per = s2d_dgrad_panels(wp) if taps == "1224" else phase_panels(wp)
    p0 = tuple(int(x) for x in np.cumsum([0] + [len(s) for s in per]))
    c = d2s_case(n, hp, wp, N, 64, sum(per, ()), d2s=1, phase_p0=p0)
    assert plan(c) == want
    p = Prob(c, dev, seed=hp + len(taps), amp="wide", bias=taps == "4444", res=res)
    go(p, p.d2s, NT, f"phases {taps} {hp}x{wp}")


# ================================================================ the persistent 3x3 kernel
def set_blocks(n):
    from siss_amd import lib
    assert lib.query("siss_gemm_nt_set_c3p_blocks", n) == (n or 256)


def qstats_check(p, q, what):
    c = p.c
    stored = p.stored()
    assert 512 * float(np.abs(stored).max()) ** 2 < 2.0 ** 24, "operands too wide: a statistics entry would not be exact in f32"
    want = R.qstats_entries(c, stored)
    got = q.cpu().double().numpy().reshape(want.shape)
    assert np.array_equal(got, want), what + ": statistics entries"
    assert np.array_equal(R.qstats_fold(c, got), R.image_sums(c, stored)), what + ": per-image fold"


def qstats_buffer(p):
    from siss_amd import lib
    words = lib.query("siss_conv_qstats_words", p.c.M, p.c.N)
    assert words == cdiv(p.c.M, R.QS_TILE) * 2 * 2 * (p.c.N // 4) * 2
    return torch.full((words,), float("nan"), dtype=F32, device=p.dev)


@pytest.mark.parametrize("n,hp,wp,N,Kp,bias,rowbias,res,amp", [
    (128, 16, 16, 128, 64, True, True, "sep", "wide"),      # rows_per_image = 256 against 254-row tiles: every tile straddles a seam
    (2, 128, 128, 128, 128, False, False, None, "wide"),    # M = 32,768: the eligibility floor; plain accumulators (the dgrad form)
    (2, 66, 131, 256, 192, True, False, "sep", "narrow"),   # N = 256, 17,292 rows, a width that is no power of two, three LDS slots' worth of K
    (128, 16, 16, 128, 192, False, True, None, "narrow"),
])
def test_persistent_kernel(dev, n, hp, wp, N, Kp, bias, rowbias, res, amp):
    """One tile per block (the default grid), four rounds with an uneven last one (40 blocks), and 17 rounds on 8 blocks."""
    c = conv_case(n, hp, wp, N, Kp, ldr=N + 16, ldrb=N + 4, alpha=0.5 if bias else 1.0)
    assert plan(c)[0] == C3P
    p = Prob(c, dev, seed=n + Kp, amp=amp, bias=bias, rowbias=rowbias, res=res)
    try:
        for blocks in (0, 40, 8):
            set_blocks(blocks)
            p.fresh()
            go(p, p.gemm_nt, C3P, f"c3p {n}x{hp}x{wp} N {N} Kp {Kp} blocks {blocks}")
    finally:
        set_blocks(0)


@pytest.mark.parametrize("n,hp,wp,N,res,blocks", [(128, 16, 16, 128, "sep", 0), (2, 66, 131, 256, None, 40)])
def test_persistent_kernel_statistics(dev, n, hp, wp, N, res, blocks):
    c = conv_case(n, hp, wp, N, 64, ldr=N + 16, ldrb=N + 4)
    p = Prob(c, dev, seed=n, amp="unit", bias=True, rowbias=True, res=res, ramp=16, bamp=8)
    q = qstats_buffer(p)
    try:
        set_blocks(blocks)
        written = []
        launch(lambda: written.append(p.qstats(q)), counts(C3P))
    finally:
        set_blocks(0)
    assert written == [1]
    p.check("c3p with statistics")
    qstats_check(p, q, "c3p")


@pytest.mark.parametrize("Kp,K2,bias2,rowbias,stats,amp", [
    (64, 128, True, True, True, "unit"),
    (128, 64, False, False, False, "wide"),
    (64, 128, True, False, False, "wide"),
])
def test_conv3x3_sc(dev, Kp, K2, bias2, rowbias, stats, amp):
    """The folded 1x1 shortcut: ONE rounding of conv3x3 + conv1x1 + both biases (the two-launch form rounds the shortcut first)."""
    c = conv_case(128, 16, 16, 128, Kp, ldrb=132, K2=K2, lda2=K2 + 16)
    assert plan(c)[0] == C3P
    p = Prob(c, dev, seed=Kp, amp=amp, bias=True, bias2=bias2, rowbias=rowbias, bamp=8 if stats else 64)
    q = qstats_buffer(p) if stats else None
    written = []
    launch(lambda: written.append(p.sc(q)), counts(C3P))
    assert written == [1 if stats else 0]
    p.check(f"conv3x3_sc Kp {Kp} K2 {K2}")
    if stats:
        qstats_check(p, q, "conv3x3_sc")


@pytest.mark.parametrize("Nx,res,amp", [(128, None, "wide"), (256, "sep", "narrow"), (256, None, "wide")])
def test_conv3x3_dgrad_sc(dev, Nx, res, amp):
    c = conv_case(128, 16, 16, 128, 128, ldr=144, Nx=Nx, ldcx=Nx + 8)
    assert plan(c)[0] == C3P
    p = Prob(c, dev, seed=Nx, amp=amp, res=res)
    go(p, p.dgrad_sc, C3P, f"dgrad_sc Nx {Nx}")
    _, _, _, halo = R.pixel(c, np.arange(c.M))
    assert not p.Xd[2 * c.ldcx:2 * c.ldcx + c.M * c.ldcx].view(c.M, c.ldcx)[torch.from_numpy(halo).to(dev), :Nx].any()


# ================================================================ the f32 entry points: exact integers, no rounding
def test_f32_entry_points(dev):
    from siss_amd import lib
    none = counts(None)
    with lib.f32_mode(True):
        c = R.Case(M=129, N=72, Kp=64, coffs=(16,), lda=88, ldc=80, ldr=96, alpha=0.5, batch=2, strideA=131 * 88, strideC=131 * 96)
        p = Prob(c, dev, seed=1, amp="wide", bias=True, res="sep", f32=True)
        go(p, p.gemm_nt, None, "f32 gemm_nt")
        c = conv_case(5, 8, 9, 72, 64, 16, ldr=88, ldrb=76)
        p = Prob(c, dev, seed=2, amp="wide", bias=True, rowbias=True, res="sep", f32=True)
        go(p, p.gemm_nt, None, "f32 3x3")
        c = R.Case(M=77, N=72, Kp=64, lda=72, ldc=80, ldr=88, batch=2, strideA=78 * 72, strideC=79 * 88, alpha=0.5, mul=True)
        p = Prob(c, dev, seed=3, amp="narrow", rowsub=True, res="sep", ramp=16, f32=True)
        go(p, p.mulsub, None, "f32 mulsub")
        for plane in (0, 3):
            c = d2s_case(2, 7, 11, 72, 64, s2d_dgrad_panels(11)[plane], d2s=1 + plane)
            p = Prob(c, dev, seed=4 + plane, amp="wide", res="c", f32=True)
            go(p, p.d2s, None, "f32 d2s")
            c = d2s_case(2, 7, 11, 72, 64, phase_panels(11)[plane], d2s=1 + plane)
            p = Prob(c, dev, seed=8 + plane, amp="wide", bias=True, f32=True)
            go(p, p.d2s, None, "f32 d2s_bias")
        per = s2d_dgrad_panels(11)
        c = d2s_case(2, 7, 11, 72, 64, sum(per, ()), d2s=1, phase_p0=(0, 1, 3, 5, 9))
        p = Prob(c, dev, seed=12, amp="wide", res="sep", f32=True)
        go(p, p.d2s, None, "f32 d2s_phases")
        c = conv_case(3, 16, 16, 72, 64, ldrb=76, K2=128, lda2=144)
        p = Prob(c, dev, seed=13, amp="wide", bias=True, bias2=True, rowbias=True, f32=True)
        launch(p.sc, none)
        p.check("f32 conv3x3_sc")
        c = conv_case(3, 16, 16, 72, 128, ldr=88, Nx=136, ldcx=144)
        p = Prob(c, dev, seed=14, amp="wide", res="sep", f32=True)
        go(p, p.dgrad_sc, None, "f32 conv3x3_dgrad_sc")

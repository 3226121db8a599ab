"""The weight-gradient family of csrc/gemm_tn.hip called DIRECTLY at its C entry points, every launch form and store mode, BITWISE
against tests/wgrad_ref.py (which tests/test_wgrad_ref_host.py pins to torch.autograd on the CPU).

csrc/gemm_tn.hip   siss_gemm_tn (gemm_tn_kernel<1>, gemm_tn_kernel<3> in its interleaved 4-deep-ring form), siss_gemm_tn_bs,
                   siss_gemm_tn_grouped, siss_gemm_tn_grouped_capped, siss_gemm_tn_pair (gemm_tn_mixed_kernel),
                   siss_gemm_tn_overwrite_log; store modes: atomics (explicit splits), read-add-write (0 on one split), overwrite (-1,
                   -2 on one split)
csrc/f32_path.hip  siss_gemm_tn_f32, siss_gemm_tn_bs_f32, siss_gemm_tn_grouped_f32 (through lib.f32_mode)

Why bitwise: Y and X hold integers in [-4, 4], the priors integers in [-8, 8], and at most 8400 rows are reduced: every product, every
partial sum in whatever order, every split's tile and every atomic add is an integer of magnitude below 8400 * 16 + 8 < 2^18 -- exact
in bf16 operands, in the MFMA's f32 accumulators and in f32 memory.  The result is therefore independent of split count, summation
order and atomics, and must equal the int64 reference bit for bit: ONE dropped or double-counted row anywhere changes it.  There is
no tolerance in this module.

What lies around the operands: every entry of Y and X outside the job's needed masks (wgrad_ref.needed_masks: rows outside
[row_begin, row_end), the columns [N, ldy) of Y, the X columns outside the panels' windows, guard rows, the rows between sets) is
NaN -- the kernels promise that nothing out of range reaches an MFMA ("0 * garbage could be NaN"), and the buffer pool relies on it.
dW, dbias and dbias2 live in sentinel-filled flat buffers with set strides larger than the sets, and the WHOLE buffers are compared:
ragged N / C tiles store nothing past N / C, no set writes into another's stride, the bias gradients ALWAYS accumulate (also under
-1 and -2) and come from c-tile 0 only.  lib.dispatch_counts is asserted for every launch: no case can silently move to another kernel.
"""
import math

import numpy as np
import pytest
import torch

import wgrad_ref as R
from siss_amd.layout import conv3x3_panels

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENT = -12345.0
TN1, TN3, PAIR = "gemm_tn_kernel<1>", "gemm_tn_kernel<3>", "gemm_tn_pair"
BN = BC = 128                        # the kernels' output tile; BR = 64 reduction rows per step
MAX_JOBS = 14                        # kMaxJobs of a grouped launch
SEEN_MINUS_TWO = set()               # outcomes of nsplits = -2 seen in this module: "overwrote", "split"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def panels(kind, C):
    """(shifts, coffs, ldx or None) of a named panel structure."""
    if kind == "p1":
        return (0,), (0,), None
    if kind == "p3":                                   # one filter row
        return (-1, 0, 1), (0, 0, 0), None
    if kind in ("p9w6", "p9w18"):
        s, c = conv3x3_panels(int(kind[3:]), C)
        return tuple(s), tuple(c), None
    if kind in ("ph4w6", "ph4w18"):                    # a 2 x 2 phase of a sub-pixel upsample: no triples
        wp = int(kind[4:])
        return (-wp - 1, -wp, -1, 0), (0, 0, 0, 0), None
    if kind == "s2d4":                                 # four space-to-depth planes: channel offsets into an X of 4 C columns
        return (-7, -6, -1, 0), (0, C, 2 * C, 3 * C), 4 * C
    if kind == "gap3":                                 # three panels, shifts NOT consecutive: the one-tap kernel
        return (-5, 0, 4), (0, 0, 0), None
    raise KeyError(kind)


def is_triples(shifts, coffs):
    return len(shifts) % 3 == 0 and all(shifts[g + 1] == shifts[g] + 1 and shifts[g + 2] == shifts[g] + 2 and
                                        coffs[g] == coffs[g + 1] == coffs[g + 2] for g in range(0, len(shifts), 3))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (what, got.shape, want.shape)
    ne = bits(got) != bits(want)
    if bool(ne.any()):
        i = ne.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, the first at flat index {i}: "
                             f"got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}")


def f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(F32)


class Out:
    """A flat f32 output buffer: sentinels everywhere but the stretches [off + s * stride, + n) of the sets, which hold the prior
    (integers in [-8, 8], or NaN for the overwriting modes).  `off` is odd on purpose: dW is only 4-byte aligned in the engine too."""

    def __init__(self, n, nsets, stride, nan, seed, off=5, tail=9):
        rng = np.random.default_rng(seed)
        self.off, self.n, self.nsets, self.stride = off, n, nsets, stride
        self.prior = np.full(off + (nsets - 1) * stride + max(n, stride) + tail, SENT)
        for s in range(nsets):
            self.prior[off + s * stride:off + s * stride + n] = np.nan if nan else rng.integers(-8, 9, n)

    def to(self, dev):
        self.d = f32(self.prior).to(dev)
        return self

    @property
    def t(self):
        return self.d[self.off:]

    def check(self, want, what):
        same(self.d.cpu(), f32(want), what)


class Prob:
    """One weight-gradient job: integer operands with their guard rows, the reference's products (computed once), the NaN-masked
    device operands.  bias: None | "one" (dbias) | "two" (dbias and dbias2) | "stride" (dbias with a bias_set_stride of its own).
    xset: "shared" (x_set_rows = 0) | "own" (rows_per_set) | "odd" (an unrelated stride, as the attention call sites pass it)."""

    def __init__(self, N, C, kind, nsets, xset, rows, rb, tail, bias, seed, y_of=None):
        rng = np.random.default_rng(seed)
        shifts, coffs, ldx = panels(kind, C)
        assert rows <= 8400                              # (the integer argument of the module docstring)
        rps = rb + rows + tail
        xsr = {"shared": 0, "own": rps, "odd": rps + 11}[xset]
        self.ldy = -(-N // 8) * 8 + 8                    # columns [N, ldy) exist and are NaN
        ldx = ldx or max(coffs) + C + 8
        floats = len(shifts) * N * C
        self.bias, self.nan = bias, False
        self.bstride = N + 3 if bias == "stride" else floats + 40
        self.j = R.Job(N=N, C=C, shifts=shifts, coffs=coffs, nsets=nsets, rows_per_set=rps, row_begin=rb, row_end=rb + rows,
                       x_set_rows=xsr, ldy=self.ldy, ldx=ldx, set_stride=floats + 40,
                       bias_set_stride=self.bstride if bias == "stride" else 0)
        self.triples = is_triples(shifts, coffs)
        if y_of is None:
            self.y0 = 3
            self.Y = rng.integers(-4, 5, (self.y0 + nsets * rps + 3, self.ldy))
        else:                                            # the pair: two jobs over one cotangent
            assert (y_of.ldy, y_of.j.rows_per_set, y_of.j.nsets) == (self.ldy, rps, nsets)
            self.y0, self.Y = y_of.y0, y_of.Y
        lo = min(0, rb + min(shifts))
        hi = (nsets - 1) * xsr + rb + rows + max(max(shifts), 0)
        self.x0 = 2 - lo
        self.X = rng.integers(-4, 5, (self.x0 + hi + 3, ldx))
        self.prods = R.products(self.Y, self.y0, self.X, self.x0, self.j)
        self.my, self.mx = R.needed_masks(self.j, self.Y.shape, self.y0, self.X.shape, self.x0)
        assert not self.my.all() and not self.mx.all() and not self.my[:, N:].any()
        self.seed = seed

    def operands(self, dev, dt=BF, my=None):
        """Device Y and X, NaN outside the needed masks."""
        self.Yd = torch.from_numpy(np.where(self.my if my is None else my, self.Y, np.nan)).to(dt).to(dev)
        self.Xd = torch.from_numpy(np.where(self.mx, self.X, np.nan)).to(dt).to(dev)
        return self

    def outputs(self, dev, nan):
        """Fresh sentinel-guarded dW / dbias / dbias2 (nan: the dW sets pre-filled with NaN instead of integers)."""
        j = self.j
        self.nan = nan
        self.dW = Out(j.floats, j.nsets, j.set_stride, nan, self.seed + 1).to(dev)
        self.b1 = Out(j.N, j.nsets, self.bstride, False, self.seed + 2, off=3).to(dev) if self.bias else None
        self.b2 = Out(j.N, j.nsets, self.bstride, False, self.seed + 3, off=1).to(dev) if self.bias == "two" else None
        return self

    def args(self, nsplits, zp):
        """The argument list of siss_gemm_tn (siss_gemm_tn_bs's with the bias stride when the job has one)."""
        from siss_amd import lib
        j = self.j
        a = [self.Yd[self.y0:], j.ldy, self.Xd[self.x0:], j.ldx, self.dW.t, j.set_stride, j.N, j.C, j.npanels,
             lib.int_array(list(j.shifts)), lib.int_array(list(j.coffs)), j.nsets, j.rows_per_set, j.x_set_rows, j.row_begin,
             j.row_end, nsplits, zp, self.b1.t if self.b1 else None, self.b2.t if self.b2 else None]
        return a + ([j.bias_set_stride] if j.bias_set_stride else [])

    def job(self, nsplits, zp):
        from siss_amd import lib
        j = self.j
        pad9 = lambda v: (lib.I * 9)(*v, *([0] * (9 - len(v))))
        t = lib.TNJob(Y=self.Yd[self.y0:].data_ptr(), ldy=j.ldy, X=self.Xd[self.x0:].data_ptr(), ldx=j.ldx, dW=self.dW.t.data_ptr(),
                      set_stride=j.set_stride, N=j.N, C=j.C, npanels=j.npanels, nsets=j.nsets, rows_per_set=j.rows_per_set,
                      row_begin=j.row_begin, row_end=j.row_end, nsplits=nsplits, x_set_rows=j.x_set_rows, zero_page=zp.data_ptr(),
                      dbias=self.b1.t.data_ptr() if self.b1 else None, dbias2=self.b2.t.data_ptr() if self.b2 else None,
                      shifts=pad9(j.shifts), coffs=pad9(j.coffs), bias_set_stride=j.bias_set_stride)
        return t

    def records(self):
        return R.overwrite_records(self.j, self.dW.t.data_ptr())

    def check(self, overwrite, what):
        """All three whole buffers against the reference.  A job that left its dW untouched passes overwrite=None."""
        if overwrite is None:
            want = (self.dW.prior, self.b1.prior if self.b1 else None, self.b2.prior if self.b2 else None)
        else:
            want = R.store(self.prods, self.j, self.dW.prior, self.dW.off, overwrite, self.b1.prior if self.b1 else None,
                           self.b1.off if self.b1 else 0, self.b2.prior if self.b2 else None, self.b2.off if self.b2 else 0)
            assert np.isfinite(want[0][self.dW.off:self.dW.off + self.j.floats]).all()
        self.dW.check(want[0], what + ": dW")
        if self.b1:
            self.b1.check(want[1], what + ": dbias")
        if self.b2:
            self.b2.check(want[2], what + ": dbias2")


def counts_are(tn1, tn3, pair=0):
    from siss_amd import lib
    cnt = lib.dispatch_counts(reset=True)
    assert (cnt[TN1], cnt[TN3], cnt[PAIR]) == (tn1, tn3, pair), cnt


def drain():
    from siss_amd import lib
    log = lib.overwrite_log()
    assert log is not None
    return log


def zero_page(dev, dt=BF):
    from siss_amd import ops
    return ops.zero_page(dev)


def expected_variant(p, nsplits):
    """Explicit splits and -1 take the variant the panel structure gives.  The automatic modes (0, -2) run the cost model of tn_setup:
    from 8192 rows on triples stay on <3> (the one-tap variant is not considered); below, both are costed with the same split
    counts, the same rounds (one, while 9 x the base grid fits 256 blocks) and the same store term, at 0.6 us per step against 1.5:
    the one-tap variant wins at every split count."""
    if not p.triples:
        return TN1
    if nsplits > 0 or nsplits == -1 or p.j.rows >= 8192:
        return TN3
    base1 = math.ceil(p.j.N / BN) * math.ceil(p.j.C / BC) * p.j.npanels * p.j.nsets
    assert base1 * max(1, p.j.rows // 256) <= 256
    return TN1


def run_single(dev, p, nsplits, dt="bf16", nan=None):
    """One siss_gemm_tn / siss_gemm_tn_bs launch of `p` and every check of its store mode."""
    from siss_amd import lib
    f = dt == "f32"
    nan = (nsplits == -1 or (nsplits == -2 and not f)) if nan is None else nan
    p.operands(dev, F32 if f else BF).outputs(dev, nan)
    zp = zero_page(dev)
    drain()
    lib.dispatch_counts(reset=True)
    with lib.f32_mode(f):
        lib.call("siss_gemm_tn_bs" if p.j.bias_set_stride else "siss_gemm_tn", *p.args(nsplits, zp))
    torch.cuda.synchronize()
    log = drain()
    v = expected_variant(p, nsplits)
    counts_are(*((0, 0) if f else (int(v == TN1), int(v == TN3))))
    what = f"N {p.j.N} C {p.j.C} panels {p.j.shifts} rows [{p.j.row_begin}, {p.j.row_end}) sets {p.j.nsets} nsplits {nsplits} {dt}"
    if f:                                               # the f32 instrument: -1 overwrites, everything else accumulates; it keeps no log
        assert log == []
        p.check(nsplits == -1, what)
    elif nsplits == -1:
        assert log == p.records(), (log, p.records())
        p.check(True, what)
    elif nsplits == -2:
        if log:
            assert log == p.records(), (log, p.records())
            SEEN_MINUS_TWO.add("overwrote")
            p.check(True, what)
        else:
            SEEN_MINUS_TWO.add("split")
            p.check(False, what)
    else:
        assert log == []
        p.check(False, what)


# ================================================================ siss_gemm_tn / siss_gemm_tn_bs: one launch
# (N, C, panels, nsets, xset, rows, row_begin, rows after row_end, bias, nsplits)
#   rows 1 .. 613 = 1 .. 10 steps of 64: the 4-deep ring's prologue (steps > 1, > 2), one full wrap, a wrap plus a ragged step, and
#   the two-buffer ring of <1>; row_begin 0 / 3 / 37 / 70; (N, C) ragged below and above one tile, 2 x 2 tiles with both edges ragged,
#   several c-tiles (the bias gradient must come from c-tile 0 only); explicit splits with EMPTY trailing splits (64 rows in 2, 128
#   in 3, 100 and 192 in 7).  8200 rows: the automatic modes on <3>.
SINGLE = [
    # ---- panel triples: <3> under explicit splits and -1 (asserted), <1> under 0 / -2 below 8192 rows (asserted)
    (128, 128, "p3", 1, "shared", 1, 0, 5, None, 1),
    (27, 128, "p9w6", 2, "shared", 63, 3, 5, "one", -1),
    (64, 8, "p3", 1, "shared", 64, 37, 2, "two", 2),
    (136, 120, "p9w18", 2, "own", 65, 70, 5, "one", 1),
    (200, 136, "p3", 2, "odd", 128, 3, 7, "stride", 3),
    (128, 320, "p3", 1, "shared", 129, 0, 0, "one", -1),
    (256, 64, "p9w6", 1, "shared", 192, 37, 5, "two", 7),
    (128, 128, "p9w18", 2, "shared", 256, 70, 3, None, 1),
    (27, 128, "p3", 1, "shared", 257, 3, 5, "one", 2),
    (136, 120, "p3", 2, "own", 320, 37, 1, "stride", -1),
    (128, 128, "p9w6", 2, "odd", 613, 70, 5, "two", 1),
    (200, 136, "p3", 1, "shared", 613, 0, 9, "one", 3),
    (128, 128, "p3", 1, "shared", 100, 3, 5, "one", 7),
    (128, 128, "p3", 1, "shared", 320, 0, 4, None, 1),
    (128, 320, "p9w6", 1, "shared", 256, 3, 5, "one", -1),
    (128, 128, "p3", 1, "shared", 192, 37, 0, "one", 3),
    (128, 128, "p3", 1, "shared", 8200, 37, 5, "one", 0),
    (128, 128, "p3", 1, "shared", 8200, 3, 5, None, -2),
    (128, 128, "p9w6", 2, "shared", 192, 70, 5, "one", 0),
    (128, 128, "p3", 1, "shared", 511, 3, 5, "one", -2),
    (200, 136, "p9w18", 1, "shared", 256, 37, 5, "two", -2),
    # ---- everything else: <1>
    (27, 128, "p1", 1, "shared", 1, 3, 5, "one", 0),
    (128, 128, "ph4w6", 2, "shared", 63, 37, 5, "two", -2),
    (136, 120, "s2d4", 1, "shared", 64, 70, 5, None, 1),
    (64, 8, "gap3", 1, "shared", 65, 0, 5, "one", -1),
    (128, 320, "p1", 2, "own", 128, 3, 5, "stride", 2),
    (200, 136, "p1", 1, "shared", 129, 37, 5, "one", -2),
    (256, 64, "gap3", 1, "shared", 256, 0, 0, None, 3),
    (27, 128, "s2d4", 2, "odd", 257, 3, 5, "one", -2),
    (64, 8, "p1", 1, "shared", 320, 37, 5, "two", 7),
    (128, 128, "p1", 1, "shared", 613, 70, 5, "one", 0),
    (136, 120, "ph4w18", 2, "own", 613, 3, 5, "stride", 1),
    (27, 128, "p1", 1, "shared", 100, 0, 5, "one", 7),
    (128, 128, "p1", 2, "odd", 128, 0, 5, None, -1),
    (200, 136, "ph4w6", 1, "shared", 192, 70, 5, "one", 0),
]


@pytest.mark.parametrize("N,C,kind,nsets,xset,rows,rb,tail,bias,nsplits", SINGLE)
def test_single_launch(dev, N, C, kind, nsets, xset, rows, rb, tail, bias, nsplits):
    # (-2: NaN pre-fill up to 511 rows -- below 512 rows tn_setup's max_ns is 1, so the product overwrites by construction)
    p = Prob(N, C, kind, nsets, xset, rows, rb, tail, bias, seed=rows * 7 + N + C)
    run_single(dev, p, nsplits, nan=(rows <= 511) if nsplits == -2 else None)


def test_both_outcomes_of_minus_two(dev):
    """nsplits = -2 on 4096 rows into ONE 128 x 128 tile on an integer pre-fill (today's cost model splits it: no log record, prior +
    product) and on 511 rows (one split by construction: logged, product alone) -- and the module has then seen both outcomes."""
    run_single(dev, Prob(128, 128, "p1", 1, "shared", 4096, 37, 5, "one", seed=41), -2, nan=False)
    run_single(dev, Prob(128, 128, "p1", 1, "shared", 511, 0, 5, "two", seed=42), -2, nan=True)
    assert SEEN_MINUS_TWO == {"overwrote", "split"}, SEEN_MINUS_TWO


# ================================================================ the f32 instrument (csrc/f32_path.hip)
F32_CASES = [
    (136, 120, "p1", 1, "shared", 65, 3, 5, "one", 0),          # ragged N and C
    (27, 128, "p9w6", 1, "shared", 129, 37, 5, "one", -1),      # nine panels, overwrite
    (64, 8, "p3", 2, "own", 257, 70, 5, None, 0),               # two sets on their own rows
    (128, 128, "ph4w6", 2, "shared", 63, 0, 5, "two", 0),       # dbias2
    (200, 136, "p1", 2, "odd", 192, 3, 5, "stride", 2),         # siss_gemm_tn_bs_f32
]


@pytest.mark.parametrize("N,C,kind,nsets,xset,rows,rb,tail,bias,nsplits", F32_CASES)
def test_single_launch_f32(dev, N, C, kind, nsets, xset, rows, rb, tail, bias, nsplits):
    run_single(dev, Prob(N, C, kind, nsets, xset, rows, rb, tail, bias, seed=rows * 5 + N), nsplits, dt="f32")


# ================================================================ siss_gemm_tn_grouped / _capped: one job table
# 17 three-tap jobs (two launches: a launch takes 14) and 3 one-tap jobs; blocks per job 1, 2, 3, 4, 9, 18 ...: hardly a multiple of 8;
# rows mixed so that longest-first differs from table order; -2, 0 and explicit splits in one table; one job with a bias stride;
# one one-panel job of 8300 rows, which the grouped launcher splits in two (128 steps of 64 rows per block at most).
TABLE = [
    # (N, C, panels, nsets, xset, rows, row_begin, bias, nsplits)
    (128, 128, "p3", 1, "shared", 65, 3, "one", -2),
    (128, 128, "p9w6", 1, "shared", 613, 0, "one", 0),
    (27, 128, "p9w18", 1, "shared", 1, 37, None, -2),
    (128, 320, "p9w6", 1, "shared", 257, 70, "one", 0),
    (128, 320, "p9w6", 2, "own", 128, 3, "two", -2),
    (136, 120, "p3", 1, "shared", 320, 0, "one", 2),
    (64, 8, "p3", 2, "shared", 63, 37, None, 0),
    (200, 136, "p3", 1, "shared", 192, 70, "stride", -2),
    (128, 128, "p9w18", 2, "odd", 129, 3, "one", 0),
    (256, 64, "p3", 1, "shared", 256, 0, "one", -2),
    (128, 128, "p3", 1, "shared", 64, 37, None, 3),
    (27, 128, "p3", 2, "shared", 511, 70, "one", -2),
    (128, 128, "p3", 1, "shared", 100, 3, "one", 0),
    (128, 128, "p9w6", 1, "shared", 200, 0, "two", -2),
    (136, 120, "p9w6", 1, "shared", 37, 37, "one", 0),
    (128, 128, "p3", 1, "shared", 700, 70, "one", -2),
    (64, 8, "p9w6", 1, "shared", 450, 3, None, 0),
    (128, 128, "p1", 1, "shared", 8300, 37, "one", -2),
    (136, 136, "s2d4", 2, "shared", 129, 0, "one", 0),
    (27, 128, "p1", 1, "shared", 300, 3, "stride", -2),
]


def table_nsplits(p, nsplits):
    """The split count a GROUPED launch gives a job: its own when explicit, else one per 128 steps of 64 rows."""
    return nsplits if nsplits > 0 else max(1, math.ceil(p.j.rows / (128 * 64)))


def table_overwrites(p, nsplits):
    return nsplits == -2 and table_nsplits(p, nsplits) == 1


def launch_totals(table, taps):
    """The block arithmetic of launch_tn_group restated: the grid of every launch of one variant -- jobs longest-first (stable) by
    rows per split, dealt round-robin to ceil(n / 14) launches, every job's block count rounded up to 8."""
    jobs = []
    for p, ns in table:
        if p.triples != (taps == 3):
            continue
        ns = table_nsplits(p, ns)
        rps = math.ceil(math.ceil(p.j.rows / ns) / 64) * 64
        jobs.append((rps, math.ceil(p.j.N / BN) * math.ceil(p.j.C / BC) * (p.j.npanels // taps) * p.j.nsets * ns))
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][0])
    nl = math.ceil(len(jobs) / MAX_JOBS)
    return [sum((jobs[i][1] + 7) & ~7 for i in order[l::nl]) for l in range(nl)], [b for _, b in jobs]


@pytest.fixture(scope="module")
def table(dev):
    """The table's problems with their operands on the device and their products from the reference, shared by every run."""
    out = []
    for k, (N, C, kind, nsets, xset, rows, rb, bias, ns) in enumerate(TABLE):
        p = Prob(N, C, kind, nsets, xset, rows, rb, 5, bias, seed=1000 + k)
        assert p.triples == (k < 17)
        out.append((p.operands(dev), ns))
    return out


def run_table(dev, table, entry, *extra, stream=None):
    from siss_amd import lib
    zp = zero_page(dev)
    jobs = []
    for p, ns in table:
        p.outputs(dev, nan=table_overwrites(p, ns) and p.j.rows <= 511)
        jobs.append(p.job(ns, zp))
    arr = (lib.TNJob * len(jobs))(*jobs)
    drain()
    lib.dispatch_counts(reset=True)
    torch.cuda.synchronize()
    if stream is None:
        lib.call(entry, arr, len(jobs), *extra)
    else:
        with torch.cuda.stream(stream):
            lib.call(entry, arr, len(jobs), *extra)
    torch.cuda.synchronize()
    counts_are(3, 17)
    log = drain()
    where = dict(log)
    assert len(where) == len(log)
    for k, (p, ns) in enumerate(table):
        recs = p.records()
        hit = [a in where for a, _ in recs]
        what = f"{entry}{extra} job {k}"
        if ns == -2 and all(hit):
            assert [(a, where.pop(a)) for a, _ in recs] == recs, what
            p.check(True, what)
        else:
            assert not any(hit), what
            assert not p.nan, what + ": a -2 job of one split did not overwrite"
            p.check(False, what)
    assert not where, f"{entry}: records of no job: {where}"
    assert sum(table_overwrites(p, ns) for p, ns in table) == 9       # (what the table is meant to mix)


def test_grouped(dev, table):
    totals3, blocks3 = launch_totals(table, 3)
    totals1, blocks1 = launch_totals(table, 1)
    assert len(totals3) == 2 and len(totals1) == 1 and len(blocks3) == 17 and blocks1[0] == 2      # (8300 rows: two splits)
    assert {1, 3, 9, 18} <= set(blocks3) and sum(b % 8 != 0 for b in blocks3 + blocks1) >= 16
    run_table(dev, table, "siss_gemm_tn_grouped")


@pytest.mark.parametrize("max_blocks,side", [(8, False), (16, False), (4096, False), (8, True)])
def test_grouped_capped(dev, table, max_blocks, side):
    """max_blocks workgroups walk all blocks of a launch (the one-tap launch gets twice the cap); at or above the total the uncapped
    kernel runs; once on a stream of its own."""
    totals3, _ = launch_totals(table, 3)
    totals1, _ = launch_totals(table, 1)
    if max_blocks == 8:            # the capped kernels run: every launch has at least three blocks per workgroup / more than its cap
        assert min(totals3) >= 24 and min(totals1) > 16, (totals3, totals1)
    elif max_blocks == 16:
        assert min(totals3) > 16 and min(totals1) > 32, (totals3, totals1)
    else:
        assert max(totals3 + totals1) <= max_blocks
    run_table(dev, table, "siss_gemm_tn_grouped_capped", max_blocks, stream=torch.cuda.Stream() if side else None)


@pytest.mark.parametrize("max_blocks", [0, 4, 12])
def test_grouped_capped_refuses(dev, table, max_blocks):
    from siss_amd import lib
    zp = zero_page(dev)
    sub = table[:2] + table[-1:]
    arr = (lib.TNJob * len(sub))(*[p.outputs(dev, nan=False).job(ns, zp) for p, ns in sub])
    drain()
    lib.dispatch_counts(reset=True)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_gemm_tn_grouped_capped", arr, len(sub), max_blocks)
    torch.cuda.synchronize()
    counts_are(0, 0)
    assert drain() == []
    for p, _ in sub:
        p.check(None, f"refused max_blocks {max_blocks}")


def test_grouped_f32(dev):
    """siss_gemm_tn_grouped_f32 through f32_mode: the table walked on the host; 0 and -2 accumulate, -1 overwrites, the bias stride."""
    from siss_amd import lib
    zp = zero_page(dev)
    spec = [(136, 120, "p9w6", 2, "shared", 65, 3, "one", 0), (27, 128, "p1", 1, "shared", 300, 37, "stride", -2),
            (128, 128, "ph4w6", 2, "own", 129, 0, "two", -1)]
    probs = [(Prob(N, C, kind, nsets, xset, rows, rb, 5, bias, seed=2000 + k).operands(dev, F32).outputs(dev, nan=ns == -1), ns)
             for k, (N, C, kind, nsets, xset, rows, rb, bias, ns) in enumerate(spec)]
    arr = (lib.TNJob * len(probs))(*[p.job(ns, zp) for p, ns in probs])
    drain()
    lib.dispatch_counts(reset=True)
    with lib.f32_mode(True):
        lib.call("siss_gemm_tn_grouped", arr, len(probs))
    torch.cuda.synchronize()
    counts_are(0, 0)
    assert drain() == []
    for k, (p, ns) in enumerate(probs):
        p.check(ns == -1, f"grouped f32 job {k}")


# ================================================================ siss_gemm_tn_pair: a nine-panel and a one-panel job in one launch
def pair_problems(dev, rows3, rows1, C3, C1, nsets):
    """A 3x3 filter's job and a one-panel job over the SAME cotangent (N = 27: conv_out's), both with bias gradients; the one-panel
    job may reduce a shorter range of it.  Y is NaN outside the UNION of the two jobs' needs."""
    rb, tail = 37, 5
    p3 = Prob(27, C3, "p9w6", nsets, "shared", rows3, rb, tail, "one", seed=rows3 + C3)
    p1 = Prob(27, C1, "p1", nsets, "own", rows1, rb, tail + rows3 - rows1, "two", seed=rows1 + C1 + 1, y_of=p3)
    my = p3.my | p1.my
    p3.operands(dev, my=my)
    p1.operands(dev, my=my)
    p1.Yd = p3.Yd
    return p3, p1


@pytest.mark.parametrize("rows3,rows1,max_blocks", [(200, 200, 16), (200, 200, 24), (200, 200, 64), (200, 200, 0), (613, 129, 24),
                                                     (613, 129, 0)])
def test_pair(dev, rows3, rows1, max_blocks):
    """With 4 (10, 3) steps of 64 rows per product and up to one block per CU the search hands out far more splits than steps: empty
    splits, barrier-only steps in the paired half, dead blocks from the round-up to 8.  Atomics throughout: prior + product."""
    from siss_amd import lib
    p3, p1 = pair_problems(dev, rows3, rows1, 128, 64 if rows1 == 200 else 320, 2)
    zp = zero_page(dev)
    p3.outputs(dev, nan=False)
    p1.outputs(dev, nan=False)
    j3, j1 = p3.job(0, zp), p1.job(0, zp)
    drain()
    lib.dispatch_counts(reset=True)
    lib.call("siss_gemm_tn_pair", lib.C.byref(j3), lib.C.byref(j1), max_blocks)
    torch.cuda.synchronize()
    counts_are(1, 1, 1)
    assert drain() == []
    p3.check(False, f"pair {rows3}/{rows1} max_blocks {max_blocks}: nine-panel job")
    p1.check(False, f"pair {rows3}/{rows1} max_blocks {max_blocks}: one-panel job")


@pytest.mark.parametrize("what", ["three panels in job1", "max_blocks 8"])
def test_pair_refuses(dev, what):
    from siss_amd import lib
    p3, p1 = pair_problems(dev, 200, 200, 128, 64, 1)
    if what == "three panels in job1":
        p1 = Prob(27, 64, "p3", 1, "shared", 200, 37, 5, "one", seed=5, y_of=p3).operands(dev)
    zp = zero_page(dev)
    j3, j1 = p3.outputs(dev, nan=False).job(0, zp), p1.outputs(dev, nan=False).job(0, zp)
    drain()
    lib.dispatch_counts(reset=True)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.call("siss_gemm_tn_pair", lib.C.byref(j3), lib.C.byref(j1), 8 if what == "max_blocks 8" else 64)
    torch.cuda.synchronize()
    counts_are(0, 0, 0)
    assert drain() == []
    p3.check(None, what)
    p1.check(None, what)

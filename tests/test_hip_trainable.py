"""siss_grad_norms_scale_ranges and siss_recombine_clip_adamw_ranges (csrc/optimizer.hip) called DIRECTLY on plain vectors: the
flat-buffer update restricted to a table of stretches (the trainable subset of SISSStepper(trainable=...)).

The buffers lie between sentinel guards (tests/test_hip_optimizer.py's Flat / Scal / State) and are compared WHOLE, bit for bit.
The shapes are the smallest at which the kernels can go wrong:

    n64      64 floats, two stretches
    tail     1030 floats: the buffer ends 2 floats (no whole granule) after the last stretch's granule range
    513      513 one-granule stretches with one-granule gaps: more stretches than a block has threads
    end      a stretch that ends exactly at the buffer's end
    stride   a compacted length of 2,097,152 + 64 floats: past what 2048 blocks x 256 threads cover in one sweep (the grid stride)

What is held to what:
* one stretch covering the whole buffer: scalars and p / m / v / shadow / g_out BITWISE those of siss_grad_norms_scale +
  siss_recombine_clip_adamw (same grid, same thread -> element map, same order of every sum);
* integer data (optimizer_ref.int_pair): norm_x, norm_a, dot exact over the gathered elements; Gaussian data: the block inside
  optimizer_ref.scalar_bounds evaluated on the gathered elements (the a-priori bounds of the whole-buffer pass: the construction
  of every sum is the same), and bitwise equal on a second launch (no atomics, a fixed thread -> element map);
* pass 2 BITWISE optimizer_ref.adamw_f32 on the gathered elements, fed the kernel's own block, scattered back;
* frozen stretches poisoned (NaN gradients, sentinel bit patterns in p / m / v / shadow / g_out): every scalar finite, every frozen
  byte unchanged;
* refused arguments (null table, no stretch, a misaligned base, more granules than the buffer holds) write nothing.
"""
import numpy as np
import pytest
import torch

import optimizer_ref as R
from test_hip_optimizer import BF, F32, Flat, Scal, T, hold, launch, refused, restate
from test_hip_small_kernels import same

pytestmark = pytest.mark.gpu

f32 = np.float32
SWEEP = R.MAX_BLOCKS * R.THREADS                           # granules one sweep of the grid covers
HP = R.hyper(*R.HYPER["sd"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _layouts():
    """name -> (floats in the buffer, starts, lengths) in 16-byte granules, starts ascending"""
    out = {"n64": (64, [2, 8], [3, 4]),
           "tail": (1030, [0, 100, 200], [5, 57, 57]),                  # granules 0 .. 256 of 257; 2 floats beyond them
           "513": (4 * 1026, list(range(0, 1026, 2)), [1] * 513),
           "end": (4096, [10, 1000], [100, 24])}
    first = 300_000
    out["stride"] = (4 * (first + 16 + SWEEP + 16 - first), [0, first + 16], [first, SWEEP + 16 - first])
    return out


LAYOUTS = _layouts()
assert LAYOUTS["tail"][0] % 4 == 2 and LAYOUTS["end"][1][-1] + LAYOUTS["end"][2][-1] == LAYOUTS["end"][0] // 4
assert len(LAYOUTS["513"][1]) == 513 > R.THREADS and sum(LAYOUTS["stride"][2]) * 4 == 2_097_152 + 64
SMALL = ["n64", "tail", "513", "end"]


def mask_of(name):
    n, starts, lens = LAYOUTS[name]
    m = np.zeros(n, bool)
    body = R.zero_mask(n, starts, lens)
    m[:len(body)] = body
    return m


def table(dev, starts, lens):
    tab, total = R.zero_table(starts, lens)
    return torch.from_numpy(tab).to(dev), len(starts), total


def norms_ranges(dev, gx, ga, tab, mode, knob, sc=None, max_norm=1.0, betas=(0.95, 0.999)):
    n = len(gx)
    bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
    sc = sc or Scal(dev)
    launch("siss_grad_norms_scale_ranges", bx.t, ba.t, n, *tab, mode, knob, max_norm, betas[0], betas[1], sc.partials.t, sc.blk.t)
    same(bx.d.cpu().view(torch.int32), bx.flat.view(torch.int32), "gx after the norms")
    same(ba.d.cpu().view(torch.int32), ba.flat.view(torch.int32), "ga after the norms")
    return sc.read(4 * tab[2]), sc


class State:
    """p, m, v, shadow, g_out in sentinel buffers"""

    def __init__(self, dev, p, m, v):
        n = len(p)
        self.p, self.m, self.v = (Flat(n, F32, dev, body=t) for t in (p, m, v))
        self.shadow, self.gout = Flat(n, BF, dev, fill=-3.0), Flat(n, F32, dev, fill=-9.0)

    def args(self):
        return self.p.t, self.m.t, self.v.t, self.shadow.t, self.gout.t


def knob_of(mode):
    return 1e-2 if mode == 1 else 5.0


# ================================================================ one covering stretch = the whole-buffer pair, bit for bit
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [64, 4 * 1026, 4 * (SWEEP + 16)])
def test_one_covering_stretch_is_the_whole_buffer_pair(dev, n, mode):
    rng = np.random.default_rng(n + mode)
    gx, ga = R.gauss_pair(n, n + mode)
    p = rng.standard_normal(n).astype(f32)
    m, v = R.warm_state(n, 3, HP, seed=5)
    tab = table(dev, [0], [n // 4])
    out = []
    for ranged in (False, True):
        bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
        sc, st = Scal(dev, step_before=2), State(dev, p, m, v)
        if ranged:
            launch("siss_grad_norms_scale_ranges", bx.t, ba.t, n, *tab, mode, knob_of(mode), 1.0, HP[1], HP[2], sc.partials.t, sc.blk.t)
            launch("siss_recombine_clip_adamw_ranges", bx.t, ba.t, *st.args(), n, *tab, *(float(h) for h in HP), sc.blk.t)
        else:
            launch("siss_grad_norms_scale", bx.t, ba.t, n, mode, knob_of(mode), 1.0, HP[1], HP[2], sc.partials.t, sc.blk.t)
            launch("siss_recombine_clip_adamw", bx.t, ba.t, *st.args(), n, *(float(h) for h in HP), sc.blk.t)
        out.append([sc.blk.d.cpu(), sc.partials.d.cpu()] + [b.d.cpu() for b in (st.p, st.m, st.v, st.shadow, st.gout, bx, ba)])
    for a, b, what in zip(out[0], out[1], ("scalars", "partial sums", "p", "m", "v", "shadow", "g_out", "gx", "ga")):
        same(b, a, f"n {n} mode {mode}: {what} of the ranges pair against the whole-buffer pair")


# ================================================================ pass 1
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_norms_on_integers_are_exact_over_the_stretches(dev, name, mode):
    n, starts, lens = LAYOUTS[name]
    gx, ga = R.int_pair(n, n)
    msk = mask_of(name)
    xx, aa, xa = R.int_sums(gx[msk], ga[msk])
    assert aa > 0
    blk, _ = norms_ranges(dev, gx, ga, table(dev, starts, lens), mode, knob_of(mode))
    assert blk[0] == f32(np.sqrt(float(xx))) and blk[1] == f32(np.sqrt(float(aa))) and blk[2] == f32(xa), (blk[:3], xx, aa, xa)
    ref = R.scalars_f64(float(xx), float(aa), float(xa), mode, knob_of(mode), 1.0, 0.95, 0.999, 1)
    for k in ("scale", "pre_clip_norm", "clip_coef"):       # doubles from exact sums, rounded once (test_hip_optimizer.py)
        assert abs(float(blk[R.NAMES[k]]) - ref[k]) <= R.U * (1 + 2.0 ** -20) * abs(ref[k]), (k, blk[R.NAMES[k]], ref[k])
    assert blk[6] == 1


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_scalars_on_gaussian_data_within_the_bounds_of_the_gathered_elements(dev, name, mode):
    n, starts, lens = LAYOUTS[name]
    gx, ga = R.gauss_pair(n, n + mode)
    msk = mask_of(name)
    tab = table(dev, starts, lens)
    blk, _ = norms_ranges(dev, gx, ga, tab, mode, knob_of(mode))
    hold(blk, gx[msk], ga[msk], mode, knob_of(mode), f"norms_scale_ranges {name} mode {mode}")
    again, _ = norms_ranges(dev, gx, ga, tab, mode, knob_of(mode))
    assert np.array_equal(blk.view(np.int32), again.view(np.int32)), "a second launch differs: not bitwise repeatable"


# ================================================================ pass 2, and both passes with the frozen stretches poisoned
def _poison_pattern(n, word):
    return np.full(n, word, np.uint32).view(f32)


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_update_is_the_restatement_on_the_stretches_and_touches_nothing_else(dev, name, poison):
    """Two steps (mode 0, then mode 1), the state carried.  poison: the frozen stretches of gx / ga hold NaN, those of p / m / v hold
    the bit patterns of a signalling NaN, -inf and a denormal -- every scalar must be finite and every frozen byte unchanged (the
    guards and the frozen stretches of shadow / g_out keep their fill in both variants: the WHOLE buffers are compared)."""
    n, starts, lens = LAYOUTS[name]
    msk = mask_of(name)
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n).astype(f32)
    m, v = R.warm_state(n, 3, HP, seed=7)
    if poison:
        p[~msk], m[~msk], v[~msk] = (_poison_pattern(int((~msk).sum()), w) for w in (0x7FA00001, 0xFF800000, 0x00000003))
    st, sc, tab = State(dev, p, m, v), Scal(dev, step_before=2), table(dev, starts, lens)
    sh_want, g_want = st.shadow.host.clone(), st.gout.host.clone()
    for step, mode in enumerate((0, 1)):
        gx, ga = R.gauss_pair(n, n + step)
        if poison:
            gx[~msk] = ga[~msk] = np.nan
        blk, _ = norms_ranges(dev, gx, ga, tab, mode, knob_of(mode), sc=sc, betas=(float(HP[1]), float(HP[2])))
        assert np.isfinite(blk[list(R.NAMES.values())]).all(), blk
        hold(blk, gx[msk], ga[msk], mode, knob_of(mode), f"norms_scale_ranges {name} step {step} poison {poison}")
        bx, ba = Flat(n, F32, dev, body=gx), Flat(n, F32, dev, body=ga)
        launch("siss_recombine_clip_adamw_ranges", bx.t, ba.t, *st.args(), n, *tab, *(float(h) for h in HP), sc.blk.t)
        got_p = st.p.np()
        rp, rm, rv, rg = restate(gx[msk], ga[msk], p[msk], m[msk], v[msk], blk, HP, got_p[msk])
        p, m, v = p.copy(), m.copy(), v.copy()
        p[msk], m[msk], v[msk] = rp, rm, rv
        for buf, want, what in ((st.p, p, "p"), (st.m, m, "m"), (st.v, v, "v")):
            e = buf.flat.clone()
            e[buf.g:buf.g + n] = T(want)
            same(buf.d.cpu().view(torch.int32), e.view(torch.int32), f"{name} step {step}: {what}")
        g_want[torch.from_numpy(msk)] = T(rg)
        sh_want[torch.from_numpy(msk)] = R.bf16(rp)
        st.gout.check(g_want, f"{name} step {step}: g_out")
        st.shadow.check(sh_want, f"{name} step {step}: shadow = bf16(new p) on the stretches, its fill elsewhere")
        same(bx.d.cpu().view(torch.int32), bx.flat.view(torch.int32), "gx after the update")
        same(ba.d.cpu().view(torch.int32), ba.flat.view(torch.int32), "ga after the update")
    assert sc.read()[6] == 4


# ================================================================ refused arguments
def test_refused_arguments_write_nothing(dev):
    n, starts, lens = LAYOUTS["n64"]
    gx, ga = R.int_pair(n, 1)
    p = np.arange(n, dtype=f32)
    bx, ba = Flat(n + 4, F32, dev, body=np.r_[gx, gx[:4]]), Flat(n + 4, F32, dev, body=np.r_[ga, ga[:4]])
    st, sc = State(dev, p, p, p), Scal(dev)
    tab, nr, total = table(dev, starts, lens)
    hp = [float(h) for h in HP]
    X, A = bx.t[:n], ba.t[:n]
    for what, a in (("null table", (X, A, n, None, nr, total)), ("no stretch", (X, A, n, tab, 0, total)),
                    ("no granule", (X, A, n, tab, nr, 0)), ("more granules than the buffer", (X, A, n, tab, nr, n // 4 + 1)),
                    ("misaligned gx", (bx.t[1:n + 1], A, n, tab, nr, total)), ("misaligned ga", (X, ba.t[2:n + 2], n, tab, nr, total)),
                    ("misaligned table", (X, A, n, tab.view(torch.int32)[1:], nr, total))):
        refused("siss_grad_norms_scale_ranges", *a, 0, 5.0, 1.0, 0.95, 0.999, sc.partials.t, sc.blk.t)
        refused("siss_recombine_clip_adamw_ranges", *a[:2], *st.args(), *a[2:], *hp, sc.blk.t)
    refused("siss_grad_norms_scale_ranges", X, A, n, tab, nr, total, 3, 5.0, 1.0, 0.95, 0.999, sc.partials.t, sc.blk.t)
    refused("siss_recombine_clip_adamw_ranges", X, A, st.p.t[1:], st.m.t, st.v.t, st.shadow.t, st.gout.t, n - 4, tab, nr, total, *hp, sc.blk.t)
    for buf, what in ((st.p, "p"), (st.m, "m"), (st.v, "v"), (st.shadow, "shadow"), (st.gout, "g_out"), (sc.blk, "scalars"),
                      (sc.partials, "partial sums"), (bx, "gx"), (ba, "ga")):
        same(buf.d.cpu(), buf.flat, f"refused launches wrote {what}")

"""Plain f64 reference of the GroupNorm (+ SiLU) kernels of csrc/groupnorm.hip, csrc/groupnorm_slab.hip and the f32 forms of
csrc/f32_path.hip -- no GPU, no HIP library -- with the error budget the kernels are held to and the dispatch plan of their
launchers, for tests/test_hip_groupnorm_exact.py (pinned to torch's f64 group_norm and autograd by tests/test_groupnorm_ref_host.py).

    mean, rstd   per (sample, group) over cnt = H W cpg elements;  xhat = (x - mean) rstd;  z = xhat gamma + beta
    y            = act(z),  act = SiLU or identity
    dz           = dy act'(z) gamma;  S1 = sum_group dz;  S2 = sum_group dz xhat
    t            = rstd (dz - S1 / cnt - xhat S2 / cnt)                       (the GroupNorm term of dx; colsum sums THIS over pixels)
    dx           = t + accum + accum2 (+ old dx2 on channels [split_c, C) of an accumulating split target)
    dgamma[set]  = sum dy act'(z) xhat,  dbeta[set] = sum dy act'(z)          over the pixels of the set's cotangent samples
Cotangent sample n2 is differentiated against saved sample n2 % nx and belongs to set n2 // set_images.

Tensors are torch f64 in NCHW; the tests move them in and out of the padded NHWC layout.  The inputs of the tests are bf16-exact,
so everything here is the exact operation on the kernels' own inputs up to f64 rounding.

The BUDGET (fwd_budget / bwd_budget) is derived below from the operation chains the kernel sources show and from the documented
accuracy of the two hardware transcendentals; nothing in it was fitted to what the kernels return.  u = 2^-24 is the unit roundoff of
f32.  Every bound is first order in u with one unit of u added per chain for the second-order products (the chains are < 2^6 long
where a second-order term is (k u)^2 / 2 < u).
"""
from dataclasses import dataclass

import torch

F64 = torch.float64
U = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------------------------
# launch shapes: make_shape (csrc/groupnorm.hip) and slab_slice (csrc/groupnorm_slab.hip) restated
# How far the restatement is CHECKED: the library exposes one number of these shapes, siss_gn_partial_words = nslices * nchunks * 2 G at
# N = 1 and the forward block target; the tests compare that (slices, chunk count, groups per slice).  lpp, ppi and chunk_px at a case's
# own N and block target, and slab_slice as a whole, have no query: they are pinned only indirectly, by the dispatch counters (whether the
# slab kernel ran at all) -- a wrong ppi here would give a wrong L in the budget, not a failing comparison.  They are short restatements
# to be read against the source.
K_THREADS, MAX_G, MAX_C = 256, 32, 1024
BLOCKS_FWD, BLOCKS_BWD, BLOCKS_BWD_STATS = 768, 512, 767
SLAB_T, SLAB_V, SLAB_MAX_CS = 512, 8, 128
QS_TILE, QS_HALF = 254, 128


def cdiv(a, b):
    return -(-a // b)


@dataclass
class Shape:
    """GNShape: C / G are the channel slice's (blockIdx.z), Gf the tensor's group count."""
    H: int
    W: int
    C: int
    G: int
    cpg: int
    lpp: int
    ppi: int
    chunk_px: int
    nchunks: int
    ld: int
    Gf: int
    nslices: int


def shape(H, W, C, G, N=16, blocks=BLOCKS_FWD):
    """make_shape: None where the launcher refuses."""
    if H <= 0 or W <= 0 or C <= 0 or G <= 0 or G > MAX_G or C % G or C % 8:
        return None
    cpg, gs = C // G, G
    if C > MAX_C:
        best, best_util, gs = 0, -1, 0
        for d in range(G, 0, -1):
            if G % d:
                continue
            cs = d * cpg
            if cs > MAX_C or cs % 8:
                continue
            lpp = cs // 8
            util = (K_THREADS // lpp) * lpp
            if util * 10 >= K_THREADS * 9:
                gs = d
                break
            if util > best_util:
                best_util, best = util, d
        gs = gs or best
        if gs == 0:
            return None
    Cs, nslices = gs * cpg, G // gs
    lpp = Cs // 8
    if lpp > K_THREADS:
        return None
    ppi = K_THREADS // lpp
    px = H * W
    nch = cdiv(blocks, N * nslices)
    nch = min(nch, cdiv(px, 16 * ppi))
    if blocks in (BLOCKS_BWD, BLOCKS_BWD_STATS):
        by32 = cdiv(px, 32 * ppi)
        if nch > by32 and by32 * N * nslices >= 256:
            nch = by32
    nch = max(1, min(nch, 256))
    chunk_px = cdiv(px, nch)
    return Shape(H, W, Cs, gs, cpg, lpp, ppi, chunk_px, cdiv(px, chunk_px), C, G, nslices)


def partial_words(n, H, W, C, G):
    """siss_gn_partial_words."""
    s = shape(H, W, C, G, 1)
    return -1 if s is None else n * s.nslices * s.nchunks * 2 * s.G


@dataclass
class Slab:
    Cs: int
    Gs: int
    lpp: int
    ppi: int
    V: int


def slab_slice(H, W, C, G, N):
    """slab_slice: None where the one-launch kernels do not cover the site."""
    if H <= 0 or W <= 0 or C <= 0 or G <= 0 or G > MAX_G or C % G or C % 8 or N <= 0:
        return None
    P, cpg = H * W, C // G
    if P > 1024 or cpg < 4:
        return None
    best = 0
    for k in range(G, 0, -1):
        if G % k:
            continue
        Cs = k * cpg
        if Cs % 8 or Cs > SLAB_MAX_CS:
            continue
        lpp = Cs // 8
        ppi = SLAB_T // lpp
        if cdiv(P, ppi) > SLAB_V:
            continue
        if not all((cc * 8 + 7) // cpg <= (cc * 8) // cpg + 1 for cc in range(lpp)):
            continue
        if Cs < 32:
            continue
        best = Cs
        if (C // Cs) * N >= 128:
            break
    if not best:
        return None
    ppi = SLAB_T // (best // 8)
    return Slab(best, best // cpg, best // 8, ppi, cdiv(P, ppi))


@dataclass
class Plan:
    """Which kernels a launch takes (the deltas of lib.dispatch_counts it must show) and the lengths L of the longest serial chains of
    f32 additions its sums pass through: stats (forward sum / sum of squares, backward S1 / S2), param (dgamma / dbeta), colsum."""
    kernel: str
    counts: dict
    L_stats: int
    L_param: int = 0
    L_colsum: int = 0
    nchunks: int = 0
    pchunks: int = 0
    nslices: int = 1


def _counts(slab=0, qstats=0):
    return {"gn_slab": slab, "gn_qstats": qstats, "gn_bwd_sc_kernel": 0}


def slab_chain(ppi):
    """A slab kernel's sum over pixels: kSlabV serial additions per lane; slab_reduce then runs four chains over ppi // 4 slots each, adds
    the last ppi % 4 slots onto the FIRST chain serially (its remainder loop), and joins the four in a two-level tree."""
    return SLAB_V + ppi // 4 + ppi % 4 + 2


def plan_fwd(H, W, C, G, N, slab_on, qs=False, f32=False):
    """siss_groupnorm_fwd_qs / _ld.  Chain lengths, from the kernel sources:
    two-pass (gn_stats_kernel): a lane adds its ceil(chunk_px / ppi) pixels two per trip (v + u, then a += : trips + 1 additions deep),
      reduce_slots adds the ppi slots serially, thread g the cpg channels serially, fold_slab ceil(nchunks / 4) slab entries; the last
      fold of four is in f64 (exact for f32 addends).
    slab (gn_slab_fwd_kernel): slab_chain(ppi); the per-group fold over channels is in f64.
    hand-over (gn_quad_stats_kernel -> gn_qstats_finalize_kernel): a quad is a two-level tree, a lane walks ceil(128 / par) rows of its
      half tile (one addition each), the block folds the par rows in flight serially; the finalize kernel sums in f64.
    f32 form (gn_fwd_f32_kernel): f64 from the first addition on."""
    if f32:
        return Plan("f32", _counts(), 0)
    s = shape(H, W, C, G, N, BLOCKS_FWD)
    assert s is not None
    sl = slab_slice(H, W, C, G, N) if (slab_on and s.nslices == 1) else None
    if sl is not None:
        return Plan("slab", _counts(slab=1), slab_chain(sl.ppi))
    if qs and s.cpg % 4 == 0 and (H + 2) * (W + 2) >= 256:      # qs: the producers' widths (siss_quad_stats runs once per producer)
        L = max(2 + cdiv(QS_HALF, K_THREADS // (w // 8)) + K_THREADS // (w // 8) for w in qs)
        return Plan("qstats", _counts(qstats=1), L, nchunks=s.nchunks, nslices=s.nslices)
    per_lane = cdiv(s.chunk_px, s.ppi)
    return Plan("two_pass", _counts(), cdiv(per_lane, 2) + 1 + s.ppi + s.cpg + cdiv(s.nchunks, 4), nchunks=s.nchunks, nslices=s.nslices)


def plan_bwd(H, W, C, G, nx, n2, set_images, slab_on, f32=False):
    """siss_groupnorm_bwd_ld.  Chain lengths:
    two-pass: gn_bwd_stats_kernel (launch shape `ss`, kBlocksBwdStats) adds one product per pixel per lane (ceil(chunk_px / ppi) fused
      multiply-adds), reduce_slots the ppi slots; from there S1 / S2 take cpg fused multiply-adds with gamma and ceil(pchunks / 4) slab
      entries in fold_slab, while dgamma / dbeta take one float atomic per (block, channel): set_images * pchunks blocks add to one
      address.  gn_bwd_apply_kernel (launch shape `s`, kBlocksBwd) sums colsum the same way: ceil(chunk_px / ppi) + ppi, then
      nchunks atomics per (cotangent sample, channel).
    slab (gn_slab_bwd_kernel, at most 16 x 16 pixels): slab_chain(ppi); S1 / S2 fold the
      channels in f64; dgamma / dbeta get one atomic per saved sample of the set (set_images), colsum one per address.
    f32 form (gn_bwd_f32_kernel): S1 / S2 and the per-channel sums in f64; dgamma / dbeta one rounding to f32 and one atomic per
      cotangent sample of the set; colsum one float atomic per PIXEL."""
    if f32:
        return Plan("f32", _counts(), 0, set_images + 1, H * W)
    s, ss = shape(H, W, C, G, nx, BLOCKS_BWD), shape(H, W, C, G, nx, BLOCKS_BWD_STATS)
    assert s is not None and ss is not None
    sl = None
    if slab_on and s.nslices == 1 and n2 // set_images <= 2 and H * W <= 256:
        sl = slab_slice(H, W, C, G, nx)
    if sl is not None:
        L = slab_chain(sl.ppi)
        return Plan("slab", _counts(slab=1), L, L + set_images, L + 1)
    lane_s, lane_a = cdiv(ss.chunk_px, ss.ppi), cdiv(s.chunk_px, s.ppi)
    return Plan("two_pass", _counts(), lane_s + ss.ppi + ss.cpg + cdiv(ss.nchunks, 4), lane_s + ss.ppi + set_images * ss.nchunks,
                lane_a + s.ppi + s.nchunks, nchunks=s.nchunks, pchunks=ss.nchunks, nslices=s.nslices)


# ---------------------------------------------------------------------------------------------------------------------
# the operation
def _sig(z):
    return torch.sigmoid(z)


def _dsilu(z):
    s = _sig(z)
    return s * (1 + z * (1 - s))


def _chan_group(C, G):
    return torch.arange(C) // (C // G)


def _group_sum(v, G):
    """[N, C, H, W] -> [N, G]: the sum over each group's channels and all pixels."""
    N, C = v.shape[:2]
    return v.reshape(N, G, -1).sum(-1)


def _forward(x, gamma, beta, eps, G, silu, cnt=None, chan_group=None):
    """cnt / chan_group: the hooks of the mutants of tests/test_groupnorm_ref_host.py (a wrong element count; the group whose
    statistics a channel is normalised with)."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    N, C, H, W = x.shape
    cnt = H * W * (C // G) if cnt is None else cnt
    cg = _chan_group(C, G) if chan_group is None else chan_group
    mean = _group_sum(x, G) / cnt
    ex2 = _group_sum(x * x, G) / cnt
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    mc, rc = mean[:, cg, None, None], rstd[:, cg, None, None]
    ga, be = gamma[None, :, None, None], beta[None, :, None, None]
    xhat = (x - mc) * rc
    z = xhat * ga + be
    y = z * _sig(z) if silu else z
    S = (x.abs() + mc.abs()) * rc * ga.abs() + be.abs()
    return dict(y=y, mean=mean, rstd=rstd, S=S, z=z, xhat=xhat, var=var, ex2=ex2, eabs=_group_sum(x.abs(), G) / cnt, mc=mc, rc=rc,
                X=(x.abs() + mc.abs()) * rc)


def forward(x, gamma, beta, eps, G, silu):
    """y, mean, rstd and the per-element magnitude sum S = (|x| + |mean|) rstd |gamma| + |beta| (with the intermediates the budget
    reads: z, xhat, var, E[x^2], E|x|)."""
    return _forward(x, gamma, beta, eps, G, silu)


def _backward(x, gamma, beta, eps, G, silu, dy, nx, set_images, accum=None, accum2=None, old2=None, split_c=0, accumulate2=True,
              cnt=None, chan_group=None, xindex=None, s12_src=None, set_of=None, second_of=None):
    """Hooks of the mutants: cnt, chan_group as in _forward; xindex(n2) the saved sample; s12_src(n2) the cotangent sample whose
    S1 / S2 normalise n2; set_of(n2) the gradient set; second_of [C] bool: the channels routed to the second part of a split."""
    f = _forward(x, gamma, beta, eps, G, silu, cnt=cnt, chan_group=chan_group)
    x, gamma, dy = x.to(F64), gamma.to(F64), dy.to(F64)
    n2, C, H, W = dy.shape
    cntv = H * W * (C // G) if cnt is None else cnt
    cg = _chan_group(C, G) if chan_group is None else chan_group
    xi = torch.tensor([(i % nx) if xindex is None else xindex(i) for i in range(n2)])
    src = torch.tensor([i if s12_src is None else s12_src(i) for i in range(n2)])
    sets = [(i // set_images) if set_of is None else set_of(i) for i in range(n2)]
    nsets = max(n2 // set_images, 1)
    ga = gamma[None, :, None, None]
    xhat, z, rc = f["xhat"][xi], f["z"][xi], f["rc"][xi]
    da = _dsilu(z) if silu else torch.ones_like(z)
    q = dy * da
    dz = q * ga
    S1, S2 = _group_sum(dz, G), _group_sum(dz * xhat, G)
    A1, A2 = _group_sum(dz.abs(), G), _group_sum((dz * xhat).abs(), G)
    m1, m2 = (S1[src] / cntv)[:, cg, None, None], (S2[src] / cntv)[:, cg, None, None]
    t = rc * (dz - m1 - xhat * m2)
    St = rc * (dz.abs() + m1.abs() + (xhat * m2).abs())
    dgamma, dbeta, Adg, Adb = (torch.zeros(nsets, C, dtype=F64) for _ in range(4))
    for i in range(n2):
        dgamma[sets[i]] += (q[i] * xhat[i]).sum((1, 2)); dbeta[sets[i]] += q[i].sum((1, 2))
        Adg[sets[i]] += (q[i] * xhat[i]).abs().sum((1, 2)); Adb[sets[i]] += q[i].abs().sum((1, 2))
    total, Stot = t.clone(), St.clone()
    for r in (accum, accum2):
        if r is not None:
            total = total + r.to(F64); Stot = Stot + r.to(F64).abs()
    out = dict(dy=dy, t=t, St=St, dgamma=dgamma, dbeta=dbeta, A_dgamma=Adg, A_dbeta=Adb, colsum=t.sum((2, 3)), A_colsum=t.abs().sum((2, 3)),
               S1=S1, S2=S2, A1=A1, A2=A2, cnt=cntv, fwd=f, xi=xi, q=q, da=da, dz=dz, xhat=xhat, z=z, rc=rc, m1=m1, m2=m2)
    if split_c:
        sec = (torch.arange(C) >= split_c) if second_of is None else second_of
        if old2 is not None and accumulate2:
            o2 = torch.zeros_like(total); o2[:, split_c:] = old2.to(F64)
            total = total + o2 * sec[None, :, None, None]; Stot = Stot + (o2 * sec[None, :, None, None]).abs()
        if second_of is not None:
            # a channel the (mutant) routing does not send to the part it belongs to never reaches it: that part keeps its old contents
            wrong = sec != (torch.arange(C) >= split_c)
            keep = torch.zeros_like(total)
            if old2 is not None:
                keep[:, split_c:] = old2.to(F64)
            total = torch.where(wrong[None, :, None, None], keep, total)
        out["first"], out["second"] = total[:, :split_c], total[:, split_c:]
    out["total"], out["Stot"] = total, Stot
    return out


def backward(x, gamma, beta, eps, G, silu, dy, nx, set_images, accum=None, accum2=None, old2=None, split_c=0, accumulate2=True):
    """dict: `t` (the GroupNorm term) and `total` (after accum, accum2 and, on channels [split_c, C) of an accumulating split target,
    the old contents `old2` of dx2) per cotangent sample, `first` / `second` = total[:, :split_c] / total[:, split_c:]; dgamma / dbeta
    [sets][C]; colsum [n2][C]; the magnitude sums St / Stot (per element), A_dgamma / A_dbeta / A_colsum, A1 / A2 (sums of the absolute
    values of the summed terms)."""
    return _backward(x, gamma, beta, eps, G, silu, dy, nx, set_images, accum, accum2, old2, split_c, accumulate2)


# ---------------------------------------------------------------------------------------------------------------------
# the budget
def half_ulp_bf16(v):
    """Half a unit in the last place of bf16 (8 significand bits) at magnitude |v|: 2^(e - 9) for |v| in [2^(e-1), 2^e)."""
    _, e = torch.frexp(v.abs().to(F64))
    return torch.ldexp(torch.ones_like(v, dtype=F64), e.clamp_min(-125) - 9)


def _rounded(ref, delta, bf16):
    """An output that is the nearest bf16 of a value v with |v - ref| <= delta lies within half_ulp(v) + delta of ref, and
    |v| <= |ref| + delta: the half ulp is taken THERE (v may sit in the binade above ref's).  f32 outputs: one rounding to f32, u |v|."""
    if bf16:
        return half_ulp_bf16(ref.abs() + delta) + delta
    return delta + U * (ref.abs() + delta)


# exp(-z) through the hardware exp2 (1 ulp = 2 u; AMD CDNA ISA guide, V_EXP_F32) of an argument that is a product / fused
# multiply-add with log2(e): the apply kernels form -z * log2e (constant rounded, product rounded: 2 u |z|), gn_bwd_stats_kernel forms
# xhat * (-gamma log2e) + (-beta log2e) (two rounded constants-times-parameter products, their own rounding, one fma: at most
# 5 u (|xhat gamma| + |beta|) of the argument); 2^a moves by ln2 * da relative, and ln2 * log2e = 1: rho_e = 2 u + 5 u Zabs, with
# Zabs = |xhat gamma| + |beta| >= |z| covering both forms.
def _rho_e(zabs):
    return 2 * U + 5 * U * zabs


# s = rcp(1 + e): the addition u, v_rcp_f32 1 ulp = 2 u, and e's relative error scaled by e / (1 + e) = 1 - s
def _rho_s(s, zabs):
    return (1 - s) * _rho_e(zabs) + 3 * U


def stats_budget(f, L, eps, f32_out=True):
    """|dmean| <= L u E|x|, |dvar| <= L u (E[x^2] + 2 m^2) (squares of bf16 values are exact in f32: only the additions round; the
    means, their square and the difference are formed in f64), plus the rounding of the two results to f32.  rstd: var is clamped at 0
    by the kernels, so the computed var + eps lies in [max(var - dvar, 0) + eps, var + dvar + eps]; the bound is the larger of the two
    excursions of 1 / sqrt over that interval -- no linearisation, it holds where dvar is not small against var + eps."""
    m, var, r = f["mean"], f["var"], f["rstd"]
    dmean = L * U * f["eabs"]
    dvar = L * U * (f["ex2"] + 2 * m * m)
    lo, hi = (var - dvar).clamp_min(0) + eps, var + dvar + eps
    drstd = torch.maximum(1 / torch.sqrt(lo) - r, r - 1 / torch.sqrt(hi))
    return dict(mean=dmean + U * (m.abs() + dmean), rstd=drstd + U * (r + drstd), dmean=dmean, drstd=drstd)


K_FWD = 8   # sc = rstd gamma (1), mean * sc (1), beta - . (1), z = fma(x, sc, sf) (1), mean and rstd rounded to f32 (2), + 1 second order;
#             and 1 for a compiler that does not contract x * sc + sf (the f32 form is built without the fp-contract pragma's guarantee)


def fwd_budget(f, gamma, beta, silu, L, eps, bf16=True):
    """|y - ref| <= half_ulp_bf16 + delta with
    delta = act'max * (K_FWD u S + |xhat gamma| drstd / rstd + |gamma| rstd dmean)          (z's own error, act' <= 1.1 for SiLU)
          + |y| (rho_s + u)                                                               (sigmoid's relative error, the product z * s)
    Returns (budget for y, budget for mean, budget for rstd)."""
    st = stats_budget(f, L, eps)
    cg = _chan_group(f["y"].shape[1], f["mean"].shape[1])
    ga = gamma.to(F64).abs()[None, :, None, None]
    dm, dr = st["dmean"][:, cg, None, None], st["drstd"][:, cg, None, None]
    dz = K_FWD * U * f["S"] + (f["xhat"] * ga).abs() * dr / f["rc"] + ga * f["rc"] * dm
    if silu:
        zabs = (f["xhat"] * ga).abs() + beta.to(F64).abs()[None, :, None, None]
        delta = 1.1 * dz + f["y"].abs() * (_rho_s(_sig(f["z"]), zabs) + U)
    else:
        delta = dz
    return _rounded(f["y"], delta, bf16), st["mean"], st["rstd"]


K_T = 8     # rstd rounded to f32 (1); d * dsl, (. ) * gamma, - m1, xhat * m2, the second subtraction, rstd * (. ): 6 roundings where
#             nothing is contracted (gn_bwd_t contracts two of them; the slab and f32 kernels leave it to the compiler); + 1 second order


def bwd_budget(b, gamma, beta, silu, plan, bf16=True):
    """The backward takes mean / rstd as f32 INPUTS (the tests hand it the f64 statistics rounded to f32): each carries u relative.
    Element chain (gn_bwd_xhat / gn_bwd_t; the slab and f32 kernels do the same arithmetic uncontracted):
      xhat = fma(x, rstd, -(mean * rstd)): rstd's rounding moves x rstd and mean rstd (u each), mean's rounding and the product's
             (2 u |mean| rstd), the fma's own rounding (u |xhat|):                       dxh  <= 4 u X,  X = (|x| + |mean|) rstd
      z    = fma(xhat, gamma, beta):                                                     dz   <= |gamma| dxh + u Zabs
      a    = SiLU'(z) = s (1 + z (1 - s)):  |SiLU''| <= 1/2; da/ds = 1 + z - 2 s z, |.| <= 1 + |z|; four roundings of magnitude
             <= s (1 + |z|):                                                             da   <= dz / 2 + (1 + |z|) s (rho_s + 4 u)
      t    = rstd (d a gamma - m1 - xhat m2):
             delta_t = rstd (|d gamma| da + dm1 + |xhat| dm2 + |m2| dxh) + K_T u St
      dx   = t + accum + accum2 + old dx2: up to three f32 additions, each u of a partial sum <= Stot:  + 3 u Stot, then ONE rounding.
    Sums (classical bound: a sum whose addends pass through at most L serial f32 additions is within L u sum|terms| of the sum of
    its COMPUTED terms; the computed terms differ from the exact ones by their element errors):
      S1 = sum d a gamma:        dS1 <= sum |d gamma| da + (L + 2) u A1          (two roundings per term: d * a, then * gamma)
      S2 = sum d a xhat gamma:   dS2 <= sum |d gamma| (|xhat| da + |a| dxh) + (L + 3) u A2
      m1 = S1 / cnt rounded to f32: dm1 = dS1 / cnt + u |m1|;  m2 likewise
      dgamma = sum d a xhat, dbeta = sum d a, colsum = sum t: the same with their own L (float atomics included: plan_bwd).
    Returns dict(dx, dgamma, dbeta, colsum) of budgets; dx is for `total` (split the columns as the outputs are split)."""
    f = b["fwd"]
    ga = gamma.to(F64).abs()[None, :, None, None]
    be = beta.to(F64).abs()[None, :, None, None]
    xi = b["xi"]
    X = f["X"][xi]
    xhat, z, rc = b["xhat"], b["z"], b["rc"]
    dxh = 4 * U * X
    zabs = xhat.abs() * ga + be
    if silu:
        s = _sig(z)
        da = (ga * dxh + U * zabs) / 2 + (1 + z.abs()) * s * (_rho_s(s, zabs) + 4 * U)
    else:
        da = torch.zeros_like(z)
    dy_abs = b["dy"].abs()
    dga = dy_abs * ga
    G = b["S1"].shape[1]
    cg = _chan_group(z.shape[1], G)
    cnt, L = b["cnt"], plan.L_stats
    dS1 = _group_sum(dga * da, G) + (L + 2) * U * b["A1"]
    dS2 = _group_sum(dga * (xhat.abs() * da + b["da"].abs() * dxh), G) + (L + 3) * U * b["A2"]
    dm1 = (dS1 / cnt)[:, cg, None, None] + U * b["m1"].abs()
    dm2 = (dS2 / cnt)[:, cg, None, None] + U * b["m2"].abs()
    dt = rc * (dga * da + dm1 + xhat.abs() * dm2 + b["m2"].abs() * dxh) + K_T * U * b["St"]
    delta = dt + 3 * U * b["Stot"]
    n2 = z.shape[0]
    nsets = b["dgamma"].shape[0]
    set_images = n2 // nsets
    edg = (dy_abs * (xhat.abs() * da + b["da"].abs() * dxh)).sum((2, 3))
    edb = (dy_abs * da).sum((2, 3))
    Lp, Lc = plan.L_param, plan.L_colsum
    ddg = edg.reshape(nsets, set_images, -1).sum(1) + (Lp + 2) * U * b["A_dgamma"]
    ddb = edb.reshape(nsets, set_images, -1).sum(1) + (Lp + 1) * U * b["A_dbeta"]
    dcs = dt.sum((2, 3)) + Lc * U * b["A_colsum"]
    return dict(dx=_rounded(b["total"], delta, bf16), dgamma=ddg + U * b["dgamma"].abs(), dbeta=ddb + U * b["dbeta"].abs(),
                colsum=dcs + U * b["colsum"].abs())


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_hip_groupnorm_exact.py (tests/test_groupnorm_ref_host.py runs the budget over the same inputs)
G32 = 32
EPS6, EPS5 = float(torch.tensor(1e-6, dtype=torch.float32)), float(torch.tensor(1e-5, dtype=torch.float32))   # the launchers take a float


def bf(v):
    return v.to(torch.bfloat16).to(F64)


@dataclass(frozen=True)
class FwdCase:
    """dist: "std" (mean 0.3, std 1.5), "offset" (mean 2, std 0.25: |mean| / std = 8), "small" (std 2^-7: var of the order of eps),
    "ones" (group 5 of every sample is all ones: its sums are exact, var = 0).  ld_extra: x is a column window of a buffer that many
    channels wider.  qs: the statistics hand-over, the producers' widths."""
    name: str
    B: int
    C: int
    H: int
    W: int
    silu: bool = True
    compact: bool = False
    ld_extra: int = 0
    eps: float = EPS6
    dist: str = "std"
    qs: tuple = ()


FWD_CASES = [
    # SD widths in one slice: cpg 10 / 20 / 30 (a lane's 8 channels straddle two groups at 10 and 30); 8 x 8 and the ragged 5 x 7
    FwdCase("sd320_8x8", 2, 320, 8, 8), FwdCase("sd640_8x8", 2, 640, 8, 8, silu=False, compact=True),
    FwdCase("sd960_8x8", 3, 960, 8, 8), FwdCase("sd320_5x7", 3, 320, 5, 7, silu=False), FwdCase("sd640_5x7", 2, 640, 5, 7),
    FwdCase("sd960_5x7", 2, 960, 5, 7, compact=True),
    FwdCase("sd320_36x36", 2, 320, 36, 36),                         # 1296 pixels: the smallest square site past the slab kernel
    # channel slices (C > 1024: 2 x 640, 2 x 960, 4 x 640), eps 1e-5 as in SD
    FwdCase("sl1280_4x4", 2, 1280, 4, 4, eps=EPS5), FwdCase("sl1920_4x4", 2, 1920, 4, 4, eps=EPS5, silu=False),
    FwdCase("sl2560_4x4", 3, 2560, 4, 4, eps=EPS5, compact=True), FwdCase("sl1280_6x5", 3, 1280, 6, 5, eps=EPS5, silu=False, compact=True),
    FwdCase("sl1920_6x5_view", 2, 1920, 6, 5, eps=EPS5, ld_extra=640), FwdCase("sl2560_6x5", 2, 2560, 6, 5, eps=EPS5),
    # many statistics blocks: 16 chunks per sample (fold_slab's strided loop runs four times), 13 at two pixels per iteration
    FwdCase("c128_64x64_b3", 3, 128, 64, 64), FwdCase("c1024_20x20", 2, 1024, 20, 20),
    # ragged walks
    FwdCase("c256_7x9", 2, 256, 7, 9), FwdCase("c128_37x1", 2, 128, 37, 1, silu=False), FwdCase("c512_1x1", 3, 512, 1, 1),
    FwdCase("c256_view_9x9", 2, 256, 9, 9, ld_extra=128),
    # numeric edges
    FwdCase("offset_c256_12x12", 2, 256, 12, 12, dist="offset"), FwdCase("offset_c128_40x40", 2, 128, 40, 40, dist="offset"),
    FwdCase("small_c320_8x8", 2, 320, 8, 8, eps=EPS5, dist="small"), FwdCase("small_c128_36x36", 2, 128, 36, 36, eps=EPS5, dist="small"),
    FwdCase("ones_c128_10x10", 2, 128, 10, 10, eps=EPS5, dist="ones"), FwdCase("ones_c256_34x34", 2, 256, 34, 34, eps=EPS5, dist="ones", silu=False),
]
QS_CASES = [
    # 17 x 17 padded = 289 rows per image: 254-row tiles straddle images
    FwdCase("qs128_15x15", 3, 128, 15, 15, qs=(128,)), FwdCase("qs256_15x15", 3, 256, 15, 15, qs=(256,), silu=False),
    FwdCase("qs384_cat_15x15", 3, 384, 15, 15, qs=(256, 128)),     # groups of 12 straddle the seam of the two producers
    FwdCase("qs320_ignored_15x15", 3, 320, 15, 15, qs=(320,)),     # cpg = 10: no whole quads -- the entries are ignored, the statistics pass runs
    FwdCase("qs128_offset_20x20", 2, 128, 20, 20, qs=(128,), dist="offset"),
]


def _seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7fffffff


def fwd_inputs(c):
    """x [B, C, H, W] (bf16-exact), gamma, beta (f32-exact), all f64."""
    g = torch.Generator().manual_seed(_seed(c.name))
    r = torch.randn(c.B, c.C, c.H, c.W, generator=g, dtype=F64)
    if c.dist == "offset":
        x = bf(r * 0.25 + 2.0)
    elif c.dist == "small":
        x = bf(r * 2.0 ** -7 + 2.0 ** -6)
    else:
        x = bf(r * 1.5 + 0.3)
    if c.dist == "ones":
        cpg = c.C // G32
        x[:, 5 * cpg:6 * cpg] = 1.0
    gamma = (1 + 0.1 * torch.randn(c.C, generator=g)).to(F64)
    beta = (0.1 * torch.randn(c.C, generator=g)).to(F64)
    return x, gamma, beta


@dataclass(frozen=True)
class BwdCase:
    """B saved samples, n2 = sets * B cotangent samples; set_images = 0 means n2 // 2 when sets == 2 and B when sets == 1 (one set).
    split: the channels of the first part of a split target (0: one target); acc_dx2: the second part accumulates."""
    name: str
    B: int
    sets: int
    C: int
    H: int
    W: int
    silu: bool = True
    cdy: bool = False
    acc: bool = False
    acc2: bool = False
    split: int = 0
    acc_dx2: bool = False
    colsum: bool = False
    ld_extra: int = 0
    set_images: int = 0
    eps: float = EPS6

    @property
    def n2(self):
        return self.sets * self.B

    @property
    def simg(self):
        return self.set_images or self.B


BWD_CASES = [
    # SD widths: 8 x 8 (slab when on) and 20 x 20 (two-pass); one and two cotangent sets; SiLU off with compact dy = the transformer's norm
    BwdCase("sd320_8x8", 2, 2, 320, 8, 8, colsum=True), BwdCase("sd640_8x8", 2, 1, 640, 8, 8), BwdCase("sd960_8x8", 3, 2, 960, 8, 8, acc=True),
    BwdCase("sd320_8x8_tf", 2, 2, 320, 8, 8, silu=False, cdy=True), BwdCase("sd640_8x8_tf", 3, 1, 640, 8, 8, silu=False, cdy=True),
    BwdCase("sd320_20x20", 2, 1, 320, 20, 20, acc=True), BwdCase("sd640_20x20", 2, 2, 640, 20, 20, colsum=True), BwdCase("sd960_20x20", 2, 2, 960, 20, 20),
    BwdCase("sd640_20x20_tf", 2, 2, 640, 20, 20, silu=False, cdy=True),
    # ... so that every width has one AND two cotangent sets at both sites
    BwdCase("sd320_8x8_one", 3, 1, 320, 8, 8, acc=True), BwdCase("sd960_8x8_one", 2, 1, 960, 8, 8, colsum=True),
    BwdCase("sd640_8x8_two", 2, 2, 640, 8, 8), BwdCase("sd320_20x20_two", 2, 2, 320, 20, 20),
    BwdCase("sd640_20x20_one", 3, 1, 640, 20, 20, acc=True), BwdCase("sd960_20x20_one", 2, 1, 960, 20, 20, colsum=True),
    # channel slices x split: 1920 = 2 x 960 with the split point 1280 INSIDE slice 1; 2560 = 4 x 640 split at a slice boundary; 1280 = 2 x 640
    BwdCase("sl1920_split1280_4x4", 2, 2, 1920, 4, 4, acc=True, split=1280, acc_dx2=True, colsum=True, eps=EPS5),
    BwdCase("sl2560_split1280_6x5", 2, 2, 2560, 6, 5, acc=True, acc2=True, split=1280, acc_dx2=True, colsum=True, eps=EPS5),
    BwdCase("sl1280_split640_6x5", 3, 1, 1280, 6, 5, acc=True, split=640, eps=EPS5),
    BwdCase("sl1280_4x4_tf", 2, 2, 1280, 4, 4, silu=False, cdy=True, eps=EPS5),
    # the EXTRA forms, each running cotangent alone and all three, on a slab site and on a two-pass site
    BwdCase("ex_acc_8x8", 2, 2, 256, 8, 8, acc=True), BwdCase("ex_acc2_8x8", 2, 2, 256, 8, 8, acc2=True),
    BwdCase("ex_dx2_8x8", 2, 2, 256, 8, 8, split=128, acc_dx2=True), BwdCase("ex_all_8x8", 2, 2, 256, 8, 8, acc=True, acc2=True, split=128, acc_dx2=True, colsum=True),
    BwdCase("ex_acc_20x20", 2, 2, 256, 20, 20, acc=True), BwdCase("ex_acc2_20x20", 2, 2, 256, 20, 20, acc2=True),
    BwdCase("ex_dx2_20x20", 2, 2, 256, 20, 20, split=128, acc_dx2=True), BwdCase("ex_all_20x20", 2, 2, 256, 20, 20, acc=True, acc2=True, split=128, acc_dx2=True, colsum=True),
    BwdCase("split_plain_8x8", 2, 1, 256, 8, 8, split=64),          # a split target that does NOT accumulate: the old contents of dx2 must be gone
    # the No-IS layout: four saved samples, one cotangent each, the set taken from the sample index
    BwdCase("nois_sd320_8x8", 4, 1, 320, 8, 8, set_images=2, colsum=True), BwdCase("nois_c128_20x20_view", 4, 1, 128, 20, 20, set_images=2, acc=True, ld_extra=128),
    # (no case has pchunks != nchunks -- the statistics launch cut into more blocks than the apply launch: the smallest such shape has
    # 31 M elements, tests/test_groupnorm_ref_host.py::test_no_small_shape_has_a_statistics_launch_cut_differently searches for it)
    # the shapes at which tests/test_hip_gn_shortcut.py and the space-to-depth test of tests/test_hip_groupnorm.py hold their kernels, bit
    # for bit, to this entry point -- with THEIR inputs (bwd_inputs draws them as those tests do), so that the chain f64 -> siss_groupnorm_bwd_ld
    # -> siss_groupnorm_bwd_sc / _s2d is closed at one set of numbers
    BwdCase("sc_c96_6x6", 2, 2, 96, 6, 6, acc=True), BwdCase("s2d_c96_24x36", 2, 2, 96, 24, 36, acc=True, split=64, acc_dx2=True, colsum=True),
]


def _inputs_of_the_bitwise_suites(c):
    """The draws of tests/test_hip_gn_shortcut.py (case a_6x6_c96: seed C + H + K + B, K = 64; its accum is a product formed on the GPU, so
    ours is drawn from a second generator) and of the space-to-depth test of tests/test_hip_groupnorm.py ((2, 96, 24, 36, 64, True): seed
    C + H + W; every input, accum and the old dx2 included, is the one that test uses)."""
    s2d = c.name.startswith("s2d_")
    g = torch.Generator().manual_seed(c.C + c.H + c.W if s2d else c.C + c.H + 64 + c.B)
    b16 = lambda v: v.to(torch.bfloat16).to(F64)
    x = b16(torch.randn(c.B, c.C, c.H, c.W, generator=g) * (1.3 if s2d else 1.5) + (0.2 if s2d else 0.3))
    gamma, beta = (1 + 0.1 * torch.randn(c.C, generator=g)).to(F64), (0.1 * torch.randn(c.C, generator=g)).to(F64)
    dy = b16(torch.randn(c.n2, c.C, c.H, c.W, generator=g))
    if s2d:
        return x, gamma, beta, dy, b16(torch.randn(c.n2, c.C, c.H, c.W, generator=g)), None, b16(torch.randn(c.n2, c.C - c.split, c.H, c.W, generator=g))
    g2 = torch.Generator().manual_seed(_seed("bwd_" + c.name))
    return x, gamma, beta, dy, b16(torch.randn(c.n2, c.C, c.H, c.W, generator=g2)), None, None


def bwd_inputs(c):
    """x, gamma, beta, dy, accum, accum2, old2 (None where the case has none)."""
    if c.name.startswith(("sc_", "s2d_")):
        return _inputs_of_the_bitwise_suites(c)
    g = torch.Generator().manual_seed(_seed("bwd_" + c.name))
    x = bf(torch.randn(c.B, c.C, c.H, c.W, generator=g, dtype=F64) * 1.5 + 0.3)
    gamma = (1 + 0.1 * torch.randn(c.C, generator=g)).to(F64)
    beta = (0.1 * torch.randn(c.C, generator=g)).to(F64)
    rnd = lambda ch: bf(torch.randn(c.n2, ch, c.H, c.W, generator=g, dtype=F64))
    dy = rnd(c.C)
    return x, gamma, beta, dy, (rnd(c.C) if c.acc else None), (rnd(c.C) if c.acc2 else None), (rnd(c.C - c.split) if c.split else None)

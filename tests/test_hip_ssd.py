"""csrc/ssd.hip and what stands on it (siss_amd/ssd.py, deletion.ssd), on the GPU.

* siss_ssd_ratio and siss_ssd_dampen bitwise against tests/ssd_ref.py, buffers between sentinel guards (tests/test_hip_optimizer.py's
  Flat), n = 1027 (two blocks, tail 3) and n = 4,197,379 (the grid-stride loop wraps twice, tail 3).  Importances are squares of
  normals scaled into [1e-12, 1e2] with planted exact zeros in either or both, so that +inf and 0 / 0 occur; no denormals.
  Counts are exact; the three sums lie within n * 2^-53 relative of the restatement's exactly summed f64 values over the same f32
  numbers (only the fold order differs: the bound is the worst case of an f64 sum of n non-negative terms); on small integers the
  sums are exact.
* Fraction mode: select returns numpy's k-th largest over the integer keys; a zero threshold is refused; targets confine the selection.
* On the tiny engines: from_batches on the f32 engine is the restatement's accumulation of the gradients the shared loop left in
  gradient set 0 (within ONE run: the f32 backward is not repeatable run to run), the training state untouched; after an apply on
  the bf16 engine the shadow is bf16(p) and a forward and a backward equal, bit for bit, those of a fresh engine loaded with the
  dampened state dict (no stale operand copy).
* FisherAnchor.from_batches through the shared loop issues the launches of the loop it had before, in the same order.
* The files round trip and refuse another layout; a second rank (torch.distributed played by a stand-in) receives the ratio, dampens
  to rank 0's bits and checks its count.
* A run without the key calls no new entry point.  delete_celeb and delete_sd through main.main, with tools/ssd_select.py on their
  files; one rank with forced collectives.
"""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import ewc_ref as E
import ssd_ref as S
from test_hip_ewc import CELEB, batch, bits, keep_batches, run_task, state_of, stepper
from test_hip_optimizer import F32, F64, Flat, T, launch, refused
from test_hip_small_kernels import same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
MAX_BLOCKS = 2048
TIE = 3.0                                                   # the ratio several elements hold exactly
SUMS = ("sum_beta", "sum_delta2", "sum_p2_selected", "sum_p2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def grid_for(n):
    return min(max((n // 4 + 255) // 256, 1), MAX_BLOCKS)


_CASES = {}


def case(n):
    """(p, F_keep, F_forget, ratio) of size n, computed once and shared (nobody writes it): the planted zeros of ssd_ref.case, plus nine
    elements whose ratio is exactly TIE (one of them in the scalar tail)."""
    if n not in _CASES:
        p, fk, ff = S.case(n, n % 1000)
        idx = np.r_[np.linspace(5, n - 8, 8).astype(np.int64), n - 1]
        fk[idx], ff[idx] = 1.0, TIE
        r = S.ratio_f32(fk, ff)
        _CASES[n] = (p, fk, ff, r, idx)
    return _CASES[n]


# ================================================================ 1. siss_ssd_ratio
@pytest.mark.parametrize("n", S.SIZES)
def test_ratio_is_bitwise_the_restatement(dev, n):
    p, fk, ff, r, idx = case(n)
    assert np.isposinf(r).sum() > 0 and ((fk == 0) & (ff == 0)).sum() > 0 and not np.isnan(r).any()
    kb, fb, rb = Flat(n, F32, dev, body=fk), Flat(n, F32, dev, body=ff), Flat(n, F32, dev)
    launch("siss_ssd_ratio", kb.t, fb.t, rb.t, n)
    rb.check(T(r), f"n {n}: the ratio")
    kb.check(T(fk), "F_keep after the ratio"); fb.check(T(ff), "F_forget after the ratio")
    assert (r[idx] == TIE).all()


def test_ratio_refuses_misaligned_and_aliased_buffers(dev):
    n = 1027
    p, fk, ff, r, _ = case(n)
    kb, fb, rb = Flat(n + 8, F32, dev, body=np.r_[fk, fk[:8]]), Flat(n + 8, F32, dev, body=np.r_[ff, ff[:8]]), Flat(n + 8, F32, dev)
    refused("siss_ssd_ratio", kb.t[1:n + 1], fb.t[:n], rb.t[:n], n)          # four bytes off a 16-byte line, each in turn
    refused("siss_ssd_ratio", kb.t[:n], fb.t[1:n + 1], rb.t[:n], n)
    refused("siss_ssd_ratio", kb.t[:n], fb.t[:n], rb.t[1:n + 1], n)
    refused("siss_ssd_ratio", kb.t[:n], fb.t[:n], kb.t[:n], n)               # the output is an input
    refused("siss_ssd_ratio", kb.t[:n], fb.t[:n], fb.t[:n], n)
    refused("siss_ssd_ratio", kb.t[:n], fb.t[:n], fb.t[4:n + 4], n)          # ... or overlaps one
    refused("siss_ssd_ratio", kb.t[4:n + 4], fb.t[:n], kb.t[:n], n)
    refused("siss_ssd_ratio", kb.t[:n], fb.t[:n], rb.t[:n], 0)
    kb.check(T(np.r_[fk, fk[:8]]), "F_keep after the refusals"); fb.check(T(np.r_[ff, ff[:8]]), "F_forget after the refusals")
    rb.check(rb.host.clone(), "the ratio buffer after the refusals")


# ================================================================ 2. siss_ssd_dampen
class Dampen:
    """One launch of siss_ssd_dampen on host arrays, every buffer between guards."""

    def __init__(self, dev, p, r, threshold, strict, lam, apply=1):
        n = len(p)
        self.n, self.p, self.r = n, Flat(n, F32, dev, body=p), Flat(n, F32, dev, body=r)
        self.partials, self.stats = Flat(8 * MAX_BLOCKS, F64, dev, fill=-5.0), Flat(8, F64, dev, fill=-5.0)
        launch("siss_ssd_dampen", self.p.t, self.r.t, n, float(threshold), int(strict), float(lam), int(apply), self.partials.t, self.stats.t)
        self.r.check(T(r), "the ratio after the dampening")
        got = self.partials.d.cpu()
        g = self.partials.g
        same(got[g + 8 * grid_for(n):], self.partials.flat[g + 8 * grid_for(n):], "partial sums beyond the grid")
        same(got[:g], self.partials.flat[:g], "partial sums: guard before")
        self.raw = self.stats.np().copy()
        self.stats.guards("the statistics")
        assert self.raw[7] == 0.0 and not np.signbit(self.raw[7])
        self.s = dict(zip(S.STATS, self.raw[:7].tolist()))


def check_stats(run, want, n, what):
    for k in ("selected", "dampened", "zeroed"):
        assert run.s[k] == want[k], (what, k, run.s[k], want[k])
    print(f"[ssd] {what}: selected {want['selected']}, dampened {want['dampened']}, zeroed {want['zeroed']}; " + ", ".join(
        f"{k} {run.s[k]!r} / {want[k]!r} (rel {abs(run.s[k] - want[k]) / want[k] if want[k] else 0.0:.3g})" for k in SUMS))
    for k in SUMS:
        assert abs(run.s[k] - want[k]) <= n * 2.0 ** -53 * want[k], (what, k, run.s[k], want[k], n * 2.0 ** -53)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("n", S.SIZES)
def test_dampen_is_bitwise_the_restatement_with_exact_counts(dev, n, strict):
    """strict = 1: an alpha inside the data (the nine elements AT it stay out).  strict = 0: the same value as a threshold that nine
    elements hold exactly (they are in).  lambda = 10: selected weights with ratio <= lambda keep beta = 1."""
    p, fk, ff, r, idx = case(n)
    lam = 10.0
    q, sel, beta = S.dampen_f32(p, r, TIE, strict, lam)
    assert sel[idx].all() != bool(strict) and sel[idx].any() != bool(strict), "the ties are all in (>=) or all out (>)"
    want = S.stats_f64(p, q, sel, beta)
    assert 0 < want["zeroed"] < want["dampened"] < want["selected"] < n, want
    run = Dampen(dev, p, r, TIE, strict, lam)
    run.p.check(T(q), f"n {n} strict {strict}: p after the dampening (every unselected float and the guards keep their bits)")
    assert (q.view(np.uint32)[~sel] == p.view(np.uint32)[~sel]).all() and (q[sel & (beta < 1)] != p[sel & (beta < 1)]).sum() > 0
    check_stats(run, want, n, f"n {n} strict {strict}")
    # the dry run: every byte of p stays, the statistics are the same bits
    dry = Dampen(dev, p, r, TIE, strict, lam, apply=0)
    dry.p.check(T(p), "p after a dry run")
    assert (dry.raw.view(np.uint64) == run.raw.view(np.uint64)).all(), (dry.raw, run.raw)


@pytest.mark.parametrize("n", S.SIZES)
def test_dampen_on_small_integers_has_exact_sums(dev, n):
    p, r = S.int_case(n, n)
    q, sel, beta = S.dampen_f32(p, r, 2.0, 0, 1.0)
    want = S.stats_f64(p, q, sel, beta)
    run = Dampen(dev, p, r, 2.0, 0, 1.0)
    run.p.check(T(q), "p on integers")
    assert want["sum_delta2"] > 0 and all(run.s[k] == want[k] for k in S.STATS), (run.s, want)
    assert run.s["selected"] == int((r >= 2).sum()) == run.s["dampened"] and run.s["zeroed"] == 0
    assert run.s["sum_p2"] == float((p.astype(np.int64) ** 2).sum())


@pytest.mark.parametrize("n", S.SIZES)
def test_a_large_lambda_selects_and_changes_no_bit(dev, n):
    p, fk, ff = S.case(n, 5, zeros=False)
    r = S.ratio_f32(fk, ff)
    assert np.isfinite(r).all() and r.max() < 1e20
    run = Dampen(dev, p, r, 1.0, 1, 1e30)
    run.p.check(T(p), "p under a lambda above every ratio")
    assert run.s["selected"] == int((r > 1).sum()) > 0 and run.s["dampened"] == 0 and run.s["zeroed"] == 0
    assert run.s["sum_beta"] == run.s["selected"] and run.s["sum_delta2"] == 0.0 and run.s["sum_p2_selected"] > 0


def test_an_infinite_threshold(dev):
    n = 1027
    p, fk, ff, r, _ = case(n)
    ninf = int(np.isposinf(r).sum())
    assert ninf > 0
    run = Dampen(dev, p, r, math.inf, 1, 1.0)                # r > +inf: nothing
    run.p.check(T(p), "p under ratio > +inf")
    assert [run.s[k] for k in S.STATS[:6]] == [0.0] * 6 and run.s["sum_p2"] > 0
    run = Dampen(dev, p, r, math.inf, 0, 1.0)                # r >= +inf: the weights no keep gradient reached, to zero
    q, sel, beta = S.dampen_f32(p, r, math.inf, 0, 1.0)
    run.p.check(T(q), "p under ratio >= +inf")
    assert run.s["selected"] == run.s["zeroed"] == run.s["dampened"] == ninf and run.s["sum_beta"] == 0.0
    assert (q[sel] == 0).all() and run.s["sum_delta2"] == run.s["sum_p2_selected"]


def test_dampen_refusals_write_nothing(dev):
    n = 1027
    p, fk, ff, r, _ = case(n)
    pb, rb = Flat(n + 4, F32, dev, body=np.r_[p, p[:4]]), Flat(n + 4, F32, dev, body=np.r_[r, r[:4]])
    partials, stats = Flat(8 * MAX_BLOCKS, F64, dev, fill=-5.0), Flat(8, F64, dev, fill=-5.0)
    ok = dict(p=pb.t[:n], r=rb.t[:n], n=n, thr=1.0, strict=1, lam=1.0)
    for change in (dict(p=pb.t[1:n + 1]), dict(r=rb.t[1:n + 1]), dict(n=0), dict(lam=0.0), dict(lam=-1.0), dict(lam=math.nan),
                   dict(lam=math.inf), dict(thr=math.nan), dict(thr=-1.0), dict(p=None), dict(r=None)):
        a = dict(ok, **change)
        refused("siss_ssd_dampen", a["p"], a["r"], a["n"], a["thr"], a["strict"], a["lam"], 1, partials.t, stats.t)
    refused("siss_ssd_dampen", ok["p"], ok["r"], n, 1.0, 1, 1.0, 1, None, stats.t)
    refused("siss_ssd_dampen", ok["p"], ok["r"], n, 1.0, 1, 1.0, 1, partials.t, None)
    pb.check(T(np.r_[p, p[:4]]), "p after the refusals")
    stats.check(stats.host.clone(), "the statistics after the refusals")
    partials.check(partials.host.clone(), "the partial sums after the refusals")


# ================================================================ 3. fraction mode and targets
def fake_engine(dev, numels=(3001, 64, 37, 1500, 770), align=64, seed=0):
    specs, off = {}, 0
    for i, n in enumerate(numels):
        specs[f"w{i}"] = types.SimpleNamespace(name=f"w{i}", off=off, numel=n)
        off += -(-n // align) * align
    flat = torch.randn(off, generator=torch.Generator().manual_seed(seed)).to(dev)
    real = np.zeros(off, bool)
    for sp in specs.values():
        real[sp.off:sp.off + sp.numel] = True
    flat[torch.from_numpy(~real).to(dev)] = 0
    eng = types.SimpleNamespace(ps=types.SimpleNamespace(specs=specs, total=off, flat=flat), device=dev, refreshed=[])
    eng.refresh_weights = lambda cast_shadow=False: eng.refreshed.append(cast_shadow)
    return eng, real


def fake_importances(eng, real, seed):
    from siss_amd.ssd import Importances
    p, fk, ff = S.case(eng.ps.total, seed)
    fk[~real], ff[~real] = 0, 0
    return Importances(eng, T(fk), T(ff)), fk, ff


def test_fraction_mode_selects_the_kth_largest_key(dev):
    from siss_amd import ssd
    eng, real = fake_engine(dev)
    imp, fk, ff = fake_importances(eng, real, 1)
    r = S.ratio_f32(fk, ff)
    same(imp.ratio.cpu(), T(r), "Importances.ratio")
    assert (r[~real] == 0).all()
    ninf = int(np.isposinf(r).sum())
    nreal = int(real.sum())
    for fraction in (0.01, 0.2, 1e-9, (ninf - 0.4) / nreal):
        k = max(1, round(fraction * nreal))
        thr, strict, got_k, gt, ge = ssd.select(imp, fraction=fraction)
        t, tb, want_gt, want_ge = S.kth_largest(r, k)
        assert got_k == k and not strict and ssd.float_bits(thr) == tb and (gt, ge) == (want_gt, want_ge), (fraction, thr, t, gt, ge)
        assert ge == int(S.selected(r, thr, False).sum()) >= k
        st = ssd.dampen(eng, imp, thr, strict, 1.0, apply=False)
        assert st["selected"] == ge and eng.refreshed == []
    assert math.isinf(ssd.select(imp, fraction=1e-9)[0]), "+inf is a legal threshold: weights no keep gradient reached rank on top"
    thr, strict, _, gt, ge = ssd.select(imp, alpha=TIE)
    assert strict and thr == TIE and (gt, ge) == (int((r > TIE).sum()), int((r >= TIE).sum()))
    with pytest.raises(ValueError, match="exactly one"):
        ssd.select(imp, alpha=1.0, fraction=0.1)
    # a buffer whose k-th largest ratio is 0
    ff2 = np.zeros_like(ff)
    ff2[:40] = 1.0
    sparse = ssd.Importances(eng, T(np.where(real, f32(1), f32(0)).astype(f32)), T(ff2))
    with pytest.raises(ValueError, match="threshold of zero would select the alignment padding"):
        ssd.select(sparse, fraction=0.5)
    assert ssd.select(sparse, fraction=40 / nreal)[3:] == (0, 40)
    # non-finite importances are refused upstream
    bad = fk.copy()
    bad[3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ssd.Importances(eng, T(bad), T(ff))


def test_targets_confine_the_selection_and_the_apply_refreshes(dev):
    from siss_amd import ssd
    eng, real = fake_engine(dev)
    imp, fk, ff = fake_importances(eng, real, 2)
    names = ["w0", "w3"]
    inside = np.zeros(eng.ps.total, bool)
    for nme in names:
        sp = eng.ps.specs[nme]
        inside[sp.off:sp.off + sp.numel] = True
    r = np.where(inside, S.ratio_f32(fk, ff), f32(0)).astype(f32)
    thr, strict, k, gt, ge = ssd.select(imp, fraction=0.1, targets=names)
    same(imp.ratio.cpu(), T(r), "the ratio restricted to the targets")
    assert ssd.float_bits(thr) == S.kth_largest(r, k)[1] and k == round(0.1 * real.sum())
    p0 = eng.ps.flat.cpu().numpy().copy()
    st = ssd.dampen(eng, imp, thr, strict, 0.5)
    q, sel, beta = S.dampen_f32(p0, r, thr, strict, 0.5)
    same(eng.ps.flat.cpu(), T(q), "the flat buffer after the dampening")
    assert not sel[~inside].any() and sel.sum() == st["selected"] == ge and eng.refreshed == [True]
    assert (eng.ps.flat.cpu().numpy().view(np.uint32)[~inside] == p0.view(np.uint32)[~inside]).all()
    want = S.stats_f64(p0, q, sel, beta)
    assert st["fraction_selected"] == st["selected"] / real.sum() and st["mean_beta"] == st["sum_beta"] / st["selected"]
    assert st["delta_norm"] == math.sqrt(st["sum_delta2"]) and st["relative_change"] == math.sqrt(st["sum_delta2"] / st["sum_p2"])
    assert abs(st["sum_delta2"] - want["sum_delta2"]) <= eng.ps.total * 2.0 ** -53 * want["sum_delta2"]
    per = ssd.per_tensor(imp, thr, strict)
    assert set(per) <= set(names) and sum(per.values()) == st["selected"]
    assert per == {nme: int(sel[eng.ps.specs[nme].off:eng.ps.specs[nme].off + eng.ps.specs[nme].numel].sum()) for nme in per}


def test_files_round_trip_and_refuse_another_layout(dev, tmp_path):
    from siss_amd import ssd
    eng, real = fake_engine(dev)
    imp, fk, ff = fake_importances(eng, real, 3)
    imp.keep_batches, imp.forget_batches, imp.batch_size, imp.seed = 5, 4, 1, 9
    assert not ssd.Importances.present(str(tmp_path))
    imp.save(str(tmp_path))
    imp.save_report(str(tmp_path), dict(threshold=2.0, stats=dict(selected=7)))
    assert ssd.Importances.present(str(tmp_path))
    c = json.load(open(tmp_path / ssd.CONFIG_FILE))
    assert (c["source"], c["keep_batches"], c["forget_batches"], c["seed"], c["threshold"], c["stats"]) == ("given", 5, 4, 9, 2.0, {"selected": 7})
    assert (c["total"], c["tensors"], c["real_params"]) == (eng.ps.total, 5, int(real.sum()))
    back = ssd.Importances.load(str(tmp_path), eng)
    same(back.keep.cpu(), T(fk), "F_keep from the file"); same(back.forget.cpu(), T(ff), "F_forget from the file")
    same(back.ratio.cpu(), imp.ratio.cpu(), "the ratio of the loaded importances")
    assert (back.source, back.keep_batches, back.forget_batches, back.batch_size, back.seed) == ("loaded", 5, 4, 1, 9)
    other, _ = fake_engine(dev, numels=(3001, 64, 37, 1500, 771))
    with pytest.raises(ValueError, match="another architecture or parameter layout"):
        ssd.Importances.load(str(tmp_path), other)
    with pytest.raises(ValueError, match="another parameter layout"):
        ssd.dampen(other, imp, 1.0, True, 1.0, apply=False)


# ================================================================ 4. the tiny engines
def forget_batches(seed=21, B=2):
    g = torch.Generator().manual_seed(seed)
    one = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    while True:
        yield one.repeat(B, 1, 1, 1)


@pytest.mark.parametrize("B", [1, 2])
def test_from_batches_accumulates_the_loops_gradients_and_leaves_the_state_alone(dev, B):
    from siss_amd import lib
    from siss_amd.ssd import Importances
    from siss_amd.variants import real_mask
    eng, st = stepper(dtype=torch.float32)
    st.step(*batch(0, dev))                                  # a warm state: non-zero moments, step count 1, a recorded fill plan
    before = state_of(eng, st)
    plans = dict(eng._fill_plans)
    fed, orig = [], lib.call

    def spy_call(name, *a, **k):
        if name == "siss_fisher_accumulate":
            assert a[0].data_ptr() == eng.ps.grads[0].data_ptr() and a[2] == eng.ps.total
            fed.append((a[0].clone(), a[3], a[1].data_ptr()))
        assert "adamw" not in name and "grad_norms" not in name, f"an optimizer launch inside from_batches: {name}"
        return orig(name, *a, **k)
    lib.call = spy_call
    try:
        imp = Importances.from_batches(st, keep_batches(B=B), forget_batches(B=B), 3, 2, generator=torch.Generator(device=dev).manual_seed(0),
                                       batch_size=B, seed=0)
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    assert [w for _, w, _ in fed] == [1.0 / 3] * 3 + [0.5] * 2
    assert [ptr for _, _, ptr in fed] == [imp.keep.data_ptr()] * 3 + [imp.forget.data_ptr()] * 2      # keep first, then forget
    want_keep = want_forget = np.zeros(eng.ps.total, f32)
    for g, w, _ in fed[:3]:
        assert float(g.abs().max()) > 0
        want_keep = E.fisher_accumulate_f32(g.cpu().numpy(), want_keep, w)
    for g, w, _ in fed[3:]:
        want_forget = E.fisher_accumulate_f32(g.cpu().numpy(), want_forget, w)
    same(imp.keep.cpu(), T(want_keep), "F_keep against the restatement's accumulation of the three keep gradients")
    same(imp.forget.cpu(), T(want_forget), "F_forget against the restatement's accumulation of the two forget gradients")
    same(imp.ratio.cpu(), T(S.ratio_f32(want_keep, want_forget)), "the ratio of the two")
    assert not torch.equal(fed[0][0], fed[1][0]) and not torch.equal(fed[3][0], fed[0][0])
    for key, t in state_of(eng, st).items():
        assert torch.equal(bits(t), bits(before[key])), f"from_batches changed {key}"
    assert int(eng.ps.grads.count_nonzero()) == 0, "the gradient buffers are not zero on return"
    assert st._micro == 0 and eng.wgrad_overwrite is False and dict(eng._fill_plans) == plans and st._pending == []
    real = real_mask(eng.ps.specs, eng.ps.total, dev)
    for F in (imp.keep, imp.forget, imp.ratio):
        assert int(F[~real].count_nonzero()) == 0 and bool((F >= 0).all())
    assert (imp.source, imp.keep_batches, imp.forget_batches, imp.batch_size) == ("computed", 3, 2, B)


def one_pass(eng, st, dev):
    """One forward and one backward of a fixed micro-batch at the engine's weights: (prediction, gradient set 0)."""
    from siss_amd.variants import backward_batch, quiet_backward
    seen, inner = [], eng.forward

    def spy(*a, **k):
        seen.append(inner(*a, **k))
        return seen[-1]
    eng.forward = spy
    try:
        with quiet_backward(st, "test"):
            backward_batch(st, next(keep_batches(seed=33)), 1, first=True, generator=torch.Generator(device=dev).manual_seed(8))
            g = eng.ps.grads[0].clone()
    finally:
        del eng.forward
    torch.cuda.synchronize()
    return seen[0].clone(), g


def test_after_an_apply_no_stale_operand_copy_survives(dev):
    from siss_amd import ssd
    eng, st = stepper()
    pred0, g0 = one_pass(eng, st, dev)
    imp = ssd.Importances.from_batches(st, keep_batches(), forget_batches(), 3, 2, generator=torch.Generator(device=dev).manual_seed(0))
    thr, strict, k, gt, ge = ssd.select(imp, fraction=0.05)
    p0 = eng.ps.flat.clone()
    dry = ssd.dampen(eng, imp, thr, strict, 1.0, apply=False)
    assert torch.equal(bits(eng.ps.flat), bits(p0))
    stats = ssd.dampen(eng, imp, thr, strict, 1.0)
    torch.cuda.synchronize()
    assert stats == dry and stats["selected"] == ge >= k and stats["dampened"] > 0 and stats["relative_change"] > 0, stats
    q, sel, beta = S.dampen_f32(p0.cpu().numpy(), imp.ratio.cpu().numpy(), thr, strict, 1.0)
    same(eng.ps.flat.cpu(), T(q), "the engine's parameters after the dampening")
    same(eng.ps.shadow.cpu(), eng.ps.flat.to(torch.bfloat16).cpu(), "the bf16 shadow after the dampening")
    pred1, g1 = one_pass(eng, st, dev)
    assert not torch.equal(pred1, pred0) and not torch.equal(g1, g0), "the dampening did not reach the forward / backward pass"
    fresh, st2 = stepper()
    fresh.load_state_dict({n: t.clone() for n, t in eng.state_dict().items()})
    same(fresh.ps.flat.cpu(), eng.ps.flat.cpu(), "a fresh engine loaded with the dampened state dict")
    pred2, g2 = one_pass(fresh, st2, dev)
    same(pred1.cpu(), pred2.cpu(), "the forward output against a fresh engine's")
    same(g1.cpu(), g2.cpu(), "the gradient set against a fresh engine's")


def test_fisher_anchor_issues_the_launches_of_its_former_loop(dev):
    """The loop FisherAnchor.from_batches had before it moved into variants.fisher_of_batches, restated here, against the call:
    the same entry points in the same order, and (bf16 engine: repeatable) the same F bit for bit."""
    from siss_amd import lib
    from siss_amd.ewc import FisherAnchor
    from siss_amd.variants import backward_batch, quiet_backward

    def former(st, it, n, generator):
        ps = st.e.ps
        F = torch.zeros_like(ps.flat)
        with quiet_backward(st, "FisherAnchor.from_batches"):
            for _ in range(n):
                backward_batch(st, next(it), 1, first=True, prepare=None, sample_noise=None, conditioning=None, timestep_low=0,
                               generator=generator)
                lib.call("siss_fisher_accumulate", ps.grads[0], F, ps.total, 1.0 / n)
        return F
    logs, Fs = [], []
    for which in ("former", "shared"):
        eng, st = stepper()
        calls, orig = [], lib.call
        lib.call = lambda name, *a, **k: (calls.append(name), orig(name, *a, **k))[1]
        try:
            gen = torch.Generator(device=dev).manual_seed(0)
            if which == "former":
                Fs.append(former(st, keep_batches(), 3, gen))
            else:
                Fs.append(FisherAnchor.from_batches(st, keep_batches(), 3, strength=2.0, generator=gen, normalize=False).fisher)
            torch.cuda.synchronize()
        finally:
            lib.call = orig
        logs.append(calls)
    assert logs[0] == logs[1] and logs[0].count("siss_fisher_accumulate") == 3 and len(logs[0]) > 30
    assert not [c for c in logs[1] if "ssd" in c]
    same(Fs[1].cpu(), Fs[0].cpu(), "F through the shared loop against the former loop's")


def test_a_second_rank_receives_the_ratio_dampens_and_checks_its_count(dev, tmp_path, monkeypatch):
    """_DeleteBase.ssd_dampen as rank 1 of 2 over a stand-in for torch.distributed that plays rank 0: the description first, then the
    ratio, then rank 0's selected count; rank 1 builds nothing, writes nothing, and ends on rank 0's parameters bit for bit."""
    import torch.distributed as dist
    from siss_amd import hydra_lite as H
    from siss_amd import ssd
    cfg = H.compose("delete_celeb", os.path.join(ROOT, "config"), [*CELEB[1:], f"output_dir={tmp_path}/out",
                                                                   "+deletion.ssd={fraction:0.05,keep_batches:3,forget_batches:2}"])
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    eng0, st0 = stepper()
    imp0 = ssd.Importances.from_batches(st0, keep_batches(), forget_batches(), 3, 2, generator=torch.Generator(device=dev).manual_seed(0),
                                        batch_size=2, seed=0)
    thr, strict, k, gt, ge = ssd.select(imp0, fraction=0.05)
    want = ssd.dampen(eng0, imp0, thr, strict, 1.0)
    words, calls = [imp0.config(), want["selected"]], []

    def objects(word, src, group):
        assert word == [None] and src == 0 and group == "group"
        word[0] = words[calls.count("objects")]
        calls.append("objects")

    def tensor(t, src, group):
        assert t.shape == imp0.ratio.shape and int(t.count_nonzero()) == 0
        t.copy_(imp0.ratio)
        calls.append("ratio")
    monkeypatch.setattr(dist, "broadcast_object_list", objects)
    monkeypatch.setattr(dist, "broadcast", tensor)
    monkeypatch.setattr(ssd.Importances, "from_batches", lambda *a, **k: pytest.fail("a rank other than 0 built the importances"))
    eng1, st1 = stepper()
    fields = task.ssd_dampen(st1, None, None, 2, None, dev, 1, 2, "group")
    torch.cuda.synchronize()
    assert calls == ["objects", "ratio", "objects"]
    assert fields == dict(ssd_selected=want["selected"], ssd_threshold=thr, ssd_lambda=1.0) and want["selected"] > 0
    same(eng1.ps.flat.cpu(), eng0.ps.flat.cpu(), "rank 1's parameters against rank 0's")
    same(eng1.ps.shadow.cpu(), eng0.ps.shadow.cpu(), "rank 1's shadow against rank 0's")
    assert not os.path.exists(tmp_path / "out"), "a rank other than 0 wrote files"
    # a rank that dampens another number of weights than rank 0 says so
    calls.clear()
    words[1] = want["selected"] + 1
    _, st2 = stepper()
    with pytest.raises(RuntimeError, match=f"rank 1 dampened {want['selected']} weights, rank 0 {want['selected'] + 1}"):
        task.ssd_dampen(st2, None, None, 2, None, dev, 1, 2, "group")


# ================================================================ 5. the tasks
ZERO = ("training_steps=0", "lr_scheduler=constant")
KEY = "+deletion.ssd={fraction:0.01,keep_batches:4,forget_batches:4}"


def logged(fn, *args):
    """(fn(*args), the names of every lib.call and lib.query it made)"""
    from siss_amd import lib
    calls, orig_call, orig_query = [], lib.call, lib.query
    lib.call = lambda name, *a, **k: (calls.append(name), orig_call(name, *a, **k))[1]
    lib.query = lambda name, *a: (calls.append(name), orig_query(name, *a))[1]
    try:
        return fn(*args), calls
    finally:
        lib.call, lib.query = orig_call, orig_query


def new_entry_points(calls):
    return [n for n in calls if "ssd" in n or "fisher" in n or "absf" in n]


def load_flat(task, rundir):
    from siss_amd.model import UNet2DConditionModel, UNet2DModel
    cls = UNet2DConditionModel if task == "delete_sd" else UNet2DModel
    m = cls.from_pretrained(rundir, subfolder="unet", device="cuda:0", compute_dtype=torch.bfloat16)
    return m.engine.ps.flat.detach().cpu().numpy().copy()


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_dampens_without_a_step_and_reloads_its_importances(dev, tmp_path, task):
    from safetensors.torch import load_file
    from siss_amd.ssd import CONFIG_FILE, IMPORTANCE_FILE
    rundir, lines = run_task(tmp_path, task, "keyed", *ZERO, KEY)
    assert lines == [] and os.path.isdir(os.path.join(rundir, "unet"))
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    imp = load_file(os.path.join(rundir, IMPORTANCE_FILE))
    assert set(imp) == {"keep", "forget"} and all(t.shape == (c["total"],) and t.dtype == torch.float32 and bool((t >= 0).all()) for t in imp.values())
    assert c["config"] == {"alpha": None, "fraction": 0.01, "lambda": 1.0, "keep_batches": 4, "forget_batches": 4, "batch_size": 1,
                           "seed": 0, "targets": None, "path": None}
    assert (c["source"], c["keep_batches"], c["forget_batches"], c["batch_size"], c["strict"]) == ("computed", 4, 4, 1, False)
    assert c["total"] >= c["real_params"] > 0 and c["tensors"] > 0 and c["k"] == max(1, round(0.01 * c["real_params"]))
    st = c["stats"]
    assert st["selected"] == c["count_ge"] >= c["k"] > c["count_gt"] and sum(c["per_tensor"].values()) == st["selected"]
    assert 0 < st["relative_change"] < 1 and 0 <= st["mean_beta"] <= 1 and st["fraction_selected"] == st["selected"] / c["real_params"]
    thr = np.array([c["threshold_bits"]], np.uint32).view(f32)[0]
    assert thr > 0 and (math.isinf(c["threshold"]) or f32(c["threshold"]) == thr)
    print(f"[ssd] {task}: threshold {thr!r}, {st}")
    # the saved unet/ is, bit for bit, the restatement's dampening of the weights a run without the key saves untouched -- a run
    # that calls no new entry point
    (plain_dir, _), calls = logged(run_task, tmp_path, task, "plain", *ZERO)
    assert calls and not new_entry_points(calls), "a run without the key reached csrc/ssd.hip"
    assert not os.path.exists(os.path.join(plain_dir, CONFIG_FILE)) and not os.path.exists(os.path.join(plain_dir, IMPORTANCE_FILE))
    p0 = load_flat(task, plain_dir)
    r = S.ratio_f32(imp["keep"].numpy(), imp["forget"].numpy())
    q, sel, beta = S.dampen_f32(p0, r, thr, False, 1.0)
    assert int(sel.sum()) == st["selected"] and S.kth_largest(r, c["k"])[1] == c["threshold_bits"]
    same(T(load_flat(task, rundir)), T(q), "the saved unet/ against the restatement's dampened buffer")
    assert not np.array_equal(q, p0)
    # the sweep tool on the first run's files and the untouched checkpoint: dry runs, the run's own value among them
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ssd_select
    rows = ssd_select.main([rundir, plain_dir, "--fraction", "0.01", "0.001", "--alpha", "1e30", "--json"] + (["--cond"] if task == "delete_sd" else []))
    assert [r.get("fraction", r.get("alpha")) for r in rows] == [1e30, 0.01, 0.001] and rows[0]["selected"] == int(np.isposinf(r).sum())
    assert {k: rows[1][k] for k in st} == st and rows[1]["threshold"] == float(thr) and rows[2]["selected"] < rows[1]["selected"]
    same(T(load_flat(task, plain_dir)), T(p0), "the checkpoint after the sweep")
    # a second run that loads the first run's importances
    rundir2, _ = run_task(tmp_path, task, "reloaded", *ZERO, KEY[:-1] + ",path:'%s'}" % rundir)
    c2 = json.load(open(os.path.join(rundir2, CONFIG_FILE)))
    imp2 = load_file(os.path.join(rundir2, IMPORTANCE_FILE))
    assert c2["source"] == "loaded" and torch.equal(bits(imp2["keep"]), bits(imp["keep"])) and torch.equal(bits(imp2["forget"]), bits(imp["forget"]))
    assert c2["threshold_bits"] == c["threshold_bits"] and c2["stats"] == c["stats"] and c2["per_tensor"] == c["per_tensor"]
    same(T(load_flat(task, rundir2)), T(q), "the reloaded run's unet/")


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_loop_follows_from_the_dampened_weights(dev, tmp_path, task):
    from siss_amd.ssd import CONFIG_FILE
    rundir, lines = run_task(tmp_path, task, "keyed3", KEY)
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    assert len(lines) == 3 and os.path.isdir(os.path.join(rundir, "unet"))
    for st in lines:
        assert (st["ssd_selected"], st["ssd_lambda"]) == (c["stats"]["selected"], 1.0) and f32(st["ssd_threshold"]) == f32(c["threshold"]), st
    (_, plain), calls = logged(run_task, tmp_path, task, "plain3")
    assert len(calls) > 100 and calls.count("siss_recombine_clip_adamw") == 3 and not new_entry_points(calls), \
        "a run without the key reached csrc/ssd.hip"
    assert len(plain) == 3 and not [k for l in plain for k in l if k.startswith("ssd")]
    assert plain[0]["norm_loss_x"] != lines[0]["norm_loss_x"], "the first step did not start from the dampened weights"


@pytest.mark.parametrize("task", ["delete_celeb", "delete_sd"])
def test_task_combines_with_the_mask_and_the_anchor(dev, tmp_path, task):
    from siss_amd.ssd import CONFIG_FILE
    for name, other, made in (("mask", "+deletion.saliency={fraction:0.5,batches:1}", "saliency.json"),
                              ("anchor", "+deletion.ewc={strength:10,batches:1}", "fisher.json")):
        rundir, lines = run_task(tmp_path, task, name, "training_steps=1", KEY, other)
        assert len(lines) == 1 and "ssd_selected" in lines[0]
        assert os.path.getmtime(os.path.join(rundir, made)) >= os.path.getmtime(os.path.join(rundir, CONFIG_FILE))
        assert ("saliency_params" in lines[0]) == (name == "mask") and ("ewc_penalty" in lines[0]) == (name == "anchor")


# ================================================================ 6. one rank, forced collectives
def test_forced_collectives_on_one_rank_equal_the_run_without_a_group(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_ssd_worker.py"), ROOT], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL_SSD ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line[-1][len("RCCL_SSD "):])
    assert out["dp_on"] and out["equal_importances"] and out["equal_dampened"] and out["equal_params"] and out["equal_moments"], out
    assert out["selected"] > 0 and out["all_reduces"] >= 1 and out["all_reduces_in_from_batches"] == 0, out

"""csrc/uce.hip and what stands on it (siss_amd/uce.py, deletion.uce), on the GPU.

* siss_uce_delta bitwise against the f32 fmaf chain of tests/uce_ref.py, every buffer between sentinel guards (tests/test_hip_optimizer.py's
  Flat): X in {4, 20, 64, 68, 132} (the tail only; one trip plus one tail step; one full column tile; a second, partial tile; three
  tiles) x rows in {1, 31, 33, 64}; a three-job table (rows 1, 33, 16) whose padded gaps in p and unnamed rows of delta hold a
  sentinel; one job of 320 x 768; E and p intact; the same values with the job order reversed.
* siss_uce_apply: p' bitwise f32(p + delta), gaps and non-target floats keep their bits; the two sums within n * 2^-53 relative of the
  exactly summed f64 values over the same f32 numbers (only the fold order differs: the worst case of an f64 sum of n non-negative
  terms -- tests/test_hip_ssd.py's bound) and exact on small integers; max |delta| and the count exact; a dry run leaves p bitwise;
  every refusal writes nothing.
* On the tiny UNetCondEngine, bf16 and f32: floats outside the targets keep their bits, the targets are the restatement's bits given
  the same f32 E, the shadow is bf16(p), a forward and a backward equal those of a fresh engine loaded with the edited state dict; the
  f32 engine matches the f64 oracle loaded with the restatement's weights at tests/test_hip_f32_mode.py's forward bound; `residuals`
  agrees with the restatement's to 1e-6 absolute (f64 on both sides over the same bits).
* The files round trip through a run's `path`; a second rank (torch.distributed played by a stand-in) receives E, applies it and
  matches rank 0's sum of delta^2 bit for bit.
* delete_sd through main.main with training_steps 0 and 2; a run without the key calls no new entry point.
"""
import json
import os
import struct

import numpy as np
import pytest
import torch

import uce_ref as R
from test_hip_optimizer import F32, F64, Flat, T, launch, refused
from test_hip_small_kernels import bits, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
SENT = 77.0
XS = [4, 20, 64, 68, 132]
ROWS = [1, 31, 33, 64]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def table(jobs):
    import ctypes
    b = R.job_bytes(jobs)
    return (ctypes.c_char * len(b)).from_buffer_copy(b)


def layout(rows_list, X, gap=64):
    """[(w_off, row_off, rows)] with every weight on a 64-float line and a gap of at least `gap` floats behind it; total floats of p"""
    jobs, off, row = [], 0, 0
    for rows in rows_list:
        jobs.append((off, row, rows))
        off += -(-(rows * X + gap) // 64) * 64
        row += rows
    return jobs, off, row


_CASES = {}


def case(rows_list, X, seed=0):
    """(jobs, p with SENT in the gaps, E, the restatement's compact delta with SENT nowhere: every row is named) -- computed once, shared"""
    key = (tuple(rows_list), X, seed)
    if key not in _CASES:
        g = np.random.default_rng(1000 * X + sum(rows_list) + seed)
        jobs, n, total_rows = layout(rows_list, X)
        p = np.full(n, SENT, f32)
        for w, _, rows in jobs:
            p[w:w + rows * X] = (g.standard_normal(rows * X) / 8).astype(f32)
        E = (g.standard_normal((X, X)) / np.sqrt(X)).astype(f32)
        d = R.compact(R.delta_ref(p, jobs, E), jobs, X, total_rows, SENT)
        _CASES[key] = (jobs, p, E, d, total_rows)
    return _CASES[key]


def run_delta(dev, jobs, p, E, total_rows, X):
    pb, eb, db = Flat(len(p), F32, dev, body=p), Flat(X * X, F32, dev, body=E.reshape(-1)), Flat(total_rows * X, F32, dev)
    launch("siss_uce_delta", pb.t, table(jobs), len(jobs), eb.t, X, db.t)
    pb.check(T(p), "p after the delta launch")
    eb.check(T(E.reshape(-1)), "E after the delta launch")
    return db


# ================================================================ 1. siss_uce_delta
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("X", XS)
def test_delta_is_bitwise_the_chain(dev, X, rows):
    jobs, p, E, d, total = case([rows], X)
    run_delta(dev, jobs, p, E, total, X).check(T(d), f"X {X}, rows {rows}: delta")
    assert np.abs(d).max() > 0


@pytest.mark.parametrize("X", [20, 132])
def test_delta_of_a_three_job_table_leaves_gaps_and_unnamed_rows_alone(dev, X):
    jobs, p, E, d, total = case([1, 33, 16], X)
    run_delta(dev, jobs, p, E, total, X).check(T(d), f"X {X}: the three jobs' delta")
    # the same jobs with a hole of 3 rows in delta that no job names, the table reversed: the same values, the hole keeps its sentinel
    holed = [(w, r0 + (3 if i else 0), rows) for i, (w, r0, rows) in enumerate(jobs)]
    want = R.compact({i: d[r0 * X:(r0 + rows) * X] for i, (_, r0, rows) in enumerate(jobs)}, holed, X, total + 3, SENT)
    assert (want[X:4 * X] == SENT).all()
    run_delta(dev, holed[::-1], p, E, total + 3, X).check(T(want), f"X {X}: reversed table, a hole in delta")


def test_delta_of_a_320_by_768_job_and_the_reversed_table(dev):
    X = 768
    jobs, p, E, d, total = case([33, 320], X)
    run_delta(dev, jobs, p, E, total, X).check(T(d), "320 x 768 behind 33 x 768: delta")
    run_delta(dev, jobs[::-1], p, E, total, X).check(T(d), "the table reversed: delta")


def test_delta_refusals_write_nothing(dev):
    X = 64
    jobs, p, E, d, total = case([33, 16], X)
    pb, eb, db = Flat(len(p), F32, dev, body=p), Flat(X * X + 8, F32, dev, body=np.r_[E.reshape(-1), E.reshape(-1)[:8]]), Flat(total * X + 8, F32, dev)
    ok = lambda **k: dict(dict(p=pb.t, jobs=jobs, E=eb.t[:X * X], X=X, delta=db.t[:total * X]), **k)
    n_t = jobs[1][0] + jobs[1][2] * X
    rows = [ok(X=66), ok(X=0), ok(jobs=[]), ok(jobs=[(0, 0, 0)]), ok(jobs=[jobs[0], (jobs[1][0], 33, -1)]), ok(jobs=[(2, 0, 33)]),
            ok(jobs=[jobs[0], (jobs[1][0], 20, 16)]), ok(p=pb.t[1:]), ok(E=eb.t[1:X * X + 1]), ok(delta=db.t[2:total * X + 2]),
            ok(delta=pb.t), ok(delta=pb.t[n_t - 4:]), ok(E=pb.t[:X * X]), ok(E=db.t[:X * X]), ok(delta=eb.t[:X * X])]
    for a in rows:
        refused("siss_uce_delta", a["p"], table(a["jobs"]) if a["jobs"] else table([(0, 0, 1)]), len(a["jobs"]), a["E"], a["X"], a["delta"])
    pb.check(T(p), "p after the refusals")
    eb.check(eb.host.clone(), "E after the refusals")
    db.check(db.host.clone(), "delta after the refusals")


# ================================================================ 2. siss_uce_apply
class Apply:
    """One launch of siss_uce_apply on host arrays, every buffer between guards."""

    def __init__(self, dev, jobs, p, delta, X, apply=1):
        from siss_amd import lib
        floats = sum(r for _, _, r in jobs) * X
        words = lib.query("siss_uce_partials_words", floats, len(jobs))
        assert words >= 4 * R.chunks(jobs, X)
        self.p, self.d = Flat(len(p), F32, dev, body=p), Flat(len(delta), F32, dev, body=delta)
        self.partials, self.stats = Flat(words, F64, dev, fill=-5.0), Flat(4, F64, dev, fill=-5.0)
        launch("siss_uce_apply", self.p.t, table(jobs), len(jobs), X, self.d.t, int(apply), self.partials.t, self.stats.t)
        self.d.check(T(delta), "delta after the add")
        got, g = self.partials.d.cpu(), self.partials.g
        used = 4 * R.chunks(jobs, X)
        same(got[g + used:], self.partials.flat[g + used:], "partial rows beyond the chunks")
        same(got[:g], self.partials.flat[:g], "partial rows: guard before")
        self.stats.guards("the statistics")
        self.s = dict(zip(R.STATS, self.stats.np().tolist()))


def check_stats(s, want, n):
    assert s["floats"] == want["floats"] == n and s["max_delta"] == want["max_delta"]
    for k in ("sum_delta2", "sum_p2"):
        assert abs(s[k] - want[k]) <= n * 2.0 ** -53 * want[k], (k, s[k], want[k])


@pytest.mark.parametrize("rows_list,X", [([1], 4), ([31], 20), ([1, 33, 16], 132), ([64, 65], 64), ([33, 320], 768)])
def test_apply_is_one_f32_add_over_the_targets_alone(dev, rows_list, X):
    jobs, p, E, d, total = case(rows_list, X)
    n = sum(rows_list) * X
    want_p, want_s = R.apply_ref(p, jobs, d, X), R.stats_f64(p, jobs, d, X)
    assert (want_p == SENT).sum() == (p == SENT).sum() > 0
    dry = Apply(dev, jobs, p, d, X, apply=0)
    dry.p.check(T(p), f"{rows_list} x {X}: p after a dry run")
    wet = Apply(dev, jobs, p, d, X, apply=1)
    wet.p.check(T(want_p), f"{rows_list} x {X}: p after the add")
    assert wet.s == dry.s
    check_stats(wet.s, want_s, n)
    rev = Apply(dev, jobs[::-1], p, d, X, apply=1)
    rev.p.check(T(want_p), f"{rows_list} x {X}: p after the add, the table reversed")
    check_stats(rev.s, want_s, n)


def test_apply_sums_on_small_integers_are_exact(dev):
    X = 68
    jobs, n, total = layout([33, 64, 7], X)
    g = np.random.default_rng(4)
    p = np.full(n, SENT, f32)
    for w, _, rows in jobs:
        p[w:w + rows * X] = g.integers(-8, 9, rows * X).astype(f32)
    d = g.integers(-16, 17, total * X).astype(f32)
    a = Apply(dev, jobs, p, d, X)
    want = R.stats_f64(p, jobs, d, X)
    assert a.s == {k: float(v) for k, v in want.items()}, (a.s, want)
    a.p.check(T(R.apply_ref(p, jobs, d, X)), "integers: p after the add")


def test_apply_refusals_write_nothing(dev):
    from siss_amd import lib
    X = 64
    jobs, p, E, d, total = case([33, 16], X)
    words = lib.query("siss_uce_partials_words", total * X, 2)
    pb, db = Flat(len(p), F32, dev, body=p), Flat(total * X + 8, F32, dev, body=np.r_[d, d[:8]])
    pt, st = Flat(words + 2, F64, dev, fill=-5.0), Flat(6, F64, dev, fill=-5.0)
    ok = lambda **k: dict(dict(p=pb.t, jobs=jobs, X=X, delta=db.t[:total * X], pt=pt.t, st=st.t), **k)
    n_t = jobs[1][0] + jobs[1][2] * X
    rows = [ok(X=66), ok(X=-4), ok(jobs=[]), ok(jobs=[(0, 0, 0)]), ok(jobs=[jobs[0], (jobs[1][0], 33, -2)]), ok(jobs=[(6, 0, 33)]),
            ok(jobs=[jobs[0], (jobs[1][0], 32, 16)]), ok(p=pb.t[3:]), ok(delta=db.t[1:total * X + 1]), ok(delta=pb.t), ok(delta=pb.t[n_t - 4:])]
    for a in rows:
        refused("siss_uce_apply", a["p"], table(a["jobs"]) if a["jobs"] else table([(0, 0, 1)]), len(a["jobs"]), a["X"], a["delta"], 1, a["pt"], a["st"])
    pb.check(T(p), "p after the refusals")
    db.check(db.host.clone(), "delta after the refusals")
    pt.check(pt.host.clone(), "the partial rows after the refusals")
    st.check(st.host.clone(), "the statistics after the refusals")


# ================================================================ 3. the tiny engines
XDIM, LTOK = 64, 13


def rows_of(seed=7):
    """(C_e, C_t, C_p): one prompt of 13 rows each way, two preserved prompts (39 rows < X)"""
    g = torch.Generator().manual_seed(seed)
    e = lambda k: torch.randn(k, LTOK, XDIM, generator=g).double().reshape(-1, XDIM)
    return e(1), e(1), e(2)


def the_edit(lam=0.1):
    from siss_amd import uce
    return uce.edit_matrix(*rows_of(), lam)


def target_names(eng):
    from siss_amd import uce
    names = uce.select_targets(list(eng.ps.specs), uce.parse_uce(dict(edit=[dict(prompt="a")])).targets)
    assert len(names) >= 4 and all(n.endswith(("attn2.to_k.weight", "attn2.to_v.weight")) for n in names)
    assert len({eng.ps.specs[n].native_shape[0] for n in names}) >= 2, "the tiny UNet should have targets of two widths"
    return names


def restated(eng, p0, names, E):
    """the restatement's flat buffer after the edit, its jobs and compact delta"""
    jobs, row = [], 0
    for n in names:
        sp = eng.ps.specs[n]
        jobs.append((sp.off, row, sp.native_shape[0]))
        row += sp.native_shape[0]
    d = R.compact(R.delta_ref(p0, jobs, E), jobs, XDIM, row, 0.0)
    return R.apply_ref(p0, jobs, d, XDIM), jobs, d


def cond_pass(eng, st, dev):
    """One forward and one backward of a fixed micro-batch at the engine's weights: (prediction, gradient set 0)."""
    from siss_amd.variants import backward_batch, quiet_backward
    from test_hip_teacher import embeddings
    seen, inner = [], eng.forward

    def spy(*a, **k):
        seen.append(inner(*a, **k))
        return seen[-1]
    eng.forward = spy
    try:
        with quiet_backward(st, "test"):
            x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(33))
            backward_batch(st, x, 1, first=True, conditioning={"encoder_hidden_states": embeddings(dev)["prompt"].repeat(2, 1, 1)},
                           generator=torch.Generator(device=dev).manual_seed(8))
            g = eng.ps.grads[0].clone()
    finally:
        del eng.forward
    torch.cuda.synchronize()
    return seen[0].clone(), g


def test_bf16_engine_after_the_edit_has_no_stale_copy(dev):
    from siss_amd import uce
    from test_hip_teacher import stepper
    eng, st = stepper(dev)
    names, ed = target_names(eng), the_edit()
    pred0, g0 = cond_pass(eng, st, dev)
    p0 = eng.ps.flat.detach().cpu().numpy().copy()
    with pytest.raises(ValueError, match="not a matrix"):
        uce.apply(eng, ed, names + [next(n for n in eng.ps.specs if n.endswith("attn1.to_k.weight") and eng.ps.specs[n].native_shape[1] != XDIM)])
    with pytest.raises(ValueError, match="not a matrix"):
        uce.apply(eng, ed, ["conv_in.weight"])
    dry = uce.apply(eng, ed, names, apply=False)
    assert torch.equal(bits(eng.ps.flat.cpu()), bits(T(p0)))
    stats = uce.apply(eng, ed, names)
    torch.cuda.synchronize()
    want, jobs, d = restated(eng, p0, names, ed.E)
    same(eng.ps.flat.cpu(), T(want), "the engine's parameters after the edit against the restatement's")
    inside = np.zeros(len(p0), bool)
    for w, _, rows in jobs:
        inside[w:w + rows * XDIM] = True
    assert np.array_equal(want.view(np.uint32)[~inside], p0.view(np.uint32)[~inside]) and (want[inside] != p0[inside]).mean() > 0.9
    same(eng.ps.shadow.cpu(), eng.ps.flat.to(torch.bfloat16).cpu(), "the bf16 shadow after the edit")
    ws = R.stats_f64(p0, jobs, d, XDIM)
    assert stats == dry and stats["floats"] == ws["floats"] == int(inside.sum()) and stats["max_delta"] == ws["max_delta"]
    for k in ("sum_delta2", "sum_p2"):
        assert abs(stats[k] - ws[k]) <= ws["floats"] * 2.0 ** -53 * ws[k]
    assert stats["relative_change"] == np.sqrt(stats["sum_delta2"] / stats["sum_p2"]) > 0
    pred1, g1 = cond_pass(eng, st, dev)
    assert not torch.equal(pred1, pred0) and not torch.equal(g1, g0), "the edit did not reach the forward / backward pass"
    fresh, st2 = stepper(dev)
    fresh.load_state_dict({n: t.clone() for n, t in eng.state_dict().items()})
    same(fresh.ps.flat.cpu(), eng.ps.flat.cpu(), "a fresh engine loaded with the edited state dict")
    pred2, g2 = cond_pass(fresh, st2, dev)
    same(pred1.cpu(), pred2.cpu(), "the forward output against a fresh engine's")
    same(g1.cpu(), g2.cpu(), "the gradient set against a fresh engine's")


def test_f32_engine_after_the_edit_matches_the_oracle_with_the_restatements_weights(dev):
    from siss_amd import uce
    from test_hip_f32_mode import RTOL
    from test_hip_lora_conv import f32_pair
    eng, net, sd, ch, xdim = f32_pair("cond", seed=5)
    assert xdim == XDIM
    names, ed = target_names(eng), the_edit()
    Ce, Ct, Cp = rows_of()
    p0 = eng.ps.flat.detach().cpu().numpy().copy()
    before = uce.values_before(eng, names, Ct, Cp)
    g = torch.Generator().manual_seed(3)
    x, t, ctx = torch.randn(2, ch, 16, 16, generator=g), torch.tensor([999, 40]), torch.randn(2, LTOK, XDIM, generator=g)
    pred0 = eng.forward(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).cpu()
    stats = uce.apply(eng, ed, names)
    torch.cuda.synchronize()
    want, jobs, d = restated(eng, p0, names, ed.E)
    same(eng.ps.flat.cpu(), T(want), "the f32 engine's parameters after the edit against the restatement's")
    assert eng.ps.shadow.data_ptr() == eng.ps.flat.data_ptr() and stats["floats"] == sum(r for _, _, r in jobs) * XDIM
    # the oracle in f64 with the restatement's weights
    after = {n: (T(want[eng.ps.specs[n].off:eng.ps.specs[n].off + eng.ps.specs[n].numel].copy()).view(sd[n].shape) if n in names else sd[n])
             for n in sd}
    net.load_state_dict({k: v.double() for k, v in after.items()})
    with torch.no_grad():
        ref = net(x.double(), t, ctx.double())[0]
    pred = eng.forward(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).cpu()
    perr = float((pred.double() - ref).abs().max() / ref.abs().max())
    moved = float((pred - pred0).abs().max() / ref.abs().max())
    print(f"\n[uce] f32 engine vs f64 oracle after the edit: pred rel err {perr:.2e}; the edit moved the prediction by {moved:.2e} of its max")
    assert perr <= RTOL, perr
    assert moved > 10 * RTOL, "the edit moves the prediction too little for the bound to tell it from no edit"
    # residuals: f64 on both sides over the same bits
    res = uce.residuals(eng, names, before, Ce, Cp)
    W0 = [p0[w:w + rows * XDIM].reshape(rows, XDIM) for w, _, rows in jobs]
    W1 = [want[w:w + rows * XDIM].reshape(rows, XDIM) for w, _, rows in jobs]
    e_ref, p_ref = R.residuals(W1, W0, Ce.numpy(), Ct.numpy(), Cp.numpy())
    assert abs(res["edit_residual"] - e_ref) <= 1e-6 and abs(res["preserve_drift"] - p_ref) <= 1e-6, (res, e_ref, p_ref)
    for (w, _, rows), n, a, b in zip(jobs, names, W1, W0):
        e1, p1 = R.residuals([a], [b], Ce.numpy(), Ct.numpy(), Cp.numpy())
        assert abs(res["per_tensor"][n]["edit_residual"] - e1) <= 1e-6 and abs(res["per_tensor"][n]["preserve_drift"] - p1) <= 1e-6
    e0, _ = R.residuals(W0, W0, Ce.numpy(), Ct.numpy(), Cp.numpy())
    assert 0 < res["edit_residual"] < e0 and 0 < res["preserve_drift"] < 1


# ================================================================ 4. the files and a second rank
SD = ["--config-name=delete_sd", "pretrained_model_name_or_path=/nonexistent",
      "+unet={sample_size:16,in_channels:4,out_channels:4,block_out_channels:[64,128],down_block_types:[CrossAttnDownBlock2D,DownBlock2D],"
      "up_block_types:[UpBlock2D,CrossAttnUpBlock2D],attention_head_dim:2,cross_attention_dim:64}"]
KEY = "+deletion.uce={edit:[{prompt:a photo of a thing,target:null},{prompt:another thing,target:a plain thing}],preserve:[a dog,a tree]}"


def sd_task(tmp_path, *extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_sd", os.path.join(ROOT, "config"), [*SD[1:], f"output_dir={tmp_path}/out", "allow_synthetic=true", "allow_random_init=true", *extra])
    return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)


def test_files_round_trip_on_the_device_and_a_foreign_x_is_refused(dev, tmp_path):
    from siss_amd import uce
    from test_hip_teacher import stepper
    ed = the_edit()
    eng, st = stepper(dev)
    names = target_names(eng)
    uce.save(str(tmp_path), ed)
    back = uce.load(str(tmp_path), XDIM)
    assert np.array_equal(back.E.view(np.uint32), ed.E.view(np.uint32))
    a = uce.apply(eng, ed, names, apply=False)
    assert uce.apply(eng, back, names, apply=False) == a
    with pytest.raises(ValueError, match="X = 64, this UNet's cross_attention_dim is 768"):
        uce.load(str(tmp_path), 768)


def test_a_second_rank_receives_e_applies_it_and_matches_rank_0s_bits(dev, tmp_path, monkeypatch):
    """DeleteSD.uce_edit as rank 1 of 2 over a stand-in for torch.distributed that plays rank 0: the description first, then E, then the
    bits of rank 0's sum of delta^2; rank 1 embeds nothing, builds nothing, writes nothing, and ends on rank 0's parameters bit for bit."""
    import torch.distributed as dist
    from siss_amd import uce
    from test_hip_teacher import stepper
    task = sd_task(tmp_path, KEY)
    eng0, st0 = stepper(dev)
    names, ed0 = target_names(eng0), the_edit()
    want = uce.apply(eng0, ed0, names)
    word_bits = struct.unpack("<Q", struct.pack("<d", want["sum_delta2"]))[0]
    words, calls = [ed0.config(), word_bits], []

    def objects(word, src, group):
        assert word == [None] and src == 0 and group == "group"
        word[0] = words[calls.count("objects")]
        calls.append("objects")

    def tensor(t, src, group):
        assert t.shape == (XDIM, XDIM) and t.dtype == torch.float32 and int(t.count_nonzero()) == 0
        t.copy_(torch.from_numpy(ed0.E))
        calls.append("E")
    monkeypatch.setattr(dist, "broadcast_object_list", objects)
    monkeypatch.setattr(dist, "broadcast", tensor)
    monkeypatch.setattr(uce, "edit_matrix", lambda *a, **k: pytest.fail("a rank other than 0 built the edit"))
    monkeypatch.setattr(type(task), "_prompt_embedding", lambda *a, **k: pytest.fail("a rank other than 0 embedded a prompt"))
    eng1, st1 = stepper(dev)
    fields = task.uce_edit(st1, dev, 1, 2, "group")
    torch.cuda.synchronize()
    assert calls == ["objects", "E", "objects"]
    assert fields == dict(uce_edits=2, uce_preserved=2, uce_lambda=0.1, uce_relative_change=want["relative_change"]) and want["relative_change"] > 0
    same(eng1.ps.flat.cpu(), eng0.ps.flat.cpu(), "rank 1's parameters against rank 0's")
    same(eng1.ps.shadow.cpu(), eng0.ps.shadow.cpu(), "rank 1's shadow against rank 0's")
    assert not os.path.exists(tmp_path / "out"), "a rank other than 0 wrote files"
    # a rank whose sum differs from rank 0's says so
    calls.clear()
    words[1] = word_bits + 1
    _, st2 = stepper(dev)
    with pytest.raises(RuntimeError, match="rank 1's sum of delta\\^2 has the bits"):
        task.uce_edit(st2, dev, 1, 2, "group")


# ================================================================ 5. the task
ZERO = ("training_steps=0", "lr_scheduler=constant")
FIELDS = ("uce_edits", "uce_preserved", "uce_lambda", "uce_relative_change")


def new_entry_points(calls):
    return [n for n in calls if "uce" in n]


def run_sd(tmp_path, name, *extra, step0=None):
    """test_hip_ssd's delete_sd run with a hook that records the weights the step-0 metrics see"""
    from siss_amd import tasks
    from test_hip_ssd import run_task
    orig = tasks.DeleteSD.metric_hooks

    def hooks(self, unet, *a, **k):
        if step0 is not None:
            yield (10 ** 9, lambda step: step0.append((step, unet.engine.ps.flat.detach().cpu().numpy().copy())))
        yield from orig(self, unet, *a, **k)
    tasks.DeleteSD.metric_hooks = hooks
    try:
        return run_task(tmp_path, "delete_sd", name, *extra)
    finally:
        tasks.DeleteSD.metric_hooks = orig


def test_task_edits_without_a_step_and_reloads_its_edit(dev, tmp_path, capsys):
    from safetensors.torch import load_file
    from siss_amd.uce import CONFIG_FILE, EDIT_FILE
    from test_hip_ssd import load_flat, logged
    seen = []
    rundir, lines = run_sd(tmp_path, "keyed", *ZERO, KEY, step0=seen)
    assert lines == [] and os.path.isdir(os.path.join(rundir, "unet"))
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    t = load_file(os.path.join(rundir, EDIT_FILE))
    assert set(t) == {"E", "M", "D"} and t["E"].dtype == torch.float32 and t["M"].dtype == t["D"].dtype == torch.float64
    assert all(v.shape == (XDIM, XDIM) for v in t.values())
    assert (c["X"], c["edit_rows"], c["preserve_rows"], c["lambda"], c["source"]) == (XDIM, 2 * 77, 2 * 77, 0.1, "computed")
    assert c["config"]["edit"] == [{"prompt": "a photo of a thing", "target": None}, {"prompt": "another thing", "target": "a plain thing"}]
    assert c["edit_prompts"] == ["a photo of a thing", "another thing"] and c["edit_targets"] == [None, "a plain thing"]
    assert c["preserved_prompts"] == ["a dog", "a tree"] and c["cond"] > 1 and len(c["embeddings"]) == 64
    st, res = c["stats"], c["residuals"]
    assert st["relative_change"] > 0 and st["floats"] > 0 and st["max_delta"] > 0
    assert set(res["per_tensor"]) == set(c["targets"]) and 0 < res["edit_residual"] and 0 < res["preserve_drift"]
    out = capsys.readouterr().out
    assert out.count("[siss_amd] deletion.uce:") == 1
    print(f"[uce] delete_sd: cond(M) {c['cond']:.4g}, {st}, edit residual {res['edit_residual']:.4g}, preserve drift {res['preserve_drift']:.4g}")
    # the saved unet/ is, bit for bit, the restatement's edit of the weights a run without the key saves untouched -- a run that calls
    # no new entry point; the step-0 metrics saw the edited weights
    (plain_dir, _), calls = logged(run_sd, tmp_path, "plain", *ZERO)
    assert calls and not new_entry_points(calls), "a run without the key reached csrc/uce.hip"
    assert not os.path.exists(os.path.join(plain_dir, CONFIG_FILE)) and not os.path.exists(os.path.join(plain_dir, EDIT_FILE))
    p0, p1 = load_flat("delete_sd", plain_dir), load_flat("delete_sd", rundir)
    from siss_amd.model import UNet2DConditionModel
    eng = UNet2DConditionModel.from_pretrained(plain_dir, subfolder="unet", device="cuda:0", compute_dtype=torch.bfloat16).engine
    assert c["targets"] == target_names(eng)
    want, jobs, d = restated(eng, p0, c["targets"], t["E"].numpy())
    same(T(p1), T(want), "the saved unet/ against the restatement's edited buffer")
    assert not np.array_equal(want, p0) and st["floats"] == sum(r for _, _, r in jobs) * XDIM
    assert len(seen) == 1 and seen[0][0] == 0
    same(T(seen[0][1]), T(want), "the weights the step-0 metric hook saw")
    # a second run that loads the first run's edit
    rundir2, _ = run_sd(tmp_path, "reloaded", *ZERO, KEY[:-1] + ",path:'%s'}" % rundir)
    c2 = json.load(open(os.path.join(rundir2, CONFIG_FILE)))
    t2 = load_file(os.path.join(rundir2, EDIT_FILE))
    assert c2["source"] == "loaded" and all(torch.equal(t2[k].view(torch.uint8), t[k].view(torch.uint8)) for k in t)
    assert c2["stats"] == c["stats"] and c2["residuals"] == c["residuals"] and c2["embeddings"] == c["embeddings"]
    same(T(load_flat("delete_sd", rundir2)), T(want), "the reloaded run's unet/")


def test_task_loop_follows_from_the_edited_weights(dev, tmp_path):
    from siss_amd.uce import CONFIG_FILE
    from test_hip_ssd import logged
    rundir, lines = run_sd(tmp_path, "keyed2", "training_steps=2", KEY)
    c = json.load(open(os.path.join(rundir, CONFIG_FILE)))
    assert len(lines) == 2 and os.path.isdir(os.path.join(rundir, "unet"))
    for st in lines:
        assert all(k in st for k in FIELDS), sorted(st)
        assert (st["uce_edits"], st["uce_preserved"], st["uce_lambda"]) == (2, 2, 0.1)
        assert st["uce_relative_change"] == c["stats"]["relative_change"] > 0
    (_, plain), calls = logged(run_sd, tmp_path, "plain2", "training_steps=2")
    assert len(calls) > 100 and calls.count("siss_recombine_clip_adamw") == 2 and not new_entry_points(calls), \
        "a run without the key reached csrc/uce.hip"
    assert len(plain) == 2 and not [k for l in plain for k in l if k.startswith("uce")]
    assert plain[0]["norm_loss_x"] != lines[0]["norm_loss_x"], "the first step did not start from the edited weights"

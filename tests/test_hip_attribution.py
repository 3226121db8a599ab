"""csrc/attribution.hip and what stands on it (siss_amd/attribution.py, tools/attribute.py), on the GPU.

The kernel, against tests/attribution_ref.py (every output sits inside a NaN-poisoned buffer and the workspace between guards, checked
after every launch):
* exact on integers: g uniform in [-A, A] with A * chunk < 2^24, n in {1027, chunk + 5, 4,197,379} x k in {32, 96, 2048}: the output
  equals (float32)(float64(integer sum) / sqrt(k)) bit for bit (the long buffer's sums are formed by the torch restatement on the
  device, which is held against the numpy one first);
* real data: normals times per-tensor scales 1e-6 .. 1e2 against f64 within the derived bound of attribution_ref.error_bound;
* unit vectors give the rows of the host matrix; a second seed gives other rows;
* a three-stretch table equals the full projection of the gradient zeroed outside, with NaN planted outside the stretches;
* two runs agree bit for bit (there is no grid override: the grid is a function of (n, k)); bad arguments are refused with nothing
  written.
The module: GradientFeatures.row launch for launch on the tiny f32 engine (the backward pass of the f32 engine is not bitwise repeatable
-- csrc/f32_path.hip sums GroupNorm's column sums atomically -- so the row is held bit for bit against a projection by hand of the
gradient its own launches left, and two backward passes against each other within the bound tests/test_hip_ewc.py uses); row
independence on the bf16 engines, plain and SD-shaped (to that bound too: their backward passes sum bias, GroupNorm-parameter and split
weight gradients with f32 atomics, and two passes over the same batch differ in the last bits); Attributor.scores / topk against f64;
tools/attribute.py end to end.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import attribution_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
GUARD = 64                       # floats / doubles on either side
BIG = 4_197_379


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import attribution, lib
    lib.load()
    attribution.require_kernels()
    return torch.device("cuda:0")


def chunk():
    from siss_amd import lib
    return int(lib.query("siss_jl_chunk"))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Launch:
    """One siss_jl_project call on a device gradient: `out` inside a NaN-poisoned buffer, the workspace between guards; .run() returns
    the k floats and checks that nothing else was written."""

    def __init__(self, dev, g, k, seed=0, table=None):
        from siss_amd import lib
        self.g, self.k, self.seed, self.n = g, k, seed, g.numel()
        self.ws_bytes = int(lib.query("siss_jl_ws_bytes", self.n, k))
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.frame = torch.full((2 * GUARD + k,), float("nan"), device=dev)
        self.wsframe = torch.full((2 * GUARD + self.ws_bytes // 8,), -5.0, dtype=torch.float64, device=dev)
        self.table = None if table is None else torch.from_numpy(table).to(dev)
        self.nr = 0 if table is None else (len(table) - 1) // 2

    @property
    def out(self):
        return self.frame[GUARD:GUARD + self.k]

    @property
    def ws(self):
        return self.wsframe[GUARD:GUARD + self.ws_bytes // 8]

    def args(self, **over):
        a = dict(g=self.g, n=self.n, table=self.table, n_ranges=self.nr, k=self.k, seed=self.seed, ws=self.ws, ws_bytes=self.ws_bytes,
                 out=self.out)
        a.update(over)
        return tuple(a.values())

    def untouched(self):
        fr, ws = self.frame.cpu(), self.wsframe.cpu()
        assert bool(torch.isnan(fr[:GUARD]).all()) and bool(torch.isnan(fr[GUARD + self.k:]).all()), "written around out[0:k]"
        assert bool((ws[:GUARD] == -5.0).all()) and bool((ws[-GUARD:] == -5.0).all()), "written around the workspace"

    def run(self):
        from siss_amd import lib
        before = self.g.clone()
        lib.call("siss_jl_project", *self.args())
        torch.cuda.synchronize()
        self.untouched()
        assert torch.equal(before.view(torch.int32), self.g.view(torch.int32)), "the gradient was written"
        out = self.out.cpu().numpy().copy()
        assert not np.isnan(out).any() or bool(torch.isnan(self.g).any())
        return out

    def refused(self, **over):
        from siss_amd import lib
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call("siss_jl_project", *self.args(**over))
        torch.cuda.synchronize()
        self.untouched()
        assert bool(torch.isnan(self.frame).all()) and bool((self.wsframe == -5.0).all()), "a refused call wrote something"


_INTS = {}


def ints(n, dev):
    """Uniform integers in [-1000, 1000] (1000 * chunk < 2^24), as f32 on the device; computed once and shared, never written."""
    if n not in _INTS:
        g = torch.randint(-1000, 1001, (n,), generator=torch.Generator().manual_seed(n % 9973), dtype=torch.int64)
        _INTS[n] = g.to(torch.float32).to(dev)
    return _INTS[n]


_SUMS = {}


def int_sums(n, k, seed, dev):
    """The exact column sums of ints(n): numpy for the short buffers, the torch restatement on the device for the long one."""
    key = (n, k, seed)
    if key not in _SUMS:
        g = ints(n, dev)
        if n <= 1 << 16:
            _SUMS[key] = R._blocks(seed, g.cpu().numpy().astype(np.int64), k, np.int64).astype(f64)
        else:
            _SUMS[key] = R.sums_torch(seed, g, k)
    return _SUMS[key]


# ================================================================ 1. exact on integers
def test_torch_restatement_is_the_numpy_restatement(dev):
    for i0 in (0, BIG - 100, 860_000_000, (1 << 32) - 40):
        assert np.array_equal(R.signs_torch(7, i0, 100, 96, dev).cpu().numpy(), R.signs(7, i0, 100, 96).astype(f64)), i0
    g = ints(1027, dev)
    assert np.array_equal(R.sums_torch(3, g, 96), R._blocks(3, g.cpu().numpy().astype(np.int64), 96, np.int64).astype(f64))


@pytest.mark.parametrize("k", [32, 96, 2048])
@pytest.mark.parametrize("n", ["1027", "chunk+5", str(BIG)])
def test_integers_are_projected_exactly(dev, n, k):
    c = chunk()
    assert 1000 * c < 2 ** 24
    n = c + 5 if n == "chunk+5" else int(n)
    seed = 12345
    want = (int_sums(n, k, seed, dev) / np.sqrt(f64(k))).astype(f32)
    got = Launch(dev, ints(n, dev), k, seed).run()
    assert np.abs(want).max() > 0
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"n {n} k {k}: {bad.size} columns differ, first {bad[:4]}: {got[bad[:4]]} against {want[bad[:4]]}"


# ================================================================ 2. real data
@pytest.mark.parametrize("n,k", [(2 * 1024 + 5, 2048), (70_001, 96), (BIG, 32)])
def test_real_data_lies_within_the_derived_bound(dev, n, k):
    c = chunk()
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen, dtype=torch.float32)
    edges = np.linspace(0, n, 10).astype(np.int64)                 # nine "tensors", scales 1e-6 .. 1e2
    for t, s in enumerate(np.logspace(-6, 2, 9)):
        g[edges[t]:edges[t + 1]] *= float(s)
    gd = g.to(dev)
    exact = R.sums_torch(5, gd, k)                                 # f64 sums of the f32 values
    sum_abs = float(gd.double().abs().sum())
    got = Launch(dev, gd, k, 5).run().astype(f64)
    err = np.abs(got - exact / np.sqrt(k))
    bound = R.error_bound(sum_abs, exact, k, c)
    print(f"[attribution] n {n} k {k}: max |err| / bound {np.max(err / bound):.3e}, max |err| {err.max():.3e}, |out| up to {np.abs(got).max():.3e}")
    assert np.all(err <= bound)


# ================================================================ 3. unit vectors
def test_unit_vectors_give_the_rows_of_the_host_matrix(dev):
    c, k = chunk(), 96
    n = c + 5
    rows = R.signs(0, 0, n, k)
    other = R.signs(1, 0, n, k)
    for i in (0, 31, 32, n - 1, c - 1, c):
        g = torch.zeros(n, device=dev)
        g[i] = 1.0
        got = Launch(dev, g, k, 0).run()
        want = (rows[i].astype(f64) / np.sqrt(f64(k))).astype(f32)
        assert np.array_equal(bits(got), bits(want)), f"e_{i}"
        assert np.array_equal(np.rint(got.astype(f64) * np.sqrt(k)).astype(np.int8), rows[i])
        second = Launch(dev, g, k, 1).run()
        assert np.array_equal(bits(second), bits((other[i].astype(f64) / np.sqrt(f64(k))).astype(f32))) and not np.array_equal(second, got)


# ================================================================ 4. ranges
@pytest.mark.parametrize("k", [32, 2048])
def test_a_table_is_the_full_projection_of_the_gradient_zeroed_outside(dev, k):
    c = chunk()
    n = 4 * c + 3
    stretches = [(8, 12), (c - 100, c + 100), (3 * c + 16, 4 * c)]
    keep = R.keep_of(n, stretches)
    g = ints(n, dev).clone()
    zeroed = torch.where(torch.from_numpy(keep).to(dev), g, torch.zeros_like(g))
    g[torch.from_numpy(~keep).to(dev)] = float("nan")
    full = Launch(dev, zeroed, k, 9).run()
    sub = Launch(dev, g, k, 9, table=R.table_of(stretches)).run()
    assert not np.isnan(sub).any(), "a NaN outside the stretches reached the output"
    assert np.array_equal(bits(sub), bits(full))
    want = R.project_int(9, zeroed.cpu().numpy(), k)
    assert np.array_equal(bits(sub), bits(want)) and np.abs(want).max() > 0
    # real numbers too: the same bits as the zeroed buffer's, whatever the rounding
    r = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev)
    rz = torch.where(torch.from_numpy(keep).to(dev), r, torch.zeros_like(r))
    assert np.array_equal(bits(Launch(dev, r, k, 9, table=R.table_of(stretches)).run()), bits(Launch(dev, rz, k, 9).run()))


# ================================================================ 5. isolation
def test_two_runs_agree_and_bad_arguments_are_refused(dev):
    from siss_amd import lib
    c = chunk()
    n, k = 70_001, 96
    g = torch.randn(n + 4, generator=torch.Generator().manual_seed(2)).to(dev)
    a, b = Launch(dev, g[:n], k, 4).run(), Launch(dev, g[:n], k, 4).run()
    assert np.array_equal(bits(a), bits(b)), "a second run differs: not bitwise repeatable"
    assert int(lib.query("siss_jl_ws_bytes", n, 48)) == 0 and int(lib.query("siss_jl_ws_bytes", 0, 64)) == 0
    L = Launch(dev, g[:n], k, 4)
    L.refused(g=g[1:n + 1])                                               # a gradient off the 16-byte rule
    L.refused(out=L.frame[GUARD + 1:GUARD + 1 + k])
    L.refused(ws=L.wsframe[GUARD:].view(torch.uint8)[4:])                  # a workspace off the 8-byte rule
    for bad_k in (16, 48, 100, 8192 + 32, 0):
        L.refused(k=bad_k)
    L.refused(ws_bytes=L.ws_bytes - 8)                                    # a short workspace
    L.refused(seed=-1)
    L.refused(seed=1 << 32)
    L.refused(n=0)
    L.refused(n=(1 << 40) + 1)
    L.refused(n_ranges=2)                                                 # ranges without a table
    tab = torch.from_numpy(R.table_of([(0, 8)])).to(dev)
    L.refused(table=tab, n_ranges=0)
    L.refused(g=None)
    L.refused(out=None)
    L.refused(ws=None)


# ================================================================ 6. GradientFeatures.row
class CallLog:
    """lib.call replaced by a spy that notes every entry point's name and, at siss_jl_project, keeps a copy of the gradient it reads."""

    def __enter__(self):
        from siss_amd import lib
        self.lib, self.orig, self.names, self.grads = lib, lib.call, [], []

        def spy(name, *a, **k):
            self.names.append(name)
            if name == "siss_jl_project":
                self.grads.append(a[0].clone())
            return self.orig(name, *a, **k)
        lib.call = spy
        return self

    def __exit__(self, *exc):
        self.lib.call = self.orig
        return False


def image(i, c=3):
    return torch.rand(c, 16, 16, generator=torch.Generator().manual_seed(500 + i)) * 2 - 1


def by_hand(st, proj, img, index, seed, S, output, batch_size, out):
    """The launch sequence the issue states, written out: mixture_fwd -> forward -> mse_bwd_seed(pred, noise or zeros, 1 / S) ->
    backward(nsets = 1) per micro-batch, then the projection of gradient set 0."""
    from siss_amd.attribution import row_seed, timestep_table
    from siss_amd.loss import mixture_fwd, mse_bwd_seed
    from siss_amd.variants import quiet_backward
    e, dev = st.e, st.e.device
    with quiet_backward(st, "by hand"):
        gen = torch.Generator(device=dev).manual_seed(row_seed(seed, index))
        a0 = img[None].to(dev).to(st.io_dtype).expand(S, *img.shape).contiguous()
        noise = torch.randn(a0.shape, device=dev, generator=gen).to(st.io_dtype).contiguous()
        t = torch.tensor(timestep_table(S, int(st.ac.numel())), device=dev, dtype=torch.int64)
        for b0 in range(0, S, batch_size):
            sl = slice(b0, b0 + batch_size)
            e.wgrad_overwrite = b0 == 0 and st.wgrad_overwrite
            if b0 == 0:
                e.zero_grad()
            m = mixture_fwd(a0[sl].contiguous(), a0[sl].contiguous(), noise[sl].contiguous(), t[sl].contiguous(),
                            torch.zeros(batch_size, device=dev), st.ac, st.gamma_tab, st.sigma_tab, 0.5)
            pred = e.forward(m.x_mix, t[sl].contiguous())
            target = noise[sl].contiguous() if output == "loss" else torch.zeros_like(noise[sl]).contiguous()
            cot, _, _ = mse_bwd_seed(pred, target, 1.0 / S)
            e.backward(cot, nsets=1)
        proj.project(e.ps.grads[0], out)
    return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_row_issues_the_stated_launches_and_projects_the_gradient_they_leave(dev):
    from siss_amd.attribution import GradientFeatures, Projector
    from test_hip_ewc import batch, state_of, stepper
    eng, st = stepper(dtype=torch.float32)
    st.step(*batch(0, dev))                                  # a warm state: non-zero moments, a recorded fill plan
    total, k, S, seed, index = int(eng.ps.total), 96, 4, 3, 5
    proj = Projector(total, k, seed=11, device=dev)
    img = image(0)
    # (the first forward after an optimizer step rebuilds the operand copies of the stepped weights, once: not part of a row's sequence)
    GradientFeatures(st, proj, timesteps=S, seed=seed).row(img, index, torch.zeros(k, device=dev))
    before = state_of(eng, st)
    got, grads, logs = {}, {}, {}
    for output in ("loss", "square"):
        for bs in (None, 2):
            feats = GradientFeatures(st, proj, timesteps=S, output=output, batch_size=bs, seed=seed)
            out = torch.full((k,), float("nan"), device=dev)
            with CallLog() as log:
                feats.row(img, index, out)
            torch.cuda.synchronize()
            assert log.names.count("siss_jl_project") == 1 and log.names[-1] == "siss_jl_project"
            g = log.grads[0]
            assert float(g.abs().max()) > 0
            # bit for bit: the row IS the projection of the gradient its launches left in gradient set 0
            hand = torch.zeros(k, device=dev)
            Projector(total, k, seed=11, device=dev).project(g, hand)
            assert torch.equal(out.view(torch.int32), hand.view(torch.int32)), (output, bs)
            want = R.sums_torch(11, g, k) / np.sqrt(k)
            assert np.all(np.abs(out.cpu().numpy().astype(f64) - want) <= R.error_bound(float(g.double().abs().sum()), want * np.sqrt(k), k, chunk()))
            # launch for launch: the sequence written out issues the same entry points in the same order
            out2 = torch.zeros(k, device=dev)
            with CallLog() as log2:
                by_hand(st, proj, img, index, seed, S, output, bs or S, out2)
            assert log2.names == log.names, (output, bs, log.names, log2.names)
            d = rel(log2.grads[0], g)
            print(f"[attribution] {output}, micro-batches of {bs or S}: |g_hand - g_row| / |g_row| = {d:.3e} (a second f32 backward pass)")
            assert d < 1e-4
            got[output, bs], grads[output, bs], logs[output, bs] = out.clone(), g, log.names
            assert int(eng.ps.grads.count_nonzero()) == 0 and eng.ps.grads.is_contiguous(), "the gradient buffers are not zero on return"
            assert eng.ps.grads[0].data_ptr() == eng.ps.grads.data_ptr() and st._micro == 0 and eng.wgrad_overwrite is False
    for output in ("loss", "square"):
        d = rel(grads[output, 2], grads[output, None])
        print(f"[attribution] {output}: two micro-batches of 2 against one batch of 4: {d:.3e}")
        assert d < 1e-4
        assert logs[output, 2].count("siss_mse_bwd_seed") == 2 and logs[output, None].count("siss_mse_bwd_seed") == 1
    assert rel(grads["square", None], grads["loss", None]) > 1e-2, "the square output is the loss output"
    for key, t in state_of(eng, st).items():
        assert torch.equal(t.view(torch.uint8), before[key].view(torch.uint8)), f"row changed {key}"
    feats = GradientFeatures(st, proj, timesteps=S, seed=seed)
    st._micro = 1
    try:
        with pytest.raises(RuntimeError, match="middle of an accumulation"):
            feats.row(img, index, torch.zeros(k, device=dev))
    finally:
        st._micro = 0
    with pytest.raises(ValueError, match="this UNet's has"):
        GradientFeatures(st, Projector(total + 64, k, device=dev))
    with pytest.raises(ValueError, match="output = 'mse'"):
        GradientFeatures(st, proj, output="mse")


# ================================================================ 7. row independence
class Images:
    def __init__(self, n, c):
        self.items = [image(i, c) for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.parametrize("kind", ["plain", "cond"])
def test_a_row_does_not_depend_on_order_or_company(dev, kind):
    from siss_amd.attribution import FeatureStore, GradientFeatures, Projector
    from test_hip_trainable_step import stepper
    eng, st = stepper(kind, None)
    k, S = 64, 4
    ds = Images(6, 3 if kind == "plain" else 4)
    ehs = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(8)).to(dev)
    cond = None if kind == "plain" else (lambda B: {"encoder_hidden_states": ehs.repeat(B, 1, 1)})
    proj = Projector(int(eng.ps.total), k, seed=2, device=dev)
    feats = GradientFeatures(st, proj, timesteps=S, output="square", seed=1, conditioning=cond)
    a = FeatureStore(6, k, device=dev)
    feats.rows(ds, range(6), a)
    # in reverse, in two calls of three and two (another grouping of the outer loop), each row into its own place
    b = FeatureStore(6, k, device=dev)
    feats.rows(ds, [5, 4, 3], b, first_row=0)
    feats.rows(ds, [2, 1], b, first_row=3)
    feats.rows(ds, [0], b, first_row=5)
    torch.cuda.synchronize()
    assert bool((a.rows.abs().sum(1) > 0).all())
    back = b.rows.flip(0)
    same = int((a.rows.view(torch.int32) == back.view(torch.int32)).sum())
    worst = max(rel(back[i], a.rows[i]) for i in range(6))
    print(f"[attribution] {kind}: {same} of {6 * k} floats equal bit for bit in the other order, worst row |b - a| / |a| = {worst:.3e}")
    # NOT bit for bit: the bf16 engine's backward pass sums GroupNorm's dgamma / dbeta, the bias gradients, conv_out's weight gradient,
    # the time embedding's dx and the split weight-gradient products with f32 atomics (docs/kernels.md), so two backward passes of the
    # same batch differ in the last bits.  The bound is the one the f32 engine's tests use for two backward passes, 1e-4 of the norm
    # (the projection is linear: a row's difference is the projection of the gradients' difference).
    assert worst < 1e-4, "a row depends on the order it is computed in"
    assert len({tuple(r.tolist()) for r in a.rows.cpu()}) == 6
    # the index is part of the row (its noise): the same image under another index is another row
    other = torch.zeros(k, device=dev)
    feats.row(ds[0], 1, other)
    assert not torch.equal(other, a.rows[0])
    if kind == "cond":                                        # a dict of the micro-batch's size serves as well as the callable
        again = torch.zeros(k, device=dev)
        GradientFeatures(st, proj, timesteps=S, output="square", seed=1, conditioning={"encoder_hidden_states": ehs.repeat(S, 1, 1)}).row(ds[2], 2, again)
        assert rel(again, a.rows[2]) < 1e-4


# ================================================================ 8. the attributor
def test_scores_and_topk_against_f64(dev):
    from siss_amd.attribution import Attributor, FeatureStore
    N, k, Q, damping = 64, 128, 8, 1e-2
    g = torch.Generator().manual_seed(21)
    st = FeatureStore(N, k, device=dev)
    st.rows.copy_(torch.randn(N, k, generator=g) * torch.logspace(-1, 1, k)[None, :])
    q = (st.rows[:Q].cpu() + 0.25 * torch.randn(Q, k, generator=g)).to(dev)
    phi = st.rows.cpu().double().numpy()
    want, v = R.scores_f64(phi, q.cpu().double().numpy(), damping)
    bound = (k + 2) * R.U * (np.abs(v) @ np.abs(phi).T)
    att = Attributor(st, damping)
    got = att.scores(q)
    assert got.shape == (Q, N) and got.dtype == torch.float32 and got.is_cuda
    err = np.abs(got.cpu().double().numpy() - want)
    print(f"[attribution] scores: max err / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound)
    top = 5
    val, idx = att.topk(q, top)
    val, idx = val.cpu().double().numpy(), idx.cpu().numpy()
    order = np.argsort(-want, axis=1, kind="stable")
    for r in range(Q):
        srt = want[r, order[r]]
        for c in range(top):
            i = order[r, c]
            gap_before = np.inf if c == 0 else srt[c - 1] - srt[c]
            gap_after = srt[c] - srt[c + 1]
            if min(gap_before, gap_after) > 2 * bound[r].max():
                assert idx[r, c] == i, (r, c)
            assert abs(val[r, c] - want[r, idx[r, c]]) <= bound[r, idx[r, c]]
    assert np.array_equal(idx[:, 0], np.arange(Q)), "a noised copy of row i must name row i first"
    # negative control: the same products without the preconditioner miss the scores by far more than the bound
    plain = q.cpu().double().numpy() @ phi.T
    assert np.max(np.abs(plain - want) / bound) >= 100
    si = att.self_influence()
    K, _ = R.preconditioner(phi, damping)
    assert np.abs(si - np.einsum("ij,ij->i", phi, np.linalg.solve(K, phi.T).T)).max() <= 1e-10 * si.max()


# ================================================================ 9. the tool
def test_attribute_tool_end_to_end(dev, tmp_path):
    from test_hip_ewc import CELEB
    from siss_amd.attribution import FeatureStore
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import attribute
    ov = [*CELEB[1:], "train_batch_size=2", "allow_random_init=true", "allow_synthetic=true", f"data_dir={tmp_path}/nodata",
          "mixed_precision=bf16", f"output_dir={tmp_path}/unused"]
    ind = tmp_path / "indices.txt"
    ind.write_text("".join(f"{i}\n" for i in range(6)))
    out = tmp_path / "store"
    store = attribute.main(["build", CELEB[0], *ov, "--out", str(out), "--k", "64", "--timesteps", "2", "--output", "square", "--indices",
                            str(ind), "--targets", "attentions"])
    assert len(store) == 6 and store.k == 64 and store.names == [str(i) for i in range(6)]
    assert sorted(os.listdir(out)) == ["build.json", "features.json", "features.safetensors"]
    fp = FeatureStore.read_meta(out)["fingerprint"]
    assert fp["timesteps"] == 2 and fp["output"] == "square" and fp["projector"]["stretches"] is not None and fp["projector"]["k"] == 64
    forget = tmp_path / "forget.txt"
    res = attribute.main(["query", "--store", str(out), "--dataset-index", "3", "--top", "4", "--write-forget-list", str(forget)])
    # a query that IS dataset image 3 (same index seed): its row is store row 3 -- to the bound of two backward passes (the row
    # independence test above says why not bit for bit) -- and it names itself first
    d = rel(res["rows"][0], store.rows[3])
    print(f"[attribution] the query that is dataset image 3 against store row 3: {d:.3e}")
    assert d < 1e-4 and max(rel(res["rows"][0], store.rows[i]) for i in (0, 1, 2, 4, 5)) > 1e-2
    saved = json.load(open(out / "attribution.json"))
    assert saved["damping"] == 0.01 and saved["damping_term"] > 0 and saved["top"] == 4 and len(saved["queries"]) == 1
    qr = saved["queries"][0]
    assert qr["query"] == "dataset[3]" and qr["index"] == 3 and qr["names"][0] == "3" and len(qr["names"]) == len(qr["scores"]) == 4
    assert qr["scores"] == sorted(qr["scores"], reverse=True) and sorted(set(qr["self_influence_rank"])) == sorted(qr["self_influence_rank"])
    assert attribute.read_forget_list(forget) == qr["names"]
    # other weights: the reload is refused by field
    with pytest.raises(ValueError, match="the store's weights is"):
        b = json.load(open(out / "build.json"))
        b["overrides"] = [o for o in b["overrides"]] + ["random_seed=123"]
        json.dump(b, open(out / "build.json", "w"))
        attribute.main(["query", "--store", str(out), "--dataset-index", "3"])

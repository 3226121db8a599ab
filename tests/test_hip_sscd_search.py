"""The launchers of csrc/sscd_search.hip called DIRECTLY (siss_sscd_search_ws_bytes, siss_sscd_topk, siss_sscd_count_above,
siss_sscd_fill_above), then siss_amd/sscd_search.py and the `metrics.sscd_nn` key on top of them, against tests/sscd_search_ref.py.

Every output lies between guard stretches filled with a sentinel and the WHOLE buffer is compared where the result is known bit for bit;
the inputs must come back bit-identical; a refusal writes nothing.

What is held to what:
* rows with entries in {-1, 0, 1} * 2^-5 (every partial sum exact in f32 in any order): topk, count_above and fill_above BITWISE against
  integer arithmetic, with exact ties planted across piece boundaries (the lowest index wins) and k > ng;
* Gaussian unit rows (numpy.random.default_rng(0), nq = 33, ng = 20011, d = 512, neighbours planted at cosines 0.9 / 0.7 / 0.55): the
  two acceptance functions of the reference under the a-priori bound b = gamma_d sum |q_i g_i| (derived there, not measured);
* a pair's value is the same bits from the full problem, a single-row query, a gallery that starts at another row, a permuted gallery,
  another k, and fill_above;
* self0, NaN rows, the refusals, the work buffer's size;
* SSCDIndex on a random-init SSCDModel, one DeleteCeleb toy run through main.main with `+metrics.sscd_nn`, and one DeleteSD run on
  the tiny checkpoint of tests/test_hip_injection.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import sscd_search_ref as R
from test_hip_small_kernels import Buf, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32, I64 = torch.float32, torch.int32, torch.int64
SENT_I = -77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from siss_amd import lib
    lib.load()
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def launch(name, *args):
    from siss_amd import lib
    lib.call(name, *args)
    torch.cuda.synchronize()


def bits1(v):
    return int(np.float32(v).view(np.int32))


def ws_bytes(nq, ng, k):
    from siss_amd import lib
    return int(lib.query("siss_sscd_search_ws_bytes", nq, ng, k))


class Rows:
    """Input rows on the device between guards; `check()` holds the whole buffer to what was uploaded."""

    def __init__(self, a, dev):
        self.a = T(a)
        self.buf = Buf(self.a.shape, F32, dev, body=self.a)

    @property
    def t(self):
        return self.buf.t

    def check(self, what):
        self.buf.check(self.a, what + " came back changed")


def work(nbytes, dev):
    return Buf((max(nbytes // 8, 1),), I64, dev, fill=SENT_I)


def run_topk(dev, q, g, nq, k, self0=-1):
    """siss_sscd_topk of the first nq rows of q (a Rows) against g (a Rows): (val, idx) as numpy; guards checked."""
    ng, d = g.a.shape
    val, idx = Buf((nq, k), F32, dev), Buf((nq, k), I32, dev, fill=SENT_I)
    ws = work(ws_bytes(nq, ng, k), dev)
    launch("siss_sscd_topk", q.t[:nq], nq, g.t, ng, d, k, self0, val.t, idx.t, ws.t, ws.n * 8)
    val.guards("topk val"); idx.guards("topk idx"); ws.guards("topk ws")
    return val.t.cpu().numpy(), idx.t.cpu().numpy()


def run_above(dev, q, g, nq, thr, self0=-1):
    """count_above -> exclusive scan on the device -> fill_above: (counts, offsets, idx, val) as numpy; guards checked."""
    ng, d = g.a.shape
    counts = Buf((nq,), I32, dev, fill=SENT_I)
    ws = work(ws_bytes(nq, ng, 0), dev)
    launch("siss_sscd_count_above", q.t[:nq], nq, g.t, ng, d, float(thr), self0, counts.t, ws.t, ws.n * 8)
    counts.guards("counts"); ws.guards("count ws")
    off = Buf((nq + 1,), I64, dev, fill=SENT_I)
    off.t[0] = 0
    off.t[1:] = torch.cumsum(counts.t, 0, dtype=I64)
    offsets = off.t.cpu().numpy().copy()
    total = int(offsets[-1])
    idx, val = Buf((max(total, 1),), I32, dev, fill=SENT_I), Buf((max(total, 1),), F32, dev)
    launch("siss_sscd_fill_above", q.t[:nq], nq, g.t, ng, d, float(thr), self0, off.t, idx.t, val.t, ws.t, ws.n * 8)
    idx.guards("fill idx"); val.guards("fill val"); ws.guards("fill ws"); off.check(T(offsets), "offsets after fill")
    if total == 0:                                   # nothing listed: the one spare slot keeps its sentinel
        idx.check(torch.full((1,), SENT_I, dtype=I32), "fill idx of an empty answer")
    return counts.t.cpu().numpy(), offsets, idx.t.cpu().numpy()[:total], val.t.cpu().numpy()[:total]


# ================================================================ exact data: bitwise
NQS, KS = (1, 15, 16, 17, 33), (1, 5, 32)


def exact_case(ng, d):
    """Queries [33, d] and a gallery [ng, d] of exact rows; in the large galleries query 0 and query 20 are planted as gallery rows on both
    sides of piece boundaries (rows 127 | 128 at ng = 20011, where a piece is 128 rows; 63 | 64 are a tile boundary everywhere), so their
    best values are exact ties that only the index decides."""
    q, g = R.exact_rows(33, d, 1), R.exact_rows(ng, d, 2)
    for rows, src in (((63, 64, 127, 128, 129, 1024), 0), ((5, 255, 256, ng - 1), 20)):
        for r in rows:
            if r < ng and ng > 1000:
                g[r] = q[src]
    return q, g


@pytest.mark.parametrize("d", [4, 20, 512])
@pytest.mark.parametrize("ng", [1, 3, 15, 17, 1027, 20011])
def test_exact_rows_are_searched_bitwise(dev, ng, d):
    qa, ga = exact_case(ng, d)
    s = R.exact_sims(qa, ga)
    q, g = Rows(qa, dev), Rows(ga, dev)
    v32, i32 = R.exact_topk(s, 32)
    thr = np.float32(max(1, int(0.5 * np.sqrt(d * 4 / 9))) * 2.0 ** -10)          # a value the data takes: `>=` is exercised
    for nq in NQS:
        for k in KS:
            val, idx = run_topk(dev, q, g, nq, k)
            same(T(idx), T(i32[:nq, :k]), f"topk idx nq={nq} ng={ng} d={d} k={k}")
            same(T(val), T(v32[:nq, :k]), f"topk val nq={nq} ng={ng} d={d} k={k}")
        wc, wo, wi, wv = R.exact_above(s[:nq], thr)
        counts, offsets, idx, val = run_above(dev, q, g, nq, thr)
        same(T(counts), T(wc), f"counts nq={nq} ng={ng} d={d}")
        same(T(idx), T(wi), f"fill idx nq={nq} ng={ng} d={d}")
        same(T(val), T(wv), f"fill val nq={nq} ng={ng} d={d}")
    if ng > 1000 and d == 512:                       # the planted ties lead (no other row reaches <q, q> at this d): the index decided
        assert i32[0, :6].tolist() == [63, 64, 127, 128, 129, 1024] and len(set(v32[0, :6].tolist())) == 1
    q.check("queries"); g.check("gallery")


def test_work_buffer_grows_with_pieces_not_with_the_gallery():
    from siss_amd import lib
    lib.load()
    nq, ng = 33, 20011
    for k in (1, 8, 32):
        w = ws_bytes(nq, ng, k)
        assert 0 < w <= nq * 256 * k * 8 and w < nq * ng * 4
        assert ws_bytes(nq, 2 ** 31 - 1, k) <= nq * 256 * k * 8            # at most 256 pieces whatever the gallery
        assert w == R.ws_bytes(nq, ng, k)
    assert ws_bytes(nq, ng, 8) == 8 * ws_bytes(nq, ng, 1) and 0 < ws_bytes(nq, ng, 0) <= 16 * ((nq * 256 * 12 + 15) // 16)
    assert ws_bytes(0, ng, 1) == -1 and ws_bytes(nq, 0, 1) == -1 and ws_bytes(nq, ng, 33) == -1 and ws_bytes(nq, ng, -1) == -1


# ================================================================ Gaussian unit rows: the acceptance functions
@pytest.fixture(scope="module")
def gauss(dev):
    qa, ga = R.gaussian_case()
    return dict(qa=qa, ga=ga, q=Rows(qa, dev), g=Rows(ga, dev), s64=R.sims64(qa, ga), b=R.bound(qa, ga))


def test_gaussian_topk_is_accepted(dev, gauss):
    val, idx = run_topk(dev, gauss["q"], gauss["g"], R.NQ, 8)
    R.accept_topk(val, idx, gauss["s64"], gauss["b"], 8)
    for i, j, c in R.PLANTED:
        assert idx[i, 0] == j and abs(float(val[i, 0]) - c) < 1e-4, (i, idx[i].tolist(), val[i].tolist())
    assert gauss["b"].max() <= R.gamma(R.D) * (1 + 1e-6) and R.gamma(R.D) < 3.06e-5
    gauss["q"].check("queries"); gauss["g"].check("gallery")


@pytest.mark.parametrize("thr", [0.1, 0.5])
def test_gaussian_threshold_lists_are_accepted(dev, gauss, thr):
    counts, offsets, idx, val = run_above(dev, gauss["q"], gauss["g"], R.NQ, thr)
    band = R.accept_above(counts, offsets, idx, val, gauss["s64"], gauss["b"], thr)
    print(f"thr = {thr}: {int(offsets[-1])} pairs listed, {band:.4%} of the pairs in the undecided band")
    if thr == 0.5:
        assert sorted(zip(np.repeat(np.arange(R.NQ), counts).tolist(), idx.tolist())) == sorted((i, j) for i, j, _ in R.PLANTED)
    # the listed values are the bits topk returns for those pairs
    tv, ti = run_topk(dev, gauss["q"], gauss["g"], R.NQ, 32)
    seen = 0
    for i in range(R.NQ):
        listed = dict(zip(idx[offsets[i]:offsets[i + 1]].tolist(), R.bits(val[offsets[i]:offsets[i + 1]]).tolist()))
        for v, j in zip(tv[i], ti[i]):
            if v >= np.float32(thr):
                assert listed.get(int(j)) == bits1(v), (i, j, v)
                seen += 1
    assert seen >= 3
    gauss["q"].check("queries"); gauss["g"].check("gallery")


def test_a_pairs_value_does_not_depend_on_the_problem_around_it(dev, gauss):
    q, g, qa, ga = gauss["q"], gauss["g"], gauss["qa"], gauss["ga"]
    val, idx = run_topk(dev, q, g, R.NQ, 8)
    want = {(i, int(j)): int(b) for i in range(R.NQ) for j, b in zip(idx[i], R.bits(val[i]))}
    # another k
    v2, i2 = run_topk(dev, q, g, R.NQ, 32)
    same(T(i2[:, :8]), T(idx), "k = 32 against k = 8: indices"); same(T(v2[:, :8]), T(val), "k = 32 against k = 8: values")
    # a single-row query (the row sits at tile row 0 instead of i % 16)
    for i in (0, 5, 16, 31, 32):
        v1, i1 = run_topk(dev, Rows(qa[i:i + 1], dev), g, 1, 8)
        same(T(i1[0]), T(idx[i]), f"query {i} alone: indices"); same(T(v1[0]), T(val[i]), f"query {i} alone: values")
    # a gallery that starts at another row (every row moves to another tile column, the pieces are cut elsewhere)
    v3, i3 = run_topk(dev, q, Rows(ga[5:], dev), R.NQ, 8)
    for i in range(R.NQ):
        for v, j in zip(v3[i], i3[i]):
            if (i, int(j) + 5) in want:
                assert want[(i, int(j) + 5)] == bits1(v), ("slice", i, j)
    assert all(i3[i, 0] + 5 == j for i, j, _ in R.PLANTED if j >= 5)
    # a permuted gallery
    perm = np.random.default_rng(5).permutation(R.NG)
    v4, i4 = run_topk(dev, q, Rows(ga[perm], dev), R.NQ, 8)
    hit = 0
    for i in range(R.NQ):
        for v, j in zip(v4[i], i4[i]):
            key = (i, int(perm[j]))
            if key in want:
                assert want[key] == bits1(v), ("permuted", i, j)
                hit += 1
    assert hit >= R.NQ * 8 - 8                       # (the sets may differ only where the 8th and 9th values tie)
    # fill_above, at the bits of each query's 8th value taken over all queries (the lowest of them)
    thr = float(val[:, 7].min())
    counts, offsets, fi, fv = run_above(dev, q, g, R.NQ, thr)
    for i in range(R.NQ):
        listed = dict(zip(fi[offsets[i]:offsets[i + 1]].tolist(), R.bits(fv[offsets[i]:offsets[i + 1]]).tolist()))
        for j, b in zip(idx[i], R.bits(val[i])):
            assert listed[int(j)] == int(b), ("fill_above", i, j)


def test_self0_skips_exactly_the_self_pairs(dev, gauss):
    g, ga = gauss["g"], gauss["ga"]
    q = Rows(ga[100:133], dev)
    v9, i9 = run_topk(dev, q, g, 33, 9)
    v8, i8 = run_topk(dev, q, g, 33, 8, self0=100)
    for i in range(33):
        keep = i9[i] != 100 + i
        assert keep.sum() == 8, (i, i9[i].tolist())              # the self pair (similarity 1) is among the first 9
        same(T(i8[i]), T(i9[i][keep]), f"self0: indices of query {i}"); same(T(v8[i]), T(v9[i][keep]), f"self0: values of query {i}")
    c0, o0, fi0, fv0 = run_above(dev, q, g, 33, 0.1)
    c1, o1, fi1, fv1 = run_above(dev, q, g, 33, 0.1, self0=100)
    rows = np.repeat(np.arange(33), c0)
    keep = fi0 != rows + 100
    assert (~keep).sum() == 33 and (c1 == c0 - 1).all()
    same(T(fi1), T(fi0[keep]), "self0: listed indices"); same(T(fv1), T(fv0[keep]), "self0: listed values")


def test_nan_rows_are_never_selected_or_counted(dev, gauss):
    qa, ga = gauss["qa"].copy(), gauss["ga"].copy()
    ga[500, 17] = np.nan
    qa[3, :] = np.nan
    q, g = Rows(qa, dev), Rows(ga, dev)
    v9, i9 = run_topk(dev, gauss["q"], gauss["g"], R.NQ, 9)
    val, idx = run_topk(dev, q, g, R.NQ, 8)
    assert (idx[3] == -1).all() and np.isneginf(val[3]).all()
    assert not (idx == 500).any() and not np.isnan(val).any()
    for i in range(R.NQ):
        if i != 3:
            keep = np.flatnonzero(i9[i] != 500)[:8]
            same(T(idx[i]), T(i9[i][keep]), f"NaN: indices of query {i}"); same(T(val[i]), T(v9[i][keep]), f"NaN: values of query {i}")
    for thr in (0.1, float("-inf")):
        counts, offsets, fi, fv = run_above(dev, q, g, R.NQ, thr)
        assert counts[3] == 0 and not (fi == 500).any() and not np.isnan(fv).any()
        if thr == float("-inf"):
            assert (np.delete(counts, 3) == R.NG - 1).all()
    q.check("queries"); g.check("gallery")


def test_refusals_write_nothing(dev):
    from siss_amd import lib
    qa, ga = R.exact_rows(17, 24, 3), R.exact_rows(40, 24, 4)
    nq, ng, d, k = 17, 40, 24, 5
    q, g = Rows(qa, dev), Rows(ga, dev)
    val, idx, counts = Buf((nq, k), F32, dev), Buf((nq, k), I32, dev, fill=SENT_I), Buf((nq,), I32, dev, fill=SENT_I)
    off = Buf((nq + 1,), I64, dev, fill=0)
    wsb = max(ws_bytes(nq, ng, k), ws_bytes(nq, ng, 0))
    ws = work(wsb, dev)
    q1 = q.buf.d[q.buf.g + 1:q.buf.g + 1 + nq * d].view(nq, d)                    # 4 bytes off a 16-byte boundary

    def topk(**kw):
        a = dict(q=q.t, nq=nq, g=g.t, ng=ng, d=d, k=k, self0=-1, val=val.t, idx=idx.t, ws=ws.t, wsb=wsb)
        a.update(kw)
        return ("siss_sscd_topk", *a.values())

    def count(**kw):
        a = dict(q=q.t, nq=nq, g=g.t, ng=ng, d=d, thr=0.0, self0=-1, counts=counts.t, ws=ws.t, wsb=wsb)
        a.update(kw)
        return ("siss_sscd_count_above", *a.values())

    def fill(**kw):
        a = dict(q=q.t, nq=nq, g=g.t, ng=ng, d=d, thr=0.0, self0=-1, off=off.t, idx=idx.t, val=val.t, ws=ws.t, wsb=wsb)
        a.update(kw)
        return ("siss_sscd_fill_above", *a.values())
    cases = [topk(d=22), topk(k=0), topk(k=33), topk(q=None), topk(g=None), topk(val=None), topk(idx=None), topk(ws=None),
             topk(wsb=ws_bytes(nq, ng, k) - 1), topk(q=q1), topk(nq=0), topk(ng=0), topk(d=0), topk(d=4100),
             count(d=22), count(q=None), count(counts=None), count(ws=None), count(wsb=ws_bytes(nq, ng, 0) - 1), count(q=q1),
             fill(d=22), fill(g=None), fill(off=None), fill(idx=None), fill(val=None), fill(ws=None), fill(wsb=ws_bytes(nq, ng, 0) - 1),
             fill(q=q1)]
    for name, *args in cases:
        with pytest.raises(RuntimeError, match="bad argument"):
            lib.call(name, *args)
    torch.cuda.synchronize()
    for b, what in ((val, "val"), (idx, "idx"), (counts, "counts"), (ws, "ws"), (off, "offsets")):
        same(b.d.cpu(), b.flat, f"{what} after the refusals")
    q.check("queries"); g.check("gallery")


# ================================================================ SSCDIndex on a random-init network
def write_images(directory, n, size=64, seed=0):
    """n PNGs of smooth random colour fields (distinct enough that a random-init network separates them); returns their paths."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    r = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        low = r.integers(0, 256, size=(4, 4, 3), dtype=np.uint8)
        img = Image.fromarray(low).resize((size, size), Image.BICUBIC)
        paths.append(os.path.join(directory, f"img_{i:03d}.png"))
        img.save(paths[-1])
    return paths


def test_index_build_save_load_and_search(dev, tmp_path):
    import shutil
    from siss_amd.sscd import SSCDModel
    from siss_amd.sscd_search import SSCDIndex, decode_u8
    torch.manual_seed(0)
    model = SSCDModel(batch_size=8).to(dev).eval()
    paths = write_images(str(tmp_path / "imgs"), 7)
    dup = str(tmp_path / "imgs" / "img_900_copy.png")
    shutil.copyfile(paths[2], dup)
    paths.append(dup)
    forget = str(tmp_path / "forget.png")
    shutil.copyfile(paths[5], forget)
    index = SSCDIndex.build(model, paths, (0.5,), (0.25,), batch_size=3, forget=[forget])
    assert len(index) == 9 and index.names[-1] == forget and index.forget.tolist() == [False] * 8 + [True]
    index.save(str(tmp_path / "index"))
    again = SSCDIndex.load(str(tmp_path / "index"), model=model, files=paths + [forget])
    same(again.emb.cpu(), index.emb.cpu(), "build -> save -> load")
    assert again.names == index.names and again.meta == index.meta and again.emb.device == index.emb.device
    torch.manual_seed(1)                                         # (the constructor draws from a fork of the global generator)
    other = SSCDModel(batch_size=8).to(dev).eval()               # other weights: refused
    with pytest.raises(ValueError, match="another model"):
        SSCDIndex.load(str(tmp_path / "index"), model=other)
    # each image is its own nearest neighbour, at similarity 1 within b (the duplicates tie: the lower index wins)
    u8 = torch.stack([decode_u8(p) for p in paths + [forget]])
    emb = model.embed_u8(u8, (0.5,), (0.25,))
    val, idx = index.topk(emb, 3)
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    e64 = index.emb.cpu().double().numpy()
    b = R.bound(e64, e64)
    assert idx[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 2, 5], idx.tolist()
    assert (np.abs(val[:, 0].astype(np.float64) - 1.0) <= np.diag(b) + 4 * R.U).all(), val[:, 0].tolist()   # (+ the rows' own norm error)
    R.accept_topk(val, idx, e64 @ e64.T, b, 3)
    # the duplicated files are found
    thr = 1.0 - 1e-4
    i, j, v = index.pairs(thr, block=4)
    found = set(zip(i.tolist(), j.tolist()))
    assert {(2, 7), (5, 8)} <= found
    s64 = e64 @ e64.T
    for a in range(9):
        for c in range(a + 1, 9):
            if s64[a, c] >= thr + b[a, c]:
                assert (a, c) in found
            if s64[a, c] < thr - b[a, c]:
                assert (a, c) not in found
    comps = index.components(thr, block=4)
    assert any({2, 7} <= set(c) for c in comps) and any({5, 8} <= set(c) for c in comps)


# ================================================================ the task: one DeleteCeleb toy run with +metrics.sscd_nn
TOY = ["training_steps=2", "train_batch_size=2", "gradient_accumulation_steps=1", "checkpoint_path=/nonexistent", "allow_random_init=true",
       "unet.sample_size=16", "unet.block_out_channels=[64,128]", "unet.down_block_types=[DownBlock2D,AttnDownBlock2D]",
       "unet.up_block_types=[AttnUpBlock2D,UpBlock2D]", "unet.layers_per_block=1", "unet.attention_head_dim=null", "save_final=false",
       "eval_every=1", "eval_batch_size=2", "pipeline.num_inference_steps=3", "metrics.denoising_injections.timestep=3",
       # the step's gradient kernels add with float atomics, so two runs' weights differ in the last bits (tests/test_hip_injection.py,
       # _same_weights); with a zero step size the weights every evaluation sees are the initial ones and the runs compare bit for bit
       "optimizer.lr=0", "optimizer.weight_decay=0"]


def run_toy(tmp_path, name, data, extra):
    """delete_celeb through main.main on the toy UNet; returns the run's directory (main.py appends <timestamp>_<uuid>)."""
    sys.path.insert(0, ROOT)
    import main
    out = tmp_path / name
    main.main(["--config-name=delete_celeb", f"data_dir={data}", f"output_dir={out}", "deletion.img_name=[img_004.png]", *TOY, *extra])
    (run,) = os.listdir(out)
    return out / run


def test_delete_celeb_toy_run_writes_replication_records(dev, tmp_path):
    data = tmp_path / "gallery"
    write_images(str(data), 12, size=16, seed=3)
    sscd = [f"metrics.denoising_injections.sscd.model_path={tmp_path}/missing.pt", "metrics.denoising_injections.sscd.allow_random_init=true"]
    key = [f"+metrics.sscd_nn.index_path={tmp_path}/index", "+metrics.sscd_nn.k=3", "+metrics.sscd_nn.threshold=0.5"]
    first = run_toy(tmp_path, "first", data, sscd + key)
    recs = [json.loads(l) for l in open(first / "replication_rank0.jsonl")]
    inj = [json.loads(l) for l in open(first / "injection_rank0.jsonl")]
    assert [r["global_step"] for r in recs] == [r["global_step"] for r in inj] == [1, 2]           # one line per evaluation
    names = {str(data / f"img_{i:03d}.png") for i in range(12)}
    for r, ir in zip(recs, inj):
        assert set(r) == {"global_step", "tag", "nn_mean", "nn_max", "nn_p95", "above", "nn_is_forget", "nn_other_max", "top"}
        assert r["tag"] == "t3" and len(r["top"]) == len(ir["sscd"]) == 2
        assert all(len(t) == 3 and all(n in names and -1.0 <= v <= 1.0 + 2.0 ** -20 for n, v in t) for t in r["top"])
        top1 = [t[0][1] for t in r["top"]]
        assert r["nn_max"] == max(top1) and abs(r["nn_mean"] - sum(top1) / 2) < 1e-12 and r["nn_max"] >= r["nn_p95"] >= r["nn_mean"]
        assert r["above"] == sum(v >= 0.5 for v in top1) and r["nn_is_forget"] in (0.0, 0.5, 1.0) and r["nn_other_max"] <= r["nn_max"]
        # the forget image is a row of the gallery: its similarity with each injection is the score injection_rank0.jsonl records
        for t, s in zip(r["top"], ir["sscd"]):
            hit = [v for n, v in t if n == str(data / "img_004.png")]
            assert not hit or abs(hit[0] - s) <= 2 * R.gamma(512)
    meta = json.load(open(tmp_path / "index" / "index.json"))
    assert meta["n"] == 12 and sum(meta["forget"]) == 1 and meta["forget"][4] and os.path.exists(tmp_path / "index" / "index.safetensors")
    stamp = os.stat(tmp_path / "index" / "index.safetensors").st_mtime_ns
    second = run_toy(tmp_path, "second", data, sscd + key)                # loads the index instead of building it
    assert os.stat(tmp_path / "index" / "index.safetensors").st_mtime_ns == stamp
    assert open(second / "replication_rank0.jsonl").read() == open(first / "replication_rank0.jsonl").read()
    without = run_toy(tmp_path, "without", data, sscd)
    assert not os.path.exists(without / "replication_rank0.jsonl")
    assert open(without / "injection_rank0.jsonl").read() == open(first / "injection_rank0.jsonl").read()
    assert sorted(set(os.listdir(first)) - set(os.listdir(without))) == ["replication_rank0.jsonl"]


def test_delete_sd_toy_run_searches_the_embeddings_of_metrics_sscd(dev, tmp_path):
    """DeleteSD on the tiny checkpoint of tests/test_hip_injection.py: one line per prompt and one for the injection, from the
    embeddings metrics.sscd computes; metrics_rank0.jsonl is byte for byte what the run without the key writes."""
    from PIL import Image
    from test_hip_injection import _run_sd, _tiny_checkpoint
    ckpt = tmp_path / "ckpt"
    _tiny_checkpoint(dev, ckpt)
    g = torch.Generator().manual_seed(1)
    torch.save(torch.rand(8, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "all.pt")
    torch.save(torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, tmp_path / "del.pt")
    torch.save(torch.randint(0, 1000, (1, 77), generator=g), tmp_path / "prompt_ids.pt")
    Image.fromarray(torch.randint(0, 256, (32, 32, 3), generator=g, dtype=torch.uint8).numpy()).save(str(tmp_path / "mem.png"))
    write_images(str(tmp_path / "gallery"), 5, size=32, seed=7)
    base = ["training_steps=1", "eval_every=1", "+eval_batches=2", "+eval_batch_size=1", "+pipeline.num_inference_steps=4", "resolution=32",
            f"data_files.mem_img_path={tmp_path}/mem.png", "metrics.denoising_injections.strength=0.5",
            "metrics.denoising_injections.num_images=4", "metrics.denoising_injections.prompt=0",
            f"metrics.sscd.model_path={tmp_path}/missing.pt", "metrics.sscd.allow_random_init=true",
            "learning_rate=0", "adam_weight_decay=0"]            # (a zero step size: the two runs see the same weights bit for bit)
    key = [f"+metrics.sscd_nn.data_path={tmp_path}/gallery", f"+metrics.sscd_nn.index_path={tmp_path}/index", "+metrics.sscd_nn.k=2"]
    prompt = str(tmp_path / "prompt_ids.pt")
    _, _, cfg0 = _run_sd(tmp_path, "without", ckpt, base, prompt)
    task, _, cfg = _run_sd(tmp_path, "with", ckpt, base + key, prompt)
    assert sorted(set(os.listdir(cfg.output_dir)) - set(os.listdir(cfg0.output_dir))) == ["replication_rank0.jsonl"]
    assert open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl")).read() == open(os.path.join(cfg0.output_dir, "metrics_rank0.jsonl")).read()
    recs = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "replication_rank0.jsonl"))]
    assert [(r["global_step"], r["tag"]) for r in recs] == [(1, 0), (1, "inj_0")] and [len(r["top"]) for r in recs] == [2, 4]
    index = task.replication.index
    assert len(index) == 6 and index.names[-1] == f"{tmp_path}/mem.png" and index.forget.tolist() == [False] * 5 + [True]
    lines = {k: v for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl")) for k, v in json.loads(l).items()}
    for r, name in zip(recs, ("sscd_0", "sscd_inj_0")):
        assert all(len(t) == 2 and t[0][1] >= t[1][1] for t in r["top"]) and r["nn_max"] == max(t[0][1] for t in r["top"])
        # the forget image is a row of the index: where every query lists it, the mean of those similarities is the recorded score
        mem = [[v for n, v in t if n == f"{tmp_path}/mem.png"] for t in r["top"]]
        if all(mem):
            assert abs(sum(m[0] for m in mem) / len(mem) - lines[name]) <= 2 * R.gamma(512)

"""siss_amd/sscd_search.py, tools/find_copies.py and the `metrics.sscd_nn` key on the CPU, with the three launchers of
csrc/sscd_search.hip emulated by tests/sscd_search_ref.py -- and that reference's own acceptance functions held to cases they must reject."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import sscd_search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def emulated(monkeypatch):
    """The module's three doors to the library answered by the reference's emulation."""
    from siss_amd import sscd_search as S

    def launch(name, *a):
        rc = R.call(name, *a)
        assert rc is not None, name
        if rc:
            raise RuntimeError(f"{name} failed with status {rc} (bad argument)")
        return 0
    monkeypatch.setattr(S, "_launch", launch)
    monkeypatch.setattr(S, "_ws_bytes", R.ws_bytes)
    monkeypatch.setattr(S, "require_kernels", lambda: None)
    return S


def unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


class FakeModel:
    """What the fingerprint and the index read of an SSCDModel."""

    def __init__(self, seed, dims=8):
        self.W = torch.randn(8, dims, generator=torch.Generator().manual_seed(seed))
        self._sd = {"backbone.fc.weight": self.W}
        self.dims, self.pool_param, self.device = dims, 3.0, torch.device("cpu")

    def to(self, device):
        return self

    def eval(self):
        return self

    def embed_u8(self, u8, mean, std):
        """A fixed linear map of the image's mean colour and two corner pixels: equal files give equal rows."""
        x = u8.float()
        f = torch.cat([x.mean((1, 2)), x[:, 0, 0], x[:, -1, -1, :2]], 1) / 255 - 0.4
        return torch.nn.functional.normalize(f @ self.W, dim=1)


# ================================================================ the reference rejects what it must
def test_acceptance_functions_reject_wrong_answers():
    q, g = unit(5, 64, 1), unit(300, 64, 2)
    g[17] = g[3]                                                   # an exact tie for every query
    s, b = R.sims64(q, g), R.bound(q, g)
    v, i = R.exact_topk(s, 6)
    v = R.chain_sims(q, g)[np.arange(5)[:, None], i]               # f32 values of those rows
    R.accept_topk(v, i, s, b, 6)
    bad = i.copy(); bad[2, 5] = int(np.argmin(s[2]))               # a wrong index (its value made consistent with it)
    bv = v.copy(); bv[2, 5] = np.float32(s[2, bad[2, 5]])
    with pytest.raises(AssertionError, match="not among"):
        R.accept_topk(bv, bad, s, b, 6)
    tq = unit(1, 64, 3); tg = np.repeat(unit(1, 64, 4), 4, 0)       # four equal rows: one value, indices must ascend
    ts, tb = R.sims64(tq, tg), R.bound(tq, tg)
    tv = np.full((1, 3), R.chain_sims(tq, tg)[0, 0], np.float32)
    R.accept_topk(tv, np.array([[0, 1, 2]]), ts, tb, 3)
    with pytest.raises(AssertionError, match="do not ascend"):
        R.accept_topk(tv, np.array([[0, 2, 1]]), ts, tb, 3)        # a swapped tie
    rep = i.copy(); rep[1, 1] = rep[1, 0]
    with pytest.raises(AssertionError, match="repeats"):
        R.accept_topk(v, rep, s, b, 6)                             # a repeated index
    off = v.copy(); off[0, 0] += np.float32(2 * b[0, i[0, 0]])
    with pytest.raises(AssertionError, match="value off"):
        R.accept_topk(off, i, s, b, 6)                             # a value off by 2b
    short = i.copy(); short[4, 5] = -1
    sv = v.copy(); sv[4, 5] = -np.inf
    with pytest.raises(AssertionError, match="entries are due"):
        R.accept_topk(sv, short, s, b, 6)                          # a skipped slot
    with pytest.raises(AssertionError, match="excluded"):
        R.accept_topk(v, i, s, b, 6, self0=int(i[0, 0]))           # the excluded self pair of query 0
    # thresholds
    thr = 0.2
    c, o, li, lv = R.exact_above(R.chain_sims(q, g).astype(np.float64), thr)
    R.accept_above(c, o, li, lv, s, b, thr)
    sure = np.argwhere(s >= thr + b)
    assert len(sure)
    row, col = sure[0]
    keep = ~((np.repeat(np.arange(5), c) == row) & (li == col))
    c2 = c.copy(); c2[row] -= 1
    o2 = np.concatenate([[0], np.cumsum(c2)])
    with pytest.raises(AssertionError, match="not listed"):
        R.accept_above(c2, o2, li[keep], lv[keep], s, b, thr)      # a missing pair
    with pytest.raises(AssertionError, match="list lengths"):
        R.accept_above(c2, o, li, lv, s, b, thr)
    with pytest.raises(AssertionError, match="band"):
        R.accept_above(c, o, li, lv, s, np.full_like(b, 0.05), thr)    # a bound so wide that the band hides everything
    assert abs(R.gamma(512) - 3.0518e-5) < 1e-8


def test_emulated_launchers_answer_the_exact_cases(emulated):
    q, g = R.exact_rows(5, 20, 1), R.exact_rows(70, 20, 2)
    s = R.exact_sims(q, g)
    val, idx = emulated.topk(torch.from_numpy(q), torch.from_numpy(g), 4, self0=-1)
    wv, wi = R.exact_topk(s, 4)
    assert np.array_equal(idx.numpy(), wi) and np.array_equal(val.numpy(), wv)
    off, li, lv = emulated.above(torch.from_numpy(q), torch.from_numpy(g), 2.0 ** -9)
    c, o, ci, cv = R.exact_above(s, 2.0 ** -9)
    assert off.tolist() == o.tolist() and np.array_equal(li.numpy(), ci) and np.array_equal(lv.numpy(), cv)
    with pytest.raises(ValueError, match="1 .. 32"):
        emulated.topk(torch.from_numpy(q), torch.from_numpy(g), 33)
    with pytest.raises(ValueError, match="rows are needed"):
        emulated.topk(torch.from_numpy(q[:, :16]), torch.from_numpy(g), 3)
    assert R.ws_bytes(33, 20011, 8) <= 33 * 256 * 8 * 8 and R.ws_bytes(33, 2 ** 31 - 1, 8) <= 33 * 256 * 8 * 8


def test_missing_entry_points_raise(monkeypatch):
    from siss_amd import lib, sscd_search as S
    monkeypatch.setattr(lib, "has", lambda name: name != "siss_sscd_topk")
    e = torch.from_numpy(unit(4, 8, 0))
    for call in (lambda: S.topk(e, e, 1), lambda: S.above(e, e, 0.5), lambda: S.SSCDIndex(e, "abcd").pairs(0.5)):
        with pytest.raises(RuntimeError, match="no siss_sscd_topk"):
            call()


# ================================================================ the index
def test_index_save_load_and_fingerprint_refusals(tmp_path, emulated):
    S = emulated
    emb = torch.from_numpy(unit(6, 8, 5))
    model = FakeModel(1)
    meta = dict(forget=[False] * 5 + [True], mean=[0.5] * 3, std=[0.25] * 3, model_fingerprint=S.model_fingerprint(model), files_fingerprint=None)
    index = S.SSCDIndex(emb, [f"n{i}" for i in range(6)], meta)
    index.save(tmp_path / "ix")
    assert sorted(os.listdir(tmp_path / "ix")) == ["index.json", "index.safetensors"]
    js = json.load(open(tmp_path / "ix" / "index.json"))
    assert js["names"] == index.names and js["forget"] == meta["forget"] and js["dims"] == 8 and js["mean"] == [0.5] * 3 and js["n"] == 6
    again = S.SSCDIndex.load(tmp_path / "ix", model=model)
    assert torch.equal(again.emb, emb) and again.names == index.names and again.meta == index.meta and again.forget.tolist() == meta["forget"]
    assert torch.equal(S.SSCDIndex.load(tmp_path / "ix").emb, emb)                     # no model: nothing to hold it against
    with pytest.raises(ValueError, match="another model"):
        S.SSCDIndex.load(tmp_path / "ix", model=FakeModel(2))
    with pytest.raises(ValueError, match="16"):
        S.SSCDIndex.load(tmp_path / "ix", model=FakeModel(1, dims=16))
    with pytest.raises(ValueError, match="names"):
        S.SSCDIndex(emb, ["a"], {})
    with pytest.raises(ValueError, match="f32 rows"):
        S.SSCDIndex(emb[:, :7], list("abcdef"), {})
    assert S.model_fingerprint(FakeModel(1)) == S.model_fingerprint(model) != S.model_fingerprint(FakeModel(2))


def write_images(directory, n, seed=0, size=8):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    r = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        paths.append(os.path.join(str(directory), f"img_{i:03d}.png"))
        Image.fromarray(r.integers(0, 256, (size, size + (i % 2), 3), dtype=np.uint8)).save(paths[-1])      # two image sizes: two runs
    return paths


def test_index_build_flags_forget_images_and_finds_a_duplicate(tmp_path, emulated):
    import shutil
    S = emulated
    paths = write_images(tmp_path / "g", 6)
    shutil.copyfile(paths[1], tmp_path / "g" / "zz_copy.png")
    shutil.copyfile(paths[4], tmp_path / "forget.png")
    files = S.list_images(tmp_path / "g")
    assert files == paths + [str(tmp_path / "g" / "zz_copy.png")]
    model = FakeModel(3)
    index = S.SSCDIndex.build(model, files, (0.0,), (1.0,), batch_size=2, forget=[str(tmp_path / "forget.png"), paths[0]])
    assert index.names == files + [str(tmp_path / "forget.png")] and index.forget.tolist() == [True] + [False] * 6 + [True]
    assert index.meta["files_fingerprint"] == S.files_fingerprint(index.names) and index.meta["mean"] == [0.0] * 3
    i, j, v = index.pairs(1 - 1e-5, block=3)
    assert set(zip(i.tolist(), j.tolist())) >= {(1, 6), (4, 7)} and (i < j).all() and (v >= np.float32(1 - 1e-5)).all()
    assert [1, 6] in index.components(1 - 1e-5, block=3) and [4, 7] in index.components(1 - 1e-5)
    index.save(tmp_path / "ix")
    assert S.SSCDIndex.load(tmp_path / "ix", model=model, files=index.names).names == index.names
    os.utime(paths[2], ns=(1, 1))                                  # a file changed since the index was built
    with pytest.raises(ValueError, match="files"):
        S.SSCDIndex.load(tmp_path / "ix", model=model, files=index.names)


def test_components_union_find():
    from siss_amd.sscd_search import components
    assert components(7, [0, 5, 1, 3], [1, 6, 2, 3]) == [[0, 1, 2], [5, 6]]
    assert components(3, [], []) == []
    assert components(4, [2, 0, 1], [3, 3, 2]) == [[0, 1, 2, 3]]


# ================================================================ the tracker
def test_replication_score_fields_on_a_hand_made_case(tmp_path, emulated):
    S = emulated
    e = np.eye(8, dtype=np.float32)
    gal = np.stack([e[0], e[1], e[2], (e[0] * 0.6 + e[3] * 0.8)]).astype(np.float32)               # rows 0 .. 3; row 1 is the forget image
    index = S.SSCDIndex(torch.from_numpy(gal), ["a", "forget", "c", "d"], dict(forget=[False, True, False, False]))
    qs = np.stack([e[1], (e[0] * 0.6 + e[4] * 0.8), e[5]]).astype(np.float32)                       # -> forget (1.0); a, d (0.6, 0.36); nothing (0)
    score = S.ReplicationScore(index, str(tmp_path / "rep.jsonl"), k=2, threshold=0.5)
    score.extra = {"sampler": "dpmsolver++", "num_inference_steps": 20}
    rec = score.record("t250", torch.from_numpy(qs), 7)
    (line,) = [json.loads(l) for l in open(tmp_path / "rep.jsonl")]
    assert line == rec and rec["global_step"] == 7 and rec["tag"] == "t250" and rec["sampler"] == "dpmsolver++"
    top1 = np.array([1.0, float(np.float32(0.6)), 0.0])
    assert rec["nn_max"] == 1.0 and abs(rec["nn_mean"] - top1.mean()) < 1e-7 and abs(rec["nn_p95"] - np.percentile(top1, 95)) < 1e-7
    assert rec["above"] == 2 and abs(rec["nn_is_forget"] - 1 / 3) < 1e-12 and abs(rec["nn_other_max"] - 0.6) < 1e-6
    assert [t[0][0] for t in rec["top"]] == ["forget", "a", "a"] and [len(t) for t in rec["top"]] == [2, 2, 2]
    assert rec["top"][1][1][0] == "d" and abs(rec["top"][1][1][1] - 0.36) < 1e-6
    assert score.record(3, torch.from_numpy(qs[:1]), 8)["tag"] == 3                                # a prompt index stays a number
    # more forget rows than the list can hold: the other rows are asked alone
    many = S.SSCDIndex(torch.from_numpy(np.concatenate([np.repeat(e[1:2], 40, 0), e[:1] * 1.0])), [f"f{i}" for i in range(40)] + ["other"],
                       dict(forget=[True] * 40 + [False]))
    rec = S.ReplicationScore(many, str(tmp_path / "many.jsonl"), k=2).record("x", torch.from_numpy((e[1] * 0.8 + e[0] * 0.6)[None]), 0)
    assert abs(rec["nn_other_max"] - 0.6) < 1e-6 and rec["nn_is_forget"] == 1.0 and rec["top"][0][0][0] == "f0"
    for bad in (dict(k=0), dict(k=33), dict(threshold=float("nan")), dict(threshold=float("inf"))):
        with pytest.raises(ValueError):
            S.ReplicationScore(index, "x", **bad)


# ================================================================ the tool
def test_find_copies_reports(tmp_path, emulated):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import find_copies
    finally:
        sys.path.pop(0)
    S = emulated
    e = np.eye(8, dtype=np.float32)
    gal = np.stack([e[0], e[1], e[0], (e[1] * 0.8 + e[2] * 0.6), e[4]]).astype(np.float32)
    index = S.SSCDIndex(torch.from_numpy(gal), list("abcde"))
    rep = find_copies.pairs_report(index, 0.7)
    assert rep["mode"] == "pairs" and rep["images"] == 5 and rep["threshold"] == 0.7
    assert [(p[0], p[1]) for p in rep["pairs"]] == [("a", "c"), ("b", "d")] and rep["pairs"][0][2] == 1.0 and abs(rep["pairs"][1][2] - 0.8) < 1e-6
    assert rep["components"] == [["a", "c"], ["b", "d"]]
    json.dumps(rep)
    rep = find_copies.gallery_report(index, torch.from_numpy(np.stack([e[1], e[5]])), ["q0", "q1"], 2, 0.5)
    assert rep["mode"] == "gallery" and rep["gallery"] == 5 and [q["name"] for q in rep["queries"]] == ["q0", "q1"]
    assert rep["queries"][0]["copy"] is True and [t[0] for t in rep["queries"][0]["top"]] == ["b", "d"]
    assert rep["queries"][1]["copy"] is False and rep["queries"][1]["top"][0] == ["a", 0.0]
    json.dumps(rep)


# ================================================================ the key of the tasks
def _compose(name, tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    return H.compose(name, os.path.join(ROOT, "config"), [f"output_dir={tmp_path}/out", *overrides])


def _checked(cls, cfg):
    task = cls(cfg)                                      # what run() does before it loads anything onto the device
    task.fill_cfg()
    task.check_supported()
    task.check_metrics()
    return task


def test_the_four_yamls_compose_unchanged_without_the_key(tmp_path):
    from siss_amd.tasks import DeleteCeleb, DeleteSD, DeleteTShirt
    for name in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        cfg = _compose(name, tmp_path)
        assert "sscd_nn" not in (cfg.get("metrics") or {})
        assert "sscd_nn" not in open(os.path.join(ROOT, "config", name + ".yaml")).read()
    for cls, name in ((DeleteCeleb, "delete_celeb"), (DeleteTShirt, "delete_tshirt"), (DeleteSD, "delete_sd")):
        assert _checked(cls, _compose(name, tmp_path)).replication is None
    assert not os.path.exists(tmp_path / "out")


def test_pixel_space_key_refusals_and_settings(tmp_path, capsys):
    from PIL import Image
    from siss_amd import sscd_search as S
    from siss_amd.tasks import DeleteCeleb, DeleteTShirt
    data = tmp_path / "celeba"
    write_images(data, 3)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "forget.png"))
    sscd = [f"metrics.denoising_injections.img_path={tmp_path}/forget.png", f"metrics.denoising_injections.sscd.model_path={tmp_path}/missing.pt",
            "metrics.denoising_injections.sscd.allow_random_init=true", f"data_dir={data}", "eval_every=1"]

    def check(*ov, cls=DeleteCeleb, name="delete_celeb"):
        return _checked(cls, _compose(name, tmp_path, *ov)).replication

    with pytest.raises(ValueError, match="needs metrics.denoising_injections.sscd"):
        check(f"data_dir={data}", "+metrics.sscd_nn.k=3")                                   # the key without its SSCD metric
    with pytest.raises(ValueError, match="needs metrics.denoising_injections.sscd"):
        check("+metrics.sscd_nn.k=3", cls=DeleteTShirt, name="delete_tshirt")
    with pytest.raises(ValueError, match="a mapping"):
        check(*sscd, "+metrics.sscd_nn=true")
    with pytest.raises(ValueError, match="unknown field"):
        check(*sscd, "+metrics.sscd_nn.kk=3")
    for k in ("0", "33", "2.5", "true"):
        with pytest.raises(ValueError, match="sscd_nn.k="):
            check(*sscd, f"+metrics.sscd_nn.k={k}")
    for t in (".nan", ".inf", "high", "true"):
        with pytest.raises(ValueError, match="threshold"):
            check(*sscd, f"+metrics.sscd_nn.threshold={t}")
    with pytest.raises(ValueError, match="batch_size"):
        check(*sscd, "+metrics.sscd_nn.batch_size=0")
    with pytest.raises(FileNotFoundError, match="data_path"):
        check(*sscd, f"+metrics.sscd_nn.data_path={tmp_path}/gone")
    with pytest.raises(FileNotFoundError, match="data_path"):                                # the default directory is not there
        check(*[o for o in sscd if not o.startswith("data_dir=")], f"data_dir={tmp_path}/gone", "+metrics.sscd_nn.k=3")
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match="data_path"):
        check(*sscd, f"+metrics.sscd_nn.data_path={tmp_path}/empty")
    # another model's index under index_path
    other = S.SSCDIndex(torch.from_numpy(unit(3, 512, 0)), list("abc"), dict(model_fingerprint="0" * 64))
    other.save(tmp_path / "foreign")
    with pytest.raises(ValueError, match="another model"):
        check(*sscd, f"+metrics.sscd_nn.index_path={tmp_path}/foreign")
    capsys.readouterr()
    got = check(*sscd, "+metrics.sscd_nn.k=3", f"+metrics.sscd_nn.index_path={tmp_path}/ix")
    assert got["k"] == 3 and got["threshold"] == 0.5 and got["batch_size"] == 16 and got["data_path"] == str(data)      # the dataset's directory
    assert got["forget"] == [f"{tmp_path}/forget.png"] and got["index_path"] == f"{tmp_path}/ix" and got["mean"] == [0.0] * 3
    assert got["out_path"] == f"{tmp_path}/out/replication_rank0.jsonl"
    assert check(*sscd, "+metrics.sscd_nn={}")["k"] == 5                                     # every field has a default
    assert not os.path.exists(tmp_path / "out") and not os.path.exists(tmp_path / "ix")


def test_delete_sd_key_refusals(tmp_path):
    from PIL import Image
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    (ckpt / "vae").mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "mem.png"))
    write_images(tmp_path / "imgs", 2)
    base = [f"base_dir={tmp_path}", f"pretrained_model_name_or_path={ckpt}", f"data_files.mem_img_path={tmp_path}/mem.png", "eval_every=1"]
    sscd = [f"metrics.sscd.model_path={tmp_path}/missing.pt", "metrics.sscd.allow_random_init=true"]

    def check(*ov):
        return _checked(DeleteSD, _compose("delete_sd", tmp_path, *ov)).replication

    assert check(*base) is None and check(*base, *sscd) is None
    with pytest.raises(ValueError, match="needs metrics.sscd"):
        check(*base, "+metrics.sscd_nn.k=3")
    with pytest.raises(FileNotFoundError, match="data_path"):
        check(*base, *sscd, "+metrics.sscd_nn.k=3", f"data_files.img_dir={tmp_path}/gone")
    with pytest.raises(ValueError, match="sscd_nn.k="):
        check(*base, *sscd, "+metrics.sscd_nn.k=40", f"data_files.img_dir={tmp_path}/imgs")
    got = check(*base, *sscd, "+metrics.sscd_nn.threshold=0.4", f"data_files.img_dir={tmp_path}/imgs")
    assert got["data_path"] == f"{tmp_path}/imgs" and got["forget"] == [f"{tmp_path}/mem.png"] and got["threshold"] == 0.4

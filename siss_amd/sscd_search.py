"""Dataset-wide SSCD copy search: an index of unit embeddings on the device and the searches over it on csrc/sscd_search.hip.

`metrics.sscd` and `metrics.denoising_injections.sscd` compare generated images with ONE image, the forget image.  This module answers
the two questions those scores leave open -- is the model copying some OTHER training image, and which images are memorized in the first
place (notebooks/sscd.ipynb of the reference: embed a directory, form all pairwise similarities on the host, list what lies above a
threshold) -- without forming the queries x gallery matrix and without copying similarities to the host:

    SSCDIndex          unit rows [N, D] on the device, a name and a forget flag per row; build / save / load; topk, above (CSR),
                       pairs (all pairs of the index in query blocks) and components (union-find on the host over pairs)
    ReplicationScore   the tracker the task loops drive (`metrics.sscd_nn`): nearest-neighbour statistics of a set of embeddings

There is no fall-back: a library without the entry points raises.  The similarity of a pair is one f32 value that depends on the two
rows alone (the launchers' contract), so `above` lists exactly the pairs `topk` would rank at or above the threshold.
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import lib
from .records import append_jsonl, finite_or_none

ENTRY_POINTS = ("siss_sscd_search_ws_bytes", "siss_sscd_topk", "siss_sscd_count_above", "siss_sscd_fill_above")
FORMAT = 1
MAX_K = 32
QUERY_BLOCK = 4096          # queries per launch: bounds the work buffer (it grows with queries x pieces x k)


def require_kernels():
    for name in ENTRY_POINTS:
        if not lib.has(name):
            raise RuntimeError(f"this libsiss_hip.so has no {name}: the SSCD search needs the kernels of csrc/sscd_search.hip (there is "
                               "no fall-back to a matrix product)")


def _ws_bytes(nq, ng, k):
    n = int(lib.query("siss_sscd_search_ws_bytes", int(nq), int(ng), int(k)))
    if n < 0:
        raise ValueError(f"siss_sscd_search_ws_bytes({nq}, {ng}, {k}) refused its arguments")
    return n


def _launch(name, *args):
    """lib.call for device tensors only: a host pointer must never reach a kernel."""
    for a in args:
        if torch.is_tensor(a) and not a.is_cuda:
            raise RuntimeError(f"{name}: a tensor on {a.device}; the search runs on the device only")
    return lib.call(name, *args)


def _rows(x, d, what):
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != d or x.shape[0] < 1:
        raise ValueError(f"{what}: [n >= 1, {d}] rows are needed, got {tuple(getattr(x, 'shape', ()))}")
    return x


def topk(queries, gallery, k, self0=-1):
    """(val [nq, k] f32, idx [nq, k] int32) of the k gallery rows of largest dot product per query row: value descending, index
    ascending among equal values, (-inf, -1) beyond the candidates.  self0 >= 0: query i is gallery row self0 + i, skipped."""
    require_kernels()
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k}: 1 .. {MAX_K}")
    ng, d = gallery.shape
    q = _rows(queries, d, "queries").to(gallery.device, torch.float32).contiguous()
    nq = q.shape[0]
    val = torch.empty(nq, k, device=gallery.device, dtype=torch.float32)
    idx = torch.empty(nq, k, device=gallery.device, dtype=torch.int32)
    ws = None
    for s in range(0, nq, QUERY_BLOCK):
        n = min(QUERY_BLOCK, nq - s)
        need = _ws_bytes(n, ng, k)
        if ws is None or ws.numel() * 8 < need:
            ws = torch.empty((need + 7) // 8, device=gallery.device, dtype=torch.int64)
        _launch("siss_sscd_topk", q[s:s + n], n, gallery, ng, d, k, self0 + s if self0 >= 0 else -1, val[s:s + n], idx[s:s + n],
                ws, ws.numel() * 8)
    return val, idx


def above(queries, gallery, thr, self0=-1):
    """CSR (offsets [nq + 1] int64, idx int32, val f32), all on the device: per query the gallery rows with similarity >= thr in
    ascending index.  Only the per-block totals (list lengths) are read by the host."""
    require_kernels()
    thr = float(thr)
    ng, d = gallery.shape
    dev = gallery.device
    q = _rows(queries, d, "queries").to(dev, torch.float32).contiguous()
    nq = q.shape[0]
    offs, idxs, vals, start, ws = [torch.zeros(1, device=dev, dtype=torch.int64)], [], [], 0, None
    for s in range(0, nq, QUERY_BLOCK):
        n = min(QUERY_BLOCK, nq - s)
        need = _ws_bytes(n, ng, 0)
        if ws is None or ws.numel() * 8 < need:
            ws = torch.empty((need + 7) // 8, device=dev, dtype=torch.int64)
        s0 = self0 + s if self0 >= 0 else -1
        counts = torch.empty(n, device=dev, dtype=torch.int32)
        _launch("siss_sscd_count_above", q[s:s + n], n, gallery, ng, d, thr, s0, counts, ws, ws.numel() * 8)
        off = torch.zeros(n + 1, device=dev, dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(off[-1])
        idx = torch.empty(max(total, 1), device=dev, dtype=torch.int32)
        val = torch.empty(max(total, 1), device=dev, dtype=torch.float32)
        _launch("siss_sscd_fill_above", q[s:s + n], n, gallery, ng, d, thr, s0, off, idx, val, ws, ws.numel() * 8)
        offs.append(off[1:] + start)
        idxs.append(idx[:total])
        vals.append(val[:total])
        start += total
    return torch.cat(offs), torch.cat(idxs), torch.cat(vals)


def decode_u8(path):
    """[H, W, 3] uint8 of `Image.open(path).convert('RGB')`."""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy())


def model_fingerprint(model):
    """sha256 over the network's parameters (name, shape and f32 / integer bytes in state-dict order), its dims and its pooling."""
    h = hashlib.sha256()
    h.update(b"siss_amd.sscd_search/%d\0" % FORMAT)
    h.update(repr((int(model.dims), float(model.pool_param))).encode())
    for k, v in model._sd.items():
        h.update(k.encode() + b"\0" + repr(tuple(v.shape)).encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def files_fingerprint(paths):
    """sha256 over each file's path, size and mtime (ns): what a row of the index was read from."""
    h = hashlib.sha256()
    for p in paths:
        st = os.stat(p)
        h.update(f"{os.path.abspath(p)}\0{st.st_size}\0{st.st_mtime_ns}\0".encode())
    return h.hexdigest()


def gallery_files(paths, forget=()):
    """(files in index order, forget flag per file): `paths`, then the forget images that are not among them."""
    paths = [str(p) for p in paths]
    forget = [str(p) for p in forget]
    have = {os.path.abspath(p) for p in paths}
    extra = [p for p in forget if os.path.abspath(p) not in have]
    marked = {os.path.abspath(p) for p in forget}
    files = paths + extra
    return files, [os.path.abspath(p) in marked for p in files]


class SSCDIndex:
    """Unit rows `emb` [N, D] f32 on the device, `names` (one per row) and `meta`: {forget: [bool per row], dims, mean, std,
    model_fingerprint, files_fingerprint} (the last two None for an index that was not built from files)."""

    def __init__(self, emb, names, meta=None):
        if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[0] < 1 or emb.shape[1] % 4:
            raise ValueError(f"SSCDIndex: f32 rows [N >= 1, D % 4 == 0] are needed, got {getattr(emb, 'dtype', None)} "
                             f"{tuple(getattr(emb, 'shape', ()))}")
        self.emb = emb.contiguous()
        self.names = [str(n) for n in names]
        meta = dict(meta or {})
        meta.setdefault("forget", [False] * len(self.names))
        meta["forget"] = [bool(f) for f in meta["forget"]]
        meta["dims"] = int(emb.shape[1])
        if len(self.names) != emb.shape[0] or len(meta["forget"]) != emb.shape[0]:
            raise ValueError(f"SSCDIndex: {emb.shape[0]} rows, {len(self.names)} names, {len(meta['forget'])} forget flags")
        self.meta = meta

    def __len__(self):
        return self.emb.shape[0]

    @property
    def forget(self):
        return np.asarray(self.meta["forget"], dtype=bool)

    # -- construction and persistence ---------------------------------------------------------------
    @classmethod
    def build(cls, model, paths, mean=(0.0,), std=(1.0,), batch_size=16, forget=()):
        """Decode with PIL and embed through `model.embed_u8`, in batches over runs of equal image size; the forget images that are
        not among `paths` are appended as flagged rows."""
        from .sscd import _three
        require_kernels()
        files, flags = gallery_files(paths, forget)
        if not files:
            raise ValueError("SSCDIndex.build: no images")
        mean, std = _three(mean, "mean"), _three(std, "std")
        rows, run = [], []

        def flush():
            if run:
                rows.append(model.embed_u8(torch.stack(run), mean, std).clone())
                run.clear()
        for p in files:
            u8 = decode_u8(p)
            if run and (u8.shape != run[0].shape or len(run) >= int(batch_size)):
                flush()
            run.append(u8)
        flush()
        meta = dict(forget=flags, mean=mean, std=std, model_fingerprint=model_fingerprint(model), files_fingerprint=files_fingerprint(files))
        return cls(torch.cat(rows), files, meta)

    def save(self, directory):
        """`index.safetensors` (the rows) and `index.json` (names, flags, dims, mean, std, fingerprints) under `directory`."""
        from safetensors.torch import save_file
        directory = str(directory)
        os.makedirs(directory, exist_ok=True)
        tmp = os.path.join(directory, f"index.safetensors.tmp{os.getpid()}")
        save_file({"emb": self.emb.detach().cpu().contiguous()}, tmp)
        os.replace(tmp, os.path.join(directory, "index.safetensors"))
        with open(os.path.join(directory, "index.json"), "w") as f:
            json.dump(dict(format=FORMAT, n=len(self), names=self.names, **self.meta), f)
        return directory

    @staticmethod
    def exists(directory):
        return all(os.path.exists(os.path.join(str(directory), f)) for f in ("index.safetensors", "index.json"))

    @staticmethod
    def read_meta(directory):
        """index.json of a saved index (names, flags, dims, mean, std, fingerprints) without its rows."""
        with open(os.path.join(str(directory), "index.json")) as f:
            return json.load(f)

    @classmethod
    def load(cls, directory, model=None, device=None, files=None):
        """The index save() wrote.  With `model`: ValueError when it was built by a network of other weights or other dims; with
        `files` (the gallery's files in index order): ValueError when their names, sizes or mtimes are not the recorded ones."""
        from safetensors.torch import load_file
        directory = str(directory)
        with open(os.path.join(directory, "index.json")) as f:
            meta = json.load(f)
        if meta.pop("format", None) != FORMAT:
            raise ValueError(f"{directory}: not an SSCD index of format {FORMAT}")
        names, n = meta.pop("names"), meta.pop("n")
        emb = load_file(os.path.join(directory, "index.safetensors"))["emb"]
        if tuple(emb.shape) != (n, meta["dims"]) or len(names) != n:
            raise ValueError(f"{directory}: index.json describes {n} rows of {meta['dims']}, index.safetensors holds {tuple(emb.shape)}")
        if model is not None:
            if int(model.dims) != meta["dims"]:
                raise ValueError(f"{directory}: an index of {meta['dims']} dims, the model embeds to {model.dims}")
            if meta.get("model_fingerprint") != model_fingerprint(model):
                raise ValueError(f"{directory}: the index was built by another model (fingerprint "
                                 f"{str(meta.get('model_fingerprint'))[:16]}..., this one {model_fingerprint(model)[:16]}...)")
            device = model.device if device is None else device
        if files is not None and ([str(p) for p in files] != names or meta.get("files_fingerprint") != files_fingerprint(files)):
            raise ValueError(f"{directory}: the gallery's files (names, sizes or mtimes) are not the ones the index was built from")
        return cls(emb.to(device if device is not None else "cpu"), names, meta)

    # -- searches -----------------------------------------------------------------------------------
    def topk(self, queries, k, self0=-1):
        return topk(queries, self.emb, k, self0)

    def above(self, queries, thr, self0=-1):
        return above(queries, self.emb, thr, self0)

    def pairs(self, thr, block=QUERY_BLOCK):
        """All pairs i < j of the index with similarity >= thr, as host arrays (i, j, sim) sorted by (i, j): the index against
        itself in query blocks with the self pairs excluded on the device; each unordered pair is kept once, from its smaller row."""
        I, J, V = [], [], []
        n = len(self)
        for s in range(0, n, int(block)):
            off, idx, val = self.above(self.emb[s:s + int(block)], thr, self0=s)
            off, idx, val = off.cpu().numpy(), idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
            rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64) + s, np.diff(off))
            keep = rows < idx
            I.append(rows[keep]); J.append(idx[keep]); V.append(val[keep])
        return np.concatenate(I), np.concatenate(J), np.concatenate(V)

    def components(self, thr, block=QUERY_BLOCK):
        """The connected components (two rows or more, each sorted, ordered by their first row) of the graph of `pairs(thr)`."""
        i, j, _ = self.pairs(thr, block)
        return components(len(self), i, j)


def components(n, i, j):
    """Union-find over the edges (i[e], j[e]) of n nodes: the components of two nodes or more, each sorted, by their first node."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for a in range(n):
        groups.setdefault(find(a), []).append(a)
    return [g for _, g in sorted(groups.items()) if len(g) > 1]


class ReplicationScore:
    """`metrics.sscd_nn` for one rank: how close a set of generated images comes to ANY row of the index.  `record(tag, emb, step)`
    appends {global_step, tag, nn_mean, nn_max, nn_p95 (over the queries' top-1 values, f64 on the host), above (queries with a
    neighbour >= threshold), nn_is_forget (share of queries whose top-1 row is a forget image), nn_other_max (the best similarity to a
    row that is not), top (per query the first k [name, sim])} to `out_path`."""

    extra = None                # fields added to every record (pipeline.sampler: the sampler's name and step count)

    def __init__(self, index, out_path, k=5, threshold=0.5):
        self.index, self.out_path, self.k, self.threshold = index, out_path, int(k), float(threshold)
        if not 1 <= self.k <= MAX_K:
            raise ValueError(f"ReplicationScore: k = {k}, 1 .. {MAX_K}")
        if not np.isfinite(self.threshold):
            raise ValueError(f"ReplicationScore: threshold = {threshold!r} is not a finite number")
        self._others = None

    def _other_best(self, emb, val, idx):
        """Per query the best similarity to a row that is not flagged forget (-inf when there is none), f64 on the host."""
        flags = self.index.forget
        nf = int(flags.sum())
        if nf == 0:
            return val[:, 0]
        if nf + 1 > val.shape[1]:                     # the first k may all be forget rows: ask the other rows alone
            if nf == len(flags):
                return np.full(val.shape[0], -np.inf)
            if self._others is None:
                keep = torch.from_numpy(np.flatnonzero(~flags)).to(self.index.emb.device)
                self._others = self.index.emb[keep].contiguous()
            return topk(emb, self._others, 1)[0][:, 0].cpu().double().numpy()
        other = np.where((idx >= 0) & ~flags[np.maximum(idx, 0)], val, -np.inf)
        return other.max(axis=1)

    def record(self, tag, emb, step, extra=None):
        flags = self.index.forget
        nf = int(flags.sum())
        val, idx = self.index.topk(emb, self.k if nf + 1 > MAX_K else max(self.k, nf + 1))    # (room for one row that is not forget)
        val, idx = val.cpu().double().numpy(), idx.cpu().numpy().astype(np.int64)
        top1 = val[:, 0]
        other = self._other_best(emb, val, idx)
        rec = {"global_step": int(step), "tag": tag if isinstance(tag, str) else int(tag),
               "nn_mean": finite_or_none(top1.mean()), "nn_max": finite_or_none(top1.max()),
               "nn_p95": finite_or_none(np.percentile(top1, 95)) if np.isfinite(top1).all() else None,
               "above": int((top1 >= self.threshold).sum()),
               "nn_is_forget": float(np.mean((idx[:, 0] >= 0) & flags[np.maximum(idx[:, 0], 0)])),
               "nn_other_max": finite_or_none(other.max()),
               "top": [[[self.index.names[j], finite_or_none(v)] for v, j in zip(vr[:self.k], ir[:self.k]) if j >= 0]
                       for vr, ir in zip(val.tolist(), idx.tolist())],
               **(self.extra or {}), **(extra or {})}
        return append_jsonl(self.out_path, rec)


# ---------------------------------------------------------------- the `metrics.sscd_nn` key of the tasks
IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp")
KEYS = ("index_path", "data_path", "k", "threshold", "batch_size")


def list_images(directory):
    """The image files under `directory` (recursively), sorted by path."""
    out = []
    for root, _, files in os.walk(str(directory)):
        out.extend(os.path.join(root, f) for f in files if f.lower().endswith(IMAGE_EXT))
    return sorted(out)


def _refuse_foreign(directory, model):
    """ValueError when the index saved under `directory` was built by a network of other weights or other dims."""
    meta = SSCDIndex.read_meta(directory)
    if meta.get("dims") != int(model.dims) or meta.get("model_fingerprint") != model_fingerprint(model):
        raise ValueError(f"metrics.sscd_nn.index_path {directory!r} holds the index of another model ({meta.get('dims')} dims, fingerprint "
                         f"{str(meta.get('model_fingerprint'))[:16]}...; this one {model.dims} dims, {model_fingerprint(model)[:16]}...): "
                         "remove it or name another directory")


def parse_config(node, need, scorer, default_dir, forget, out_path):
    """`metrics.sscd_nn: {index_path, data_path, k, threshold, batch_size}` (null / absent: None) -> the settings open_index takes.
    A host-side check, before the first step: ValueError for a node that is no mapping or has an unknown field, for the key without
    `need` (the SSCD metric whose `scorer` -- an sscd.SSCDScore -- supplies the network and the transforms), for k outside 1 .. 32, a
    threshold that is not a finite number, a batch_size that is no positive integer and an index_path that holds another model's
    index; FileNotFoundError for a data_path (default `default_dir`) that is no directory with images."""
    if node is None:
        return None
    what = "metrics.sscd_nn"
    if not isinstance(node, dict):
        raise ValueError(f"{what}={node!r}: a mapping {{{', '.join(KEYS)}}} is needed")
    unknown = sorted(set(node) - set(KEYS))
    if unknown:
        raise ValueError(f"{what}: unknown field(s) {unknown}; the fields are {list(KEYS)}")
    if scorer is None:
        raise ValueError(f"{what} needs {need}: the SSCD network and its transforms come from there")
    k, thr, bs = node.get("k", 5), node.get("threshold", 0.5), node.get("batch_size", 16)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}.k={k!r}: an integer in 1 .. {MAX_K} is needed")
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not np.isfinite(thr):
        raise ValueError(f"{what}.threshold={thr!r}: a finite number is needed")
    if not isinstance(bs, int) or isinstance(bs, bool) or bs < 1:
        raise ValueError(f"{what}.batch_size={bs!r}: a positive integer is needed")
    data = node.get("data_path") or default_dir
    if not data or not os.path.isdir(str(data)) or not list_images(data):
        raise FileNotFoundError(f"{what}.data_path {data!r} (the gallery the generated images are searched in) is not a directory with "
                                "images on disk")
    index_path = node.get("index_path")
    if index_path and SSCDIndex.exists(index_path):
        _refuse_foreign(str(index_path), scorer.model)
    return dict(model=scorer.model, mean=scorer.mean, std=scorer.std, data_path=str(data), forget=[str(f) for f in forget if f],
                index_path=str(index_path) if index_path else None, k=k, threshold=float(thr), batch_size=bs, out_path=out_path)


def open_index(s, device):
    """The ReplicationScore of parse_config's settings: the index under index_path when it is there and describes this gallery (the same
    files, sizes, mtimes and transforms; another model's is refused), else built from data_path plus the forget images and saved there."""
    model = s["model"].to(device).eval()
    files, _ = gallery_files(list_images(s["data_path"]), s["forget"])
    d, index = s["index_path"], None
    if d and SSCDIndex.exists(d):
        _refuse_foreign(d, model)
        meta = SSCDIndex.read_meta(d)
        if (meta.get("names") == files and meta.get("files_fingerprint") == files_fingerprint(files)
                and meta.get("mean") == list(s["mean"]) and meta.get("std") == list(s["std"])):
            index = SSCDIndex.load(d, model=model, device=device)
            print(f"[siss_amd] metrics.sscd_nn: index of {len(index)} rows loaded from {d}")
        else:
            print(f"[siss_amd] metrics.sscd_nn: the index under {d} describes other files or transforms: built again")
    if index is None:
        index = SSCDIndex.build(model, list_images(s["data_path"]), s["mean"], s["std"], s["batch_size"], s["forget"])
        print(f"[siss_amd] metrics.sscd_nn: index of {len(index)} rows built from {s['data_path']}"
              + (f", saved to {index.save(d)}" if d else ""))
    return ReplicationScore(index, s["out_path"], s["k"], s["threshold"])


class KeepEmbeddings:
    """An sscd.SSCDScore in a scorer chain (metric_net.score_chain) that keeps the unit rows its one pass made in `.emb`: the same
    launches on the same bytes as SSCDScore.score_decoded / score_u8, so the scores are theirs bit for bit; records go through the
    wrapped scorer."""

    def __init__(self, scorer):
        self.scorer, self.emb = scorer, None

    def score_decoded(self, img):
        s = self.scorer
        self.emb, u8, scores = s.model.embed_decoded(img, s.mean, s.std, ref=s.reference(img.device))
        return scores, u8

    def score_u8(self, u8):
        s = self.scorer
        ref = s.reference(u8.device if torch.is_tensor(u8) and u8.is_cuda else s.model.device)
        self.emb, scores = s.model.embed_u8(u8, s.mean, s.std, ref=ref)
        return scores

    def record(self, *a):
        return self.scorer.record(*a)

    @property
    def extra(self):
        return self.scorer.extra

    @extra.setter
    def extra(self, v):
        self.scorer.extra = v

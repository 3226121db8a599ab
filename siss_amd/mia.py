"""Membership inference attacks on the pixel-space UNet (OPT-IN: `metrics.mia`, tools/mia.py) -- the instrument the unlearning
literature verifies forgetting with, beside the reference's mean eps-MSE diagnostic (siss_amd/membership.py).  Every image gets a
score per attack, LOWER = "more like a member"; the scores are calibrated on holdout images the model never saw (roc_stats /
forget_stats: AUC, TPR at a low FPR, where the forget images fall at that operating point).

  secmi  SecMI (Duan et al., ICML 2023), the t-error of a deterministic DDIM round trip: invert x_0 to level t_sec in steps of
         `stride`, go one step further, come one step back, score ||x^ - x_t||^2.  t_sec / stride + 2 forwards per image.
  pia    PIA (Kong et al., ICLR 2024), the proximal initialisation: e0 = eps(x_0, 0), x_t = sqrt(ab_t) x_0 + sqrt(1 - ab_t) e0, score
         sum |e0 - eps(x_t, t)|^p (the p-th root is monotone and not taken).  Two forwards per image.
  loss   the threshold attack on the training loss: the mean over `noises` shared noises of ||eps(x_t, t) - noise||^2, on the launchers of
         the membership-loss metric (siss_pair_noise / siss_pair_sqerr).

The chains are restated from the papers (the authors' code was not at hand) and pinned to the f64 restatement of tests/mia_ref.py.
One deterministic DDIM transfer between two levels is y = cx x + ce e (transfer_coefficients: formed in f64 from the f32
alphas_cumprod, rounded once to f32); on the device it is one launch of csrc/mia.hip between two forwards.  The N images of an
evaluation lie in one [N, chw] pool; the whole chain of one batch of b rows -- gather, every forward, every transfer, the final f64
reduction -- is captured once per shape into a hipGraph whose only per-batch input is a device scalar (the row offset) and whose
timesteps lie in one constant device table.  No host read between forwards; the scores stay on the device until the caller reads them.
"""
import math
import os
import time

import numpy as np
import torch

from . import lib
from .records import append_jsonl
from .variants import is_int, need_fields, need_int

ATTACKS = ("secmi", "pia", "loss")
DEFAULTS = {"secmi": dict(t_sec=100, stride=10), "pia": dict(t=200, p=4), "loss": dict(t=100, noises=4)}
FIELDS = ("attacks", "step_frequency", "num_members", "num_forget", "batch_size", "holdout", "fpr", "secmi", "pia", "loss", "seed")
EXAMPLE = "{attacks: [secmi, pia], step_frequency: 50}"


# ---------------------------------------------------------------------------------------------------------------- the chains' constants
def transfer_coefficients(ab, kind, t_from, t_to):
    """(cx, ce) of y = cx * x + ce * e as Python floats that hold f32 values.  ab: alphas_cumprod (f32 values).  kind "transfer":
    the deterministic DDIM step from level ab[t_from] to ab[t_to], cx = sqrt(a_to / a_from), ce = sqrt(1 - a_to) -
    sqrt(a_to (1 - a_from) / a_from); kind "noise": x_0 noised to level ab[t_to] with e (t_from is ignored), cx = sqrt(a_to),
    ce = sqrt(1 - a_to).  Formed in f64 from the f32 table, rounded once."""
    ab = np.asarray(ab.detach().cpu() if torch.is_tensor(ab) else ab, dtype=np.float32).astype(np.float64)
    a_to = float(ab[int(t_to)])
    if kind == "noise":
        cx, ce = math.sqrt(a_to), math.sqrt(1.0 - a_to)
    elif kind == "transfer":
        a_from = float(ab[int(t_from)])
        cx, ce = math.sqrt(a_to / a_from), math.sqrt(1.0 - a_to) - math.sqrt(a_to * (1.0 - a_from) / a_from)
    else:
        raise ValueError(f"transfer_coefficients: kind {kind!r} is neither 'transfer' nor 'noise'")
    return float(np.float32(cx)), float(np.float32(ce))


def check_settings(attacks, T, secmi=None, pia=None, loss=None, key="MembershipAttack"):
    """(attacks tuple, {attack: settings with the defaults filled in}); ValueError for an unknown attack or field, a timestep outside
    [0, T), t_sec that is no multiple of stride or leaves no level for the step further, p outside {2, 4}.  Pure host code."""
    if isinstance(attacks, str) or not hasattr(attacks, "__iter__"):
        raise ValueError(f"{key}.attacks={attacks!r}: a list out of {list(ATTACKS)} is needed")
    attacks = tuple(attacks)
    if not attacks or len(set(attacks)) != len(attacks) or any(a not in ATTACKS for a in attacks):
        raise ValueError(f"{key}.attacks={list(attacks)!r}: a non-empty list out of {list(ATTACKS)} without repeats is needed")
    given = {"secmi": secmi, "pia": pia, "loss": loss}
    out = {}
    for name in ATTACKS:
        s = dict(DEFAULTS[name])
        if given[name] is not None:
            s.update(need_fields(f"{key}.{name}", given[name], tuple(DEFAULTS[name]), str(DEFAULTS[name]).replace("'", "")))
        for f, v in s.items():
            need_int(f"{key}.{name}.{f}", v)
        out[name] = s
    T = int(T)
    s = out["secmi"]
    if s["stride"] < 1 or s["t_sec"] < s["stride"] or s["t_sec"] % s["stride"] != 0 or s["t_sec"] + s["stride"] >= T:
        raise ValueError(f"{key}.secmi={s}: t_sec must be a positive multiple of stride with t_sec + stride < num_train_timesteps = {T}")
    for name in ("pia", "loss"):
        if not 0 <= out[name]["t"] < T:
            raise ValueError(f"{key}.{name}.t={out[name]['t']}: outside [0, num_train_timesteps = {T})")
    if out["pia"]["p"] not in (2, 4):
        raise ValueError(f"{key}.pia.p={out['pia']['p']}: 2 or 4 is needed")
    if out["loss"]["noises"] < 1:
        raise ValueError(f"{key}.loss.noises={out['loss']['noises']}: a positive count is needed")
    return attacks, out


# ---------------------------------------------------------------------------------------------------------------- the scores
class MembershipAttack:
    """The attacks on the HIP forward.  `unet` is a siss_amd.model.UNet2DModel (or a UNetEngine).  batch_size: rows per chain (a
    score does not depend on it, nor on which other images share the pool).  use_graph=False runs the same launches eagerly."""

    def __init__(self, unet, noise_scheduler, device, attacks=ATTACKS, batch_size=16, secmi=None, pia=None, loss=None, use_graph=True):
        self.unet, self.noise_scheduler, self.device = unet, noise_scheduler, torch.device(device)
        self.T = int(noise_scheduler.config.num_train_timesteps)
        self.attacks, self.settings = check_settings(attacks, self.T, secmi, pia, loss)
        self.batch_size = need_int("MembershipAttack.batch_size", batch_size, positive=True, what="a positive count")
        self.use_graph = bool(use_graph)
        self._states = {}

    def forwards_per_image(self, attack):
        s = self.settings[attack]
        return s["t_sec"] // s["stride"] + 2 if attack == "secmi" else 2 if attack == "pia" else s["noises"]

    def _engine(self):
        from .unet import UNetEngine
        eng = getattr(self.unet, "engine", self.unet)
        if type(eng) is not UNetEngine:
            raise NotImplementedError(f"{type(eng).__name__}: the membership attacks are built for the unconditional UNet2DModel only "
                                      "(UNetCondEngine: no latent-space form is built)")
        return eng

    # ---- one batch of each attack: every launch between the offset and the sums ---------------------------------------------
    def _secmi(self, eng, st):
        b, chw, n, K = st["b"], st["chw"], st["n"], st["K"]
        cur, nxt = st["xa"], st["xb"]
        lib.call("siss_mia_gather", st["pool"], st["offset"], n, b, chw, cur)
        for k in range(K + 1):                                    # the inversion to t_sec, then one step further
            e = eng.forward(cur, st["ts"][k])
            lib.call("siss_mia_transfer", cur, e, None, b, b, chw, *st["coef"][k], nxt, None)
            cur, nxt = nxt, cur
        e = eng.forward(cur, st["ts"][K + 1])                     # cur = x~, nxt = x_t: one step back, against x_t
        lib.call("siss_mia_transfer_sqerr", cur, e, nxt, st["offset"], n, b, chw, *st["coef"][K + 1], st["sums"], st["partials"])

    def _pia(self, eng, st):
        b, chw, n = st["b"], st["chw"], st["n"]
        lib.call("siss_mia_gather", st["pool"], st["offset"], n, b, chw, st["xa"])
        e0 = eng.forward(st["xa"], st["ts"][0])
        # x_t from the pool's own rows; e0 is kept, the engine's prediction buffer is overwritten by the next forward
        lib.call("siss_mia_transfer", st["pool"], e0, st["offset"], n, b, chw, *st["coef"][0], st["xb"], st["e0"])
        e1 = eng.forward(st["xb"], st["ts"][1])
        lib.call("siss_mia_powdiff", st["e0"], e1, st["offset"], n, b, chw, st["p"], st["sums"], st["partials"])

    def _loss(self, eng, st):
        b, chw = st["b"], st["chw"]
        lib.call("siss_pair_noise", st["pool"], st["noise"], st["items"], st["offset"], st["n_items"], st["n"], st["noise"].shape[0],
                 st["ac"], st["ac"].numel(), b, chw, st["xa"], st["tsl"])
        pred = eng.forward(st["xa"], st["tsl"])
        lib.call("siss_pair_sqerr", pred, st["noise"], st["items"], st["offset"], st["n_items"], st["noise"].shape[0], b, chw,
                 st["sums"], st["partials"])

    def _state(self, attack, shape, n):
        """The fixed-address buffers (and, once captured, the graph) of one (attack, image shape, pool size)."""
        key = (attack, shape, n, self.use_graph)
        st = self._states.get(key)
        if st is not None:
            return st
        dev, b, s = self.device, self.batch_size, self.settings[attack]
        chw = int(np.prod(shape))
        ab = self.noise_scheduler.alphas_cumprod
        f32 = lambda *sz: torch.zeros(sz, dtype=torch.float32, device=dev)
        st = dict(b=b, chw=chw, n=n, graph=None, body=getattr(self, "_" + attack), pool=f32(n, chw), xa=f32(b, *shape), xb=f32(b, *shape),
                  offset=torch.zeros(1, dtype=torch.long, device=dev))
        if attack == "secmi":
            t_sec, stride = s["t_sec"], s["stride"]
            levels = list(range(0, t_sec + stride, stride))        # 0, stride, ..., t_sec: every transfer goes one level up ...
            steps = [(a, a + stride) for a in levels] + [(t_sec + stride, t_sec)]             # ... and the last one comes back
            st.update(K=t_sec // stride, coef=[transfer_coefficients(ab, "transfer", a, c) for a, c in steps],
                      ts=torch.tensor([[a] * b for a, _ in steps], dtype=torch.long, device=dev))
        elif attack == "pia":
            st.update(coef=[transfer_coefficients(ab, "noise", None, s["t"])], p=s["p"], e0=f32(b, chw),
                      ts=torch.tensor([[0] * b, [s["t"]] * b], dtype=torch.long, device=dev))
        else:
            J = s["noises"]
            items = [(i, j, s["t"]) for i in range(n) for j in range(J)]
            st.update(n_items=n * J, noise=f32(J, chw), items=torch.tensor(items, dtype=torch.long, device=dev),
                      ac=ab.to(dev, torch.float32).contiguous(), tsl=torch.zeros(b, dtype=torch.long, device=dev))
        rows = st.get("n_items", n)
        words = int(lib.query("siss_pair_partials_words" if attack == "loss" else "siss_mia_partials_words", b, chw))
        st.update(rows=rows, sums=torch.zeros(rows, dtype=torch.float64, device=dev),
                  partials=torch.zeros(words, dtype=torch.float64, device=dev))
        self._states[key] = st
        return st

    def _capture(self, eng, st):
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st["body"](eng, st)                                   # settle every buffer of this shape before the capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                st["body"](eng, st)
        torch.cuda.current_stream().wait_stream(side)
        st["graph"] = graph

    @torch.no_grad()
    def scores(self, images, generator=None):
        """{attack: f64 [N] on the device}, lower = more member-like.  images: [N, C, H, W] f32.  generator: the device generator the
        `loss` attack's shared noises are drawn from (else the global one); the other attacks are deterministic.  No host
        synchronisation in here: reading the scores is the caller's."""
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f"scores: images of shape {tuple(images.shape)}; [N, C, H, W] with N >= 1 is needed")
        eng = self._engine()
        images = images.to(self.device, torch.float32).contiguous()
        n, shape = int(images.shape[0]), tuple(images.shape[1:])
        eng.refresh_weights(cast_shadow=True)                     # the master may have been stepped since the last evaluation
        out = {}
        self.forwards = {}
        for attack in self.attacks:
            st = self._state(attack, shape, n)
            st["pool"].copy_(images.reshape(n, -1))
            if attack == "loss":
                st["noise"].copy_(torch.randn((st["noise"].shape[0], *shape), device=self.device, generator=generator).reshape(st["noise"].shape))
            if self.use_graph and st["graph"] is None:
                self._capture(eng, st)
            for off in range(0, st["rows"], st["b"]):
                st["offset"].fill_(off)
                if self.use_graph:
                    st["graph"].replay()
                else:
                    st["body"](eng, st)
            self.forwards[attack] = -(-st["rows"] // st["b"]) * (1 if attack == "loss" else self.forwards_per_image(attack))
            out[attack] = st["sums"].view(n, -1).mean(dim=1) if attack == "loss" else st["sums"].clone()
        return out


# ---------------------------------------------------------------------------------------------------------------- the statistics
def _f64(scores, what):
    s = np.asarray(scores.detach().cpu() if torch.is_tensor(scores) else scores, dtype=np.float64).reshape(-1)
    if s.size == 0 or not np.isfinite(s).all():
        raise ValueError(f"{what}: {s.size} scores, {int((~np.isfinite(s)).sum())} of them not finite")
    return s


def fpr_key(alpha):
    return f"{float(alpha):g}"


def operating_threshold(holdout, alpha):
    """The (k + 1)-th smallest holdout score, k = floor(alpha * n_h): an image is flagged as a member iff its score lies STRICTLY below
    it, so at most k holdout images are flagged, ties included -- the realised FPR never exceeds alpha.  With n_h < 1 / alpha this is
    the smallest holdout score."""
    h = np.sort(_f64(holdout, "holdout"))
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"fpr={alpha!r}: a level in (0, 1) is needed")
    k = int(math.floor(float(alpha) * h.size + 1e-9))             # (0.29 * 100 is 28.999...: the level's own count, not one below)
    return float(h[k])


def _pair_counts(s, h_sorted):
    """Per score: (#holdout strictly below, #holdout equal) -- exact integers."""
    lo, hi = np.searchsorted(h_sorted, s, side="left"), np.searchsorted(h_sorted, s, side="right")
    return lo.astype(np.int64), (hi - lo).astype(np.int64)


def _auc(s, h_sorted):
    below, equal = _pair_counts(s, h_sorted)
    above = h_sorted.size - below - equal                        # holdout scores strictly above: the pairs the attack orders rightly
    return (int(above.sum()) + 0.5 * int(equal.sum())) / (s.size * h_sorted.size)


def roc_stats(member, holdout, fpr=(0.01, 0.001)):
    """{"auc", "tpr_at_fpr_<a>" per level}: auc = (#{s_m < s_h} + 0.5 #{s_m = s_h}) / (n_m n_h) by exact counting; tpr_at_fpr is the
    share of the members flagged at operating_threshold(holdout, a)."""
    m, h = _f64(member, "member"), np.sort(_f64(holdout, "holdout"))
    out = {"auc": _auc(m, h)}
    for a in fpr:
        out[f"tpr_at_fpr_{fpr_key(a)}"] = int((m < operating_threshold(h, a)).sum()) / m.size
    return out


def forget_stats(forget, holdout, fpr=(0.01, 0.001)):
    """{"forget_auc", "forget_flagged_at_fpr_<a>" per level, "forget_percentile"}: roc_stats' auc and flagged share with the forget
    images in the members' place, and the mean over the forget images of the share of holdout scores below theirs (ties count 0.5):
    0 = every forget image looks more member-like than every holdout image, 0.5 = indistinguishable from unseen images."""
    f, h = _f64(forget, "forget"), np.sort(_f64(holdout, "holdout"))
    below, equal = _pair_counts(f, h)
    out = {"forget_auc": _auc(f, h)}
    for a in fpr:
        out[f"forget_flagged_at_fpr_{fpr_key(a)}"] = int((f < operating_threshold(h, a)).sum()) / f.size
    out["forget_percentile"] = (int(below.sum()) + 0.5 * int(equal.sum())) / (f.size * h.size)
    return out


def calibrated_keys(fpr):
    """The fields of roc_stats and forget_stats, in a record's order."""
    return (["auc"] + [f"tpr_at_fpr_{fpr_key(a)}" for a in fpr] + ["forget_auc"] + [f"forget_flagged_at_fpr_{fpr_key(a)}" for a in fpr] +
            ["forget_percentile"])


# ---------------------------------------------------------------------------------------------------------------- the config key
def parse_config(mia, T, need_frequency=True):
    """`metrics.mia` checked and with its defaults filled in (pure host code; raises before anything is loaded):
    {attacks, step_frequency, num_members, num_forget, batch_size, holdout: null | {path, limit}, fpr, secmi, pia, loss, seed}."""
    key = "metrics.mia"
    c = need_fields(key, mia, FIELDS, EXAMPLE)
    out = dict(step_frequency=c.get("step_frequency"), num_members=c.get("num_members", 64), num_forget=c.get("num_forget", 16),
               batch_size=c.get("batch_size", 16), seed=c.get("seed", 0))
    for f in ("num_members", "num_forget", "batch_size") + (("step_frequency",) if need_frequency else ()):
        need_int(f"{key}.{f}", out[f], positive=True, what="a positive count")
    need_int(f"{key}.seed", out["seed"])
    attacks = c.get("attacks", list(ATTACKS))
    plain = lambda v: dict(v) if hasattr(v, "keys") else v
    out["attacks"], out["settings"] = check_settings(list(attacks) if isinstance(attacks, (list, tuple)) else attacks, T,
                                                     plain(c.get("secmi")), plain(c.get("pia")), plain(c.get("loss")), key=key)
    fpr = c.get("fpr", [0.01, 0.001])
    if not isinstance(fpr, (list, tuple)) or not fpr or any(isinstance(a, bool) or not isinstance(a, (int, float)) or not 0 < a < 1 for a in fpr):
        raise ValueError(f"{key}.fpr={fpr!r}: a non-empty list of levels in (0, 1) is needed")
    out["fpr"] = [float(a) for a in fpr]
    ho = c.get("holdout")
    if ho is not None:
        ho = need_fields(f"{key}.holdout", ho, ("path", "limit"), "{path: data/holdout, limit: 256}")
        ho = dict(path=ho.get("path"), limit=ho.get("limit", 256))
        if ho["path"] is not None and not isinstance(ho["path"], str):
            raise ValueError(f"{key}.holdout.path={ho['path']!r}: null, a directory of images or an .npz file is needed")
        need_int(f"{key}.holdout.limit", ho["limit"], positive=True, what="a positive count")
    out["holdout"] = ho
    return out


def load_holdout(path, limit, transform, channels, image_key="image"):
    """[n, C, H, W] f32: up to `limit` images the model never trained on, through the task's own transform.  path: a directory of
    image files (sorted by name), or an .npz whose `image` is uint8 [N, H, W] or [N, H, W, C] as HFDataset reads it."""
    if str(path).endswith(".npz") and os.path.isfile(str(path)):
        with np.load(str(path)) as z:
            raw = list(z[image_key][:limit])
    elif os.path.isdir(str(path)):
        from PIL import Image
        names = sorted(f for f in os.listdir(str(path)) if f.lower().endswith((".jpg", ".jpeg", ".png")))[:limit]
        raw = [Image.open(os.path.join(str(path), f)).convert("RGB" if channels == 3 else "L") for f in names]
    else:
        raise FileNotFoundError(f"metrics.mia.holdout.path {path!r} is neither a directory of images nor an .npz file on disk")
    if not raw:
        raise FileNotFoundError(f"metrics.mia.holdout.path {path!r} holds no images")
    return torch.stack([transform(r) if transform is not None else torch.as_tensor(r) for r in raw]).float()


def unique_in_order(indices):
    """The indices with repeats dropped, first occurrences kept (a forget set that repeats one image is scored once)."""
    return list(dict.fromkeys(int(i) for i in indices))


def draw_members(n_keep, num_members, seed):
    """num_members distinct indices of the keep dataset from a generator of their own (no other stream is touched)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randperm(int(n_keep), generator=g)[:min(int(num_members), int(n_keep))].tolist()


# ---------------------------------------------------------------------------------------------------------------- one evaluation
class MiaEvaluation:
    """The groups of one run (member / forget / holdout images, drawn once) and the evaluation the hook and tools/mia.py share: all
    groups in ONE pool, one scores() call, one host read, the statistics, one record."""

    def __init__(self, attack, members, forget, holdout, fpr, seed, path):
        self.attack, self.fpr, self.seed, self.path = attack, list(fpr), int(seed), path
        self.sizes = (int(members.shape[0]), int(forget.shape[0]), 0 if holdout is None else int(holdout.shape[0]))
        self.pool = torch.cat([g.float() for g in (members, forget, holdout) if g is not None]).to(attack.device).contiguous()

    def __call__(self, global_step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen = torch.Generator(device=self.attack.device).manual_seed(self.seed + 1)       # every evaluation: the same shared noises
        scores = self.attack.scores(self.pool, generator=gen)
        host = torch.stack([scores[a] for a in self.attack.attacks]).cpu().numpy()          # the one host read
        nm, nf, nh = self.sizes
        rec = dict(global_step=int(global_step), seconds=time.perf_counter() - t0, members=nm, forget=nf, holdout=nh)
        for a, s in zip(self.attack.attacks, host):
            m, f, h = s[:nm], s[nm:nm + nf], s[nm + nf:]
            if nh:
                stats = {**roc_stats(m, h, self.fpr), **forget_stats(f, h, self.fpr)}
            else:
                stats = dict.fromkeys(calibrated_keys(self.fpr))              # no holdout: the calibrated fields are null
            rec.update({f"{a}_{k}": v for k, v in stats.items()})
            rec.update({f"{a}_member_mean": float(m.mean()), f"{a}_forget_mean": float(f.mean()),
                        f"{a}_holdout_mean": float(h.mean()) if nh else None})
        append_jsonl(self.path, rec)
        say = ", ".join(f"{a}: " + (f"auc {rec[f'{a}_auc']:.3f}, forget percentile {rec[f'{a}_forget_percentile']:.3f}" if nh else
                                    f"forget / member mean {rec[f'{a}_forget_mean'] / rec[f'{a}_member_mean']:.4f}")
                        for a in self.attack.attacks)
        print(f"[siss_amd] membership attacks at step {global_step}: {say} ({rec['seconds']:.1f} s)")
        return rec

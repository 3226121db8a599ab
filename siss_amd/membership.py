"""Membership loss (the reference's ``metrics.class_membership.MembershipLoss``): the LiRA-style probe "does the model still fit the
forget images better than the images it keeps".  For ``num_image_samples`` kept images, as many forget images, ``num_noise_samples``
shared noises and a list of timesteps, every (image, noise) pair is noised, run through the UNet, and
``sum_chw (eps_theta(x_t, t) - noise)^2`` is averaged over the pairs of the kept group and of the forget group.

The reference expands images and noises to three ``I * J * C * H * W`` tensors per timestep and walks them in batches of
``eval_batch_size`` with a concatenation and a host read per timestep.  Here the whole evaluation -- both groups, every timestep --
is ONE flat device table of work items ``(image row, noise row, timestep)`` (``build_work_table``), consumed ``b`` items per forward:

  * ``siss_pair_noise`` writes the forward's input rows straight from the [I, C, H, W] images and the [J, C, H, W] noises,
  * the UNet forward runs on the model's own engine,
  * ``siss_pair_sqerr`` leaves each item's sum in an f64 device vector,

the three captured once per shape into a hipGraph whose only per-forward input is a device scalar (the offset into the table).
Nothing is expanded, nothing is read by the host between forwards.  Forget rows that repeat a dataset index (every shipped delete
config has ONE forget image) are computed once and their sums shared (``dedupe``): identical inputs, so this is exact.
"""
import random

import numpy as np
import torch

from . import lib
from .records import append_jsonl


def build_work_table(all_indices, deletion_indices, num_noise_samples, timesteps, dedupe=True):
    """The work items of one evaluation and where each (timestep, group, image, noise) pair finds its sum.  Pure host code.

    all_indices / deletion_indices: the dataset indices of the sampled kept / forget images, in sampling order (I each).  The image
    pool the table indexes is the I kept images followed by the I forget images (rows 0 .. 2I - 1).
    Returns (items, pair_item): items int64 [n, 3] = (image row, noise row, timestep), ordered timestep-major, then group (kept,
    forget), then image, then noise; pair_item int64 [len(timesteps), 2, I, J] = the item holding that pair's sum.  With dedupe, an
    image of a group whose dataset index already appeared in that group adds no items: its pairs point at the first one's."""
    I, J = len(all_indices), int(num_noise_samples)
    if len(deletion_indices) != I:
        raise ValueError(f"{I} kept and {len(deletion_indices)} forget images: the two groups must be of one size")
    if I <= 0 or J <= 0 or len(timesteps) == 0:
        raise ValueError("membership loss needs at least one image, one noise and one timestep")
    items = []
    pair_item = np.empty((len(timesteps), 2, I, J), dtype=np.int64)
    for ti, t in enumerate(timesteps):
        for g, indices in enumerate((all_indices, deletion_indices)):
            first = {}
            for i, idx in enumerate(indices):
                key = int(idx) if dedupe else i
                if key not in first:
                    first[key] = len(items)
                    items.extend((g * I + i, j, int(t)) for j in range(J))
                pair_item[ti, g, i] = np.arange(first[key], first[key] + J)
    return np.asarray(items, dtype=np.int64).reshape(-1, 3), pair_item


class MembershipLoss:
    """metrics.class_membership.MembershipLoss on the HIP forward.  `unet` is a siss_amd.model.UNet2DModel (or a UNetEngine).

    eval_batch_size is the number of work items per forward unless pairs_per_forward is given (a pair's sum does not depend on which
    other pairs share its forward).  use_graph=False launches every forward eagerly."""

    def __init__(self, dataset_all, dataset_deletion, noise_scheduler, unet, num_image_samples, num_noise_samples, eval_batch_size,
                 device, pairs_per_forward=None, dedupe=True, use_graph=True):
        self.dataset_all, self.dataset_deletion = dataset_all, dataset_deletion
        self.noise_scheduler, self.unet = noise_scheduler, unet
        self.num_image_samples, self.num_noise_samples = int(num_image_samples), int(num_noise_samples)
        self.eval_batch_size = int(eval_batch_size)
        self.device = torch.device(device)
        self.pairs_per_forward = int(pairs_per_forward) if pairs_per_forward else self.eval_batch_size
        if self.pairs_per_forward <= 0:
            raise ValueError(f"pairs_per_forward / eval_batch_size = {self.pairs_per_forward}: a positive count is needed")
        self.dedupe, self.use_graph = bool(dedupe), bool(use_graph)
        self.pair_sums = self.means = None
        self._graphs = {}

    # ---- sampling (class_membership.py:30-66) ---------------------------------------------------
    def sample_images(self):
        """random.sample over the two datasets, in the reference's order of draws (Python's global `random`); a forget set of
        length 1 is index 0 repeated."""
        n_all, n_del = len(self.dataset_all), len(self.dataset_deletion)
        self.all_indices = random.sample(range(n_all), self.num_image_samples)
        if n_del == 1:
            self.deletion_indices = [0] * self.num_image_samples
        else:
            self.deletion_indices = random.sample(range(n_del), self.num_image_samples)
        stack = lambda ds, idx: torch.stack([ds[i] for i in idx], dim=0).to(self.device).float().contiguous()
        self.all_sampled_images = stack(self.dataset_all, self.all_indices)
        self.deletion_sampled_images = stack(self.dataset_deletion, self.deletion_indices)

    def sample_noises(self, generator=None):
        """[J, C, H, W] f32 on the device (sample_images first).  generator: a device generator (else the global one)."""
        self.noise = torch.randn((self.num_noise_samples, *self.all_sampled_images.shape[1:]), device=self.device, generator=generator)

    # ---- the evaluation -------------------------------------------------------------------------
    def _engine(self):
        from .unet import UNetEngine
        eng = getattr(self.unet, "engine", self.unet)
        if type(eng) is not UNetEngine:
            raise NotImplementedError(f"{type(eng).__name__}: the membership loss is built for the unconditional UNet2DModel only "
                                      "(UNetCondEngine: the reference's SD task has no such metric)")
        return eng

    def _body(self, eng, st):
        b, chw = st["b"], st["chw"]
        lib.call("siss_pair_noise", st["pool"], st["noise"], st["items"], st["offset"], st["n_items"], st["pool"].shape[0],
                 st["noise"].shape[0], st["ac"], st["ac"].numel(), b, chw, st["xs"], st["ts"])
        pred = eng.forward(st["xs"], st["ts"])
        lib.call("siss_pair_sqerr", pred, st["noise"], st["items"], st["offset"], st["n_items"], st["noise"].shape[0], b, chw,
                 st["sums"], st["partials"])

    def _state(self, eng, n_items):
        """The fixed-address buffers one (items per forward, image shape, table length) runs on, with its captured graph."""
        shape = tuple(self.all_sampled_images.shape[1:])
        b = self.pairs_per_forward
        key = (b, shape, n_items, self.use_graph)
        st = self._graphs.get(key)
        if st is None:
            dev, I = self.device, self.num_image_samples
            chw = int(np.prod(shape))
            st = dict(b=b, chw=chw, n_items=n_items,
                      pool=torch.zeros(2 * I, chw, dtype=torch.float32, device=dev),
                      noise=torch.zeros(self.num_noise_samples, chw, dtype=torch.float32, device=dev),
                      items=torch.zeros(n_items, 3, dtype=torch.long, device=dev),
                      offset=torch.zeros(1, dtype=torch.long, device=dev),
                      ac=self.noise_scheduler.alphas_cumprod.to(dev, torch.float32).contiguous(),
                      xs=torch.zeros((b, *shape), dtype=torch.float32, device=dev),
                      ts=torch.zeros(b, dtype=torch.long, device=dev),
                      sums=torch.zeros(n_items, dtype=torch.float64, device=dev),
                      partials=torch.zeros(int(lib.query("siss_pair_partials_words", b, chw)), dtype=torch.float64, device=dev),
                      graph=None)
            self._graphs[key] = st
        return st

    def _capture(self, eng, st):
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._body(eng, st)                           # settle every buffer of this shape before the capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                self._body(eng, st)
        torch.cuda.current_stream().wait_stream(side)
        st["graph"] = graph

    @torch.no_grad()
    def compute_membership_losses(self, timesteps):
        """[[all_membership_loss, deletion_membership_loss], ...] per timestep (0-d f32 device tensors: the means over the I * J pairs
        of each group); self.pair_sums holds every pair's sum, f64 [len(timesteps), 2, I, J] (image-major, noise-minor), and
        self.means the group means in f64 [len(timesteps), 2].  No host synchronisation in here: reading the result is the caller's."""
        assert self.all_sampled_images.shape == self.deletion_sampled_images.shape
        timesteps = [int(t) for t in timesteps]
        T = int(self.noise_scheduler.config.num_train_timesteps)
        if not timesteps or min(timesteps) < 0 or max(timesteps) >= T:
            raise ValueError(f"timesteps {timesteps}: a non-empty list within [0, {T}) is needed")
        eng = self._engine()
        items, pair_item = build_work_table(self.all_indices, self.deletion_indices, self.num_noise_samples, timesteps, self.dedupe)
        n_items = int(items.shape[0])
        st = self._state(eng, n_items)
        I = self.num_image_samples
        st["pool"][:I].copy_(self.all_sampled_images.reshape(I, -1))
        st["pool"][I:].copy_(self.deletion_sampled_images.reshape(I, -1))
        st["noise"].copy_(self.noise.reshape(self.num_noise_samples, -1))
        st["items"].copy_(torch.from_numpy(items))
        eng.refresh_weights(cast_shadow=True)             # the master may have been stepped since the last evaluation
        if self.use_graph and st["graph"] is None:
            self._capture(eng, st)
        for off in range(0, n_items, st["b"]):
            st["offset"].fill_(off)
            if self.use_graph:
                st["graph"].replay()
            else:
                self._body(eng, st)
        self.forwards = -(-n_items // st["b"])
        self.pair_sums = st["sums"][torch.from_numpy(pair_item).to(self.device)]
        self.means = self.pair_sums.mean(dim=(2, 3))
        out = self.means.float()
        return [[out[i, 0], out[i, 1]] for i in range(len(timesteps))]


def log_membership(metric, timesteps, global_step, path):
    """One evaluation, appended to `path` as a JSON line with the reference's wandb keys (delete_celeb.py:516-518): one host read."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metric.compute_membership_losses(timesteps)
    means = metric.means.cpu()
    rec = dict(global_step=int(global_step), seconds=time.perf_counter() - t0)
    for i, t in enumerate(timesteps):
        a, d = float(means[i, 0].float()), float(means[i, 1].float())
        rec[f"all_membership_loss_t={int(t)}"] = a
        rec[f"deletion_membership_loss_t={int(t)}"] = d
        rec[f"membership_ratio_t={int(t)}"] = d / a
    append_jsonl(path, rec)
    print(f"[siss_amd] membership loss at step {global_step}: " +
          ", ".join(f"t={int(t)}: ratio {rec[f'membership_ratio_t={int(t)}']:.4f}" for t in timesteps) + f" ({rec['seconds']:.1f} s)")
    return rec

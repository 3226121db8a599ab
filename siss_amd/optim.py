"""Flat-buffer norm-fix + recombine + clip + AdamW (HIP).  Mirrors the semantics of
delete_celeb.py:714-773 (reference) in two streaming passes; see csrc/optimizer.hip."""
import torch

from . import lib
from .variants import SHARD, exclusive

MODE_NORM_FIX, MODE_ERASEDIFF, MODE_NORM_FIX_INF_GUARD = 0, 1, 2
EMA_STEP, EMA_ONE_MINUS_DECAY, EMA_DECAY = 5, 6, 7        # slots of the single-set block (csrc/train_state.hip TrainScalars)


def _mode_knob(scaling_norm, eta, inf_guard):
    """(mode, knob) of pass 1: eta selects EraseDiff's recombination, else the norm fix with or without the inf guard."""
    if eta is not None:
        return MODE_ERASEDIFF, float(eta)
    return (MODE_NORM_FIX_INF_GUARD if inf_guard else MODE_NORM_FIX), float(scaling_norm)


class FlatAdamW:
    """torch.optim.AdamW semantics over ONE flat f32 parameter buffer, fed with the flat
    gradient pair [g_x ; g_a].  All step scalars stay on the device (graph-replay safe)."""

    def __init__(self, flat_params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 max_grad_norm=1.0, shadow=None):
        assert flat_params.dtype == torch.float32 and flat_params.is_cuda and flat_params.dim() == 1
        self.p = flat_params
        self.m = torch.zeros_like(flat_params)
        self.v = torch.zeros_like(flat_params)
        self.lr, self.betas, self.eps, self.wd = float(lr), tuple(betas), float(eps), float(weight_decay)
        self.max_grad_norm = float(max_grad_norm)
        self.shadow = shadow                       # optional bf16 copy of p, refreshed every step
        dev = flat_params.device
        self.partials = torch.zeros(lib.query("siss_opt_partials_words"), dtype=torch.float64, device=dev)
        self.scalars = torch.zeros(lib.query("siss_opt_scalars_words"), dtype=torch.float32, device=dev)
        self.last_grad = None

    def launch(self, grads, *, scaling_norm=None, eta=None, inf_guard=False, want_grad=False, ranges=None, mask=None, ewc=None,
               surgery=None, fixed_weight=None):
        """Enqueue both passes (no host sync).  grads: [2, P] f32 = (g_x, g_a).  ranges: (device table, stretches, granules) of a
        trainable subset (siss_amd.trainable.Subset.table) -- norms, scaling factor, clip and update over the listed stretches
        only, every other byte of p / m / v / shadow untouched; the caller keeps the table alive (a captured step holds its address).
        mask: the packed words of a siss_amd.saliency.SaliencyMask over this buffer (int32, one bit per float) -- the same passes on
        the elements whose bit is set (csrc/saliency.hip); the caller keeps the words alive likewise.
        ewc: a siss_amd.ewc.FisherAnchor over this buffer -- pass 1 folds strength * F * (p - pstar) into the keep-side set first
        (csrc/ewc.hip) and grads[0] IS OVERWRITTEN with g_x + that term; pass 2 is the plain one.  Not with ranges / mask; the caller
        keeps the anchor alive likewise.
        surgery: a siss_amd.surgery.Surgery over this buffer -- both passes are those of csrc/surgery.hip: per group of the buffer the
        conflicting component of the pair is projected out before the norm fix (not with eta: EraseDiff's mode is refused).  Not with
        the other three; the caller keeps the object alive likewise.
        fixed_weight: a positive float w -- the teacher-target objective's plain weighted sum g = clip (g_x + w g_a): pass 1 is
        siss_grad_norms_weighted (csrc/teacher.hip: the scaling factor fixed at s = -w; scaling_norm and inf_guard are not read), pass 2
        the plain one.  Not with ranges / mask / ewc / surgery / eta: their pass 1 has no weighted form."""
        n = self.p.numel()
        assert grads.dtype == torch.float32 and grads.shape == (2, n) and grads.is_contiguous()
        if fixed_weight is not None:
            return self._launch_weighted(grads, fixed_weight, want_grad, {"surgery=": surgery, "ewc=": ewc, "mask=": mask,
                                                                          "ranges=": ranges, "eta=": eta})
        mode, knob = _mode_knob(scaling_norm, eta, inf_guard)
        exclusive("FlatAdamW.launch", {"surgery=": surgery, "ranges=": ranges, "mask=": mask, "ewc=": ewc})
        if surgery is not None:
            return self._launch_surgery(grads, surgery, mode, knob, want_grad)
        # pass 1 takes (gx, ga, *head, mode .. partials, *tail, scalars), pass 2 (gx .. g_out, n, *sel, lr .. scalars)
        one, two, head, tail, sel = "siss_grad_norms_scale", "siss_recombine_clip_adamw", None, (), ()
        if ewc is not None:
            self._ewc_check(ewc)
            one, head, tail = "siss_grad_norms_scale_ewc", (self.p, ewc.pstar, ewc.fisher, n, ewc.strength), (self.ewc_partials,)
        elif mask is not None:
            if mask is not getattr(self, "_mask_checked", None):      # once per mask, not per step
                for name in ("siss_grad_norms_scale_masked", "siss_recombine_clip_adamw_masked"):
                    if not lib.has(name):
                        raise RuntimeError(f"this libsiss_hip.so has no {name}: a saliency mask needs the masked kernels of "
                                           "csrc/saliency.hip (there is no fall-back to the full update)")
                if not (mask.dtype == torch.int32 and mask.device == self.p.device and mask.dim() == 1 and mask.is_contiguous()
                        and mask.numel() == (n + 31) // 32 and mask.data_ptr() % 16 == 0):
                    raise ValueError(f"FlatAdamW.launch(mask=...): {(n + 31) // 32} contiguous int32 words on {self.p.device}, 16-byte "
                                     f"aligned, are needed (one bit per float of the buffer); got {tuple(mask.shape)} {mask.dtype} on "
                                     f"{mask.device} at offset {mask.data_ptr() % 16} of a 16-byte line")
                self._mask_checked = mask
            one, two, sel = "siss_grad_norms_scale_masked", "siss_recombine_clip_adamw_masked", (mask,)
        elif ranges is not None:
            if not lib.has("siss_recombine_clip_adamw_ranges"):
                raise RuntimeError("this libsiss_hip.so has no siss_recombine_clip_adamw_ranges: a trainable subset needs the "
                                   "subset kernels of csrc/optimizer.hip (there is no fall-back to the full update)")
            tab, nr, granules = ranges
            assert tab.dtype == torch.int64 and tab.device == self.p.device and tab.numel() == 2 * nr + 1 and n % 4 == 0
            one, two, sel = "siss_grad_norms_scale_ranges", "siss_recombine_clip_adamw_ranges", (tab, nr, granules)
        if want_grad and (self.last_grad is None):
            # (ranges / mask write their stretches / set bits only: zero elsewhere)
            self.last_grad = torch.zeros_like(self.p) if sel else torch.empty_like(self.p)
        lib.call(one, grads[0], grads[1], *(head or (n, *sel)), mode, knob, self.max_grad_norm, self.betas[0], self.betas[1],
                 self.partials, *tail, self.scalars)
        lib.call(two, grads[0], grads[1], self.p, self.m, self.v, self.shadow, self.last_grad if want_grad else None, n, *sel,
                 self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.scalars)

    def _launch_weighted(self, grads, weight, want_grad, others):
        """Pass 1 of csrc/teacher.hip (s = -weight), then the plain pass 2."""
        from .teacher import fixed_weight_exclusive, require_kernels
        fixed_weight_exclusive("FlatAdamW.launch", others)
        weight = float(weight)
        if not (0.0 < weight < float("inf")):
            raise ValueError(f"FlatAdamW.launch(fixed_weight={weight!r}): a positive finite weight is needed")
        require_kernels()
        n = self.p.numel()
        if want_grad and (self.last_grad is None):
            self.last_grad = torch.empty_like(self.p)
        lib.call("siss_grad_norms_weighted", grads[0], grads[1], n, weight, self.max_grad_norm, self.betas[0], self.betas[1],
                 self.partials, self.scalars)
        lib.call("siss_recombine_clip_adamw", grads[0], grads[1], self.p, self.m, self.v, self.shadow,
                 self.last_grad if want_grad else None, n, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.scalars)

    def _launch_surgery(self, grads, sg, mode, knob, want_grad):
        """Both passes of csrc/surgery.hip on the plan and the slabs `sg` owns."""
        self._surgery_check(sg)
        if mode == MODE_ERASEDIFF:
            raise ValueError("FlatAdamW.launch(surgery=..., eta=...): gradient surgery runs with the norm fix; EraseDiff's s <= 0 is "
                             "that mode's own conflict rule")
        n = self.p.numel()
        if want_grad and (self.last_grad is None):
            self.last_grad = torch.empty_like(self.p)
        lib.call("siss_grad_norms_scale_surgery", grads[0], grads[1], n, sg.group_offsets, sg.groups, sg.plan, sg.jobs, sg.smode, mode,
                 knob, self.max_grad_norm, self.betas[0], self.betas[1], sg.partials, sg.group_sums, sg.coef, self.scalars)
        lib.call("siss_recombine_clip_adamw_surgery", grads[0], grads[1], self.p, self.m, self.v, self.shadow,
                 self.last_grad if want_grad else None, n, sg.group_offsets, sg.groups, sg.plan, sg.jobs, sg.coef, self.lr,
                 self.betas[0], self.betas[1], self.eps, self.wd, self.scalars)

    def _surgery_check(self, sg):
        """Once per object, not per step: the kernels are there and the plan covers this buffer on its device (before a step is
        captured: SISSStepper.set_surgery calls this)."""
        if sg is getattr(self, "_surgery_checked", None):
            return
        from .surgery import require_kernels
        require_kernels()
        n = self.p.numel()
        if not (sg.total == n and sg.offsets[0] == 0 and sg.offsets[-1] == n and sg.plan.device == self.p.device
                and sg.plan.numel() == 2 * sg.jobs + 2 * (sg.groups + 1) and sg.chunk == lib.query("siss_surgery_chunk")
                and sg.partials.numel() >= 3 * sg.jobs and sg.group_sums.numel() == 3 * sg.groups and sg.coef.numel() == 2 * sg.groups
                and not sg.group_offsets.is_cuda):
            raise ValueError(f"FlatAdamW.launch(surgery=...): the plan must cover this buffer of {n} floats on {self.p.device}; got one "
                             f"over {sg.total} floats on {sg.plan.device}")
        self._surgery_checked = sg

    def _ewc_check(self, ewc):
        """Once per anchor, not per step: the kernels are there, F and pstar cover this buffer on its device, and the slab of the
        penalty sums exists (before a step is captured: SISSStepper.set_ewc calls this)."""
        if ewc is getattr(self, "_ewc_checked", None):
            return
        n = self.p.numel()
        for name in ("siss_grad_norms_scale_ewc", "siss_ewc_partials_words"):
            if not lib.has(name):
                raise RuntimeError(f"this libsiss_hip.so has no {name}: a Fisher anchor needs the kernels of csrc/ewc.hip (there is no "
                                   "fall-back to the plain update)")
        for name, t in (("fisher", ewc.fisher), ("pstar", ewc.pstar)):
            if not (t.dtype == torch.float32 and t.device == self.p.device and t.dim() == 1 and t.is_contiguous() and t.numel() == n
                    and t.data_ptr() % 16 == 0):
                raise ValueError(f"FlatAdamW.launch(ewc=...): {name} must be {n} contiguous f32 values on {self.p.device}, 16-byte "
                                 f"aligned; got {tuple(t.shape)} {t.dtype} on {t.device}")
        if getattr(self, "ewc_partials", None) is None:
            self.ewc_partials = torch.zeros(lib.query("siss_ewc_partials_words"), dtype=torch.float64, device=self.p.device)
        self._ewc_checked = ewc

    def launch_sharded(self, gx_shard, ga_shard, lo, hi, group, *, scaling_norm=None, eta=None, inf_guard=False, ranges=None, mask=None,
                       ewc=None, surgery=None, fixed_weight=None):
        """The same update on THIS rank's parameter shard [lo, hi) (sharded data-parallel exchange):
        gx_shard / ga_shard are the rank-summed gradients of the shard.  The three norm sums are all-reduced (24 bytes),
        so every rank forms the same scaling factor and clip coefficient as the replicated update; p / m / v / shadow are
        touched on [lo, hi) only -- the caller all-gathers the parameters afterwards."""
        import ctypes
        import torch.distributed as dist
        if fixed_weight is not None:
            raise NotImplementedError("FlatAdamW.launch_sharded: fixed_weight= and a parameter shard do not combine -- the teacher "
                                      "target's weighted pass 1 has no sharded form (use the all-reduce)")
        exclusive("FlatAdamW.launch_sharded", {"surgery=": surgery, "ranges=": ranges, "mask=": mask, "ewc=": ewc, SHARD: True},
                  NotImplementedError)
        n = hi - lo
        assert gx_shard.numel() == n and ga_shard.numel() == n and gx_shard.dtype == torch.float32
        mode, knob = _mode_knob(scaling_norm, eta, inf_guard)
        nblk = ctypes.c_int(0)
        lib.call("siss_grad_norm_partials", gx_shard, ga_shard, n, self.partials, ctypes.byref(nblk))
        sums = self.partials.view(-1, 3)[:nblk.value].sum(dim=0, keepdim=True)      # [1, 3] f64 on the device
        dist.all_reduce(sums, group=group)
        lib.call("siss_grad_scalars", sums, 1, mode, knob, self.max_grad_norm, self.betas[0], self.betas[1], self.scalars)
        lib.call("siss_recombine_clip_adamw", gx_shard, ga_shard, self.p[lo:hi], self.m[lo:hi], self.v[lo:hi],
                 self.shadow[lo:hi] if self.shadow is not None else None, None, n, self.lr, self.betas[0],
                 self.betas[1], self.eps, self.wd, self.scalars)

    # ------------------------------------------------------------------ the single-set update (csrc/train_state.hip)
    def _train_block(self):
        """The scalar block of the single-set update (its own: `scalars` above belongs to launch / launch_sharded), the f64 slabs,
        and the host's mirror of the block's EMA step count (every launch adds exactly one: no read-back needed to know it)."""
        if getattr(self, "train_scalars", None) is None:
            dev = self.p.device
            self.train_scalars = torch.zeros(lib.query("siss_train_scalars_words"), dtype=torch.float32, device=dev)
            self.train_partials = torch.zeros(lib.query("siss_train_partials_words"), dtype=torch.float64, device=dev)
            self.train_ema_step = 0
        return self.train_scalars

    def launch_single(self, g, ema=None, want_grad=False):
        """Enqueue clip + AdamW on ONE gradient set g [P] f32 (train_unconditional.py:409-415 of the reference), with the EMA of the
        weights in the same pass (ema: siss_amd.ema.EMAModel over this parameter buffer, or None).  No host sync."""
        n = self.p.numel()
        assert g.dtype == torch.float32 and g.shape == (n,) and g.is_contiguous()
        blk = self._train_block()
        if ema is not None:
            assert ema.flat.shape == self.p.shape and ema.flat.device == self.p.device
            if ema.optimization_step != self.train_ema_step:      # the EMA was stepped (or loaded) elsewhere: the block follows it
                blk[EMA_STEP:EMA_STEP + 1].fill_(float(ema.optimization_step))
                self.train_ema_step = ema.optimization_step
            sched = ema.schedule_args()
        else:
            sched = (0.0, 0.0, 1.0, 1.0, 0, 0)
        lib.call("siss_grad_norm_single", g, n, self.max_grad_norm, self.betas[0], self.betas[1], *sched,
                 self.train_partials, blk)
        if want_grad and (self.last_grad is None):
            self.last_grad = torch.empty_like(self.p)
        lib.call("siss_clip_adamw_ema", g, self.p, self.m, self.v, None if ema is None else ema.flat, self.shadow,
                 self.last_grad if want_grad else None, n, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, blk)
        self.train_ema_step += 1
        if ema is not None:
            ema.optimization_step += 1

    @staticmethod
    def train_stats_from(s):
        """stats_from for the single-set block (siss_train_scalars_words: ||g||, clip, step, bc1, bc2_sqrt, EMA step, 1 - decay, decay)."""
        return {"pre_clip_norm": float(s[0]), "clip_coef": float(s[1]), "step": int(s[2]), "ema_decay": float(s[EMA_DECAY])}

    def stats(self):
        """One small D2H copy: the logged gradient scalars (delete_celeb.py:748)."""
        return self.stats_from(self.scalars.cpu())

    @staticmethod
    def stats_from(s):
        """The same from a host copy of the scalar block (SISSStepper.stats fetches it together with the loss rows)."""
        return {"norm_loss_x": float(s[0]), "norm_loss_a": float(s[1]), "dot": float(s[2]),
                "scaling_factor": float(s[3]), "pre_clip_norm": float(s[4]), "clip_coef": float(s[5]),
                "step": int(s[6])}

    def step(self, grads, **kw):
        self.launch(grads, **kw)
        return self.stats()


class AdamWSpec:
    """What ``_target_: torch.optim.AdamW`` resolves to (hydra_lite.TARGET_REMAP): the hyper-parameters of
    config/delete_celeb.yaml:127-133, consumed by the fused flat-buffer optimizer."""

    def __init__(self, params=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **unused):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(float(b) for b in betas), float(eps), float(weight_decay)

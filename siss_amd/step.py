"""One SISS unlearning optimizer step on HIP -- the hot loop body of the reference's
delete_celeb.py:557-773 (delete_tshirt.py:501-717), in closed form:

    per micro-batch k:  x_mix, iw     = mixture_fwd(x0, a0, noise, t, u)                   [fused pre-kernel]
                        pred          = UNet(x_mix, t)                                      [one forward]
                        c_x, c_a      = d/dpred sum(iw * (pred - eps)^2) / (B_total * GA)   [fused post-kernel]
                        [g_x ; g_a]  += J^T [c_x ; c_a]                                    [ONE dual-cotangent backward]
    sync step:          (all-reduce [g_x ; g_a] over ranks)                                 [one RCCL collective]
                        s = scaling_norm / ||g_a|| ; g = g_x - s g_a ; clip ; AdamW         [two flat passes]

What the reference does with two ``backward`` calls, three 450-tensor clone loops, two norm
loops and a foreach optimizer is here a fixed kernel schedule with no host synchronisation;
the logged scalars stay on the device until ``stats()`` is called.

Data parallelism: every rank runs the same schedule on its own keep / forget
shard; the only exchange is one sum all-reduce of the flat [g_x ; g_a] buffer per optimizer
step.  Loss normaliser = global batch (train_batch_size * world_size), so the result equals
the single-process step on the concatenated batch.
"""
import torch

from . import lib
from . import dp
from .dp import EXCHANGES, allreduce_flat_grads, allreduce_pieces, can_shard
from .loss import loss_bwd_seed, mixture_fwd, mse_bwd_seed, teacher_seed
from .optim import FlatAdamW
from .unet import UNetEngine
from .variants import VARIANTS, exchange_refusal, exclusive, same_layout

SISS = "importance_sampling_with_mixture"
NO_IS = "double_forward_with_neg_del"
ERASEDIFF = "erasediff"
NEG_GRAD = "simple_neg_del"
NAIVE = "naive_del"
SUBSCORE = "subscore_bernoulli"
TEACHER = "teacher_target"          # opt-in, not the reference's: siss_amd/teacher.py


class SISSStepper:
    _warned_fp32 = False
    wgrad_overwrite = True          # (A/B switch; see UNetEngine.wgrad_overwrite)
    teacher = teacher_cfg = None    # the frozen teacher of loss_fn="teacher_target" and its parsed key (siss_amd/teacher.py)

    def __init__(self, engine: UNetEngine, alphas_cumprod, *, lr, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, scaling_norm=None, eta=None, lambd=0.5, train_batch_size,
                 grad_accum=1, max_grad_norm=1.0, loss_fn=SISS, inf_guard=False, process_group=None,
                 mixed_precision="bf16", superfactor=1.0, superfactor_decay=None, trainable=None, lora=None, saliency=None,
                 ewc=None, surgery=None, teacher=None, teacher_cfg=None):
        """trainable: None (every parameter: the reference's protocol), an iterable of parameter names, or "requires_grad" (the flags
        of the parameters of the UNet2DModel / UNet2DConditionModel that owns the engine).  With a subset the norms, the scaling
        factor, the clip and the AdamW update run over the trainable tensors only; the rest keep every byte.  The selection (the
        flags included) is read ONCE, here, and set on the engine (UNetEngine.set_trainable), where it stays until another stepper is
        built over the engine: flags changed afterwards do not change what this stepper updates.  (A loss.backward() through the
        class surface drops products by the flags as they are at that backward, not by this selection.)

        lora: None, or a siss_amd.lora.LoRAState over this engine (opt-in, not the reference's protocol): the base weights stay frozen
        and the optimizer runs on the adapters' flat buffer -- after the backward pass the weight gradients of the targets are
        projected to (dA, dB) of both sets, the norms / scaling factor / clip / AdamW run in adapter space, and one merge pass rewrites
        the targets' stretches of the master and its shadow.  Only the targets' weight-gradient products run; no full-size m / v.

        saliency: None, or a siss_amd.saliency.SaliencyMask over this engine (opt-in, not the reference's protocol): one bit per float
        of the flat buffer -- the norms, the scaling factor, the clip and the AdamW update run over the elements whose bit is set
        (csrc/saliency.hip), every other byte of the parameters, their moments and their shadow keeps its value.  The backward pass
        and the gradient exchange are the full update's (every weight-gradient product runs, the whole buffer is summed); exclusive
        with trainable= and lora=.  The mask's words live as long as the stepper: a captured step holds their address.

        ewc: None, or a siss_amd.ewc.FisherAnchor over this engine (opt-in, not the reference's protocol): once per optimizer step,
        after the accumulation and the data-parallel exchange, strength * F * (theta - theta*) is added to the keep-side gradient set
        inside pass 1 of the update (csrc/ewc.hip), so that the norms, the scaling factor, the clip and AdamW see it; exclusive with
        trainable=, lora= and saliency=.  F and theta* live as long as the stepper: a captured step holds their addresses.

        surgery: None, or a siss_amd.surgery.Surgery over this engine (opt-in, not the reference's protocol): once per optimizer step,
        after the accumulation and the data-parallel exchange, the conflicting component of the (keep, forget) gradient pair is
        projected out per group of the buffer before the norm fix (csrc/surgery.hip); for the two-set losses with the norm fix only;
        exclusive with the other four.  Its plan and slabs live as long as the stepper: a captured step holds their addresses.

        teacher, teacher_cfg: a siss_amd.teacher.Teacher beside this engine and a TeacherConfig (None: its defaults), with
        loss_fn="teacher_target" (opt-in, not the reference's protocol; each without the other is refused): the rows are regressed onto
        targets built from the frozen teacher's predictions (csrc/teacher.hip) and the update is the plain weighted sum g_x + weight g_a.
        Combines with lora=; refused with the other four, whose pass 1 has no weighted form."""
        self.e = engine
        self.lora = lora
        self.saliency = self.ewc = self.surgery = None
        self.teacher, self.teacher_cfg = self._teacher_args(loss_fn, teacher, teacher_cfg, {
            "surgery=": surgery, "ewc=": ewc, "saliency=": saliency, "trainable=": trainable})
        exclusive("SISSStepper", {"surgery=": surgery, "ewc=": ewc, "saliency=": saliency, "lora=": lora, "trainable=": trainable})
        if lora is not None:
            if lora.engine is not engine:
                raise ValueError("SISSStepper(lora=...): the LoRAState was built over another engine")
            trainable = list(lora.names) + list(lora.conv_names)     # (exactly the targets' weight-gradient products run)
        if hasattr(engine, "check_trainable"):
            engine.check_trainable()                # a site without a backward kernel is refused here, not inside the first step
        dev = engine.device
        ac = alphas_cumprod.to(device=dev, dtype=torch.float32).contiguous()
        self.ac = ac
        self.gamma_tab = (ac ** 0.5).contiguous()           # delete_celeb.py:367-371
        self.sigma_tab = ((1 - ac) ** 0.5).contiguous()
        self.lambd, self.scaling_norm, self.eta, self.inf_guard = float(lambd), scaling_norm, eta, inf_guard
        self.train_batch_size, self.ga = int(train_batch_size), int(grad_accum)
        self.loss_fn = loss_fn
        self.superfactor = float(superfactor)
        self.superfactor_decay = None if superfactor_decay is None else float(superfactor_decay)   # delete_celeb.py:658-662
        if loss_fn == ERASEDIFF:
            assert eta is not None, "erasediff needs eta (delete_celeb.py:740-742)"
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        # the step runs its collectives: more than one rank (or dp.FORCE_COLLECTIVES, the test-only switch for a 1-rank RCCL group)
        self.dp_on = process_group is not None and (self.world > 1 or dp.FORCE_COLLECTIVES)
        self.io_dtype = torch.bfloat16 if mixed_precision == "bf16" else torch.float32
        f32_engine = getattr(engine, "f32", False)
        if f32_engine and mixed_precision == "bf16":
            raise ValueError("mixed_precision='bf16' on an f32 engine: build the engine with dtype=torch.bfloat16")
        if mixed_precision != "bf16" and not f32_engine and not SISSStepper._warned_fp32:
            # config/delete_*.yaml ship mixed_precision: null (fp32 everywhere in the reference).  On an f32 ENGINE
            # (UNetEngine(dtype=torch.float32): what the task loop builds for null) that is what runs.  On a bf16 engine it selects
            # f32 image / noise I/O, f32 master weights, gradients and optimizer state -- with bf16 MFMA operands.
            import warnings
            warnings.warn("siss_amd: mixed_precision is not 'bf16' on a bf16 engine: I/O, master weights, gradients and optimizer "
                          "state are f32, but convolutions / linears run on bf16 MFMA operands with f32 accumulation -- results "
                          "match an fp32 run to bf16 tolerance; UNetEngine(cfg, device, dtype=torch.float32) is the f32 path",
                          RuntimeWarning, stacklevel=2)
            SISSStepper._warned_fp32 = True
        if lora is None:
            self.opt = FlatAdamW(engine.ps.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                 max_grad_norm=max_grad_norm, shadow=None if f32_engine else engine.ps.shadow)
        else:
            # the adapters' buffer is the optimizer's: m / v of L floats, no shadow (the merge writes the operand copies)
            self.opt = FlatAdamW(lora.p, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                 shadow=None)
        self.subset = self._subset(trainable)
        engine.set_trainable(self.subset)
        # the ONE resolved variant (siss_amd/variants.py: at most one is active); set_saliency / set_ewc move a `full` stepper to theirs
        self.variant = "lora" if lora is not None else "trainable" if self.subset is not None else "full"
        # what FlatAdamW.launch takes beside the gradients (the table is built once and lives as long as the stepper: a captured step
        # holds its address)
        self._launch_kw = {"ranges": self.subset.table(dev)} if self.variant == "trainable" else {}
        self._micro = 0
        self.last = None
        self._pending = []
        # Data-parallel overlap: the tail [split, P) of the flat gradient buffer (up / mid / deep down blocks,
        # ~85 % of the bytes) is final long before the high-resolution down blocks finish their backward;
        # its all-reduce is started from a hook inside the backward pass and runs beside the rest of it.
        import os
        self.exchange = os.environ.get("SISS_DP_EXCHANGE", "allreduce")      # serial mode: "allreduce" | "sharded"
        self._state_shard = None                # (lo, hi) while AdamW's moments are current on this rank's shard only
        assert self.exchange in EXCHANGES
        if self.teacher is not None and self.exchange == "sharded":
            print("[siss_amd] teacher target: the weighted pass 1 has no sharded form; using the all-reduce")
            self.exchange = "allreduce"
        self._fit_exchange(self.dp_on and engine.ps.split < engine.ps.total and os.environ.get("SISS_DP_OVERLAP", "1") != "0")
        if saliency is not None:
            self.set_saliency(saliency)
        if ewc is not None:
            self.set_ewc(ewc)
        if surgery is not None:
            self.set_surgery(surgery)

    def _fit_exchange(self, overlap):
        """set_overlap with what the variant may use of (overlap, self.exchange): a LoRA / subset step has ONE collective after the
        backward pass, a masked / anchored step the whole-buffer all-reduce (overlapped or serial) -- saying what it switched off."""
        if self.dp_on:
            why = exchange_refusal(self.variant, overlap, "allreduce")
            if why:
                print(f"[siss_amd] {why}")
                overlap = False
            why = exchange_refusal(self.variant, False, self.exchange)
            if why:
                print(f"[siss_amd] {why}; using the all-reduce")
                self.exchange = "allreduce"
        self.set_overlap(overlap)

    def _teacher_args(self, loss_fn, teacher, teacher_cfg, others):
        """(teacher, its config) of SISSStepper(loss_fn="teacher_target", teacher=...), or (None, None): each of the two without the
        other, a teacher over another architecture or device, a missing embedding and the four variants without a weighted pass 1
        are refused here, before any launch."""
        if (loss_fn == TEACHER) != (teacher is not None):
            raise ValueError("SISSStepper: loss_fn='teacher_target' needs teacher= (a siss_amd.teacher.Teacher)" if teacher is None else
                             f"SISSStepper: teacher= is set but loss_fn={loss_fn!r}: the teacher serves loss_fn='teacher_target' only")
        if teacher is None:
            if teacher_cfg is not None:
                raise ValueError("SISSStepper: teacher_cfg= without teacher=")
            return None, None
        from .teacher import parse_teacher, require_kernels, teacher_exclusive
        teacher_exclusive("SISSStepper", "teacher=", teacher, others)
        require_kernels()
        cfg = teacher_cfg if teacher_cfg is not None else parse_teacher({})
        if not same_layout(teacher, self.e) or teacher.engine.adt != self.e.adt:
            raise ValueError("SISSStepper(teacher=...): the teacher was built over another engine's parameter layout or dtype")
        if teacher.engine.ps.flat.device != self.e.ps.flat.device:
            raise ValueError("SISSStepper(teacher=...): the teacher is on another device than the engine")
        teacher.check(cfg)
        teacher.cfg = cfg
        return teacher, cfg

    def _adopt(self, name, obj, tensor, require_kernels, launch_kw, ready=None):
        """set_saliency / set_ewc / set_surgery: a `full` stepper moves to variant `name` (another object of the stepper's own variant
        replaces the first).  tensor: a device tensor of obj (per float, or the surgery's plan), which must live on the engine's
        device; obj must cover this engine's flat buffer; ready(obj): what has to exist before a step is captured."""
        present = {"surgery=": getattr(self, "surgery", None), "ewc=": self.ewc, "saliency=": self.saliency, "lora=": self.lora,
                   "trainable=": self.subset}
        del present[name + "="]
        if self.teacher is not None:
            from .teacher import teacher_exclusive
            teacher_exclusive(f"SISSStepper.set_{name}", "teacher=", self.teacher, {name + "=": obj})
        exclusive(f"SISSStepper.set_{name}", {name + "=": obj, **present})
        require_kernels()
        what = VARIANTS[name].what
        if not same_layout(obj, self.e):
            raise ValueError(f"SISSStepper({name}=...): the {what} was built over another engine's parameter layout")
        if tensor.device != self.e.ps.flat.device:
            raise ValueError(f"SISSStepper({name}=...): the {what}'s tensors are on another device than the engine")
        if ready is not None:
            ready(obj)
        setattr(self, name, obj)
        self.variant, self._launch_kw = name, launch_kw
        self._fit_exchange(self.overlap)

    def set_ewc(self, anchor):
        """Fold the penalty gradient of `anchor` (siss_amd.ewc.FisherAnchor over this engine) into the keep-side set from the next step
        on -- what SISSStepper(ewc=anchor) does; a task calls it once its Fisher is computed (FisherAnchor.from_batches needs the
        stepper).  Before a step is captured: a captured step holds the addresses of F and theta*."""
        from .ewc import require_kernels
        # (ready: the slab of the penalty sums is allocated now, not inside a captured step)
        self._adopt("ewc", anchor, anchor.fisher, require_kernels, {"ewc": anchor}, ready=self.opt._ewc_check)

    def set_surgery(self, surgery):
        """Project the conflicting component out of the gradient pair with `surgery` (siss_amd.surgery.Surgery over this engine) from
        the next step on -- what SISSStepper(surgery=...) does.  Before a step is captured: a captured step holds the addresses of the
        plan and the slabs.  Refused for the losses without a gradient pair under the norm fix."""
        from .surgery import check_loss, require_kernels
        check_loss(self.loss_fn, "SISSStepper(surgery=...)")
        self._adopt("surgery", surgery, surgery.plan, require_kernels, {"surgery": surgery}, ready=self.opt._surgery_check)

    def set_saliency(self, mask):
        """Restrict the update to the set bits of `mask` (siss_amd.saliency.SaliencyMask over this engine) from the next step on -- what
        SISSStepper(saliency=mask) does; a task calls it once its mask is computed (forget_gradient needs the stepper).  Before a step
        is captured: a captured step holds the address of the words it was captured with."""
        from .saliency import require_kernels
        self._adopt("saliency", mask, mask.bits, require_kernels, {"mask": mask.bits})

    def _subset(self, trainable):
        """SISSStepper(trainable=...) as a siss_amd.trainable.Subset of the engine's flat buffer (None: the full update)."""
        if trainable is None:
            return None
        from .trainable import Subset, from_flags
        from .unet import ALIGN
        ps = self.e.ps
        if isinstance(trainable, str):
            if trainable != "requires_grad":
                raise ValueError(f"trainable={trainable!r}: None, an iterable of parameter names or 'requires_grad'")
            owner = getattr(self.e, "owner", None)
            model = owner() if owner is not None else None
            if model is None:
                raise ValueError("trainable='requires_grad' reads the flags of the UNet2DModel / UNet2DConditionModel that owns the "
                                 "engine; this engine has none -- pass the parameter names")
            trainable = from_flags(model.named_parameters())
        names = list(trainable)
        if len(set(names)) == len(ps.specs) and all(n in ps.specs for n in names):
            return None                                 # every parameter: the full update
        if self.lora is not None:                       # (the adapter-space update needs no subset kernels: the full ones on lora.p)
            return Subset(ps.specs, names, ps.total, ALIGN)
        if not lib.has("siss_recombine_clip_adamw_ranges"):
            raise RuntimeError("this libsiss_hip.so has no siss_recombine_clip_adamw_ranges: a trainable subset needs the subset "
                               "kernels of csrc/optimizer.hip (there is no fall-back to the full update)")
        return Subset(ps.specs, names, ps.total, ALIGN)

    def set_overlap(self, on, exchange=None):
        """Overlapped (tail all-reduce started from inside the backward) or serial (one exchange after it: RCCL's
        all-reduce, or the sharded update).  Moments left on a shard by sharded steps are re-gathered where the next
        replicated update needs them (_sync_and_update), whichever way the mode was changed."""
        self.overlap = bool(on)
        if exchange is not None:
            assert exchange in EXCHANGES
            self.exchange = exchange
        why = exchange_refusal(self.variant, self.overlap, self.exchange) if self.dp_on else None
        if why:
            raise NotImplementedError(f"{why}: set_overlap({'on' if VARIANTS[self.variant].overlap is None else 'False'}, 'allreduce')")
        self.e.on_early_grads_final = self._early_allreduce if self.overlap else None

    def _gather_optimizer_state(self):
        """The sharded update advances AdamW's moments on this rank's parameter shard only.  Before a REPLICATED update
        follows (another exchange mode, a checkpoint of the optimizer) the shards are all-gathered once, so that every
        rank holds identical full moments again."""
        if self._state_shard is None:
            return
        from .dp import all_gather_params
        lo, hi = self._state_shard
        all_gather_params(self.opt.m, lo, hi, self.pg)
        all_gather_params(self.opt.v, lo, hi, self.pg)
        self._state_shard = None

    def optimizer_state(self):
        """(m, v, scalars) with the moments complete on every rank -- what a checkpoint of the optimizer saves."""
        self._gather_optimizer_state()
        return self.opt.m, self.opt.v, self.opt.scalars

    def _save_state(self):
        """For callers that run REAL optimizer steps only to time them (autotune_overlap, try_captured_serial): clones parameters, AdamW
        moments and the step counter, notes the stepper's own state (NegGrad's decaying superfactor, the last step's statistics, the
        accumulation count) and returns the function that puts all of it back -- the run that follows starts from what it was given."""
        self._gather_optimizer_state()          # sharded steps before this call left the moments current on the owner's shard only
        tensors = (self.opt.p, self.opt.m, self.opt.v, self.opt.scalars)
        saved = [t.clone() for t in tensors]
        state = (self.superfactor, self.last, self._micro)

        def restore():
            self._state_shard = None            # (the moments are overwritten as a whole)
            for dst, src in zip(tensors, saved):
                dst.copy_(src)
            self.superfactor, self.last, self._micro = state
            if self.lora is not None:
                # opt.p is the adapters' buffer: the master follows it (autotune_overlap returns early for a LoRA stepper, so only
                # try_captured_serial reaches this)
                self.lora.merge()
            self.e.refresh_weights(cast_shadow=True)
        return restore

    def autotune_overlap(self, step_fn, iters=3):
        """Measure, don't guess: the overlapped exchange shares the chip with the persistent one-block-per-CU GEMMs of
        the high-resolution backward, and whether RCCL's workgroups cost those kernels more than the overlap hides
        depends on the node.  Times `iters` steps each way (max over ranks) and keeps the faster setting."""
        # the three settings a node can tell apart: one all-reduce after the backward, the same exchange overlapped with it,
        # and the sharded update (reduce-scatter -> shard-local AdamW -> all-gather of the parameters) -- those the variant may use
        candidates = {"overlap": (True, "allreduce"), "serial": (False, "allreduce")}
        if can_shard(self.e.ps.total, self.world):
            candidates["serial_sharded"] = (False, "sharded")
        candidates = {name: c for name, c in candidates.items() if exchange_refusal(self.variant, *c) is None}
        if not self.dp_on or self.e.ps.split >= self.e.ps.total or "overlap" not in candidates:
            return self.overlap                      # (a subset / LoRA step has one exchange mode: nothing to choose)
        import time
        dist = torch.distributed
        results, errors = {}, {}
        restore = self._save_state()            # (the timed steps are real optimizer steps)
        for name, (mode, exch) in candidates.items():
            self.set_overlap(mode, exch)
            exc = None
            try:
                step_fn()                                        # settle (scratch buffers, communicator channels)
            except (RuntimeError, NotImplementedError) as e:
                exc = e
            # A failure may be rank-LOCAL (torch's OOM is a RuntimeError; a launch error): the ranks AGREE on it before any of
            # them decides -- a rank that skipped the candidate alone would leave the others waiting in the barrier below.
            gathered = [None] * self.world
            dist.all_gather_object(gathered, exc is not None, group=self.pg)
            if any(gathered):
                # collectives a backward hook already started must retire before the next candidate rewrites the gradient
                # buffer they read -- wait on them, do not just forget them
                for work in self._pending:
                    try:
                        if work is not None:
                            work.wait()
                    except Exception:
                        pass
                torch.cuda.synchronize()
                self._pending, self._micro, self._state_shard = [], 0, None
                if name == "serial":            # the serial all-reduce must work or the run has no exchange
                    raise exc if exc is not None else RuntimeError("the serial gradient exchange failed on another rank")
                errors[name] = ((str(exc) or type(exc).__name__) if exc is not None else "failed on another rank")[:200]
                continue
            dist.barrier(group=self.pg); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step_fn()
            dist.barrier(group=self.pg); torch.cuda.synchronize()
            tt = torch.tensor([time.perf_counter() - t0], device=self.e.device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=self.pg)
            results[name] = float(tt.item()) / iters
        best = min(results, key=results.get)
        restore()
        self.set_overlap(best.startswith("overlap"), candidates[best][1])
        self.overlap_timings = {k + "_ms": v * 1e3 for k, v in results.items()}
        if errors:
            self.overlap_timings["errors"] = errors
        return self.overlap

    def try_captured_serial(self, step_fn, iters=3):
        """N > 1 insurance (round 6): the step with its SERIAL all-reduce captured into a hipGraph, as one more candidate beside the eager
        exchange modes (a world-size-1 RCCL communicator captured and replayed such a step: tests/test_hip_rccl.py; whether the
        multi-rank kernels do is the node's to say).  Captures on every rank, AGREES on the outcome (a rank-local failure makes every
        rank fall back: nobody replays a graph the others do not have), times `iters` replays (max over ranks) and restores
        parameters / moments / stepper state.  Returns (graph, seconds per step, None) with the stepper left on the serial exchange,
        or (None, None, reason) with the previous exchange mode restored -- in process, no re-exec, no relaunch."""
        dist = torch.distributed
        import time
        restore = self._save_state()
        prev = (self.overlap, self.exchange)
        self.set_overlap(False, "allreduce")
        graph, err, secs = None, None, None
        try:
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream(device=self.e.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                step_fn()                                            # settle allocations on the capture stream
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    step_fn()
            cur.wait_stream(side)
            graph.replay()
            torch.cuda.synchronize()
        except Exception as e:                                       # capture refused / launch error: eager it is
            err, graph = (str(e) or type(e).__name__)[:200], None
        flags = [None] * self.world
        dist.all_gather_object(flags, err is None, group=self.pg)
        if all(flags):
            dist.barrier(group=self.pg); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                graph.replay()
            dist.barrier(group=self.pg); torch.cuda.synchronize()
            tt = torch.tensor([time.perf_counter() - t0], device=self.e.device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=self.pg)
            secs = float(tt.item()) / iters
        else:
            graph, err = None, err or "capture failed on another rank"
            torch.cuda.synchronize()
        self._pending = []
        restore()
        if graph is None:
            self.set_overlap(*prev)
        return graph, secs, err

    # ------------------------------------------------------------------ one micro-batch
    def micro_step(self, x0, a0, noise, t, u, conditioning=None, erase_target=None):
        """Inputs: x0/a0/noise [B,C,H,W] (cast to the io dtype like delete_celeb.py:561-581),
        t [B] int64, u [B] keep/forget uniforms; conditioning: the dict the reference splats into the UNet
        call ({} or {'encoder_hidden_states': [B,77,768]}, delete_sd.py:974-976).  Enqueues fwd + dual
        backward; no host sync."""
        e = self.e
        cond = dict(conditioning or {})
        # first micro-batch of a step: one-split weight gradients overwrite their tiles (ONE backward pass per micro-batch below)
        e.wgrad_overwrite = self._micro == 0 and self.wgrad_overwrite
        if self._micro == 0:
            # the fill runs beside the forward pass (joined by the backward pass) and skips what that backward pass will overwrite:
            # the key names everything its split decisions depend on
            key = (self.loss_fn, tuple(x0.shape), tuple(sorted((k, tuple(v.shape)) for k, v in cond.items())))
            e.zero_grad(beside_forward=True, sparse_key=key)
        x0, a0, noise = (v.to(device=e.device, dtype=self.io_dtype).contiguous() for v in (x0, a0, noise))
        B = x0.shape[0]
        scale = 1.0 / (self.train_batch_size * self.world * self.ga)
        if self.loss_fn == SISS:
            m = mixture_fwd(x0, a0, noise, t, u, self.ac, self.gamma_tab, self.sigma_tab, self.lambd)
            pred = e.forward(m.x_mix, t, **cond)
            cot = e._buf("cot", (2 * B, *pred.shape[1:]))
            # c_x / c_a go straight into the stacked cotangent buffer that seeds the dual backward
            seed = loss_bwd_seed(pred, m, x0, a0, scale, c_out=cot, partials=self._partials(B, pred[0].numel()))
            e.backward(cot, nsets=2)
            chw = pred[0].numel()
            self.last = dict(loss_x=seed.sum_loss_x / chw, loss_a=seed.sum_loss_a / chw, iw_x=m.iw_x, iw_a=m.iw_a)
        elif self.loss_fn == NO_IS:
            # two forwards as ONE batch-2B forward (ddpm_deletion_loss.py:60-67), plain noise target
            m = mixture_fwd(x0, a0, noise, t, torch.ones(B, device=e.device), self.ac, self.gamma_tab,
                            self.sigma_tab, 0.0)   # u=1 > 0: keep rows -> q_sample(x0)
            mf = mixture_fwd(x0, a0, noise, t, torch.zeros(B, device=e.device), self.ac, self.gamma_tab,
                             self.sigma_tab, 0.5)  # u=0 <= .5: forget rows -> q_sample(a0)
            xin = torch.cat([m.x_mix, mf.x_mix], 0)
            cond2 = {k: torch.cat([v, v], 0) for k, v in cond.items()}
            pred = e.forward(xin, torch.cat([t, t], 0), **cond2)
            tgt = torch.cat([noise, noise], 0)
            cot, _, sums = mse_bwd_seed(pred, tgt, scale)
            e.backward(cot, nsets=2)
            chw = pred[0].numel()
            self.last = dict(loss_x=sums[:B] / chw, loss_a=sums[B:] / chw)
        elif self.loss_fn == ERASEDIFF:
            # ddpm_deletion_loss.py:70-78: keep half against the noise, forget half against U[0,1) "noise"; the
            # recombination is s = -max(eta - <g_x, g_a> / |g_a|^2, 0) (delete_celeb.py:740-742, optimizer mode)
            m = mixture_fwd(x0, a0, noise, t, torch.ones(B, device=e.device), self.ac, self.gamma_tab,
                            self.sigma_tab, 0.0)
            mf = mixture_fwd(x0, a0, noise, t, torch.zeros(B, device=e.device), self.ac, self.gamma_tab,
                             self.sigma_tab, 0.5)
            xin = torch.cat([m.x_mix, mf.x_mix], 0)
            cond2 = {k: torch.cat([v, v], 0) for k, v in cond.items()}
            pred = e.forward(xin, torch.cat([t, t], 0), **cond2)
            if erase_target is None:
                erase_target = torch.rand(noise.shape, device=e.device, dtype=torch.float32)
            tgt = torch.cat([noise.float(), erase_target.to(device=e.device, dtype=torch.float32)], 0)
            cot, _, sums = mse_bwd_seed(pred, tgt, scale)
            e.backward(cot, nsets=2)
            chw = pred[0].numel()
            self.last = dict(loss_x=sums[:B] / chw, loss_a=sums[B:] / chw)
        elif self.loss_fn in (NEG_GRAD, NAIVE):
            # a `loss` is returned (ddpm_deletion_loss.py:82-96): ONE backward, no gradient split
            # (delete_celeb.py:682-684); NegGrad ascends on the forget batch with -superfactor
            keep = self.loss_fn == NAIVE
            m = mixture_fwd(x0, a0, noise, t, torch.full((B,), 1.0 if keep else 0.0, device=e.device), self.ac,
                            self.gamma_tab, self.sigma_tab, 0.5)
            pred = e.forward(m.x_mix, t, **cond)
            cot, _, sums = mse_bwd_seed(pred, noise, scale if keep else -self.superfactor * scale)
            # the second gradient set stays zero (zero_grad above): g = g_x through the inf-guarded s = 0
            e.backward(cot, nsets=1)
            per = sums / pred[0].numel()
            # the returned 7-tuple (ddpm_deletion_loss.py:88,:96): naive = (loss_x, loss_x, None, ...), NegGrad = (-sf loss_a, None, loss_a, ...)
            self.last = dict(loss=per, loss_x=per) if keep else dict(loss=-self.superfactor * per, loss_a=per,
                                                                   superfactor=self.superfactor)
            if not keep and self.superfactor_decay is not None:
                self.superfactor *= self.superfactor_decay         # applied after the loss call (delete_celeb.py:658-662)
        elif self.loss_fn == TEACHER:
            # NOT the reference's: keep / forget rows as the NO_IS branch makes them, regressed onto targets the frozen teacher supplies
            tc, th = self.teacher_cfg, self.teacher
            keep_none = tc.keep == "none"
            mf = mixture_fwd(x0, a0, noise, t, torch.zeros(B, device=e.device), self.ac, self.gamma_tab,
                             self.sigma_tab, 0.5)  # u=0 <= .5: forget rows -> q_sample(a0)
            if keep_none:
                m, xin, tin, cond2 = None, mf.x_mix, t, cond
            else:
                m = mixture_fwd(x0, a0, noise, t, torch.ones(B, device=e.device), self.ac, self.gamma_tab,
                                self.sigma_tab, 0.0)   # u=1 > 0: keep rows -> q_sample(x0)
                xin, tin = torch.cat([m.x_mix, mf.x_mix], 0), torch.cat([t, t], 0)
                cond2 = {k: torch.cat([v, v], 0) for k, v in cond.items()}
            pred = e.forward(xin, tin, **cond2)
            teach = th.predict(tc, None if m is None else m.x_mix, mf.x_mix, t, cond)      # forward only, constants
            # keep: none -- the forget rows alone, ONE set, the weight folded into the scale; the second set stays zero (zero_grad
            # above) and g = g_x through the inf-guarded s = 0, as the NegGrad branch runs
            sums = teacher_seed(pred, noise, teach, B, tc, scale * tc.weight if keep_none else scale,
                                cot=e._buf("cot", tuple(pred.shape)), sums=e._buf("teacher_sums", (pred.shape[0],)),
                                partials=self._teacher_partials(pred.shape[0], pred[0].numel()))
            e.backward(e._buf("cot", tuple(pred.shape)), nsets=1 if keep_none else 2)
            chw = pred[0].numel()
            self.last = dict(loss_a=sums / chw) if keep_none else dict(loss_x=sums[:B] / chw, loss_a=sums[B:] / chw)
        elif self.loss_fn == SUBSCORE:
            # ddpm_deletion_loss.py:99-122: Bernoulli keep/forget rows against the plain noise target; the row
            # selection loss[mask] / (1 - lambd), loss[~mask] is a per-sample weight on the shared forward
            uu = u.to(device=e.device, dtype=torch.float32)
            m = mixture_fwd(x0, a0, noise, t, uu, self.ac, self.gamma_tab, self.sigma_tab, self.lambd)
            pred = e.forward(m.x_mix, t, **cond)
            c, _, sums = mse_bwd_seed(pred, noise, scale)
            keep = (uu > self.lambd).float()
            any_keep = (keep.sum() > 0).float()    # no keep rows: BOTH losses are zeroed (:113-116)
            wx = (keep / (1.0 - self.lambd)).view(B, 1, 1, 1)
            wa = ((1.0 - keep) * any_keep).view(B, 1, 1, 1)
            cot = e._buf("cot", (2 * B, *pred.shape[1:]))
            torch.mul(c, wx, out=cot[:B])
            torch.mul(c, wa, out=cot[B:])
            e.backward(cot, nsets=2)
            # loss[mask] / (1 - lambd) and loss[~mask] are ROW SELECTIONS (ddpm_deletion_loss.py:109-110): the logged
            # statistics run over the selected rows only; the zero-size guards (:113-120) log one zero
            self.last = dict(loss_x=sums / pred[0].numel() / (1.0 - self.lambd), loss_a=sums / pred[0].numel(),
                             rows_x=keep, rows_a=(1.0 - keep) * any_keep, subscore=True)
        else:
            raise ValueError(f"loss_fn {self.loss_fn!r} is not on the HIP fast path")
        self._micro += 1
        if self._micro == self.ga:
            self._micro = 0
            self._sync_and_update()

    def _partials(self, B, chw):
        return self.e._buf("loss_partials", (lib.query("siss_loss_partials_words", B, chw),), torch.float64)

    def _teacher_partials(self, R, chw):
        return self.e._buf("teacher_partials", (lib.query("siss_teacher_partials_words", R, chw),), torch.float64)

    def _early_allreduce(self):
        if self._micro + 1 != self.ga:          # only the sync micro-step communicates
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the overlapped gradient exchange issues async collectives from inside the backward pass "
                               "and cannot be captured into a hipGraph: run N > 1 eagerly or set_overlap(False)")
        ps = self.e.ps
        # ONE grouped collective: the early-final tails of both gradient sets
        self._pending.append(allreduce_pieces([ps.grads[k, ps.split:] for k in range(ps.grads.shape[0])], self.pg, async_op=True))

    def _sync_and_update(self):
        if self.lora is not None:
            return self._lora_update()
        g = self.e.ps.grads
        sharded = (self.dp_on and self.exchange == "sharded" and not self.overlap
                   and can_shard(g.shape[1], self.world))
        if not sharded:
            self._gather_optimizer_state()      # a replicated update after sharded ones: every rank needs the whole m / v
        if self.dp_on and not sharded:
            # the exchange of the step: sum of [g_x ; g_a] over ranks (RCCL over xGMI) -- one flat buffer; with
            # the overlap hook the early-final tail is already in flight and only the head remains
            if self.subset is not None:
                # ONE grouped collective: the trainable pieces (merged across small frozen gaps) of both gradient sets
                allreduce_pieces([g[k, a:b] for k in range(g.shape[0]) for a, b in self.subset.pieces()], self.pg)
            elif self.overlap and self._pending:
                split = self.e.ps.split                 # ... the second (and last) grouped collective of the step: the heads
                self._pending.append(allreduce_pieces([g[k, :split] for k in range(g.shape[0])], self.pg, async_op=True))
                for w in self._pending:
                    if w is not None:
                        w.wait()
                self._pending = []
            else:
                (EXCHANGES.get(self.exchange) or allreduce_flat_grads)(g, self.pg)     # 'sharded' that cannot shard: all-reduce
        okw = self._update_kw()
        if sharded:
            # reduce-scatter -> this rank's 1/N of the norm sums (3 doubles all-reduced) and of the recombine / clip / AdamW
            # pass -> all-gather of the updated f32 parameters (3 P (N-1)/N floats on the wire instead of 4 P (N-1)/N,
            # optimizer traffic / N); the bf16 operand shadow is recast from the gathered master
            from .dp import all_gather_params, reduce_scatter_param_shards
            gx_s, ga_s, lo, hi = reduce_scatter_param_shards(g, self.pg)
            self.opt.launch_sharded(gx_s, ga_s, lo, hi, self.pg, **okw)
            self._state_shard = (lo, hi)                        # m / v are current on [lo, hi) only
            all_gather_params(self.e.ps.flat, lo, hi, self.pg)
            self.e.refresh_weights(cast_shadow=True)
            return
        # (with an anchor g[0] becomes g_x + strength * F * (theta - theta*): zeroed before the next step)
        self.opt.launch(g, **self._launch_kw, **okw)
        self.e.refresh_weights(lazy=True)               # (the dgrad weight copies: beside the next forward pass)

    def _update_kw(self):
        """The recombination of the step as FlatAdamW's keywords: the single-set objectives run the inf-guarded norm fix with s = 0."""
        if self.teacher is not None and self.teacher_cfg.keep != "none":
            return dict(fixed_weight=self.teacher_cfg.weight)          # g = g_x + weight g_a (csrc/teacher.hip: s = -weight)
        single = self._single_set()
        return dict(scaling_norm=self.scaling_norm if not single else 1.0, eta=self.eta if self.loss_fn == ERASEDIFF else None,
                    inf_guard=self.inf_guard or single)

    def _single_set(self):
        """The objectives with ONE gradient set (the second stays zero): NegGrad, naive, and the teacher target with keep: none."""
        return self.loss_fn in (NEG_GRAD, NAIVE) or (self.teacher is not None and self.teacher_cfg.keep == "none")

    def _lora_update(self):
        """The update of a LoRA step: project -> (all-reduce of the adapter gradients) -> norms / recombine / clip / AdamW on the
        adapters -> merge -> operand copies.  Same stream, persistent tables, no host sync, no allocation: capturable like the rest."""
        lora = self.lora
        single = self._single_set()
        lora.project(nsets=1 if single else 2)
        if self.dp_on:
            allreduce_flat_grads(lora.g, self.pg)       # (the projection is linear: the sum of the ranks' dW projected = this sum)
        self.opt.launch(lora.g, **self._update_kw())
        lora.merge()
        lora.steps += 1
        self.e.refresh_weights(lazy=True)               # every derived operand copy comes out of the refresh that follows AdamW today

    def step(self, x0, a0, noise, t, u, conditioning=None, erase_target=None):
        """GA=1 convenience."""
        assert self.ga == 1
        self.micro_step(x0, a0, noise, t, u, conditioning, erase_target)

    # ------------------------------------------------------------------ logging (one small D2H)
    def stats(self):
        """The scalars the reference logs for the LAST micro-batch (delete_celeb.py:626-663: loss / loss_x / loss_a mean
        over all elements and max / min / unbiased std over the per-sample means; importance-weight mean / max / min /
        std; superfactor) plus the optimizer step's gradient scalars (:748) -- fetched with ONE device-to-host copy."""
        return self.stats_async().get()

    def stats_async(self):
        """The same without stalling the launch stream: the scalars are gathered on the device and copied to pinned host memory
        behind the step's kernels NOW; `.get()` waits for that copy and forms the dictionary.  A training loop calls `.get()`
        one step later (siss_amd/tasks.py), so the device always has the next step queued behind the one it is running."""
        last = dict(self.last or {})
        keys = [k for k in ("loss", "loss_x", "loss_a", "iw_x", "iw_a", "rows_x", "rows_a") if last.get(k) is not None]
        sizes = [self.opt.scalars.numel()] + [last[k].numel() for k in keys]
        dev = torch.cat([self.opt.scalars.float().flatten()] + [last[k].float().flatten() for k in keys])
        if dev.is_cuda:
            host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
            host.copy_(dev, non_blocking=True)                  # the one D2H of the step
            done = torch.cuda.Event()
            done.record()
        else:
            host, done = dev.clone(), None
        # (a variant with fields of its own in the optimizer's scalar block reads them from the same copy: FisherAnchor.stats_from)
        return _PendingStats(host, done, keys, sizes, last.get("subscore"), last.get("superfactor") if "superfactor" in last else None,
                             self.opt.stats_from, getattr(self._active(), "stats_from", None))

    def _active(self):
        """The object of the active variant that carries log fields (None: the full update, a trainable subset)."""
        return getattr(self, self.variant) if self.variant in ("lora", "saliency", "ewc", "surgery") else None

    def log_fields(self):
        """What every log line of the run carries beside the step's statistics: the parameters the optimizer updates and the active
        variant's own fields."""
        params, tensors = self.trainable_counts()
        active = self._active()
        teacher = self.teacher.log_fields(self.teacher_cfg, self.train_batch_size) if self.teacher is not None else {}
        return dict(trainable_params=params, trainable_tensors=tensors, **(active.log_fields() if active is not None else {}), **teacher)

    def trainable_counts(self):
        """(trainable_params, trainable_tensors) of every log line: the parameters the optimizer updates."""
        if self.lora is not None:
            return self.lora.params, self.lora.tensors
        if self.subset is not None:
            return self.subset.params, self.subset.tensors
        specs = self.e.ps.specs
        if self.saliency is not None:
            return self.saliency.count, len(specs)
        return sum(int(sp.numel) for sp in specs.values()), len(specs)


class _PendingStats:
    """Handle of SISSStepper.stats_async()."""

    def __init__(self, host, done, keys, sizes, subscore, superfactor, opt_stats_from, variant_stats_from=None):
        self.host, self.done, self.keys, self.sizes = host, done, keys, sizes
        self.subscore, self.superfactor = subscore, superfactor
        self.opt_stats_from, self.variant_stats_from = opt_stats_from, variant_stats_from

    def get(self):
        import math
        if self.done is not None:
            self.done.synchronize()
        host = self.host
        st = self.opt_stats_from(host[:self.sizes[0]])
        if self.variant_stats_from is not None:
            st.update(self.variant_stats_from(host[:self.sizes[0]]))
        off = self.sizes[0]
        vals = {}
        for k, n in zip(self.keys, self.sizes[1:]):
            vals[k] = host[off:off + n].double()
            off += n

        def block(name, v):
            st[name + "/mean"] = float(v.mean())
            st[name + "/max"], st[name + "/min"] = float(v.max()), float(v.min())
            st[name + "/std"] = float(v.std()) if v.numel() > 1 else math.nan      # torch.std of one value: nan, as logged

        for k in ("loss", "loss_x", "loss_a"):
            if k in vals:
                v = vals[k]
                if self.subscore and k != "loss":
                    v = v[vals["rows_" + k[-1]] > 0]
                    if v.numel() == 0:
                        v = torch.zeros(1, dtype=torch.float64)                 # ddpm_deletion_loss.py:113-120
                block(k, v)
        for k in ("iw_x", "iw_a"):
            if k in vals:
                block("importance_weight_" + k[-1], vals[k])
        if self.superfactor is not None:
            st["superfactor"] = self.superfactor
        return st

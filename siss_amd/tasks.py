"""Task classes behind the reference's entry points (main.py:9-35): ``Task.run()``,
``delete_celeb.DeleteCeleb(cfg)``, ``delete_tshirt.DeleteTShirt(cfg)``, ``delete_sd.DeleteSD(cfg)``, and the pre-training task
``train_unconditional.TrainUnconditional(cfg)`` that produces the T-shirt experiment's base checkpoint.

The loop is the hot path of delete_celeb.py:557-773 / delete_tshirt.py:501-717 driven through
``SISSStepper`` (fused kernels, one dual-cotangent backward, one collective per optimizer step).
Evaluation / sampling / wandb (log_metrics, delete_celeb.py:484-545) are outside this path; the
per-step scalars the reference logs are returned by ``stepper.stats()`` and written as JSON lines.
"""
import contextlib
import json
import os
import time
from abc import ABC, abstractmethod

import torch

from . import hydra_lite
from .config import UNet2DConditionConfig, UNet2DConfig
from .data import IndexBatch, InfiniteSampler, Prefetcher, RepeatedSampler, SyntheticImages, batches, index_batches
from .records import LaggedLog, append_jsonl
from .scheduler import DDPMScheduler
from .step import SISSStepper


class Task(ABC):
    default_unet = staticmethod(UNet2DConfig.celebahq256)
    unet_engine = "siss_amd.unet.UNetEngine"

    def __init__(self, cfg):
        self.cfg = cfg

    @abstractmethod
    def run(self):
        pass

    def compute_dtype(self):
        """`mixed_precision: null` -- the reference's shipped default: fp32 everywhere (delete_celeb.yaml:103) -- runs the f32 engine
        (every tensor and product f32: the parity mode, 1/16 of the bf16 MFMA rate at best); `bf16` the bf16 MFMA path."""
        mp = self.cfg.get("mixed_precision")
        if mp == "bf16":
            return torch.bfloat16
        if mp not in (None, "no", "null", "None"):
            # the reference's YAML lists fp16 / fp8 as choices of accelerate; there is no fp16 path here (and no loss scaler in the
            # reference's loop either): refuse instead of silently running something else
            raise NotImplementedError(f"mixed_precision={mp!r}: this build computes in 'bf16' or in f32 (null / 'no'); "
                                      "fp16 / fp8 are not provided")
        print("[siss_amd] mixed_precision is null / 'no': true f32 compute for the UNet, the loss and the optimizer (the reference's "
              "default; a parity mode here, far slower than mixed_precision=bf16, which is what the benchmark runs; the SD front end -- "
              "VAE / text encoder -- stays bf16)")
        return torch.float32

    # -- the UNet's configuration, resolved in one place: what load_unet() builds from ---------------------------------------------
    def unet_checkpoint(self):
        """The directory whose config.json and weights load_unet() reads, or None (no checkpoint on disk: cfg.unet / default_unet)."""
        return None

    def unet_config(self):
        """The configuration of the UNet the task builds, from the host alone (no device, no weights): the checkpoint's config.json
        when the checkpoint is on disk, else cfg.unet without its `_`-prefixed keys, else the task's default architecture."""
        cls = type(self.default_unet())
        d = self.unet_checkpoint()
        if d is not None:
            return cls.from_json(os.path.join(d, "config.json"))
        raw = {k: v for k, v in (self.cfg.get("unet") or {}).items() if not k.startswith("_")}
        return cls.from_dict(raw) if raw else self.default_unet()

    def unet_param_specs(self):
        """{name: PSpec} of that UNet, from its configuration alone."""
        import importlib
        mod, name = self.unet_engine.rsplit(".", 1)
        return getattr(importlib.import_module(mod), name).param_specs(self.unet_config())

    def unet_param_names(self):
        """The diffusers parameter names of that UNet."""
        return list(self.unet_param_specs())

    def _image_channels(self):
        return self.unet_config().in_channels


def _dist():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    pg = None
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        pg = dist.group.WORLD
    return world, rank, local, pg


def _sscd_normalize(node, what):
    """(mean, std) of `<what>.data_transforms`: null, or a Compose of exactly one Normalize with one or three means and non-zero
    stds (the ToTensor in front of it is part of the fused preprocessing)."""
    from .data import Compose, Normalize
    mean, std = [0.0], [1.0]
    if node is not None:
        tf = hydra_lite.instantiate(node) if isinstance(node, dict) and "_target_" in node else node
        ts = tf.transforms if isinstance(tf, Compose) else None
        if ts is None or len(ts) != 1 or not isinstance(ts[0], Normalize):
            raise ValueError(f"{what}.data_transforms={node!r}: null or a Compose of exactly one Normalize is needed "
                             "(ToTensor and the normalisation run fused on the device)")
        mean, std = list(ts[0].mean), list(ts[0].std)
        if len(mean) not in (1, 3) or len(std) not in (1, 3) or not all(float(v) != 0 for v in std):
            raise ValueError(f"{what}.data_transforms: Normalize(mean={mean}, std={std}) needs one or three means and "
                             "non-zero stds")
    return mean, std


def _load_sscd(path, allow_random_init, what):
    """The SSCDModel of `<what>.model_path`: the file when it is on disk, else (allow_random_init) a random-init network, loudly."""
    from .sscd import SSCDModel
    if os.path.isfile(str(path)):
        return SSCDModel.load(str(path))
    if not allow_random_init:
        raise FileNotFoundError(f"{what}.model_path {path!r} is not a file on disk (pass allow_random_init=true for "
                                "random-init weights of the same architecture)")
    print(f"[siss_amd] allow_random_init: SSCD checkpoint {path!r} not on disk, RANDOM-INIT ResNet-50: the SSCD figures are "
          "NOT comparable with published ones")
    return SSCDModel()


def _open_image_stores(task, cfg, datasets, device):
    """The image stores of a task: `datasets` {which: dataset} -> task.<which>_store, all of them or none (siss_amd/image_store.py)."""
    from .image_store import ImageStore, has_rule, parse_config
    ic = parse_config(cfg.get("image_store"))
    if ic is None:
        return
    without = [f"{which} ({type(ds).__name__})" for which, ds in datasets.items() if not has_rule(ds)]
    if without:
        print(f"[siss_amd] image_store.enabled is set but unused: the dataset(s) {', '.join(without)} hold no raw uint8 images "
              "(synthetic or pre-built tensors): the batches are produced as without it")
        return
    for which, ds in datasets.items():
        store = ImageStore(ds, device=device, max_bytes=ic["max_bytes"], workers=ic["workers"], name=f"image store ({which})")
        setattr(task, f"{which}_store", store)
        print(f"[siss_amd] {store.name}: {store.n} images x {store.shape} uint8, {store.nbytes} bytes on {device}")


def _inference_steps(cfg):
    return int(((cfg.get("pipeline") or {}).get("num_inference_steps")) or 50)


def _positive_int(v):
    return isinstance(v, int) and not isinstance(v, bool) and v > 0


def _scheduler_kwargs(cfg):
    sc = cfg.get("scheduler") or {}
    return {k: sc[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type") if k in sc}


def _start_hooks(built):
    """The loop's metric hooks [(every, fn)] from an iterable of them (a generator: the next one is built only when it is asked
    for), each called with step 0 -- before the first optimizer step -- as it arrives.  None is no hook; (None, None) says that
    metric was the whole run (membership_loss.plot_params): None is returned, and nothing later is built or called."""
    hooks = []
    for hook in built:
        if hook == (None, None):
            return None
        if hook is not None:
            hook[1](0)
            hooks.append(hook)
    return hooks


def _run_hooks(hooks, global_step):
    for every, fn in hooks:
        if global_step % every == 0:
            fn(global_step)


def _pipeline_sampler(cfg, base=None, **defaults):
    """`pipeline.sampler` (OPT-IN, null by default): {name: dpmsolver++, solver_order, timestep_spacing, steps_offset} -> the
    DPMSolverMultistepScheduler the evaluation sampling then runs pipeline.num_inference_steps steps of, or None -- the task's own
    DDPM / DDIM sampling, launch for launch what it was.  base: where the betas come from (the task's noise scheduler; for SD the
    checkpoint's scheduler_config.json).  Another name is a ValueError, an option the solver does not implement a
    NotImplementedError.  Every record written from such samples carries {"sampler", "num_inference_steps"}: they are another
    protocol than the reference's and must not be mixed with its numbers silently."""
    from .scheduler import DPMSolverMultistepScheduler
    solver = DPMSolverMultistepScheduler.from_sampler_config((cfg.get("pipeline") or {}).get("sampler"), base, **defaults)
    if solver is not None:
        solver.set_timesteps(_inference_steps(cfg))              # (a step count the grid cannot hold is refused here too)
    return solver


def _sampler_fields(cfg, solver):
    return None if solver is None else solver.record_fields(_inference_steps(cfg))


def _built_on_rank0(failed, build, describe, empty, tensor_of, save_dir, rank, world, pg, check=None):
    """An object the run builds once from its data, the same on every rank (the saliency mask, the Fisher anchor): rank 0 alone runs
    build(); the others learn FIRST whether it did -- describe(obj), or the error as a string: a refusal (a zero threshold, a non-finite
    or all-zero F, a file of another layout) is raised on every rank, so nobody waits in a broadcast for values that never come --
    then make empty(description) and receive tensor_of(obj); check(obj, description) runs on every rank after the broadcast; rank 0
    saves into save_dir.  failed: how the other ranks' error begins."""
    if world == 1:
        obj = build()
    else:
        import torch.distributed as dist
        obj, err = None, None
        if rank == 0:
            try:
                obj = build()
            except Exception as e:
                err = e
        word = [None if rank != 0 else (f"{type(err).__name__}: {err}" if err is not None else describe(obj))]
        dist.broadcast_object_list(word, src=0, group=pg)
        if isinstance(word[0], str):
            raise err if err is not None else RuntimeError(f"{failed} ({word[0]})")
        if rank != 0:
            obj = empty(word[0])
        dist.broadcast(tensor_of(obj), src=0, group=pg)
        if check is not None:
            check(obj, word[0])
    if rank == 0:
        obj.save(save_dir)
    return obj


class _DeleteBase(Task):
    timestep_low = 999          # delete_celeb.py:593 hard-codes randint(999, 1000)
    inf_guard = False

    # -- pieces a subclass may override --------------------------------------------------------
    def unet_checkpoint(self):
        path = str(self.cfg.get("checkpoint_path") or "")
        if not os.path.isdir(path):
            return None
        sub = (self.cfg.get("subfolders") or {}).get("unet")
        d = os.path.join(path, sub) if sub else path
        if not os.path.exists(os.path.join(d, "config.json")) and os.path.exists(os.path.join(path, "unet")):
            d = os.path.join(path, "unet")                           # (UNet2DModel.from_pretrained's fall-back)
        return d

    def load_unet(self, device):
        from .model import UNet2DModel
        cfg = self.cfg
        path = cfg.get("checkpoint_path")
        dt = self.compute_dtype()
        if self.unet_checkpoint() is not None:
            sub = (cfg.get("subfolders") or {}).get("unet")
            return UNet2DModel.from_pretrained(path, subfolder=sub, device=device, compute_dtype=dt)
        # The reference hard-fails here (DDPMPipeline.from_pretrained, delete_celeb.py:181).  Random-init weights of the
        # same architecture are for benchmarks / smoke runs only and must be asked for: allow_random_init=true.
        if not cfg.get("allow_random_init"):
            raise FileNotFoundError(
                f"checkpoint_path {path!r} is not a directory on disk (no network: hub ids cannot be fetched); "
                "pass allow_random_init=true to train random-init weights of the configured architecture instead")
        m = UNet2DModel(self.unet_config(), device=device, compute_dtype=dt)
        m.engine.init_random(seed=int(cfg.random_seed))
        print(f"[siss_amd] allow_random_init: checkpoint {path!r} not on disk, RANDOM-INIT weights of the same architecture")
        return m

    def load_scheduler(self):
        return DDPMScheduler(**_scheduler_kwargs(self.cfg))

    def datasets(self, shape):
        cfg = self.cfg
        try:
            if cfg.get("dataset_all") is None or cfg.get("dataset_deletion") is None:
                raise FileNotFoundError("no dataset_all / dataset_deletion configured")
            transform = hydra_lite.instantiate(cfg.transform)
            ds_all = hydra_lite.instantiate(cfg.dataset_all, transform=transform)
            ds_del = hydra_lite.instantiate(cfg.dataset_deletion, transform=transform)
            return ds_all, ds_del
        except FileNotFoundError as e:
            # Only a MISSING dataset can be replaced, and only when asked for (allow_synthetic=true: benchmarks / smoke
            # runs; the datasets are not in the repo, reference .gitignore:7).  Every other error -- a typo in a target,
            # a bad transform, a decode failure -- surfaces, as it does in the reference.
            if not cfg.get("allow_synthetic"):
                raise
            print(f"[siss_amd] allow_synthetic: dataset unavailable ({e}); using SYNTHETIC images")
            return SyntheticImages(4096, shape, seed=1), SyntheticImages(1, shape, seed=2)

    def check_supported(self):
        """Refuse, loudly, the configured features of the reference loop this loop does not implement -- rather than
        run something else than what the config says."""
        cfg = self.cfg
        ema = cfg.get("ema") or {}
        if ema.get("use_ema") or cfg.get("use_ema"):
            raise NotImplementedError("ema.use_ema=true: EMA of the unlearned weights is not implemented "
                                      "(delete_celeb.py:235-251; every shipped delete config has it off)")
        for key in ("checkpointing_steps", "resume_from_checkpoint"):
            if cfg.get(key) not in (None, "null", False, 0):
                raise NotImplementedError(f"{key}={cfg.get(key)!r}: accelerate-state checkpoints are not implemented "
                                          "(delete_celeb.py:786-825; null in every shipped delete config); the final model "
                                          "is written in the diffusers layout")
        if cfg.get("mixed_precision") not in (None, "null", "no", "bf16"):
            raise NotImplementedError(f"mixed_precision={cfg.get('mixed_precision')!r}: only null / bf16 (no loss scaler)")
        _pipeline_sampler(cfg)                                   # pipeline.sampler: a bad name / option is refused before the first step
        # deletion.teacher / loss_fn=teacher_target: each without the other, a task whose forget target is not defined through prompts, a
        # malformed mapping, an unknown field or value, the key together with deletion.trainable / saliency / ewc / surgery, a path
        # without unet/ and (DeleteSD) an anchor prompt that cannot be embedded are settled here, before the other keys speak
        self.teacher_config()
        # deletion.ssd: a malformed mapping, an unknown field, both or neither of alpha / fraction, a value out of range, a targets entry
        # that matches no parameter of the configured UNet and the key together with deletion.lora / deletion.trainable (said first: what
        # those two select does not matter then) are settled here
        sc = self.ssd_config()
        if sc is not None:
            from .ssd import select_targets as ssd_targets
            ssd_targets(self.unet_param_names(), sc.targets)
        # deletion.uce: a task without cross-attention, a malformed mapping, an unknown field, a missing or empty edit list, a value out of
        # range, a target that matches nothing or is no [*, cross_attention_dim] matrix, a prompt that cannot be embedded and the key
        # together with deletion.lora are settled here
        self.uce_check()
        # deletion.trainable: a malformed entry, an entry that matches no parameter of the configured UNet and a selection of every
        # parameter (said, then the full update) are settled here, from the parameter names the configuration implies
        from .trainable import select
        pats = self.trainable_patterns()
        if pats is not None:
            select(self.unet_param_names(), pats)
        # deletion.lora: a malformed mapping, a rank outside 1..64, a target that matches nothing or is no linear / 1x1 weight, a conv
        # target that is no 3x3 convolution's weight, and the key together with deletion.trainable are settled here too
        lcfg = self.lora_config()
        if lcfg is not None:
            from .lora import resolve_targets
            resolve_targets(self.unet_param_specs(), lcfg)
        # deletion.saliency: a malformed mapping, an unknown field, a fraction outside (0, 1), batches < 1 and the key together with
        # deletion.trainable / deletion.lora are settled here too
        self.saliency_config()
        # deletion.ewc: a malformed mapping, an unknown field, a missing or non-positive strength, batches / batch_size < 1 and the key
        # together with deletion.trainable / deletion.lora / deletion.saliency are settled here too
        self.ewc_config()
        # deletion.surgery: a malformed mapping, an unknown field or value, the key together with deletion.trainable / deletion.lora /
        # deletion.saliency / deletion.ewc, and a loss without a gradient pair under the norm fix are settled here too
        self.surgery_config()

    # -- deletion.teacher: null | {forget, keep, guidance, weight, anchor_prompt, path} (OPT-IN; siss_amd/teacher.py) -----------------------
    teacher_refusal = "both forget targets (esd, anchor) are defined through prompts, and this task's UNet takes none"

    def teacher_config(self):
        """The parsed deletion.teacher (siss_amd.teacher.TeacherConfig) of a loss_fn=teacher_target run, or None (neither is set: today's
        run).  The task says in `teacher_refusal` why it does not take the key (None: it does -- delete_sd)."""
        from .teacher import KEY, LOSS, check_path, parse_teacher
        d = self.cfg.get("deletion") or {}
        value, loss = d.get("teacher"), d.get("loss_fn")
        if value is None and loss != LOSS:
            return None
        if self.teacher_refusal is not None:
            raise NotImplementedError(f"{KEY} / deletion.loss_fn={LOSS}: {self.teacher_refusal} (the teacher target belongs to delete_sd)")
        if value is None:
            raise ValueError(f"deletion.loss_fn={LOSS} needs the key {KEY} (e.g. +{KEY}={{forget:esd,keep:teacher}})")
        if loss != LOSS:
            raise ValueError(f"{KEY} is set but deletion.loss_fn={loss!r}: the teacher serves deletion.loss_fn={LOSS} only (set it, or "
                             "leave the key out)")
        tc = parse_teacher(value, trainable=d.get("trainable"), saliency=d.get("saliency"), ewc=d.get("ewc"), surgery=d.get("surgery"))
        if tc.path is not None:
            check_path(tc.path)
        return tc

    def build_teacher(self, eng, device, rank=0):
        """(Teacher, TeacherConfig) of a loss_fn=teacher_target run -- built from the weights the run loaded, before anything touches them
        -- or (None, None)."""
        tc = self.teacher_config()
        if tc is None:
            return None, None
        from .teacher import Teacher
        teacher = Teacher.from_path(eng, tc.path) if tc.path is not None else Teacher(eng)
        teacher.set_embeddings(**self.teacher_embeddings(tc, device))
        teacher.cfg = tc
        if rank == 0:
            os.makedirs(self.cfg.output_dir, exist_ok=True)
            teacher.save_config(self.cfg.output_dir, tc)
            print(f"[siss_amd] deletion.teacher: forget {tc.forget}, keep {tc.keep}, guidance {tc.guidance:g}, weight {tc.weight:g}; a frozen "
                  f"copy of the UNet from {teacher.source}, {teacher.nbytes} bytes")
        return teacher, tc

    def teacher_embeddings(self, tc, device):
        raise NotImplementedError(self.teacher_refusal)

    # -- deletion.surgery: null | {mode, granularity} (OPT-IN; siss_amd/surgery.py) ------------------------------------------------------
    def surgery_config(self):
        """The parsed deletion.surgery (siss_amd.surgery.SurgeryConfig), or None (absent / null: the plain update, today's run)."""
        from .surgery import check_loss, parse_surgery
        d = self.cfg.get("deletion") or {}
        sc = parse_surgery(d.get("surgery"), trainable=d.get("trainable"), lora=d.get("lora"), saliency=d.get("saliency"),
                           ewc=d.get("ewc"))
        if sc is not None:
            check_loss(d.get("loss_fn"))
        return sc

    # -- deletion.uce: null | {edit, preserve, preserve_file, lambda, edit_scale, preserve_scale, targets, path} (OPT-IN; siss_amd/uce.py) ----
    uce_refusal = "no cross-attention: this task's UNet takes no prompt, and the edit rewrites the key / value projections of one"

    def uce_config(self):
        """The parsed deletion.uce (siss_amd.uce.UCEConfig), or None (absent / null: no edit, today's run).  The task says in
        `uce_refusal` why it does not take the key (None: it does -- delete_sd)."""
        from .uce import KEY, parse_uce
        d = self.cfg.get("deletion") or {}
        if d.get("uce") is None:
            return None
        if self.uce_refusal is not None:
            raise NotImplementedError(f"{KEY}: {self.uce_refusal} (Unified Concept Editing belongs to delete_sd)")
        return parse_uce(d.get("uce"), lora=d.get("lora"))

    def uce_check(self):
        self.uce_config()

    def uce_edit(self, stepper, device, rank, world, pg):
        return None

    # -- deletion.ssd: null | {alpha, fraction, lambda, keep_batches, forget_batches, batch_size, seed, targets, path} (OPT-IN; siss_amd/ssd.py)
    def ssd_config(self):
        """The parsed deletion.ssd (siss_amd.ssd.SSDConfig), or None (absent / null: no dampening, today's run)."""
        from .ssd import parse_ssd
        d = self.cfg.get("deletion") or {}
        return parse_ssd(d.get("ssd"), trainable=d.get("trainable"), lora=d.get("lora"))

    def ssd_forget_batches(self, ds_del, bs):
        """saliency_batches at the micro-batch size of the importances."""
        src = getattr(self, "forget_cache", None) or self.forget_store
        if src is not None:
            return index_batches(self.deletion_sampler(ds_del, bs), bs, src)
        return batches(ds_del, self.deletion_sampler(ds_del, bs), bs)

    def ssd_dampen(self, stepper, ds_all, ds_del, B, cond, device, rank, world, pg):
        """Selective Synaptic Dampening of the run (None without the key), once, at the weights the run loaded, before the mask, the
        anchor and the step-0 metrics: the importances loaded from `path` when both files are there, else F_keep on `keep_batches`
        micro-batches of `batch_size` from a keep iterator of its own and then F_forget on `forget_batches` from a forget iterator
        of its own (the task's prepare_batch, sample_noise and conditioning, timesteps uniform in [timestep_low, T), ONE generator
        seeded with `seed` -- the loop's iterators and generator are not advanced); then the selection, the dampening and the
        report.  More than one rank: rank 0 alone builds or loads the importances, the ranks agree on success, the ratio is broadcast,
        every rank selects and dampens and checks its selected count against rank 0's.  Rank 0 writes the two files into output_dir.
        Returns the fields every train-log line carries."""
        sc = self.ssd_config()
        if sc is None:
            return None
        from . import ssd
        eng = stepper.e
        bs = int(sc.batch_size)
        out = str(self.cfg.output_dir)

        def build():
            if sc.path is not None and ssd.Importances.present(sc.path):
                imp = ssd.Importances.load(sc.path, eng)
                print(f"[siss_amd] deletion.ssd: importances loaded from {sc.path}")
                return imp
            if sc.path is not None:
                print(f"[siss_amd] deletion.ssd.path {sc.path!r} holds no importance files: computing the importances")
            gen = torch.Generator(device=device).manual_seed(sc.seed)
            it_keep = self.ewc_batches(ds_all, bs, device)
            try:
                cond_b = cond if bs == B else self.conditioning(bs, device)
                imp = ssd.Importances.from_batches(stepper, it_keep, self.ssd_forget_batches(ds_del, bs), sc.keep_batches,
                                                   sc.forget_batches, prepare=self.prepare_batch, sample_noise=self.sample_noise,
                                                   conditioning=cond_b, timestep_low=self.timestep_low, generator=gen, batch_size=bs,
                                                   seed=sc.seed)
            finally:
                it_keep.close()
            print(f"[siss_amd] deletion.ssd: empirical Fishers of {sc.keep_batches} keep and {sc.forget_batches} forget micro-batches "
                  f"of {bs}")
            return imp

        def empty(c):
            z = torch.zeros_like(eng.ps.flat)
            return ssd.Importances(eng, z, z, ratio=torch.zeros_like(z),
                                   **{k: c[k] for k in ("keep_batches", "forget_batches", "batch_size", "seed", "source")})

        imp = _built_on_rank0("deletion.ssd: rank 0 could not build the importances", build, ssd.Importances.config, empty,
                              lambda imp: imp.ratio, out, rank, world, pg)
        names = ssd.select_targets(list(eng.ps.specs), sc.targets)
        thr, strict, k, count_gt, count_ge = ssd.select(imp, alpha=sc.alpha, fraction=sc.fraction, targets=names)
        stats = ssd.dampen(eng, imp, thr, strict, sc.lam, apply=True)
        if world > 1:
            import torch.distributed as dist
            word = [stats["selected"] if rank == 0 else None]
            dist.broadcast_object_list(word, src=0, group=pg)
            if word[0] != stats["selected"]:
                raise RuntimeError(f"deletion.ssd: rank {rank} dampened {stats['selected']} weights, rank 0 {word[0]}")
        if rank == 0:
            imp.save_report(out, dict(config=sc.as_dict(), threshold=thr, threshold_bits=ssd.float_bits(thr), strict=bool(strict), k=k,
                                      count_gt=count_gt, count_ge=count_ge, stats=stats, per_tensor=ssd.per_tensor(imp, thr, strict)))
            print(f"[siss_amd] deletion.ssd: ratio {'>' if strict else '>='} {thr:.6g} selects {stats['selected']} of {imp.params} "
                  f"parameters ({stats['dampened']} dampened, {stats['zeroed']} to zero, mean beta {stats['mean_beta']}), relative "
                  f"change of the weights {stats['relative_change']:.6g}")
        return dict(ssd_selected=stats["selected"], ssd_threshold=thr, ssd_lambda=sc.lam)

    # -- deletion.ewc: null | {strength, batches, batch_size, seed, normalize, path} (OPT-IN; siss_amd/ewc.py) -------------------------
    def ewc_config(self):
        """The parsed deletion.ewc (siss_amd.ewc.EWCConfig), or None (absent / null: no anchor, today's run)."""
        from .ewc import parse_ewc
        d = self.cfg.get("deletion") or {}
        return parse_ewc(d.get("ewc"), trainable=d.get("trainable"), lora=d.get("lora"), saliency=d.get("saliency"))

    def ewc_batches(self, ds_all, bs, device):
        """A SEPARATE iterator (with close()) over the keep dataset for the Fisher estimate (the loop's own keep iterator is not
        advanced): the rows of the keep store / latent cache the loop opened, or the dataset itself through a prefetcher of its own."""
        src = getattr(self, "keep_cache", None) or self.keep_store
        if src is not None:
            return index_batches(InfiniteSampler(ds_all, rank=0, num_replicas=1), bs, src)
        return _DeleteBase.keep_batches(self, ds_all, bs, 0, 1, device)

    def ewc_anchor(self, stepper, ds_all, B, cond, device, rank, world, pg):
        """The FisherAnchor of the run (None without the key), built once, at the pretrained weights, before step 1: F loaded from
        `path` when both files are there, else the empirical Fisher of the keep eps-MSE on `batches` keep micro-batches of
        `batch_size` (null: train_batch_size) from a keep iterator of its own (keep_batches: with an image store or a latent cache on,
        the index batches go to prepare_batch unchanged), the task's prepare_batch, sample_noise and conditioning, timesteps uniform in
        [timestep_low, T), and a generator of its own seeded with `seed` -- the loop's iterators and generator are not advanced.  More
        than one rank: rank 0 alone builds F, the ranks agree on success, then F is broadcast.  Rank 0 writes the two files into
        output_dir."""
        ec = self.ewc_config()
        if ec is None:
            return None
        from .ewc import FisherAnchor
        eng = stepper.e
        bs = int(ec.batch_size or B)

        def build():
            if ec.path is not None and FisherAnchor.present(ec.path):
                anchor = FisherAnchor.load(ec.path, eng, ec.strength)
                print(f"[siss_amd] deletion.ewc: Fisher loaded from {ec.path} (strength {ec.strength:g})")
                return anchor
            if ec.path is not None:
                print(f"[siss_amd] deletion.ewc.path {ec.path!r} holds no Fisher files: computing the Fisher")
            gen = torch.Generator(device=device).manual_seed(ec.seed)
            it = self.ewc_batches(ds_all, bs, device)
            try:
                cond_b = cond if bs == B else self.conditioning(bs, device)
                anchor = FisherAnchor.from_batches(stepper, it, ec.batches, strength=ec.strength, prepare=self.prepare_batch,
                                                   sample_noise=self.sample_noise, conditioning=cond_b,
                                                   timestep_low=self.timestep_low, generator=gen, normalize=ec.normalize,
                                                   batch_size=bs, seed=ec.seed)
            finally:
                it.close()
            print(f"[siss_amd] deletion.ewc: empirical Fisher of {ec.batches} keep micro-batches of {bs} (mean {anchor.mean:.6g}, max "
                  f"{anchor.max:.6g}, {anchor.zeros} zeros before normalisation), strength {ec.strength:g}")
            return anchor

        def empty(c):
            return FisherAnchor(eng, torch.zeros_like(eng.ps.flat), eng.ps.flat.detach().clone(), ec.strength,
                                **{k: c[k] for k in ("batches", "batch_size", "seed", "normalize", "mean", "max", "zeros", "source")})

        return _built_on_rank0("deletion.ewc: rank 0 could not build the Fisher", build, FisherAnchor.config, empty,
                               lambda anchor: anchor.fisher, str(self.cfg.output_dir), rank, world, pg)

    # -- deletion.saliency: null | {fraction, batches, seed, path} (OPT-IN; siss_amd/saliency.py) --------------------------------------
    def saliency_config(self):
        """The parsed deletion.saliency (siss_amd.saliency.SaliencyConfig), or None (absent / null: the full update, today's run)."""
        from .saliency import parse_saliency
        d = self.cfg.get("deletion") or {}
        return parse_saliency(d.get("saliency"), trainable=d.get("trainable"), lora=d.get("lora"))

    def saliency_batches(self, ds_del, B):
        """A SEPARATE iterator over the forget dataset for the mask's gradient (the loop's own forget iterator is not advanced): the
        rows of the forget store / latent cache the loop opened, or the dataset itself."""
        src = getattr(self, "forget_cache", None) or self.forget_store
        if src is not None:
            return index_batches(self.deletion_sampler(ds_del, B), B, src)
        return batches(ds_del, self.deletion_sampler(ds_del, B), B)

    def saliency_mask(self, stepper, ds_del, B, cond, device, rank, world, pg):
        """The SaliencyMask of the run (None without the key), built once, at the pretrained weights, before step 1: loaded from
        `path` when both files are there, else computed on `batches` forget micro-batches (the task's own prepare_batch, sample_noise
        and conditioning `cond`, timesteps uniform in [timestep_low, T)) from a generator of its own seeded with `seed` -- the loop's
        samplers and generator are not advanced.  More than one rank: rank 0 alone builds it, its words are broadcast and every rank
        checks the count.  Rank 0 writes the two mask files into output_dir."""
        sc = self.saliency_config()
        if sc is None:
            return None
        from .saliency import SaliencyMask, count_bits, forget_gradient
        eng = stepper.e

        def build():
            if sc.path is not None and SaliencyMask.present(sc.path):
                mask = SaliencyMask.load(sc.path, eng)
                print(f"[siss_amd] deletion.saliency: mask loaded from {sc.path} ({mask.count} of {mask.params} parameters)")
                return mask
            if sc.path is not None:
                print(f"[siss_amd] deletion.saliency.path {sc.path!r} holds no mask files: computing the mask")
            gen = torch.Generator(device=device).manual_seed(sc.seed)
            g = forget_gradient(stepper, self.saliency_batches(ds_del, B), sc.batches, prepare=self.prepare_batch,
                                sample_noise=self.sample_noise, conditioning=cond, timestep_low=self.timestep_low, generator=gen)
            mask = SaliencyMask.from_gradient(eng, g, sc.fraction, batches=sc.batches, seed=sc.seed)
            print(f"[siss_amd] deletion.saliency: |g| >= {mask.threshold:.6g} keeps {mask.count} of {mask.params} parameters "
                  f"(k = {mask.k}, {sc.batches} forget micro-batches)")
            return mask

        def empty(c):
            bits = torch.zeros((eng.ps.total + 31) // 32, dtype=torch.int32, device=device)
            return SaliencyMask(eng, bits, c["count"], **{k: c[k] for k in ("k", "threshold", "fraction", "batches", "seed")})

        def same_count(mask, c):
            mine = count_bits(mask.bits)
            if mine != c["set_bits"]:
                raise RuntimeError(f"deletion.saliency: rank {rank} holds {mine} set bits after the broadcast, rank 0 holds {c['set_bits']}")

        return _built_on_rank0("deletion.saliency: rank 0 could not build the mask", build,
                               lambda mask: dict(mask.config(), set_bits=count_bits(mask.bits)), empty, lambda mask: mask.bits,
                               str(self.cfg.output_dir), rank, world, pg, check=same_count)

    # -- deletion.lora: null | {rank, alpha, targets, conv_targets, seed} (OPT-IN; siss_amd/lora.py) ------------------------------------------------
    def lora_config(self):
        """The parsed deletion.lora (siss_amd.lora.LoRAConfig), or None (absent / null: no adapter, today's run)."""
        from .lora import parse_lora
        d = self.cfg.get("deletion") or {}
        return parse_lora(d.get("lora"), trainable=d.get("trainable"))

    def lora_state(self, unet):
        """The LoRAState of the loaded `unet` under deletion.lora (None without the key)."""
        lcfg = self.lora_config()
        if lcfg is None:
            return None
        from .lora import LoRAState, resolve_targets
        names, conv_names = resolve_targets(unet.engine.ps.specs, lcfg)
        st = LoRAState(unet.engine, names, lcfg.rank, lcfg.alpha, lcfg.seed, conv_names=conv_names)
        st.base = str(self.cfg.get("checkpoint_path") or self.cfg.get("pretrained_model_name_or_path") or "") or None
        return st

    # -- deletion.trainable: null | [regular expressions over the diffusers parameter names] (OPT-IN; siss_amd/trainable.py) -----------
    def trainable_patterns(self):
        """The compiled expressions of deletion.trainable, or None (absent / null: every parameter, the reference's protocol).  Refused:
        anything but a list, an empty list, an entry that does not compile."""
        from .trainable import parse_patterns
        return parse_patterns((self.cfg.get("deletion") or {}).get("trainable"))

    def trainable_names(self, unet):
        """The parameter names deletion.trainable selects in the loaded `unet` (None: the full update -- no key, or a selection of
        everything).  check_supported() has refused an unmatched entry already; this is the same selection on the model's own names."""
        from .trainable import select
        return select([n for n, _ in unet.named_parameters()], self.trainable_patterns(), announce=False)

    def optimizer_args(self):
        """(lr, betas, eps, weight_decay) of the AdamW the reference instantiates from cfg.optimizer
        (delete_celeb.py:232)."""
        opt = hydra_lite.instantiate(self.cfg.optimizer)
        return opt.lr, opt.betas, opt.eps, opt.weight_decay

    def conditioning(self, B, device):
        """The dict the reference splats into the UNet call (delete_celeb.py:622: {})."""
        return None

    def lr_schedule_args(self, world):
        """(num_warmup_steps, num_training_steps) as the reference hands them to get_scheduler
        (delete_celeb.py:296-301: cfg.warmup_steps, cfg.training_steps)."""
        cfg = self.cfg
        return int(cfg.get("warmup_steps") or 0), int(cfg.get("training_steps") or 0)

    def sample_noise(self, shape, device, generator):
        """noise = torch.randn_like(images) (delete_celeb.py:583); the SAME noise for the keep and the forget batch."""
        return torch.randn(shape, device=device, generator=generator)

    def seed(self):
        return int(self.cfg.random_seed)

    def prepare_batch(self, x, generator):
        """Images -> what the loss is taken on (identity for the pixel-space tasks; VAE latents for SD).  image_store on: the batch is
        an IndexBatch, gathered from its store's rows in one launch -- the same bits as the stacked batch."""
        if isinstance(x, IndexBatch):
            return x.cache.images(x)
        return x

    # -- image_store: null | {enabled, max_bytes, workers} (OPT-IN; siss_amd/image_store.py) -----------------------------------
    keep_store = None
    forget_store = None

    def open_image_stores(self, ds_all, ds_del, device):
        """One ImageStore per dataset (keep, forget) when image_store is enabled and BOTH datasets have a rule for their raw bytes --
        on for both or for neither; each rank has its own, there are no collectives.  Synthetic and pre-built tensor datasets are
        left alone: one line says the store is enabled but unused, and why."""
        _open_image_stores(self, self.cfg, dict(keep=ds_all, forget=ds_del), device)

    def close_image_stores(self):
        for store in (self.keep_store, self.forget_store):
            if store is not None:
                store.close()                            # (its decode threads; the rows and the counters stay readable)

    def evaluate(self, unet, sched, forget_image, step, device):
        """The image part of the reference's log_metrics (delete_celeb.py:376-436, :484-545): `eval_batch_size`
        samples from the current model (DDPMPipeline, `pipeline.num_inference_steps`) and the forget image noised to
        `metrics.denoising_injections.timestep` and denoised back, written as PNG grids instead of wandb images.
        Runs every `eval_every` optimizer steps -- OPT-IN (null by default): the reference's `sampling_steps: 1`
        spends ~300 UNet forwards per optimizer step on it.  With `metrics.denoising_injections.sscd` (check_injection_score) the
        denoised injections are quantised on the device by the grid's own rule, those bytes go through the SSCD network against the
        forget image's embedding, and {global_step, timestep, sscd_mean, sscd_max, sscd} is appended to injection_rank0.jsonl; the
        grid is then made of the same bytes."""
        import numpy as np
        from PIL import Image
        from .sampler import Evaluator
        cfg = self.cfg
        ev = Evaluator(cfg)
        ev.load_model(unet, sched)
        n = int(cfg.get("eval_batch_size") or 4)
        imgs = ev.sample_images(n, num_inference_steps=_inference_steps(cfg), set_generator=True,           # [n, H, W, C] in [0, 1]
                                sampler=_pipeline_sampler(cfg, sched))
        inj = ((cfg.get("metrics") or {}).get("denoising_injections")) or {}
        t_inj = int(inj.get("timestep", 250))
        g = torch.Generator(device=device).manual_seed(self.seed())
        clean = forget_image.to(device).float()
        noise = torch.randn((n, *clean.shape), generator=g, device=device)
        noisy = sched.add_noise(clean.expand(n, *clean.shape), noise, torch.full((n,), t_inj, device=device))
        den = ev.denoise_images(noisy, t_inj)                                                # [n, H, W, C] in [0, 1], on the device
        if self.injection is not None:
            if den.shape[-1] != 3:
                raise ValueError(f"metrics.denoising_injections.sscd: the SSCD network takes 3-channel images, got {den.shape[-1]}")
            den = (den.clamp(0, 1) * 255).to(torch.uint8).contiguous()                       # grid()'s rule: truncation
            if self.replication is None:
                scores = self.injection.score_u8(den)
            else:                                            # score_u8's own launches, keeping the rows they normalise for the search
                sc = self.injection
                emb, scores = sc.model.embed_u8(den, sc.mean, sc.std, ref=sc.reference(den.device))
            self.injection.record(scores, step, t_inj)                                       # only the n scores leave the device
            if self.replication is not None:
                self.replication.record(f"t{t_inj}", emb, step)
        den = den.cpu().numpy()

        def grid(a):
            if a.dtype != np.uint8:
                a = (np.clip(a, 0, 1) * 255).astype(np.uint8)
            row = np.concatenate(list(a), axis=1)
            return Image.fromarray(row[..., 0] if row.shape[-1] == 1 else row)
        grid(imgs).save(os.path.join(cfg.output_dir, f"samples_step{step}.png"))
        grid(den).save(os.path.join(cfg.output_dir, f"denoised_forget_t{t_inj}_step{step}.png"))

    def likelihood_metric(self, unet, forget_image, device):
        """`metrics.likelihood` (class_cfg, step_frequency) of the reference's T-shirt config: the forget image's bits/dim under the
        current model (delete_tshirt.py:438-461).  OPT-IN (absent from the repo's configs): None when not configured.  Returns
        (step_frequency, log(global_step)); each evaluation appends {global_step, bpd, nfe, seconds} to likelihood_rank0.jsonl.
        The image is metrics.classifier.tshirt_path through cfg.transform when that file exists, else the first forget image.  The
        Hutchinson probe comes from a generator of its own, seeded from random_seed."""
        cfg = self.cfg
        metrics = cfg.get("metrics") or {}
        lk = metrics.get("likelihood")
        if not lk:
            return None
        from .likelihood import log_likelihood
        freq = int(lk.get("step_frequency") or 0)
        if freq <= 0:
            raise ValueError(f"metrics.likelihood.step_frequency={lk.get('step_frequency')!r}: a positive step count is needed")
        evaluator = hydra_lite.instantiate(lk.class_cfg)
        path = (metrics.get("classifier") or {}).get("tshirt_path")
        if path and os.path.isfile(str(path)):
            from PIL import Image
            image = hydra_lite.instantiate(cfg.transform)(Image.open(str(path)))
        else:
            image = forget_image
        image = image.to(device).float()
        gen = torch.Generator(device=device).manual_seed(self.seed())
        out = os.path.join(cfg.output_dir, "likelihood_rank0.jsonl")
        return freq, lambda global_step: log_likelihood(evaluator, unet, image, global_step, out, gen)

    def check_metrics(self):
        """Refuse, before the first step, a metrics block that cannot run (a host-side check: no GPU needed)."""
        self.check_membership()
        self.mia = self.check_mia()
        self.injection = self.check_injection_score()
        self.replication = self.check_sscd_nn()

    membership_supported = True
    mia_supported = True        # metrics.mia: the pixel-space tasks (no latent-space form of the attacks is built)
    mia = None                  # metrics.mia: its settings (check_mia), None when not configured
    injection = None            # the injection check's scorer / settings (check_injection_score), None when not configured
    replication = None          # metrics.sscd_nn: its settings (check_sscd_nn) until the index is there (open_replication), then the tracker

    def sscd_nn_sources(self):
        """What metrics.sscd_nn takes from the task: (the SSCD metric it needs, that metric's scorer or None, the default gallery
        directory, the forget images)."""
        cfg = self.cfg
        inj = (cfg.get("metrics") or {}).get("denoising_injections")
        inj = inj if isinstance(inj, dict) else {}
        ds = cfg.get("dataset_all")
        return ("metrics.denoising_injections.sscd", self.injection, ds.get("data_path") if isinstance(ds, dict) else None,
                [inj.get("img_path")])

    def check_sscd_nn(self):
        """metrics.sscd_nn: {index_path, data_path, k, threshold, batch_size} (OPT-IN, absent from the repo's configs): at each
        evaluation the images the SSCD metric embeds are also searched in an index of the whole gallery -- data_path (default: the
        dataset's image directory) plus the forget image(s), flagged -- and {global_step, tag, nn_mean, nn_max, nn_p95, above,
        nn_is_forget, nn_other_max, top} is appended to replication_rank0.jsonl (sscd_search.ReplicationScore).  Refused here, before
        the first step: the key without its SSCD metric, a missing data_path, k outside 1 .. 32, a threshold that is no finite number,
        an index_path that holds another model's index.  Returns the settings, or None."""
        nn = (self.cfg.get("metrics") or {}).get("sscd_nn")
        if nn is None:
            return None
        from .sscd_search import parse_config
        need, scorer, default_dir, forget = self.sscd_nn_sources()
        settings = parse_config(nn, need, scorer, default_dir, forget, os.path.join(str(self.cfg.output_dir), "replication_rank0.jsonl"))
        self._note_eval_every("metrics.sscd_nn", "the search runs")
        return settings

    def open_replication(self, device):
        """Rank 0, once, before step 0: the index of metrics.sscd_nn loaded from index_path, or built and saved there."""
        if isinstance(self.replication, dict):
            from .sscd_search import open_index
            self.replication = open_index(self.replication, device)

    def check_injection_score(self):
        """metrics.denoising_injections.sscd: {model_path, data_transforms} (null / absent: nothing): the SSCD similarity of the
        denoised injections with the forget image.  Needs model_path on disk (or allow_random_init=true, there or at the top level:
        a random-init network, loudly), data_transforms null or a Compose of exactly one Normalize, a 3-channel UNet, and the forget
        image at metrics.denoising_injections.img_path (the reference's key) on disk -- refused here, before the first step.
        Returns the sscd.InjectionScore, or None."""
        cfg = self.cfg
        inj = (cfg.get("metrics") or {}).get("denoising_injections")
        sc = inj.get("sscd") if isinstance(inj, dict) else None
        if not sc:
            return None
        what = "metrics.denoising_injections.sscd"
        path = sc.get("model_path") if isinstance(sc, dict) else None
        if not path:
            raise ValueError(f"{what}={sc!r}: model_path is needed (sscd_disc_mixup.torchscript.pt, or a state dict of it)")
        mean, std = _sscd_normalize(sc.get("data_transforms"), what)
        ch = self._image_channels()
        if ch != 3:
            raise ValueError(f"{what}: the SSCD network takes 3-channel images, the UNet has in_channels={ch!r}")
        img = inj.get("img_path")
        if not img or not os.path.isfile(str(img)):
            raise FileNotFoundError(f"{what}: metrics.denoising_injections.img_path {img!r} (the forget image the injections are "
                                    "compared with) is not a file on disk")
        model = _load_sscd(path, sc.get("allow_random_init") or cfg.get("allow_random_init"), what)
        self._note_eval_every(what, "the score is taken")
        from .sscd import InjectionScore
        return InjectionScore(model, str(img), os.path.join(str(cfg.output_dir), "injection_rank0.jsonl"), mean, std)

    def _note_eval_every(self, what, happens):
        if not self.cfg.get("eval_every"):
            print(f"[siss_amd] {what} is set but eval_every is not: {happens} at evaluations only")

    def check_membership(self, n_all=None, n_deletion=None):
        """metrics.membership_loss needs class_cfg, a positive step_frequency (unless plot_params stops the run before the first
        step), a non-empty timesteps list within [0, num_train_timesteps) and -- once the datasets' lengths are known -- no more
        num_image_samples than random.sample can draw from either of them (a forget set of length 1 is repeated instead)."""
        cfg = self.cfg
        ml = (cfg.get("metrics") or {}).get("membership_loss")
        if not ml:
            return None
        if not self.membership_supported:
            raise NotImplementedError("metrics.membership_loss: built for the pixel-space tasks (DeleteCeleb, DeleteTShirt) only")
        cc = ml.get("class_cfg")
        if not cc:
            raise ValueError("metrics.membership_loss needs class_cfg (metrics.class_membership.MembershipLoss and its sample counts)")
        T = int((cfg.get("scheduler") or {}).get("num_train_timesteps", 1000))
        plot = ml.get("plot_params")
        if plot:
            if not _positive_int(plot.get("time_frequency")):
                raise ValueError(f"metrics.membership_loss.plot_params.time_frequency={plot.get('time_frequency')!r}: a positive "
                                 "timestep stride is needed")
        else:
            if not _positive_int(ml.get("step_frequency")):
                raise ValueError(f"metrics.membership_loss.step_frequency={ml.get('step_frequency')!r}: a positive step count is needed")
            ts = ml.get("timesteps")
            if not isinstance(ts, list) or len(ts) == 0:
                raise ValueError(f"metrics.membership_loss.timesteps={ts!r}: a non-empty list of timesteps is needed")
            bad = [t for t in ts if not (isinstance(t, int) and not isinstance(t, bool) and 0 <= t < T)]
            if bad:
                raise ValueError(f"metrics.membership_loss.timesteps: {bad} outside [0, num_train_timesteps = {T})")
        for key in ("num_image_samples", "num_noise_samples", "eval_batch_size"):
            if not _positive_int(cc.get(key)):
                raise ValueError(f"metrics.membership_loss.class_cfg.{key}={cc.get(key)!r}: a positive count is needed")
        n = cc.get("num_image_samples")
        for what, have in (("dataset_all", n_all), ("dataset_deletion", n_deletion)):
            if have is not None and n > have and not (what == "dataset_deletion" and have == 1):
                raise ValueError(f"metrics.membership_loss.class_cfg.num_image_samples={n} is larger than {what} ({have} images): "
                                 "random.sample cannot draw that many")
        return ml

    def membership_metric(self, unet, sched, ds_all, ds_del, device):
        """`metrics.membership_loss` (class_cfg, timesteps, step_frequency, plot_params) of the reference's configs
        (delete_celeb.py:438-462, :512-518).  OPT-IN (absent from the repo's configs): None when not configured.  The images and the
        noises are drawn ONCE, here (the noises from a generator of its own, seeded from random_seed).  Returns
        (step_frequency, log(global_step)); each evaluation appends {global_step, seconds, all_membership_loss_t=<t>,
        deletion_membership_loss_t=<t>, membership_ratio_t=<t>} to membership_rank0.jsonl.  With plot_params the kept-group curve over
        range(0, num_train_timesteps, time_frequency) goes to membership_curve_rank0.json and (None, None) is returned: the run
        stops there, as the reference's does."""
        cfg = self.cfg
        ml = self.check_membership(len(ds_all), len(ds_del))
        if not ml:
            return None
        from .membership import log_membership
        metric = hydra_lite.instantiate(ml.class_cfg, dataset_all=ds_all, dataset_deletion=ds_del, noise_scheduler=sched, unet=unet,
                                        device=device)
        metric.sample_images()
        metric.sample_noises(generator=torch.Generator(device=device).manual_seed(self.seed()))
        plot = ml.get("plot_params")
        if plot:
            timesteps = list(range(0, int(sched.config.num_train_timesteps), int(plot.time_frequency)))
            metric.compute_membership_losses(timesteps)
            means = metric.means.cpu()
            with open(os.path.join(cfg.output_dir, "membership_curve_rank0.json"), "w") as f:
                json.dump(dict(timesteps=timesteps, all_membership_loss=means[:, 0].float().tolist(),
                               deletion_membership_loss=means[:, 1].float().tolist()), f)
            return None, None
        timesteps = [int(t) for t in ml.timesteps]
        out = os.path.join(cfg.output_dir, "membership_rank0.jsonl")
        return int(ml.step_frequency), lambda global_step: log_membership(metric, timesteps, global_step, out)

    def check_mia(self, in_loop=True):
        """metrics.mia (OPT-IN, absent from the repo's configs): {attacks, step_frequency, num_members, num_forget, batch_size,
        holdout: {path, limit}, fpr, secmi, pia, loss, seed} -- membership inference attacks (siss_amd/mia.py) on members drawn from
        the keep dataset, the forget images and holdout images the model never saw.  Refused here, before the UNet is loaded: a task
        without a pixel-space UNet, an unknown field or attack, a timestep outside [0, num_train_timesteps), a holdout path that is not
        on disk.  Returns the settings, or None.  in_loop=False (tools/mia.py: one evaluation outside a run): step_frequency is not
        needed and an absent key means the defaults."""
        cfg = self.cfg
        metrics = cfg.get("metrics") or {}
        if metrics.get("mia") is None:
            if in_loop:
                return None
            metrics = {"mia": {}}
        if not self.mia_supported:
            raise NotImplementedError("metrics.mia: the membership inference attacks are built for the pixel-space tasks (DeleteCeleb, "
                                      "DeleteTShirt) only -- no latent-space form of SecMI / PIA is built")
        from .mia import parse_config
        T = int((cfg.get("scheduler") or {}).get("num_train_timesteps", 1000))
        settings = parse_config(hydra_lite._plain(metrics.get("mia")), T, need_frequency=in_loop)
        ho = settings["holdout"]
        if ho is not None and ho["path"] is None and not cfg.get("allow_synthetic"):
            raise ValueError("metrics.mia.holdout.path is needed: a directory of images, or an .npz, the model never trained on "
                             "(allow_synthetic=true: synthetic stand-ins; holdout=null: score means only)")
        if ho is not None and ho["path"] is not None and not os.path.exists(ho["path"]):
            raise FileNotFoundError(f"metrics.mia.holdout.path {ho['path']!r} is not on disk")
        return settings

    def mia_evaluation(self, unet, sched, ds_all, ds_del, device, path):
        """The MiaEvaluation of the checked settings: the members (num_members keep indices from a generator of their own, seeded with
        metrics.mia.seed), the forget images (each dataset index once, up to num_forget) and the holdout images, drawn ONCE, here.  No
        stream of the loop and no global generator is touched."""
        from . import mia
        cfg, s = self.cfg, self.mia
        attack = mia.MembershipAttack(unet, sched, device, attacks=s["attacks"], batch_size=s["batch_size"], **s["settings"])
        stack = lambda ds, idx: torch.stack([ds[i] for i in idx]).float()
        members = stack(ds_all, mia.draw_members(len(ds_all), s["num_members"], s["seed"]))
        forget = stack(ds_del, mia.unique_in_order(range(len(ds_del)))[:s["num_forget"]])
        ho, holdout = s["holdout"], None
        if ho is not None and ho["path"] is not None:
            transform = hydra_lite.instantiate(cfg.transform) if cfg.get("transform") is not None else None
            holdout = mia.load_holdout(ho["path"], ho["limit"], transform, int(members.shape[1]))
            if tuple(holdout.shape[1:]) != tuple(members.shape[1:]):
                raise ValueError(f"metrics.mia.holdout: images of shape {tuple(holdout.shape[1:])}, the task's are {tuple(members.shape[1:])}")
        elif ho is not None:
            print(f"[siss_amd] metrics.mia: allow_synthetic and no holdout.path -- {ho['limit']} SYNTHETIC holdout images")
            holdout = stack(SyntheticImages(ho["limit"], tuple(members.shape[1:]), seed=3 + s["seed"]), range(ho["limit"]))
        return mia.MiaEvaluation(attack, members, forget, holdout, s["fpr"], s["seed"], path)

    def mia_metric(self, unet, sched, ds_all, ds_del, device):
        """`metrics.mia`: None when not configured, else (step_frequency, evaluate(global_step)); each evaluation appends one record to
        mia_rank0.jsonl (mia.MiaEvaluation)."""
        if self.mia is None:
            return None
        out = os.path.join(self.cfg.output_dir, "mia_rank0.jsonl")
        return int(self.mia["step_frequency"]), self.mia_evaluation(unet, sched, ds_all, ds_del, device, out)

    def deletion_metrics(self, unet, sched, forget_image, device):
        """The tracker of the configured deletion metrics (a callable of global_step), or None: none here."""
        return None

    def metric_hooks(self, unet, sched, ds_all, ds_del, device, rank=0):
        """The loop's metric hooks (every, fn) | None | (None, None), generated in the loop's order: likelihood, the task's
        deletion_metrics (a tracker that owns its schedule enters as (1, tracker)), membership.  fn(global_step) runs at step 0 and at
        every multiple of `every`; (None, None) ends the run (_start_hooks).  Rank 0 measures; the others only learn that it ended."""
        if rank != 0:
            yield (None, None) if (self.check_membership() or {}).get("plot_params") else None
            return
        yield self.likelihood_metric(unet, ds_del[0], device)
        tracker = self.deletion_metrics(unet, sched, ds_del[0], device)
        yield None if tracker is None else (1, tracker)
        yield self.membership_metric(unet, sched, ds_all, ds_del, device)
        yield self.mia_metric(unet, sched, ds_all, ds_del, device)

    def fill_cfg(self):
        """Placeholders of the config that are read from files before anything else (delete_sd.py:342-348): none here."""

    # -- the loop ------------------------------------------------------------------------------
    def run(self):
        cfg = self.cfg
        world, rank, local, pg = _dist()
        device = torch.device("cuda", local)
        torch.cuda.set_device(device)
        seed = self.seed()
        torch.manual_seed(seed + rank)
        self.fill_cfg()
        self.check_supported()
        self.check_metrics()
        unet = self.load_unet(device)
        eng = unet.engine
        teacher, teacher_cfg = self.build_teacher(eng, device, rank)     # (the weights the run loaded: before deletion.ssd, before a step)
        sched = self.load_scheduler()
        lr, betas, eps, wd = self.optimizer_args()
        from .scheduler import lr_multiplier
        lr_name = str(cfg.get("lr_scheduler") or "constant")
        # get_scheduler(cfg.lr_scheduler, num_warmup_steps=..., num_training_steps=...): delete_celeb.py:296-301 passes
        # cfg.warmup_steps / cfg.training_steps, delete_sd.py:714-719 cfg.lr_warmup_steps * num_processes / cfg.training_steps
        warm, total = self.lr_schedule_args(world)
        lr_multiplier(lr_name, 0, warm, total)                  # raises now for a schedule that is not implemented
        d = cfg.deletion
        B, ga = int(cfg.train_batch_size), int(cfg.gradient_accumulation_steps)
        stepper = SISSStepper(
            eng, sched.alphas_cumprod, lr=lr, betas=betas, eps=eps, weight_decay=wd,
            scaling_norm=float(d.scaling_norm) if d.loss_fn != "erasediff" else None,
            eta=float(d.eta) if d.loss_fn == "erasediff" else None,
            lambd=float((d.loss_params or {}).get("lambd", 0.5)), train_batch_size=B, grad_accum=ga,
            loss_fn=d.loss_fn, inf_guard=self.inf_guard, process_group=pg,
            mixed_precision=cfg.get("mixed_precision"),
            superfactor=float((d.loss_params or {}).get("superfactor", 1.0)),
            superfactor_decay=d.get("superfactor_decay"), trainable=self.trainable_names(unet), lora=self.lora_state(unet),
            teacher=teacher, teacher_cfg=teacher_cfg)
        lora = stepper.lora
        shape = (unet.config.in_channels, unet.config.sample_size, unet.config.sample_size)
        ds_all, ds_del = self.datasets(shape)
        self.open_image_stores(ds_all, ds_del, device)
        it_all = self.keep_batches(ds_all, B, rank, world, device)
        it_del = self.forget_batches(ds_del, B, device)
        n_steps = int(cfg.training_steps) * max(1, len(d.get("img_name") or [1]))
        cond = self.conditioning(B, device)
        os.makedirs(cfg.output_dir, exist_ok=True)
        uce_fields = self.uce_edit(stepper, device, rank, world, pg)      # (before deletion.ssd: its Fishers are the edited model's)
        ssd_fields = self.ssd_dampen(stepper, ds_all, ds_del, B, cond, device, rank, world, pg)
        saliency = self.saliency_mask(stepper, ds_del, B, cond, device, rank, world, pg)
        if saliency is not None:
            stepper.set_saliency(saliency)
        ewc = self.ewc_anchor(stepper, ds_all, B, cond, device, rank, world, pg)
        if ewc is not None:
            stepper.set_ewc(ewc)
        sgc = self.surgery_config()
        if sgc is not None:
            from .surgery import Surgery
            stepper.set_surgery(Surgery(eng, sgc.mode, sgc.granularity))
            if rank == 0:
                sg = stepper.surgery
                print(f"[siss_amd] deletion.surgery: mode {sg.mode}, {sg.groups} group(s) ({sg.granularity}), {sg.jobs} jobs of "
                      f"{sg.chunk} floats")
        if rank == 0 and self.replication is not None:
            self.open_replication(device)

        def record(handle, meta):
            st = handle.get()
            st["global_step"], st["lr"], st["elapsed_s"] = meta          # (elapsed: stamped when the step was queued)
            st.update(stepper.log_fields())         # (the parameters the optimizer updates and the active variant's own fields)
            if uce_fields is not None:
                st.update(uce_fields)
            if ssd_fields is not None:
                st.update(ssd_fields)
            return st

        def say(st, meta):
            if rank == 0:
                print(f"step {meta[0]}/{n_steps}  |g_x| {st['norm_loss_x']:.4g}  |g_a| {st['norm_loss_a']:.4g}  "
                      f"s {st['scaling_factor']:.4g}")

        g = torch.Generator(device=device).manual_seed(seed + rank)
        T = sched.config.num_train_timesteps
        t0 = time.perf_counter()
        eval_every = int(cfg.get("eval_every") or 0)
        # (the last COMPLETED step reaches the log also when the next one raises or the job is interrupted: ADVICE r05)
        with LaggedLog(os.path.join(cfg.output_dir, f"train_log_rank{rank}.jsonl"), record, say) as log:
            hooks = _start_hooks(self.metric_hooks(unet, sched, ds_all, ds_del, device, rank))
            if hooks is None:
                it_all.close()                           # the curve is the run (delete_celeb.py:444-462 exits here)
                self.close_image_stores()
                return stepper
            for step in range(n_steps):
                # lr_scheduler.step() after every optimizer step (delete_celeb.py:770); accelerate's wrapper advances the
                # schedule once per PROCESS per optimizer step (AcceleratedScheduler, split_batches=False)
                stepper.opt.lr = lr * lr_multiplier(lr_name, step * world, warm, total)
                for _ in range(ga):
                    x0 = self.prepare_batch(next(it_all).to(device, non_blocking=True), g)
                    a0 = self.prepare_batch(next(it_del).to(device, non_blocking=True), g)
                    noise = self.sample_noise(x0.shape, device, g)                      # SAME noise for both batches
                    t = torch.randint(self.timestep_low, T, (B,), device=device, generator=g)
                    u = torch.rand(B, device=device, generator=g)
                    stepper.micro_step(x0, a0, noise, t, u, cond)
                log.push(stepper.stats_async(), (step + 1, stepper.opt.lr, time.perf_counter() - t0))
                if eval_every and (step + 1) % eval_every == 0:
                    log.flush()                         # every rank flushes at an evaluation step (the logs stay in step)
                    if rank == 0:
                        self.evaluate(unet, sched, ds_del[0], step + 1, device)
                _run_hooks(hooks, step + 1)
        it_all.close()
        self.close_image_stores()
        if rank == 0 and cfg.get("save_final", True):
            unet.save_pretrained(os.path.join(cfg.output_dir, "unet"))
            if lora is not None:                    # the adapter, beside the merged model
                lora.steps = n_steps
                lora.save(os.path.join(cfg.output_dir, "lora"))
        return stepper

    def deletion_sampler(self, ds, B):
        return InfiniteSampler(ds, shuffle=False) if len(ds) >= B else RepeatedSampler(ds, 1 << 30)

    def keep_batches(self, ds_all, B, rank, world, device):
        """The keep batches of the loop, an iterator with close(): the rank's shard decoded / pinned / copied in the background,
        `depth` batches ahead -- or, with image_store on, the sampler's indices alone (prepare_batch gathers the images)."""
        if self.keep_store is not None:
            return index_batches(InfiniteSampler(ds_all, rank=rank, num_replicas=world), B, self.keep_store)
        return Prefetcher(ds_all, InfiniteSampler(ds_all, rank=rank, num_replicas=world), B, device=device,
                          workers=int(self.cfg.get("dataloader_num_workers") or 4))

    def forget_batches(self, ds_del, B, device):
        """The forget batches of the loop (the forget set is one or a few images repeated: a plain iterator is enough)."""
        if self.forget_store is not None:
            return index_batches(self.deletion_sampler(ds_del, B), B, self.forget_store)
        return batches(ds_del, self.deletion_sampler(ds_del, B), B)


class DeleteCeleb(_DeleteBase):
    """config/delete_celeb.yaml -- CelebA-HQ 256, forget set = listed jpgs repeated (RepeatedSampler)."""

    def check_metrics(self):
        """metrics.fid (delete_celeb.py:469-471,:532-542) needs class_cfg, a positive integer step_frequency, at least 2 images to
        generate (a covariance needs two), a positive batch_size, a 3-channel UNet, the Inception checkpoint on disk (unless
        class_cfg.allow_random_init) and the real-image directory (or an existing class_cfg.real_stats_path) -- all refused here,
        before the first step."""
        super().check_metrics()
        cfg = self.cfg
        fid = (cfg.get("metrics") or {}).get("fid")
        if not fid:
            return
        from .fid import DEFAULT_CKPT
        cc = fid.get("class_cfg")
        if not cc:
            raise ValueError("metrics.fid needs class_cfg (metrics.fid.FIDEvaluator and its inception_batch_size)")
        if not _positive_int(fid.get("step_frequency")):
            raise ValueError(f"metrics.fid.step_frequency={fid.get('step_frequency')!r}: a positive step count is needed")
        n = fid.get("num_imgs_to_generate")
        if not _positive_int(n) or n < 2:
            raise ValueError(f"metrics.fid.num_imgs_to_generate={n!r}: at least 2 images are needed (the covariance of one is undefined)")
        if not _positive_int(fid.get("batch_size")):
            raise ValueError(f"metrics.fid.batch_size={fid.get('batch_size')!r}: a positive batch size is needed")
        ch = self._image_channels()
        if ch != 3:
            raise ValueError(f"metrics.fid: the Inception-v3 takes 3-channel images, the UNet has in_channels={ch!r}")
        ckpt = str(cc.get("inception_ckpt") or DEFAULT_CKPT)
        if not cc.get("allow_random_init") and not os.path.isfile(ckpt):
            raise FileNotFoundError(f"metrics.fid.class_cfg.inception_ckpt {ckpt!r} is not a file on disk (pass "
                                    "metrics.fid.class_cfg.allow_random_init=true for random-init weights of the same architecture)")
        stats = cc.get("real_stats_path")
        data = str(cc.get("data_path") or "data/examples/celeba_hq_256")
        if not (stats and os.path.isfile(str(stats))) and not os.path.isdir(data):
            raise FileNotFoundError(f"metrics.fid.class_cfg.data_path {data!r} (the real images of the FID) is not a directory on disk")
        if fid.get("sets") is not None:                  # OPT-IN: KID and precision / recall / density / coverage on the same features
            from . import feature_sets
            feature_sets.parse_config(hydra_lite._plain(fid.get("sets")), n)
            if not os.path.isdir(data):
                raise FileNotFoundError(f"metrics.fid.sets needs metrics.fid.class_cfg.data_path {data!r} (the real images: their features "
                                        "are kept, and the FID's statistics file holds none) as a directory on disk")

    def deletion_metrics(self, unet, sched, forget_image, device):
        """`metrics.fid` (class_cfg, step_frequency, num_imgs_to_generate, batch_size), OPT-IN: None when not configured.  The
        evaluator is built and its real side loaded here, once, before step 0; at step 0 and every step_frequency steps
        num_imgs_to_generate samples (`pipeline.num_inference_steps` steps, batches of batch_size, a generator of its own seeded from
        random_seed) go through add_fake_images batch by batch (each batch comes back from Evaluator.sample_images as a host array and
        is copied to the device again: one round trip per batch, negligible next to its sampling), and {global_step, fid, fake_images, real_images, seconds} is
        appended to fid_rank0.jsonl (fid.FIDTracker).  `metrics.fid.sets` (absent: nothing changes) keeps the features and adds the KID and
        precision / recall / density / coverage to the record (feature_sets.FeatureSets; NOT the reference's protocol)."""
        cfg = self.cfg
        fid = (cfg.get("metrics") or {}).get("fid")
        if not fid:
            return None
        from .fid import FIDTracker
        from .sampler import Evaluator
        sets = None
        if fid.get("sets") is not None:                  # OPT-IN (`+metrics.fid.sets={kid:{...},prdc:{...}}`); refused in check_metrics
            from . import feature_sets
            sets = feature_sets.FeatureSets(feature_sets.parse_config(hydra_lite._plain(fid.get("sets")), int(fid.num_imgs_to_generate)),
                                            int(fid.num_imgs_to_generate), device)
        evaluator = hydra_lite.instantiate(fid.class_cfg, device=device, **({} if sets is None else {"feature_sets": sets}))
        evaluator.load_celeb()
        steps = _inference_steps(cfg)
        gen = torch.Generator(device=device).manual_seed(self.seed())
        held = {}

        def begin():                                     # one sampler (and its captured forward) per evaluation, as evaluate() has
            held["ev"] = Evaluator(cfg)
            held["ev"].load_model(unet, sched)

        def end():                                       # ... dropped with its graphs and static buffers before training goes on
            held.clear()

        solver = _pipeline_sampler(cfg, sched)

        def sample(n):
            imgs = held["ev"].sample_images(n, num_inference_steps=steps, generator=gen, sampler=solver)
            return torch.from_numpy(imgs).permute(0, 3, 1, 2).to(device)

        tracker = FIDTracker(evaluator, os.path.join(cfg.output_dir, "fid_rank0.jsonl"), sample, fid.step_frequency,
                             fid.num_imgs_to_generate, fid.batch_size, begin=begin, end=end, sets=sets)
        tracker.extra = _sampler_fields(cfg, solver)
        return tracker


class DeleteTShirt(_DeleteBase):
    """config/delete_tshirt.yaml -- MNIST + T-shirt: t ~ U{0..999} (delete_tshirt.py:535-540) and the
    inf guard on the scaling factor (:688-690)."""
    timestep_low = 0
    inf_guard = True
    default_unet = staticmethod(UNet2DConfig.mnist_tshirt)

    def check_metrics(self):
        """metrics.fraction_deletion needs a positive sampling_steps; metrics.inception_score needs metrics.classifier_cfg, a positive
        step_frequency and, when classifier_ckpt is set, that file on disk -- all refused here, before the first step."""
        super().check_metrics()
        cfg = self.cfg
        m = cfg.get("metrics") or {}
        if m.get("fraction_deletion"):
            ss = cfg.get("sampling_steps")
            if not _positive_int(ss):
                raise ValueError(f"metrics.fraction_deletion=true needs a positive sampling_steps (the reference's key: the T-shirt "
                                 f"fraction runs every sampling_steps optimizer steps); got sampling_steps={ss!r}")
        isc = m.get("inception_score")
        if isc:
            cc = m.get("classifier_cfg")
            if not cc:
                raise ValueError("metrics.inception_score needs metrics.classifier_cfg (the classifier the score is taken with)")
            freq = isc.get("step_frequency")
            if not _positive_int(freq):
                raise ValueError(f"metrics.inception_score.step_frequency={freq!r}: a positive step count is needed")
            ckpt = cc.get("classifier_ckpt")
            if ckpt is not None and not os.path.isfile(str(ckpt)):
                raise FileNotFoundError(f"metrics.classifier_cfg.classifier_ckpt {ckpt!r} is not a file on disk")

    def deletion_metrics(self, unet, sched, forget_image, device):
        """delete_tshirt.py:438-482 without wandb, OPT-IN (absent from the repo's configs): `metrics.fraction_deletion` -- the share of
        `eval_images` samples (batches of `eval_batch_size`, `pipeline.num_inference_steps` steps) within L2 distance 10 of the T-shirt,
        at step 0 and every `sampling_steps` steps, `deletion_steps` = the first step where it is 0 -- and `metrics.inception_score`
        (class_cfg, step_frequency, num_imgs_to_generate, batch_size) -- the Inception Score under metrics.classifier_cfg of the
        samples that do not match the T-shirt, at step 0, every step_frequency steps and at deletion_steps.  Lines go to
        metrics_rank0.jsonl (classifier.TShirtMetrics).  The T-shirt is metrics.classifier.tshirt_path through ToTensor when that
        file exists, else the first forget image mapped to [0, 1].  The sampling noise and the score's permutation come from
        generators of their own, seeded once from random_seed; the classifier is built here, and only when the score is configured."""
        import numpy as np
        from .classifier import InceptionScore, TShirtMetrics
        from .sampler import Evaluator
        cfg = self.cfg
        m = cfg.get("metrics") or {}
        frac, isc = bool(m.get("fraction_deletion")), m.get("inception_score") or None
        if not frac and not isc:
            return None
        path = (m.get("classifier") or {}).get("tshirt_path")
        if path and os.path.isfile(str(path)):
            from PIL import Image
            from .data import ToTensor
            tshirt = ToTensor()(Image.open(str(path)))
        else:
            tshirt = forget_image.float() * 0.5 + 0.5
        tshirt = tshirt.to(device).float()
        steps = _inference_steps(cfg)
        gen = torch.Generator(device=device).manual_seed(self.seed())
        solver = _pipeline_sampler(cfg, sched)

        def sample(n, batch_size):
            ev = Evaluator(cfg)
            ev.load_model(unet, sched)
            out = [ev.sample_images(min(batch_size, n - s), num_inference_steps=steps, generator=gen, sampler=solver)
                   for s in range(0, n, batch_size)]
            return torch.from_numpy(np.concatenate(out)).permute(0, 3, 1, 2).to(device)

        inception = None
        if isc:
            classifier = hydra_lite.instantiate(m.classifier_cfg, device=device)
            node = isc.get("class_cfg")
            inception = ((lambda: hydra_lite.instantiate(node, classifier=classifier)) if node
                         else (lambda: InceptionScore(classifier)))
        isc = isc or {}
        tracker = TShirtMetrics(tshirt, os.path.join(cfg.output_dir, "metrics_rank0.jsonl"), sample,
                                sampling_steps=cfg.get("sampling_steps") if frac else None,
                                eval_images=int(cfg.get("eval_images") or 128), eval_batch_size=cfg.get("eval_batch_size"),
                                inception=inception, is_every=isc.get("step_frequency"),
                                is_images=int(isc.get("num_imgs_to_generate") or 1024), is_batch_size=isc.get("batch_size"),
                                generator=torch.Generator().manual_seed(self.seed()))
        tracker.extra = _sampler_fields(cfg, solver)
        return tracker


class DeleteSD(_DeleteBase):
    """config/delete_sd.yaml -- Stable Diffusion: the same loop on VAE latents with text conditioning
    (delete_sd.py:864-1127).  On the path: the SISS step through ``UNet2DConditionModel``.  Not on it (SURVEY.md §8f
    rank 4, not built): the frozen VAE encoder and CLIP text encoder of delete_sd.py:879-888,:941-944 -- latents and the
    prompt embedding are read from ``.pt`` files when configured (``latents_all`` / ``latents_deletion`` [N,4,h,w],
    already multiplied by vae.config.scaling_factor; ``validation_prompts[0]`` ending in .pt [77,768] or [1,77,768],
    the reference's own ``using_augmented_prompt`` branch, delete_sd.py:938) and synthetic otherwise."""
    default_unet = staticmethod(UNet2DConditionConfig.sd15)
    VAE_SCALE = 0.18215            # vae.config.scaling_factor (delete_sd.py:883,888)
    membership_supported = False   # (delete_sd.py has no membership loss)
    mia_supported = False          # (metrics.mia: no latent-space form of the attacks is built)
    vae = None
    text_encoder = None

    def load_front_end(self, device):
        """Frozen VAE encoder + CLIP text encoder from the checkpoint directory, when it is on disk
        (delete_sd.py:464-474): images are then encoded per micro-batch and the prompt once."""
        path = str(self.cfg.get("pretrained_model_name_or_path") or "")
        if os.path.isdir(os.path.join(path, "vae")):
            from .vae import VAEEncoder
            self.vae = VAEEncoder.from_pretrained(path, "vae", device)
        if os.path.isdir(os.path.join(path, "text_encoder")):
            from .text_encoder import CLIPTextEncoder
            self.text_encoder = CLIPTextEncoder.from_pretrained(path, "text_encoder", device)

    def prepare_batch(self, x, generator):
        if isinstance(x, IndexBatch):                           # latent_cache on: indices -> the cached moments, sampled in one launch
            return x.cache.latents(x, generator)
        if self.vae is not None and x.shape[1] == self.vae.cfg.in_channels and x.shape[1] != 4:
            return self.vae.encode(x, generator=generator)      # latent_dist.sample() * scaling_factor (:879-888)
        return x

    # -- latent_cache: null | {enabled, path, max_bytes, chunk} (OPT-IN; siss_amd/latent_cache.py) -----------------------------
    encodes_images = False      # set by datasets(): the loop's batches are images the VAE encodes (not latents)
    keep_cache = None
    forget_cache = None

    def latent_cache_cfg(self):
        """The latent_cache block when it is enabled AND the loop encodes images, else None.  The cache holds the frozen VAE's
        posterior moments per image, so it has nothing to do for pre-encoded latents_all / latents_deletion or synthetic latents."""
        lc = self.cfg.get("latent_cache")
        if not lc:
            return None
        if not isinstance(lc, dict):
            raise ValueError(f"latent_cache={lc!r}: null or a mapping {{enabled, path, max_bytes, chunk}} is needed")
        unknown = sorted(set(lc) - {"enabled", "path", "max_bytes", "chunk"})
        if unknown:
            raise ValueError(f"latent_cache: unknown keys {unknown} (enabled, path, max_bytes, chunk)")
        if not lc.get("enabled"):
            return None
        if not self.encodes_images:
            print("[siss_amd] latent_cache.enabled is set but this run encodes no images (latents_all / latents_deletion or synthetic "
                  "latents): the cache does not apply")
            return None
        return lc

    def _latent_cache(self, ds, which, lc, device):
        """The cache of one dataset (`which`: keep / forget): its budget is latent_cache.max_bytes, its file <path>/<which>.safetensors
        (read by every rank at the start when it is there and belongs)."""
        from .data import TensorImages
        from .latent_cache import LatentCache
        vc = self.vae.cfg
        down = 2 ** (len(vc.block_out_channels) - 1)
        hw = tuple(ds.t.shape[-2:]) if isinstance(ds, TensorImages) else (int(self.cfg.resolution),) * 2
        if hw[0] % down or hw[1] % down:
            raise ValueError(f"latent_cache: images of {hw[0]} x {hw[1]} are no multiple of the VAE's factor {down}")
        cache = LatentCache(self.vae, ds, (vc.latent_channels, hw[0] // down, hw[1] // down), device=device,
                            max_bytes=lc.get("max_bytes"), chunk=lc.get("chunk"), name=f"latent cache ({which})")
        if lc.get("path"):
            cache.load(os.path.join(str(lc.get("path")), f"{which}.safetensors"))
        return cache

    def keep_batches(self, ds_all, B, rank, world, device):
        lc = self.latent_cache_cfg()
        if lc is None:
            return super().keep_batches(ds_all, B, rank, world, device)
        self.keep_cache = self._latent_cache(ds_all, "keep", lc, device)
        return index_batches(InfiniteSampler(ds_all, rank=rank, num_replicas=world), B, self.keep_cache)

    def forget_batches(self, ds_del, B, device):
        lc = self.latent_cache_cfg() if self.keep_cache is not None else None       # (on for both or for neither)
        if lc is None:
            return super().forget_batches(ds_del, B, device)
        self.forget_cache = self._latent_cache(ds_del, "forget", lc, device)
        return index_batches(self.deletion_sampler(ds_del, B), B, self.forget_cache)

    def run(self):
        stepper = super().run()
        path = (self.cfg.get("latent_cache") or {}).get("path")
        if path and int(os.environ.get("RANK", "0")) == 0:      # rank 0 writes at the end of the run; every rank reads at the start
            for which, cache in (("keep", self.keep_cache), ("forget", self.forget_cache)):
                if cache is not None:
                    rows = cache.save(os.path.join(str(path), f"{which}.safetensors"))
                    print(f"[siss_amd] {cache.name}: {rows} of {cache.n} rows written to {path}/{which}.safetensors "
                          f"({cache.encoded} encoded in this run)")
        return stepper

    def seed(self):
        return int(self.cfg.get("seed", 42))                   # config/delete_sd.yaml:80

    def load_unet(self, device):
        from .model import UNet2DConditionModel
        cfg = self.cfg
        self.load_front_end(device)
        path = cfg.get("pretrained_model_name_or_path")
        dt = self.compute_dtype()                                # (the frozen VAE / text encoder front end stays on the bf16 path)
        if self.unet_checkpoint() is not None:
            return UNet2DConditionModel.from_pretrained(path, subfolder="unet", device=device, compute_dtype=dt)   # delete_sd.py:458-462
        if not cfg.get("allow_random_init"):                     # the reference hard-fails (from_pretrained, delete_sd.py:458-462)
            raise FileNotFoundError(
                f"pretrained_model_name_or_path {path!r} has no unet/ directory on disk (no network: hub ids cannot be "
                "fetched); pass allow_random_init=true to train random-init weights of the configured architecture instead")
        m = UNet2DConditionModel(self.unet_config(), device=device, compute_dtype=dt)
        m.engine.init_random(seed=self.seed())
        print(f"[siss_amd] allow_random_init: {path!r}/unet not on disk, RANDOM-INIT weights of the same architecture")
        return m

    unet_engine = "siss_amd.unet_cond.UNetCondEngine"
    teacher_refusal = None      # deletion.teacher is this task's: the prompts the two forget targets need are here

    def teacher_config(self):
        tc = super().teacher_config()
        if tc is not None and tc.forget == "anchor":
            self._check_embeddable(tc.anchor_prompt, "deletion.teacher.anchor_prompt")
        path = str(self.cfg.get("pretrained_model_name_or_path") or "")
        if tc is not None and tc.forget == "esd" and not (os.path.isdir(os.path.join(path, "text_encoder")) or self.cfg.get("allow_synthetic")):
            raise FileNotFoundError("deletion.teacher (forget: esd) needs the empty prompt's embedding: no text_encoder/ in the checkpoint "
                                    "directory (pass allow_synthetic=true for a synthetic one)")
        return tc

    uce_refusal = None          # deletion.uce is this task's: the cross-attention projections and the prompts are here

    def _cross_dim(self):
        return int(self.unet_config().cross_attention_dim)

    def uce_check(self):
        uc = self.uce_config()
        if uc is None:
            return
        from .uce import KEY, check_targets, select_targets
        specs = self.unet_param_specs()
        check_targets(specs, select_targets(list(specs), uc.targets), self._cross_dim())
        path = str(self.cfg.get("pretrained_model_name_or_path") or "")
        for i, (p, t) in enumerate(uc.edit):
            self._check_embeddable(p, f"{KEY}.edit[{i}].prompt")
            if t is not None:
                self._check_embeddable(t, f"{KEY}.edit[{i}].target")
            elif not (os.path.isdir(os.path.join(path, "text_encoder")) or self.cfg.get("allow_synthetic")):
                raise FileNotFoundError(f"{KEY}.edit[{i}].target=null needs the empty prompt's embedding: no text_encoder/ in the "
                                        "checkpoint directory (pass allow_synthetic=true for a synthetic one)")
        for i, p in enumerate(uc.preserved_prompts()):
            self._check_embeddable(p, f"{KEY}.preserve[{i}]")

    def uce_rows(self, uc, device):
        """(C_e, C_t, C_p) [rows, X] of the parsed key: every token row of every prompt's embedding.  Synthetic embeddings
        (allow_synthetic) are seeded seed() + 16 + i, i running over the edit sources, their destinations and the preserved prompts, so
        that distinct prompts get distinct rows; a null destination is the empty prompt's embedding."""
        X = self._cross_dim()
        pres = uc.preserved_prompts()
        n = len(uc.edit)
        src = [self._prompt_embedding(p, device, synthetic_seed=16 + i) for i, (p, _) in enumerate(uc.edit)]
        dst = [self._empty_prompt_embedding(device, "deletion.uce (target: null)") if t is None
               else self._prompt_embedding(t, device, synthetic_seed=16 + n + i) for i, (_, t) in enumerate(uc.edit)]
        keep = [self._prompt_embedding(p, device, synthetic_seed=16 + 2 * n + i) for i, p in enumerate(pres)]
        for i, (a, b) in enumerate(zip(src, dst)):
            if a.shape != b.shape or a.shape[-1] != X:
                raise ValueError(f"deletion.uce.edit[{i}]: the prompt embeds to {tuple(a.shape)}, its destination to {tuple(b.shape)}; both "
                                 f"must be [1, L, {X}] with one L")
        rows = lambda es: torch.cat([e.reshape(-1, X) for e in es]).double().cpu() if es else torch.zeros(0, X, dtype=torch.float64)
        return rows(src), rows(dst), rows(keep), pres

    def uce_edit(self, stepper, device, rank, world, pg):
        """Unified Concept Editing of the run (None without the key), once, at the weights the run loaded -- after the teacher took its
        copy, before deletion.ssd, the mask, the anchor and the step-0 metrics: the edit loaded from `path` when both files are there
        (a foreign X or other embeddings are refused by field), else built from the prompts' embeddings; then the two launches, the
        statistics and the residuals.  More than one rank: rank 0 alone builds or loads the edit, the ranks agree on success, E is
        broadcast, every rank applies and compares the bits of its sum of delta^2 with rank 0's.  Rank 0 writes the two files into
        output_dir.  Returns the fields every train-log line carries."""
        uc = self.uce_config()
        if uc is None:
            return None
        import struct
        from . import uce
        eng = stepper.e
        X = self._cross_dim()
        out = str(self.cfg.output_dir)
        names = uce.check_targets(eng.ps.specs, uce.select_targets(list(eng.ps.specs), uc.targets), X)
        rows = {}

        def build():
            Ce, Ct, Cp, pres = rows["all"] = self.uce_rows(uc, device)
            if uc.path is not None and uce.present(uc.path):
                ed = uce.load(uc.path, X)
                digest = uce.embeddings_digest(X, Ce.numpy(), Ct.numpy(), Cp.numpy())
                if ed.digest != digest:
                    raise ValueError(f"{os.path.join(uc.path, uce.CONFIG_FILE)}: embeddings = {ed.digest!r}, this run's prompts embed to "
                                     f"{digest!r} -- the edit was computed for other prompts or another text encoder")
                print(f"[siss_amd] deletion.uce: edit loaded from {uc.path}")
            else:
                if uc.path is not None:
                    print(f"[siss_amd] deletion.uce.path {uc.path!r} holds no edit files: computing the edit")
                ed = uce.edit_matrix(Ce, Ct, Cp, uc.lam, uc.edit_scale, uc.preserve_scale)
            ed.E_dev = torch.from_numpy(ed.E).to(device)
            return ed

        def empty(c):
            import numpy as np
            ed = uce.UCEEdit(np.zeros((X, X), np.float32), None, None, c["edit_rows"], c["preserve_rows"], c["lambda"], c["edit_scale"],
                             c["preserve_scale"], c["cond"], digest=c["embeddings"], source=c["source"])
            ed.E_dev = torch.zeros(X, X, dtype=torch.float32, device=device)
            return ed

        ed = _built_on_rank0("deletion.uce: rank 0 could not build the edit", build, uce.UCEEdit.config, empty, lambda ed: ed.E_dev,
                             out, rank, world, pg)
        before = None
        if rank == 0:
            Ce, Ct, Cp, pres = rows["all"]
            before = uce.values_before(eng, names, Ct, Cp)
        stats = uce.apply(eng, ed, names, apply=True)
        if world > 1:
            import torch.distributed as dist
            mine = struct.unpack("<Q", struct.pack("<d", stats["sum_delta2"]))[0]
            word = [mine if rank == 0 else None]
            dist.broadcast_object_list(word, src=0, group=pg)
            if word[0] != mine:
                raise RuntimeError(f"deletion.uce: rank {rank}'s sum of delta^2 has the bits {mine:#018x}, rank 0's {word[0]:#018x}")
        if rank == 0:
            res = uce.residuals(eng, names, before, Ce, Cp)
            ed.save_report(out, dict(config=uc.as_dict(), edit_prompts=[p for p, _ in uc.edit], edit_targets=[t for _, t in uc.edit],
                                     preserved_prompts=pres, targets=names, stats=stats, residuals=res))
            drift = res["preserve_drift"]
            print(f"[siss_amd] deletion.uce: {len(uc.edit)} edit(s) over {ed.n_edit} rows, {len(pres)} preserved prompt(s) over "
                  f"{ed.n_preserve} rows, lambda {uc.lam:g}, cond(M) {ed.cond:.4g}; {len(names)} tensors, {stats['floats']} floats, "
                  f"relative change {stats['relative_change']:.6g}, edit residual {res['edit_residual']:.6g}, preserve drift "
                  f"{'none' if drift is None else format(drift, '.6g')}")
        return dict(uce_edits=len(uc.edit), uce_preserved=len(uc.preserved_prompts()), uce_lambda=uc.lam,
                    uce_relative_change=stats["relative_change"])

    def _check_embeddable(self, p, key):
        """_prompt_embedding's rules, from the disk alone (check_supported runs before anything is loaded)."""
        cfg = self.cfg
        path = str(cfg.get("pretrained_model_name_or_path") or "")
        if (str(p).endswith(".pt") and os.path.exists(str(p))) or cfg.get("allow_synthetic") or all(
                os.path.isdir(os.path.join(path, sub)) for sub in ("text_encoder", "tokenizer")):
            return
        raise FileNotFoundError(f"{key}={p!r} cannot be embedded: it is neither a .pt embedding / token file on disk nor a prompt with a "
                                "text_encoder/ + tokenizer/ on disk; pass allow_synthetic=true for a synthetic embedding")

    def teacher_embeddings(self, tc, device):
        """What the teacher's extra rows are conditioned on: the empty prompt (esd) or the anchor prompt (anchor; its synthetic stand-in
        is a seeded embedding of its own, not the prompt's)."""
        if tc.forget == "esd":
            return dict(empty=self._empty_prompt_embedding(device, "deletion.teacher (forget: esd)"))
        return dict(anchor=self._prompt_embedding(tc.anchor_prompt, device, synthetic_seed=2))

    def unet_checkpoint(self):
        path = self.cfg.get("pretrained_model_name_or_path")
        return os.path.join(str(path), "unet") if path and os.path.isdir(os.path.join(str(path), "unet")) else None

    def load_scheduler(self):
        # the SD v1 scheduler_config.json: scaled-linear betas 0.00085 -> 0.012 (delete_sd.py:412)
        return DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")

    def check_supported(self):
        """delete_sd.py reads more knobs than the pixel-space loops; the ones this loop does not implement are refused
        instead of silently training something else (all at their shipped defaults in config/delete_sd.yaml:99-102,125)."""
        super().check_supported()
        cfg = self.cfg
        if cfg.get("image_store") is not None:
            raise NotImplementedError(f"image_store={cfg.get('image_store')!r}: the image store serves the pixel-space tasks; the SD "
                                      "loop trains on VAE latents, and what it keeps on the device is `latent_cache` (config/delete_sd.yaml)")
        if cfg.get("input_perturbation"):
            raise NotImplementedError(f"input_perturbation={cfg.get('input_perturbation')!r}: perturbed noising with an unperturbed "
                                      "target (delete_sd.py:899-903,:920-926) is not implemented; null in config/delete_sd.yaml")
        if cfg.get("snr_gamma") is not None:
            raise NotImplementedError(f"snr_gamma={cfg.get('snr_gamma')!r}: the reference's only live loss branch is "
                                      "`if self.cfg.snr_gamma is None` (delete_sd.py:962); min-SNR weighting is not implemented")
        if cfg.get("prediction_type") not in (None, "null", "epsilon"):
            raise NotImplementedError(f"prediction_type={cfg.get('prediction_type')!r}: only the epsilon objective is on this "
                                      "path (the v-prediction target is commented out in the reference too: delete_sd.py:953-958)")
        if cfg.get("use_8bit_adam"):
            raise NotImplementedError("use_8bit_adam=true: bitsandbytes' 8-bit AdamW (delete_sd.py:555-565) is not implemented; "
                                      "the fused step keeps f32 moments")

    def lr_schedule_args(self, world):
        cfg = self.cfg                                          # delete_sd.py:714-719
        return int(cfg.get("lr_warmup_steps") or 0) * world, int(cfg.get("training_steps") or 0)

    def sample_noise(self, shape, device, generator):
        noise = torch.randn(shape, device=device, generator=generator)
        off = float(self.cfg.get("noise_offset") or 0.0)
        if off:                                                 # delete_sd.py:893-898 (offset noise, one draw per (sample, channel))
            noise = noise + off * torch.randn((shape[0], shape[1], 1, 1), device=device, generator=generator)
        return noise

    def optimizer_args(self):
        c = self.cfg                                            # delete_sd.py:546-552 (scale_lr), :567-573
        lr = float(c.learning_rate)
        if c.get("scale_lr"):
            world = int(os.environ.get("WORLD_SIZE", "1"))
            lr *= int(c.gradient_accumulation_steps) * int(c.train_batch_size) * world
        return lr, (float(c.adam_beta1), float(c.adam_beta2)), float(c.adam_epsilon), float(c.adam_weight_decay)

    def fill_cfg(self):
        """delete_sd.py:343-348: with deletion.frac_deletion null and data_files.clustering_info_path on disk (tools/make_sd_clusters.py
        writes it), frac_deletion and data_files.mem_img_path = img_dir/<images_name>_<mem_idx:03d>.png come from that file.  (The
        reference fails without the file; here the placeholders then stay null, as they did before.)"""
        cfg = self.cfg
        d, df = cfg.get("deletion"), cfg.get("data_files")
        if d is None or not df or d.get("frac_deletion") is not None:
            return
        path = df.get("clustering_info_path")
        if not path or not os.path.isfile(str(path)):
            return
        with open(str(path), "r", encoding="utf-8") as f:
            info = json.load(f)
        d.frac_deletion = info["frac_deletion"]
        name = str(cfg.images_name) + "_" + str(info["mem_idx"]).zfill(3) + ".png"
        df.mem_img_path = os.path.join(str(df.get("img_dir") or ""), name)

    kmeans = None               # metrics.fraction_deletion's classifier (check_fraction_deletion), its tracker built at the first use
    fraction = None
    sscd = None                 # metrics.sscd's tracker (check_sscd): the network on the host until the first evaluation
    clip_iqa = None             # metrics.clip_iqa's tracker (check_clip_iqa): likewise

    def check_metrics(self):
        super().check_metrics()
        self.kmeans = self.check_fraction_deletion()
        self.sscd = self.check_sscd()
        self.clip_iqa = self.check_clip_iqa()
        self.replication = self.check_sscd_nn(ready=True)

    def check_sscd_nn(self, ready=False):
        """(the base's check_metrics asks before metrics.sscd is settled: answered once it is)"""
        return super().check_sscd_nn() if ready else None

    def sscd_nn_sources(self):
        df = self.cfg.get("data_files") or {}
        return "metrics.sscd", self.sscd, df.get("img_dir"), [df.get("mem_img_path")]

    def _need_vae(self, what, does):
        ckpt = str(self.cfg.get("pretrained_model_name_or_path") or "")
        if not os.path.isdir(os.path.join(ckpt, "vae")):
            raise FileNotFoundError(f"{what} {does}: no vae/ under {ckpt!r}")

    def _need_mem_image(self, what):
        mem = (self.cfg.get("data_files") or {}).get("mem_img_path")
        if not mem or not os.path.isfile(str(mem)):
            raise FileNotFoundError(f"{what}: data_files.mem_img_path {mem!r} (the memorized image; set from "
                                    "clustering_info_path when deletion.frac_deletion is null) is not a file on disk")
        return mem

    def check_clip_iqa(self):
        """metrics.clip_iqa (delete_sd.py:222-223,:264-267; null / absent / false: nothing; bare true: the mapping with no keys) needs
        model_path (OpenAI's RN50.pt, or a state dict of it) on disk -- or allow_random_init=true: a random-init network of the same
        architecture, loudly --, a checkpoint the loader accepts, a vae/ in the checkpoint directory (the network sees decoded
        images), and the anchor prompts' token ids: prompt_ids_path (a .pt of ids [2, L]: "Good photo." / "Bad photo."), else a CLIP
        tokenizer directory at tokenizer_path (default <pretrained_model_name_or_path>/tokenizer) -- refused here, before the first
        step.  Returns the clip_iqa.CLIPIQAScore, or None."""
        cfg = self.cfg
        ci = (cfg.get("metrics") or {}).get("clip_iqa")
        if not ci:
            return None
        ci = ci if isinstance(ci, dict) else {}
        from .clip_iqa import PROMPTS, CLIPIQAModel, CLIPIQAScore, tokenize
        path = ci.get("model_path")
        if not path:
            raise ValueError("metrics.clip_iqa: model_path is needed (OpenAI's CLIP RN50.pt, or a state dict of it)")
        self._need_vae("metrics.clip_iqa", "scores decoded validation images")
        bs = int(ci.get("batch_size") or 16)
        if os.path.isfile(str(path)):
            model = CLIPIQAModel.load(str(path), batch_size=bs)
        elif not (ci.get("allow_random_init") or cfg.get("allow_random_init")):
            raise FileNotFoundError(f"metrics.clip_iqa.model_path {path!r} is not a file on disk (pass allow_random_init=true for "
                                    "random-init weights of the same architecture)")
        else:
            model = CLIPIQAModel(batch_size=bs)
            print(f"[siss_amd] allow_random_init: CLIP checkpoint {path!r} not on disk, RANDOM-INIT CLIP RN50: the CLIP-IQA figures "
                  "are NOT comparable with published ones")
        ids_path = ci.get("prompt_ids_path")
        tok_dir = str(ci.get("tokenizer_path") or os.path.join(str(cfg.get("pretrained_model_name_or_path") or ""), "tokenizer"))
        if ids_path:
            if not os.path.isfile(str(ids_path)):
                raise FileNotFoundError(f"metrics.clip_iqa.prompt_ids_path {ids_path!r} is not a file on disk")
            ids = torch.as_tensor(torch.load(str(ids_path), map_location="cpu"))
            if ids.is_floating_point() or ids.dim() != 2 or ids.shape[0] != 2:
                raise ValueError(f"metrics.clip_iqa.prompt_ids_path {ids_path!r}: integer token ids [2, L] are needed (the rows of "
                                 f"{PROMPTS['quality'][0]!r} and {PROMPTS['quality'][1]!r}), got {ids.dtype} {tuple(ids.shape)}")
        elif os.path.isdir(tok_dir):
            ids = tokenize(PROMPTS["quality"], tok_dir, model.context_length)
        else:
            raise FileNotFoundError(f"metrics.clip_iqa needs the anchor prompts' token ids: neither prompt_ids_path nor a CLIP "
                                    f"tokenizer directory at tokenizer_path ({tok_dir!r})")
        if ids.shape[1] > model.context_length or int(ids.min()) < 0 or int(ids.max()) >= model.vocab_size:
            raise ValueError(f"metrics.clip_iqa: prompt ids [2, {ids.shape[1]}] reaching {int(ids.max())} do not fit the text tower "
                             f"({model.context_length} positions, vocabulary {model.vocab_size}): prompt_ids_path / tokenizer_path "
                             "belong to another model")
        self._note_eval_every("metrics.clip_iqa", "the score is taken")
        return CLIPIQAScore(model, ids, os.path.join(str(cfg.output_dir), "metrics_rank0.jsonl"))

    def check_sscd(self):
        """metrics.sscd (delete_sd.py:226-228,:277-283; null / absent: nothing) needs model_path on disk (or allow_random_init=true:
        a random-init network of the same architecture, loudly), a checkpoint the loader accepts, a vae/ in the checkpoint directory
        (the network sees decoded images), data_files.mem_img_path on disk, and data_transforms null or a Compose of exactly one
        Normalize with one or three means and stds (the ToTensor in front of it is part of the fused preprocessing) -- refused
        here, before the first step.  Returns the sscd.SSCDScore, or None."""
        cfg = self.cfg
        sc = (cfg.get("metrics") or {}).get("sscd")
        if not sc:
            return None
        from .sscd import SSCDScore
        path = sc.get("model_path") if isinstance(sc, dict) else None
        if not path:
            raise ValueError(f"metrics.sscd={sc!r}: model_path is needed (sscd_disc_mixup.torchscript.pt, or a state dict of it)")
        mean, std = _sscd_normalize(sc.get("data_transforms"), "metrics.sscd")
        self._need_vae("metrics.sscd", "embeds decoded validation images")
        mem = self._need_mem_image("metrics.sscd")
        model = _load_sscd(path, sc.get("allow_random_init") or cfg.get("allow_random_init"), "metrics.sscd")
        self._note_eval_every("metrics.sscd", "the score is taken")
        return SSCDScore(model, str(mem), os.path.join(str(cfg.output_dir), "metrics_rank0.jsonl"), mean, std)

    def check_injection_score(self):
        """metrics.denoising_injections: {strength, num_images, prompt} (null / absent: nothing): at each evaluation the memorized
        image is noised part of the way (strength of pipeline.num_inference_steps) and denoised under validation_prompts[prompt]
        (SDSampler.denoise_injection).  Needs a vae/ in the checkpoint directory (encoder and decoder), data_files.mem_img_path on
        disk, 0 < strength with at least one step left (strength * num_inference_steps >= 1), a positive num_images and a prompt
        index inside validation_prompts -- refused here, before the first step.  Returns the settings, or None."""
        cfg = self.cfg
        inj = (cfg.get("metrics") or {}).get("denoising_injections")
        if not inj:
            return None
        if not isinstance(inj, dict):
            raise ValueError(f"metrics.denoising_injections={inj!r}: a mapping {{strength, num_images, prompt}} is needed")
        number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        strength = inj.get("strength", 0.5)
        if not number(strength) or not strength > 0:
            raise ValueError(f"metrics.denoising_injections.strength={strength!r}: a positive number is needed")
        steps = _inference_steps(cfg)
        if int(steps * strength) < 1:
            raise ValueError(f"metrics.denoising_injections.strength={strength!r} of pipeline.num_inference_steps={steps} leaves no "
                             "denoising step (strength * num_inference_steps < 1)")
        n = inj.get("num_images", 1)
        if not _positive_int(n):
            raise ValueError(f"metrics.denoising_injections.num_images={n!r}: a positive count is needed")
        vp = cfg.get("validation_prompts") or [None]
        prompt = inj.get("prompt", 0)
        if not isinstance(prompt, int) or isinstance(prompt, bool) or not 0 <= prompt < len(vp):
            raise ValueError(f"metrics.denoising_injections.prompt={prompt!r}: an index into validation_prompts ({len(vp)} entries) "
                             "is needed")
        self._need_vae("metrics.denoising_injections", "encodes the memorized image and decodes the result")
        mem = self._need_mem_image("metrics.denoising_injections")
        self._note_eval_every("metrics.denoising_injections", "the check runs")
        return dict(strength=float(strength), num_images=n, prompt=prompt, mem_img_path=str(mem))

    def check_fraction_deletion(self):
        """metrics.fraction_deletion (delete_sd.py:224-225,:269-275; null / absent: nothing) needs classifier_path, that file on disk,
        a vae/ in the checkpoint directory (the classifier sees decoded images), centres of 3 * resolution^2 features and exactly two
        clusters (the reference's `preds.mean()` is a fraction only then) -- refused here, before the first step.  Returns the
        KMeansClassifier, or None."""
        cfg = self.cfg
        fd = (cfg.get("metrics") or {}).get("fraction_deletion")
        if not fd:
            return None
        path = fd.get("classifier_path") if isinstance(fd, dict) else None
        if not path:
            raise ValueError(f"metrics.fraction_deletion={fd!r}: classifier_path is needed (a scikit-learn KMeans .joblib / .pkl, or "
                             "the .npz tools/make_sd_clusters.py writes)")
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f"metrics.fraction_deletion.classifier_path {path!r} is not a file on disk")
        self._need_vae("metrics.fraction_deletion", "classifies decoded validation images")
        from .kmeans import KMeansClassifier
        clf = KMeansClassifier.load(str(path))
        res = int(cfg.get("resolution") or 512)
        if clf.n_features != 3 * res * res:
            raise ValueError(f"metrics.fraction_deletion: the classifier's centres have {clf.n_features} features, images of "
                             f"resolution {res} have 3 * {res}^2 = {3 * res * res}")
        if clf.n_clusters != 2:
            raise ValueError(f"metrics.fraction_deletion: {clf.n_clusters} clusters; the deletion fraction is the mean label, a "
                             "fraction only for two (label 1 = memorized)")
        self._note_eval_every("metrics.fraction_deletion", "the fraction is taken")
        return clf

    def datasets(self, shape):
        cfg = self.cfg
        la, ld = cfg.get("latents_all"), cfg.get("latents_deletion")
        ia, idl = cfg.get("images_all"), cfg.get("images_deletion")
        from .data import ImagesOnly, TensorImages
        df = cfg.get("data_files") or {}
        img_dir, lp = df.get("img_dir"), df.get("labels_path")
        if self.vae is not None and img_dir and lp and os.path.isdir(str(img_dir)) and os.path.isfile(str(lp)):
            # delete_sd.py:656,:681-682: the image directory split by kmeans_labels.json; the loop takes batch[0], the images
            kw = dict(img_dir=str(img_dir), labels_fpath=str(lp), transform=hydra_lite.instantiate(cfg.get("data_transforms")))
            self.encodes_images = True
            return ImagesOnly(hydra_lite.instantiate(cfg.all_data, **kw)), ImagesOnly(hydra_lite.instantiate(cfg.memorized_data, **kw))
        if self.vae is not None and ia and idl and os.path.exists(str(ia)) and os.path.exists(str(idl)):
            self.encodes_images = True
            return TensorImages(torch.load(ia)), TensorImages(torch.load(idl))     # [N,3,H,W] in [-1,1]: encoded per batch
        if la and ld and os.path.exists(str(la)) and os.path.exists(str(ld)):
            return TensorImages(torch.load(la)), TensorImages(torch.load(ld))
        if not cfg.get("allow_synthetic"):
            raise FileNotFoundError("no images_all / images_deletion (with a vae/ on disk) or latents_all / latents_deletion "
                                    "tensor files configured; pass allow_synthetic=true for synthetic latents")
        print("[siss_amd] allow_synthetic: no image / latent files configured, SYNTHETIC latents")
        return (SyntheticImages(4096, shape, seed=1, scale=self.VAE_SCALE, normal=True),
                SyntheticImages(1, shape, seed=2, scale=self.VAE_SCALE, normal=True))

    def _prompt_embedding(self, p, device, synthetic_seed=0):
        """[1, L, X] f32 embedding of one validation prompt: a .pt embedding / token-id file, a string through text_encoder/ +
        tokenizer/, or (allow_synthetic) a seeded synthetic embedding (seed() + synthetic_seed: 0 the prompt, 1 the empty prompt, 2 the
        teacher's anchor)."""
        cfg = self.cfg
        X = int((cfg.get("unet") or {}).get("cross_attention_dim", 768))
        if p and str(p).endswith(".pt") and os.path.exists(str(p)):
            e = torch.load(str(p)).to(device)
            if not e.is_floating_point():                       # token ids [77] / [1,77]: run the text encoder
                assert self.text_encoder is not None, "token ids given but no text_encoder/ in the checkpoint directory"
                e = self.text_encoder(e.reshape(1, -1))[0]
            e = e.float().reshape(-1, e.shape[-2], e.shape[-1])[:1]
        elif p and self.text_encoder is not None:
            from transformers import CLIPTokenizer               # delete_sd.py:395-410 tokenize_captions
            tok = CLIPTokenizer.from_pretrained(str(cfg.pretrained_model_name_or_path), subfolder="tokenizer")
            ids = tok([str(p)], max_length=tok.model_max_length, padding="max_length", truncation=True,
                      return_tensors="pt").input_ids
            e = self.text_encoder(ids)[0].float()
        elif cfg.get("allow_synthetic"):
            e = torch.randn(1, 77, X, generator=torch.Generator().manual_seed(self.seed() + synthetic_seed)).to(device)
        else:
            raise FileNotFoundError("validation_prompts[0] is neither a .pt embedding / token file on disk nor a prompt with a "
                                    "text_encoder/ + tokenizer/ on disk; pass allow_synthetic=true for a synthetic embedding")
        return e

    def conditioning(self, B, device):
        vp = self.cfg.get("validation_prompts")
        e = self._prompt_embedding(vp[0] if vp else None, device)
        return {"encoder_hidden_states": e.repeat(B, 1, 1)}     # one prompt for the whole batch (delete_sd.py:941-944)

    pipeline = None             # the validation pipeline (SDSampler), built at the first evaluation

    def _empty_prompt_embedding(self, device, what):
        """[1, L, X] f32 embedding of the empty prompt: the text encoder's output for it, or (allow_synthetic) a seeded synthetic one --
        the negative prompt of the validation pipeline and the unconditional rows of the teacher's esd target."""
        from .sd_sampler import uncond_ids
        cfg = self.cfg
        path = str(cfg.get("pretrained_model_name_or_path") or "")
        if self.text_encoder is not None:
            ids = uncond_ids(path)
            if int(ids.max()) >= self.text_encoder.tok.shape[0]:      # (checked here: a bad id would fault the gather on the device)
                raise ValueError(f"empty-prompt token ids reach {int(ids.max())}, beyond the text encoder's vocabulary of "
                                 f"{self.text_encoder.tok.shape[0]}: put the checkpoint's tokenizer/ beside it")
            return self.text_encoder(ids)[0].float()
        if cfg.get("allow_synthetic"):
            X = int((cfg.get("unet") or {}).get("cross_attention_dim", 768))
            return torch.randn(1, 77, X, generator=torch.Generator().manual_seed(self.seed() + 1)).to(device)
        raise FileNotFoundError(f"{what} needs the empty prompt's embedding: no text_encoder/ in the checkpoint directory "
                                "(pass allow_synthetic=true for a synthetic one)")

    def _validation_pipeline(self, unet, device):
        """The SD pipeline of log_validation (delete_sd.py:185-204), built at the first evaluation: the VAE decoder is read from
        vae/ only now (no vae/ on disk: noise norms without images); the negative prompt is the text encoder's output for the
        empty prompt, or a seeded synthetic embedding where the prompts are synthetic too."""
        from .scheduler import DDIMScheduler
        from .sd_sampler import SDSampler
        cfg = self.cfg
        path = str(cfg.get("pretrained_model_name_or_path") or "")
        vae = None
        if os.path.isdir(os.path.join(path, "vae")):
            from .vae import VAEDecoder
            vae = VAEDecoder.from_pretrained(path, "vae", device)
        else:
            print(f"[siss_amd] evaluation: no vae/ under {path!r}: noise norms only, no validation images")
        neg = self._empty_prompt_embedding(device, "evaluation")
        self.pipeline = SDSampler(unet, vae=vae, scheduler=self._sd_solver() or DDIMScheduler.from_pretrained(path or None),
                                  vae_encoder=self.vae)
        self._negative_embeds = neg
        return self.pipeline

    def _sd_solver(self):
        """pipeline.sampler for the validation pipeline: the betas of the checkpoint's scheduler/scheduler_config.json (else the SD v1
        values), "leading" spacing and that file's steps_offset where the key leaves them out -- the DDIM grid's conventions."""
        from .scheduler import SD_V1_SCHEDULER
        fn = os.path.join(str(self.cfg.get("pretrained_model_name_or_path") or ""), "scheduler", "scheduler_config.json")
        base = SD_V1_SCHEDULER
        if os.path.isfile(fn):
            with open(fn) as f:
                base = json.load(f)
        return _pipeline_sampler(self.cfg, base, timestep_spacing="leading", steps_offset=int(base.get("steps_offset", 0)))

    def evaluate(self, unet, sched, forget_image, step, device):
        """The image and noise-norm part of log_validation (delete_sd.py:170-340): per validation prompt, eval_batches x
        eval_batch_size images (DDIM, pipeline.num_inference_steps or 50 steps, guidance 7.5) from ONE generator seeded from
        cfg.seed per evaluation (:213-218), written as a PNG grid (nrow = int(sqrt(N)), :246), and the per-step text-conditional
        and unconditional noise norms averaged over the images, index 0 = the smallest timestep (:284-291), appended to
        noise_norms_rank0.jsonl.  Opt-in through eval_every; its own RNG; the engine's weights are only read.  The configured scorers
        of the decoder's output run as one chain (metric_net.score_chain) in the order fraction, SSCD, CLIP-IQA: the first makes the
        grid's uint8 images in its fused launch, the others read those bytes, and each appends one record per prompt to
        metrics_rank0.jsonl -- {global_step, deletion_fraction_<i>}: the mean k-means label over the images (:271-273), with
        deletion_steps_<i> on the first evaluation whose fraction is 0 (:274-275); {global_step, sscd_<i>}: the mean cosine with the
        memorized image's embedding (:277-283); {global_step, clip_iqa_<i>}: the mean probability of "Good photo." against "Bad
        photo." (:264-267).  Only the scores, the labels and the grid's bytes leave the device.  With metrics.denoising_injections
        the memorized image is then injected and denoised (evaluate_injection)."""
        import numpy as np
        cfg = self.cfg
        sampler = self.pipeline or self._validation_pipeline(unet, device)
        nb, bs = int(cfg.get("eval_batches") or 8), int(cfg.get("eval_batch_size") or 1)
        steps = _inference_steps(cfg)
        vp = cfg.get("validation_prompts") or [None]
        g = torch.Generator(device=device).manual_seed(self.seed())
        from .metric_net import score_chain
        from .scheduler import DPMSolverMultistepScheduler
        fields = sampler.scheduler.record_fields(steps) if isinstance(sampler.scheduler, DPMSolverMultistepScheduler) else None
        if self.kmeans is not None and self.fraction is None:
            from .kmeans import DeletionFraction
            self.fraction = DeletionFraction(self.kmeans, os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))
        # the scorers of the decoder's output in the order of their records: the first makes the uint8 bytes, the others read them
        active = [(what, scorer) for what, scorer in (("metrics.fraction_deletion", self.fraction), ("metrics.sscd", self.sscd),
                                                      ("metrics.clip_iqa", self.clip_iqa)) if scorer is not None]
        if active and sampler.vae is None:
            raise FileNotFoundError(f"{active[0][0]}: the validation pipeline has no VAE decoder")
        keep = None
        if self.replication is not None:             # metrics.sscd's pass keeps its rows: they serve sscd_<i> and the search
            from .sscd_search import KeepEmbeddings
            keep = KeepEmbeddings(self.sscd)
            active = [(what, keep if scorer is self.sscd else scorer) for what, scorer in active]
            self.replication.extra = fields
        for _, scorer in active:
            scorer.extra = fields                               # pipeline.sampler: every record says which sampler made the images
        out_type = "decoded" if active else "np" if sampler.vae is not None else "latent"
        with sampler.holding_graphs():
            for i, p in enumerate(vp):
                e = self._prompt_embedding(p, device)
                imgs, text_n, uncond_n, results, rows = [], [], [], [[] for _ in active], []
                for _ in range(nb):
                    im, st = sampler(e, negative_prompt_embeds=self._negative_embeds, num_inference_steps=steps,
                                     guidance_scale=7.5, num_images_per_prompt=bs, generator=g, output_type=out_type)
                    if active:
                        out, im = score_chain([scorer for _, scorer in active], im)     # uint8 [n, H, W, 3], still on the device
                        for got, one in zip(results, out):
                            got.append(one)
                        if keep is not None:
                            rows.append(keep.emb)
                        imgs.extend(list(im.cpu().numpy()))
                    elif out_type == "np":
                        imgs.extend(list(im))
                    text_n.extend(st["text_noise_norm"])
                    uncond_n.extend(st["uncond_noise_norm"])
                for (_, scorer), got in zip(active, results):
                    if got:
                        scorer.record(i, torch.cat(got).cpu(), step)
                if rows:
                    self.replication.record(i, torch.cat(rows), step)
                if imgs:
                    _grid(imgs, int(np.sqrt(len(imgs)))).save(os.path.join(cfg.output_dir, f"validation_p{i}_step{step}.png"))
                rec = {"step": step, "prompt": i, "prompt_text": None if p is None else str(p),
                       "timesteps": sampler.scheduler.timesteps[::-1],
                       "text_noise_norm": np.mean(np.asarray(text_n), axis=0)[::-1].tolist(),
                       "uncond_noise_norm": np.mean(np.asarray(uncond_n), axis=0)[::-1].tolist(), **(fields or {})}
                append_jsonl(os.path.join(cfg.output_dir, "noise_norms_rank0.jsonl"), rec)
            if self.injection is not None:
                self.evaluate_injection(sampler, step, device, steps)

    _mem_image = None           # the memorized image [1, 3, H, W] in [-1, 1] on the device, read at the first injection

    def evaluate_injection(self, sampler, step, device, steps):
        """metrics.denoising_injections (check_injection_score): data_files.mem_img_path -- (bytes - 127.5) / 127.5, as
        data_transforms maps the training images -- through the VAE encoder, noised to the first of the last int(steps * strength)
        DDIM timesteps and denoised under validation_prompts[prompt] at the validation pass's guidance scale, num_images times
        from a generator of its own seeded from cfg.seed.  The images go to injected_mem_s<strength>_step<k>.png; with metrics.sscd
        their mean cosine with the memorized image's embedding is appended to metrics_rank0.jsonl as sscd_inj_<prompt>."""
        import numpy as np
        cfg, inj = self.cfg, self.injection
        if sampler.vae is None or sampler.vae_encoder is None:
            raise FileNotFoundError("metrics.denoising_injections: the validation pipeline has no VAE encoder / decoder")
        if self._mem_image is None:
            from PIL import Image
            u8 = np.asarray(Image.open(inj["mem_img_path"]).convert("RGB"), dtype=np.uint8)
            self._mem_image = ((torch.from_numpy(u8.copy()).to(device).float() - 127.5) / 127.5).permute(2, 0, 1)[None].contiguous()
        vp = cfg.get("validation_prompts") or [None]
        e = self._prompt_embedding(vp[inj["prompt"]], device)
        g = torch.Generator(device=device).manual_seed(self.seed())
        im, _ = sampler.denoise_injection(self._mem_image, e, strength=inj["strength"], negative_prompt_embeds=self._negative_embeds,
                                          num_inference_steps=steps, guidance_scale=7.5, num_images_per_prompt=inj["num_images"],
                                          generator=g, output_type="decoded" if self.sscd is not None else "np")
        if self.sscd is not None:
            scorer = self.sscd
            if self.replication is not None:
                from .sscd_search import KeepEmbeddings
                scorer = KeepEmbeddings(self.sscd)
            scores, im = scorer.score_decoded(im)               # bytes and embeddings in one pass
            self.sscd.record(f"inj_{inj['prompt']}", scores.cpu(), step)
            if self.replication is not None:
                self.replication.record(f"inj_{inj['prompt']}", scorer.emb, step)
            im = im.cpu().numpy()
        name = f"injected_mem_s{inj['strength']:g}_step{step}.png"
        _grid(list(im), int(np.sqrt(len(im)))).save(os.path.join(cfg.output_dir, name))


class TrainUnconditional(Task):
    """config/train_tshirt_mnist.yaml -- DDPM pre-training (train_unconditional.py:76-532 of the reference): `num_epochs` epochs of
    the plain eps-MSE step (siss_amd/train.py) with the EMA of the weights, a sample grid from the EMA weights every `sampling_steps`,
    a resumable `checkpoint-<global_step>/` every `checkpointing_steps` (siss_amd/checkpoint.py), `unet/` and `unet_ema/` at the end."""

    default_unet = staticmethod(UNet2DConfig.mnist_tshirt)
    train_store = None          # image_store on: the ImageStore of the training set (siss_amd/image_store.py)

    def check_supported(self):
        cfg = self.cfg
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("WORLD_SIZE > 1: the pre-training task runs on one GPU (no sharded epoch loader, no all-reduce "
                                      "of the single gradient set yet)")
        pt = (cfg.get("scheduler") or {}).get("prediction_type", "epsilon")
        if pt != "epsilon":
            raise NotImplementedError(f"scheduler.prediction_type={pt!r}: only the epsilon objective (train_unconditional.py:388-391) "
                                      "is implemented; 'sample' with its SNR weights (:392-403) is not")
        if cfg.get("mixed_precision") == "fp16":
            raise NotImplementedError("mixed_precision='fp16': this build computes in 'bf16' or in f32 (null / 'no'); there is no "
                                      "loss scaler")
        if cfg.get("enable_xformers_memory_efficient_attention"):
            raise NotImplementedError("enable_xformers_memory_efficient_attention=true: xformers is not used here (the attention "
                                      "kernels are this package's own)")
        _pipeline_sampler(cfg)                                   # pipeline.sampler: a bad name / option is refused before the first step
        if (cfg.get("deletion") or {}).get("lora") is not None:
            raise NotImplementedError("deletion.lora: LoRA adapters belong to the unlearning tasks (delete_celeb / delete_tshirt / "
                                      "delete_sd); the pre-training task updates every parameter")
        if (cfg.get("deletion") or {}).get("saliency") is not None:
            raise NotImplementedError("deletion.saliency: the saliency mask belongs to the unlearning tasks (delete_celeb / delete_tshirt "
                                      "/ delete_sd); the pre-training task has no forget set and updates every parameter")
        if (cfg.get("deletion") or {}).get("ewc") is not None:
            raise NotImplementedError("deletion.ewc: the Fisher anchor belongs to the unlearning tasks (delete_celeb / delete_tshirt / "
                                      "delete_sd); the pre-training task has no pretrained weights to stay near")
        if (cfg.get("deletion") or {}).get("surgery") is not None:
            raise NotImplementedError("deletion.surgery: gradient surgery belongs to the unlearning tasks (delete_celeb / delete_tshirt "
                                      "/ delete_sd); the pre-training task has one gradient set and nothing to project")
        if (cfg.get("deletion") or {}).get("teacher") is not None:
            raise NotImplementedError("deletion.teacher: the teacher target belongs to the unlearning task delete_sd; the pre-training "
                                      "task has no forget set and no pretrained network to take targets from")
        if (cfg.get("deletion") or {}).get("ssd") is not None:
            raise NotImplementedError("deletion.ssd: Selective Synaptic Dampening belongs to the unlearning tasks (delete_celeb / "
                                      "delete_tshirt / delete_sd); the pre-training task has no forget set to dampen for")
        if (cfg.get("deletion") or {}).get("uce") is not None:
            raise NotImplementedError("deletion.uce: no cross-attention: the pre-training task's UNet takes no prompt (Unified Concept "
                                      "Editing belongs to the unlearning task delete_sd)")
        if (cfg.get("metrics") or {}).get("mia") is not None:
            raise NotImplementedError("metrics.mia: the membership inference attacks belong to the pixel-space unlearning tasks "
                                      "(delete_celeb / delete_tshirt); the pre-training task has no forget set to place among holdout images")

    def dataset(self, shape):
        cfg = self.cfg
        try:
            if cfg.get("dataset") is None:
                raise FileNotFoundError("no dataset configured")
            return hydra_lite.instantiate(cfg.dataset, transform=hydra_lite.instantiate(cfg.transform))
        except FileNotFoundError as e:
            if not cfg.get("allow_synthetic"):
                raise
            n = int(cfg.get("synthetic_images") or 4096)
            print(f"[siss_amd] allow_synthetic: dataset unavailable ({e}); using {n} SYNTHETIC images")
            return SyntheticImages(n, shape, seed=1)

    def run(self):
        from .checkpoint import load_state, save_state, step_of
        from .data import EpochSampler
        from .ema import EMAModel
        from .model import UNet2DModel
        from .scheduler import lr_multiplier
        from .train import TrainStepper
        cfg = self.cfg
        self.check_supported()
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
        seed = int(cfg.random_seed)
        torch.manual_seed(seed)
        dt = self.compute_dtype()
        unet = UNet2DModel(self.unet_config(), device=device, compute_dtype=dt)     # (cfg.unet / the default: checkpoint_path is a state to resume)
        unet.engine.init_random(seed=seed)
        sched = DDPMScheduler(**_scheduler_kwargs(cfg))
        ecfg = cfg.get("ema") or {}
        ema = None
        if ecfg.get("use_ema"):                                  # train_unconditional.py:186-194
            ema = EMAModel(unet, decay=float(ecfg.get("ema_max_decay", 0.9999)), use_ema_warmup=True,
                           inv_gamma=float(ecfg.get("ema_inv_gamma", 1.0)), power=float(ecfg.get("ema_power", 2 / 3)),
                           model_cls=UNet2DModel, model_config=unet.config)
        opt = hydra_lite.instantiate(cfg.optimizer)
        B, ga = int(cfg.train_batch_size), int(cfg.gradient_accumulation_steps)
        stepper = TrainStepper(unet.engine, sched.alphas_cumprod, lr=opt.lr, betas=opt.betas, eps=opt.eps,
                               weight_decay=opt.weight_decay, grad_accum=ga, ema=ema, mixed_precision=cfg.get("mixed_precision"))
        shape = (unet.config.in_channels, unet.config.sample_size, unet.config.sample_size)
        ds = self.dataset(shape)
        _open_image_stores(self, cfg, dict(train=ds), device)    # image_store on: train_store, one gather launch per micro-batch
        store = self.train_store
        num_epochs = int(cfg.num_epochs)
        sampler = EpochSampler(len(ds), B, seed, num_epochs)
        per_epoch = -(-len(sampler) // ga)                       # num_update_steps_per_epoch (:297-299)
        max_steps = num_epochs * per_epoch
        lr_name = str(cfg.get("lr_scheduler") or "constant")
        warm, total = int(cfg.get("lr_warmup_steps") or 0) * ga, len(sampler) * num_epochs        # :277-282
        lr_multiplier(lr_name, 0, warm, total)                   # raises now for a schedule that is not implemented
        g = torch.Generator(device=device).manual_seed(seed)
        T = sched.config.num_train_timesteps
        global_step = lr_pos = 0
        path = cfg.get("checkpoint_path")
        if path:                                                 # :320-345
            print(f"Resuming from checkpoint {path}")
            state = load_state(str(path), unet, ema, stepper, generator=g)
            global_step = step_of(path)
            if state["global_step"] != global_step:
                raise ValueError(f"{path}: the directory name says step {global_step}, its state.json {state['global_step']}")
            sampler.epoch, sampler.position, lr_pos = int(state["epoch"]), int(state["position"]), int(state["lr_position"])
        os.makedirs(cfg.output_dir, exist_ok=True)
        sampling_steps, ckpt_steps = int(cfg.get("sampling_steps") or 0), int(cfg.get("checkpointing_steps") or 0)
        limit = cfg.get("checkpoints_total_limit")
        t0 = time.perf_counter()

        def record(handle, meta):
            st = handle.get()
            st["step"], st["epoch"], st["elapsed_s"] = meta
            return st

        def say(st, meta):
            print(f"step {meta[0]}/{max_steps}  loss {st['loss']:.4g}  lr {st['lr']:.3g}  |g| {st['pre_clip_norm']:.4g}")

        # (on the way out the log writes the last completed step and closes, then the store does)
        with (contextlib.closing(store) if store is not None else contextlib.nullcontext()), \
                LaggedLog(os.path.join(cfg.output_dir, "train_log_rank0.jsonl"), record, say) as log:
            for epoch, pos, idx in sampler:
                # lr_scheduler.step() (:414): accelerate's wrapper advances the schedule once per optimizer step that really happens,
                # not per micro-batch (AcceleratedScheduler under accumulate()); lr_pos counts those
                if stepper._micro == 0:
                    stepper.opt.lr = opt.lr * lr_multiplier(lr_name, lr_pos, warm, total)
                x0 = store.images(idx) if store is not None else torch.stack([ds[i] for i in idx]).to(device, non_blocking=True)
                noise = torch.randn(x0.shape, device=device, generator=g)
                t = torch.randint(0, T, (x0.shape[0],), device=device, generator=g)
                stepper.micro_step(x0, noise, t)
                if pos + 1 == len(sampler):
                    stepper.flush()                              # a partial accumulation group at the end of an epoch steps on what it has
                if stepper._micro != 0:
                    continue
                global_step += 1
                lr_pos += 1
                log.push(stepper.stats_async(), (global_step, epoch, time.perf_counter() - t0))
                if sampling_steps and global_step % sampling_steps == 0:
                    self.sample_grid(unet, ema, sched, global_step)
                if ckpt_steps and global_step % ckpt_steps == 0:
                    save_state(os.path.join(cfg.output_dir, f"checkpoint-{global_step}"), unet, ema, stepper,
                               dict(global_step=global_step, epoch=sampler.epoch + (sampler.position == len(sampler)),
                                    position=sampler.position % len(sampler), lr_position=lr_pos, generator=g),
                               limit=None if limit is None else int(limit))
        unet.save_pretrained(os.path.join(cfg.output_dir, (cfg.get("subfolders") or {}).get("unet") or "unet"))
        if ema is not None:
            ema.save_pretrained(os.path.join(cfg.output_dir, (cfg.get("subfolders") or {}).get("unet_ema") or "unet_ema"))
        return stepper

    def sample_grid(self, unet, ema, sched, global_step):
        """train_unconditional.py:427-452: `eval_batch_size` samples from the EMA weights (swapped under the engine for the
        evaluation), as a make_grid image samples_step<N>.png."""
        import numpy as np
        from .sampler import Evaluator
        cfg = self.cfg
        if getattr(self, "_evaluator", None) is None:           # one per run: the captured forward is reused by every grid
            self._evaluator = Evaluator(cfg)
            self._evaluator.load_model(unet, sched)
        ev = self._evaluator
        n = int(cfg.get("eval_batch_size") or 16)
        with (ema.applied(unet) if ema is not None else contextlib.nullcontext()):
            imgs = ev.sample_images(n, sampler=_pipeline_sampler(cfg, sched))
        imgs = (np.clip(imgs, 0, 1) * 255).astype(np.uint8)
        if imgs.shape[-1] == 1:
            imgs = np.repeat(imgs, 3, axis=-1)
        _grid(list(imgs), int(np.sqrt(n))).save(os.path.join(cfg.output_dir, f"samples_step{global_step}.png"))


def _grid(images, nrow, padding=2):
    """torchvision.utils.make_grid's layout (nrow images per row, 2-pixel black padding) of uint8 [H, W, 3] images, as a PIL image."""
    import numpy as np
    from PIL import Image
    n, (h, w, c) = len(images), images[0].shape
    cols = min(max(1, nrow), n)
    rows = -(-n // cols)
    out = np.zeros((rows * (h + padding) + padding, cols * (w + padding) + padding, c), dtype=np.uint8)
    for k, im in enumerate(images):
        r, q = divmod(k, cols)
        out[r * (h + padding) + padding:r * (h + padding) + padding + h, q * (w + padding) + padding:q * (w + padding) + padding + w] = im
    return Image.fromarray(out)

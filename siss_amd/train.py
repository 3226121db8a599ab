"""One DDPM pre-training optimizer step on HIP -- the loop body of the reference's train_unconditional.py:366-415:

    per micro-batch:  x_t   = add_noise(x0, noise, t), t ~ U{0..T-1}        [siss_mixture_fwd with u = 1, a0 = x0]
                      pred  = UNet(x_t, t)                                   [one forward]
                      c     = d/dpred F.mse_loss(pred, noise) / GA           [siss_mse_bwd_seed]
                      g    += J^T c                                          [ONE single-cotangent backward]
    sync step:        clip_grad_norm_(1.0); AdamW; EMAModel.step             [siss_grad_norm_single + siss_clip_adamw_ema]

The parts are SISSStepper's (siss_amd/step.py); the update is the single-set pair of csrc/train_state.hip, which reads ONE gradient set
and writes the EMA of the weights in the pass that updates them.  No host synchronisation; the logged scalars travel in one
asynchronous device-to-host copy (stats_async).
"""
import torch

from .loss import mixture_fwd, mse_bwd_seed
from .optim import FlatAdamW
from .unet import UNetEngine


class TrainStepper:
    wgrad_overwrite = True          # (A/B switch; see UNetEngine.wgrad_overwrite)

    def __init__(self, engine: UNetEngine, alphas_cumprod, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_accum=1,
                 max_grad_norm=1.0, ema=None, mixed_precision="bf16"):
        self.e = engine
        if hasattr(engine, "check_trainable"):
            engine.check_trainable()
        dev = engine.device
        ac = alphas_cumprod.to(device=dev, dtype=torch.float32).contiguous()
        self.ac, self.gamma_tab, self.sigma_tab = ac, (ac ** 0.5).contiguous(), ((1 - ac) ** 0.5).contiguous()
        self.ga, self.ema = int(grad_accum), ema
        f32_engine = getattr(engine, "f32", False)
        if f32_engine and mixed_precision == "bf16":
            raise ValueError("mixed_precision='bf16' on an f32 engine: build the engine with dtype=torch.bfloat16")
        self.io_dtype = torch.bfloat16 if mixed_precision == "bf16" else torch.float32
        self.opt = FlatAdamW(engine.ps.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                             shadow=None if f32_engine else engine.ps.shadow)
        self._micro = self._last = 0
        self._loss = None                   # [GA] device: each micro-batch's F.mse_loss, as the reference logs it per iteration

    def micro_step(self, x0, noise, t):
        """x0 / noise [b, C, H, W] (cast to the I/O dtype first, train_unconditional.py:366-370), t [b] int64.  Enqueues forward +
        backward, and after the last micro-batch of the step the update; no host sync."""
        e = self.e
        found = e.wgrad_overwrite
        try:
            # first micro-batch of a step: one-split weight gradients overwrite their tiles
            e.wgrad_overwrite = self._micro == 0 and self.wgrad_overwrite
            if self._micro == 0:
                e.zero_grad(beside_forward=True, sparse_key=("train_mse", tuple(x0.shape)))
                self._loss = torch.zeros(self.ga, dtype=torch.float32, device=e.device)
            x0, noise = (v.to(device=e.device, dtype=self.io_dtype).contiguous() for v in (x0, noise))
            b = x0.shape[0]
            m = mixture_fwd(x0, x0, noise, t, torch.ones(b, device=e.device), self.ac, self.gamma_tab, self.sigma_tab, 0.0)
            pred = e.forward(m.x_mix, t)
            chw = pred[0].numel()
            # F.mse_loss is a mean over b * chw elements and accelerate divides by GA: c = 2 (pred - noise) / (b chw GA); the kernel's
            # cotangent is 2 * scale * (pred - noise) with the per-sample sums left un-normalised, so 1 / chw goes into the scale here
            # and the loss mean divides the sums by chw
            cot, _, sums = mse_bwd_seed(pred, noise, 1.0 / (b * self.ga * chw))
            e.backward(cot, nsets=1)
            self._loss[self._micro] = sums.sum() / (b * chw)
        finally:
            e.wgrad_overwrite = found
        self._last = self._micro
        self._micro += 1
        if self._micro == self.ga:
            self.flush()

    def flush(self):
        """The update on what has been accumulated: after the last micro-batch of a step, or at the end of an epoch whose batch count
        is no multiple of GA (accelerate synchronises at the end of the dataloader)."""
        if self._micro == 0:
            return
        self._micro = 0
        self.opt.launch_single(self.e.ps.grads[0], ema=self.ema)
        self.e.refresh_weights(lazy=True)               # (the dgrad weight copies: beside the next forward pass)

    def step(self, x0, noise, t):
        """GA = 1 convenience."""
        assert self.ga == 1
        self.micro_step(x0, noise, t)

    def stats_async(self):
        """The step's logged scalars (train_unconditional.py:521-527: loss, lr, step, ema_decay; and the pre-clip gradient norm)
        gathered on the device and copied to pinned host memory behind the step's kernels; `.get()` waits for that copy."""
        blk = self.opt._train_block()
        dev = torch.cat([blk, self._loss[self._last:self._last + 1] if self._loss is not None else blk.new_zeros(1)])
        host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
        host.copy_(dev, non_blocking=True)                      # the one D2H of the step
        done = torch.cuda.Event()
        done.record()
        return _PendingTrainStats(host, done, blk.numel(), self.opt.lr, self.ema is not None)

    def stats(self):
        return self.stats_async().get()


class _PendingTrainStats:
    def __init__(self, host, done, nblk, lr, has_ema):
        self.host, self.done, self.nblk, self.lr, self.has_ema = host, done, nblk, lr, has_ema

    def get(self):
        self.done.synchronize()
        st = FlatAdamW.train_stats_from(self.host[:self.nblk])
        if not self.has_ema:
            del st["ema_decay"]
        st["loss"] = float(self.host[-1])                       # the LAST micro-batch's loss, as the reference's `logs`
        st["lr"] = self.lr
        return st

#!/usr/bin/env python
"""Regenerate tests/golden/membership_ref.npz from the reference implementation (run by hand, on the CPU, where a checkout of the
reference is at hand -- never part of a test run):

    python tests/make_membership_golden.py /path/to/reference

Imports the reference's metrics/class_membership.py by path and drives its MembershipLoss with oracle.unet.OracleUNet2D (built under
torch.manual_seed at CELEB_TINY) and siss_amd.scheduler.DDPMScheduler.  Two cases, a forget set of length 1 and one of length 9;
I = 5 images, J = 3 noises, eval_batch_size = 4 (15 % 4 != 0: the reference's last batch is ragged), timesteps [200, 900].  The file
holds the image pools, the indices random.sample drew under the recorded random.seed, the noises, the timesteps, the reference's
f32 outputs and an f64 checksum of the network's state dict (the weights are rebuilt from the seed, not stored).

Also confirms the condition the GPU negative control relies on: at t = 200 the f64 pair sums of the kept group with the kept images
rolled by one differ from the true ones by more than 10 times the f32 bound, for every pair."""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from membership_ref import CELEB_TINY, f32_bound, membership_f64, seeded_oracle, state_checksum   # noqa: E402

# DATA_SEED: the first of the image seeds 70 .. 89 whose pools meet the negative control's condition in BOTH cases (a property of
# the f64 oracle and the images alone; 15 random pairs do not all move by 10 bounds under every draw)
NET_SEED, DATA_SEED, I, J, EVAL_BATCH, TIMESTEPS = 1234, 75, 5, 3, 4, [200, 900]
CASES = {"del1": dict(n_del=1, random_seed=11, noise_seed=21), "del9": dict(n_del=9, random_seed=12, noise_seed=22)}


def main(reference_root):
    spec = importlib.util.spec_from_file_location("ref_class_membership", os.path.join(reference_root, "metrics", "class_membership.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from siss_amd.scheduler import DDPMScheduler
    sched = DDPMScheduler()
    net = seeded_oracle(NET_SEED)
    shape = (CELEB_TINY["in_channels"], CELEB_TINY["sample_size"], CELEB_TINY["sample_size"])
    chw = int(np.prod(shape))
    g = torch.Generator().manual_seed(DATA_SEED)
    pool_all = torch.rand((12, *shape), generator=g) * 2 - 1
    out = dict(net_seed=NET_SEED, checksum=np.float64(state_checksum(net.state_dict())), timesteps=np.asarray(TIMESTEPS),
               pool_all=pool_all.numpy(), I=I, J=J, eval_batch_size=EVAL_BATCH)
    net64 = seeded_oracle(NET_SEED).double()
    for name, c in CASES.items():
        pool_del = torch.rand((c["n_del"], *shape), generator=g) * 2 - 1
        random.seed(c["random_seed"])
        idx_all = random.sample(range(len(pool_all)), I)
        idx_del = [0] * I if c["n_del"] == 1 else random.sample(range(c["n_del"]), I)
        random.seed(c["random_seed"])
        m = ref.MembershipLoss(list(pool_all), list(pool_del), sched, net, I, J, EVAL_BATCH, "cpu")
        m.sample_images()
        assert torch.equal(m.all_sampled_images, pool_all[idx_all]) and torch.equal(m.deletion_sampled_images, pool_del[idx_del])
        torch.manual_seed(c["noise_seed"])
        m.sample_noises()
        losses = m.compute_membership_losses(TIMESTEPS)
        ref_out = np.asarray([[float(a), float(b)] for a, b in losses], dtype=np.float32)
        sums, means, pmax = membership_f64(net64, sched.alphas_cumprod, pool_all[idx_all], pool_del[idx_del], m.noise, TIMESTEPS,
                                           with_pred_max=True)
        rel = float((np.abs(means.numpy() - ref_out.astype(np.float64)) / np.abs(means.numpy())).max())
        # the negative control's condition (t = 200, kept group)
        rolled, _ = membership_f64(net64, sched.alphas_cumprod, torch.roll(pool_all[idx_all], 1, 0), pool_del[idx_del], m.noise, TIMESTEPS[:1])
        shift = (rolled[0, 0] - sums[0, 0]).abs().numpy()
        bound = f32_bound(sums[0, 0].numpy(), chw, pmax)
        print(f"{name}: reference f32 vs f64 restatement {rel:.2e} relative; max|pred| {pmax:.3f}; S in [{float(sums.min()):.1f}, "
              f"{float(sums.max()):.1f}]; t = {TIMESTEPS[0]}: smallest shift {shift.min():.3g} against a largest bound {bound.max():.3g}")
        assert rel <= 1e-6, rel
        assert (shift > 10 * bound).all(), "the fixture misses the negative control's factor: choose a smaller first timestep"
        out.update({f"{name}_pool_del": pool_del.numpy(), f"{name}_random_seed": c["random_seed"], f"{name}_idx_all": np.asarray(idx_all),
                    f"{name}_idx_del": np.asarray(idx_del), f"{name}_noise": m.noise.numpy(), f"{name}_ref": ref_out})
    path = os.path.join(HERE, "golden", "membership_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

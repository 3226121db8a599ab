"""Host reference of the membership-loss metric (test infrastructure only): the reference's
``MembershipLoss.compute_membership_losses`` (metrics/class_membership.py:68-130) restated in torch f64 on a torch network, pair by
pair, plus the pieces the fixture and the tests share (the network's configuration, its seeded construction, its checksum)."""
import numpy as np
import torch

# google/ddpm-celebahq-256's block kinds at two levels (tests/test_hip_likelihood.py CELEB_TINY)
CELEB_TINY = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
                  down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
                  layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6, downsample_padding=0,
                  flip_sin_to_cos=False, freq_shift=1)


def seeded_oracle(seed):
    """oracle.unet.OracleUNet2D at CELEB_TINY with torch's default initialisation under torch.manual_seed(seed) (f32)."""
    from oracle.unet import OracleUNet2D, UNetConfig
    torch.manual_seed(int(seed))
    return OracleUNet2D(UNetConfig(**CELEB_TINY)).eval()


def state_checksum(sd):
    """An f64 number that moves with every weight: sum_k sum_i w_k[i] * cos(i + k) over the state dict in key order."""
    total = 0.0
    for k, name in enumerate(sorted(sd)):
        w = sd[name].detach().double().reshape(-1)
        total += float((w * torch.cos(torch.arange(w.numel(), dtype=torch.float64) + k)).sum())
    return total


@torch.no_grad()
def membership_f64(net, ac, images_all, images_del, noise, timesteps, with_pred_max=False, batch=16):
    """(pair_sums f64 [T, 2, I, J], means f64 [T, 2]) of the reference's metric in f64: for every timestep, group (kept, forget),
    image i and noise j, sum_chw (net(sqrt(ac[t]) x_i + sqrt(1 - ac[t]) n_j, t) - n_j)^2; the means run over the I * J pairs.
    net: a torch module in f64 called as net(x, t)[0]; ac: alphas_cumprod (f32 values, used as they are).
    with_pred_max: also return max |net output| over everything evaluated."""
    I, J = images_all.shape[0], noise.shape[0]
    ac = ac.double()
    n = noise.double()
    sums = torch.zeros(len(timesteps), 2, I, J, dtype=torch.float64)
    pred_max = 0.0
    for ti, t in enumerate(timesteps):
        sa, sb = torch.sqrt(ac[int(t)]), torch.sqrt(1.0 - ac[int(t)])
        for g, imgs in enumerate((images_all, images_del)):
            x = (sa * imgs.double()[:, None] + sb * n[None]).reshape(I * J, *noise.shape[1:])     # image-major, noise-minor
            tgt = n[None].expand(I, *n.shape).reshape(I * J, *noise.shape[1:])
            out = []
            for s in range(0, I * J, batch):
                pred = net(x[s:s + batch], torch.full((x[s:s + batch].shape[0],), int(t), dtype=torch.long))[0]
                pred_max = max(pred_max, float(pred.abs().max()))
                out.append(((pred - tgt[s:s + batch]) ** 2).sum(dim=(1, 2, 3)))
            sums[ti, g] = torch.cat(out).view(I, J)
    means = sums.mean(dim=(2, 3))
    return (sums, means, pred_max) if with_pred_max else (sums, means)


def f32_bound(S, chw, pred_max):
    """The f32 instrument bound of a pair sum S: 1e-4 of max|pred| per element (tests/test_hip_f32_mode.py) carried through
    dS = 2 (p - n) dp over chw elements: |dS| <= 2 sqrt(chw * S) * 1e-4 * max|pred| (Cauchy-Schwarz)."""
    return 2.0 * np.sqrt(chw * np.asarray(S, dtype=np.float64)) * 1e-4 * float(pred_max)

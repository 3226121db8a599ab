#!/usr/bin/env python
"""Regenerate include/siss_hip.h from the extern "C" blocks of siss_amd/csrc/*.hip (declarations + the
comment above each launcher), with the per-file notes on what each group replaces in the reference."""
import os
import re
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = {
    'f32_path.hip': "The f32 PARITY MODE: the entry points above with f32 tensors (`mixed_precision: null`, config/delete_celeb.yaml:103 of the\n * reference: fp32 everywhere).  Same argument lists; every product on v_mfma_f32_16x16x4_f32; simple kernels -- the instrument\n * that holds the HIP network against the fp32 oracle at 1e-4, not a fast path.",
    'siss_loss.hip': "Fused SISS pre/post kernels.  Replaces losses/ddpm_deletion_loss.py:12-53 (mixture select, eps_x/eps_a,\n * dist_x/dist_a, ratios, importance weights, weighted losses) and delete_celeb.py:602-603 (add_noise x2 with\n * the same noise) / :686-687 (loss normalisation that seeds the two backward passes).",
    'gemm_nt.hip': "Panelled NT GEMM on bf16 MFMA: conv3x3 / conv1x1 / linear fprop and dgrad.  Replaces the cuDNN/cuBLAS\n * kernels the reference reaches through diffusers' ResnetBlock2D / Downsample2D / Upsample2D / Attention\n * (call site: losses/ddpm_deletion_loss.py:24 `unet(...)`, backward: delete_celeb.py:691,:702).",
    'gemm_tn.hip': "Panelled TN GEMM on bf16 MFMA: weight (and bias) gradients for both cotangent sets (g_x, g_a) in one pass.\n * Replaces the wgrad half of the two `accelerator.backward` calls (delete_celeb.py:691,:702) and the\n * clone / subtract split of :694-711.",
    'groupnorm.hip': "GroupNorm(+SiLU) forward / backward on padded NHWC.  Replaces torch.nn.GroupNorm + F.silu inside\n * diffusers' ResnetBlock2D.norm1/norm2, Attention.group_norm and UNet2DModel.conv_norm_out.",
    'optimizer.hip': "Flat-buffer norm-fix + recombine + clip + AdamW.  Replaces delete_celeb.py:714-753 (five 450-tensor\n * loops), :767 (clip_grad_norm_) and :769 (torch.optim.AdamW.step).",
    'train_state.hip': "The training state of the DDPM pre-training task (train_unconditional.py:366-415 of the reference: F.mse_loss ->\n * clip_grad_norm_(1.0) -> torch.optim.AdamW.step -> diffusers' EMAModel.step): ONE gradient set, the EMA of the weights written by the\n * same pass that updates them, and the swap that puts the EMA weights under the engine for an evaluation (EMAModel.store /\n * copy_to / restore in one pass each way).",
    'elementwise.hip': "Data movement on the padded-NHWC layout: F.interpolate(nearest 2x), torch.cat of skip connections,\n * Downsample2D's F.pad+stride-2 gather (space-to-depth), attention reshape/residual, bias-gradient column sums.",
    'conv_small.hip': "conv_out (Cout = image channels): direct kernels for UNet2DModel.conv_out and its backward.",
    'attention.hip': "Row softmax fwd/bwd of the single-head attention block (diffusers Attention, upcast_softmax=True).",
    'attn1h.hip': "Fused SINGLE-HEAD spatial self-attention (diffusers Attention with attention_head_dim = None: the six attention sites of\n * `google/ddpm-celebahq-256`, D = 512, S = 256 / 64): QK^T -> softmax -> .V in one kernel, backward in two; replaces torch's\n * scaled_dot_product_attention behind losses/ddpm_deletion_loss.py:24 and its two differentiations (delete_celeb.py:691,:702).",
    'flash_attn.hip': "Fused multi-head attention (QK^T -> softmax -> .V in one kernel, FlashAttention-2 style backward) for the SD\n * UNet's BasicTransformerBlock attn1 / attn2 (delete_sd.py:977-985 -> losses/ddpm_deletion_loss.py:24): replaces torch's\n * scaled_dot_product_attention; the S x S matrices never reach HBM.",
    'transformer.hip': "Token-space pieces of the SD UNet's Transformer2DModel (diffusers BasicTransformerBlock: LayerNorm,\n * GEGLU feed-forward, multi-head self / cross attention reshapes and softmax).  Call site: delete_sd.py:977-985\n * -> losses/ddpm_deletion_loss.py:24 with conditioning['encoder_hidden_states'].",
    'likelihood.hip': "The forget-set likelihood metric (metrics/likelihood.py + metrics/song_likelihood of the reference): the probability-flow\n * drift of the VP-SDE with its Hutchinson divergence (get_div_fn) and the f64 stage / error-norm arithmetic of scipy's RK45\n * (solve_ivp) over the joint state [x ; delta log p].",
    'membership.hip': "The membership-loss metric (metrics/class_membership.py of the reference, MembershipLoss.compute_membership_losses):\n * the (image, noise, timestep) work items of an evaluation noised straight into the forward's input and their squared errors\n * summed per pair, both driven by one device index table -- replaces the three expanded I x J tensors, add_noise x2 and\n * torch.sum((out - noise) ** 2) of :77-110.",
    'mia.hip': "Opt-in membership inference attacks (siss_amd/mia.py, `metrics.mia`, tools/mia.py; SecMI, Duan et al., ICML 2023; PIA,\n * Kong et al., ICLR 2024; NOT the reference's protocol, whose only membership evidence is the mean eps-MSE above): the element-wise\n * passes between the forwards of a deterministic DDIM chain over the rows of one image pool -- the gather of a batch, the transfer\n * y = cx x + ce e, SecMI's last transfer fused with its squared t-error, PIA's |e0 - e1|^p; explicit f32 round-to-nearest operations,\n * one f64 partial per (row, block) folded in index order, no atomics.",
    'kmeans.hip': "The SD deletion fraction (delete_sd.py:224-225,:269-275: joblib's scikit-learn KMeans.predict on 255 * ToTensor(PIL) of the\n * validation images, on the CPU) and the fit that produces that classifier: the decoder's output to uint8 with its distances to the\n * centres in one pass, Lloyd's assignment and update over uint8 rows; f64 / integer sums in fixed orders, no atomics.",
    'metric_conv.hip': "What the four f32 metric networks share (the MNIST ResNet-18 of metrics/mnist_resnet.py, the FID Inception-v3, the SSCD\n * ResNet-50 and the CLIP RN50 image tower; siss_amd/metric_net.py): one implicit-GEMM convolution for every layer, fc and projection\n * (NHWC gather with zero fill, or the NCHW image; independent KH / KW / padding; folded-BN bias, optional residual, optional ReLU,\n * written into a channel slice; deterministic split-K) and the 3 x 3 max pool.",
    'metric_train.hip': "Training of the MNIST ResNet-18 metric classifier (notebooks/cnn-resnet18-mnist.ipynb of the reference: train-mode\n * BatchNorm, F.cross_entropy, autograd, torch.optim.Adam; siss_amd/classifier_train.py), f32: the convolution's data and weight\n * gradients on the packed weights of siss_metric_conv above, batch-statistics BatchNorm forward / backward, the 3 x 3 / 2 max pool's\n * backward and softmax cross-entropy; sums in f64 or in fixed orders, no atomics.",
    'inception.hip': "The FID metric (metrics/fid.py of the reference: torchmetrics' FrechetInceptionDistance on the FID Inception-v3 of\n * torch-fidelity), f32: the preprocessing (uint8 truncation, TF1 bilinear resize to 299 x 299, (x - 128) / 128) in one launch, the\n * average pools, and the f64 feature statistics sum / cov_sum; the 94 BasicConv2d layers and the max pools run on siss_metric_conv /\n * siss_metric_maxpool3 above.",
    'sscd.hip': "The SD copy-detection score (delete_sd.py:226-228,:277-283: torch.jit.load of the SSCD ResNet-50, Normalize(ToTensor(PIL)),\n * the mean of mem_embedding @ all_embeddings.T), f32: the trunk and the 2048 -> 512 linear layer run on siss_metric_conv /\n * siss_metric_maxpool3 above; these are the preprocessing (from uint8, or fused with the decoder output's quantisation), GeM pooling and\n * F.normalize with the score, sums in f64 in fixed orders, no atomics.",
    'clip_iqa.hip': "The SD image-quality score (delete_sd.py:222-223,:264-267: torchmetrics' CLIPImageQualityAssessment, the OpenAI CLIP RN50\n * image tower against the anchors \"Good photo.\" / \"Bad photo.\"), f32: the convolutions and the q / c_proj projections run on\n * siss_metric_conv, the preprocessing on siss_sscd_preprocess above; these are the anti-aliasing average pool, the attention pool with the\n * query folded into the key projection and the value projection taken after the pooling (no T x E x E product, no token tensor), and\n * the score; sums in f64 or in fixed orders, no atomics.",
    'prompt_grad.hip': "Prompt-embedding gradients and the augmented prompt (data/src/local_sd_pipeline.py:325-445 get_text_cond_grad, :474-663\n * aug_prompt of the reference: autograd through the UNet with respect to encoder_hidden_states, torch.norm, torch.optim.AdamW): a\n * cross-attention site's text gradient dK W_k + dV W_v with f32 output, the fixed-order sum over sites and samples, the noise-norm\n * loss with its cotangent, and the embedding's masked / penalised AdamW step.",
    'injection.hip': "The img2img entry of the SD pipeline (data/src/local_sd_pipeline.py:250-323 prepare_latents_img2img: latent_dist.sample()\n * of the VAE encoder's moments, * scaling_factor, torch.cat to the batch, DDIMScheduler.add_noise at the first timestep): the noised\n * starting latents of the inject-then-denoise check in one streaming launch.",
    'dpm_solver.hip': "The opt-in DPM-Solver++ (2M) evaluation sampler (siss_amd/scheduler.py DPMSolverMultistepScheduler; no counterpart in the\n * reference, whose samplers are diffusers' DDPMScheduler / DDIMScheduler at 50 steps): classifier-free guidance, the x0-prediction and the\n * first / second order multistep update in one streaming launch per sampling step, with the noise norms of siss_cfg_ddim_step.",
    'latent_cache.hip': "The latent cache of the SD task (siss_amd/latent_cache.py; delete_sd.py:879-888 vae.encode(x).latent_dist.sample() *\n * vae.config.scaling_factor, once per micro-batch and batch): the frozen encoder's posterior moments of the dataset stay on the device and a\n * micro-batch of latents is one gather-and-sample launch over the rows its indices name.",
    'image_store.hip': "The image store of the pixel-space tasks (siss_amd/image_store.py; the DataLoader in front of delete_celeb.py:571-580 and\n * train_unconditional.py:366-372: decode, ToTensor / Normalize, stack and a host-to-device copy of f32 images per micro-batch): the dataset\n * stays on the device as uint8 and a micro-batch of images is one table-gather launch over the rows its indices name.",
    'lora.hip': "Opt-in LoRA unlearning on the UNet's linear projections and 3x3 convolutions (siss_amd/lora.py, `deletion.lora`; no counterpart\n * in the reference, whose runs update every parameter): the engine runs on the merged weight W = W0 + s B A, so these are the chain\n * rule from the weight gradients of both sets to the adapter's (dB = s dW A^T, dA = s B^T dW) and the merge back into the f32 master\n * and its bf16 shadow, each ONE launch over a device job table of all targets; the *_conv forms take the tap-major [9, Co, Ci]\n * weights with B shared by the taps (peft's Conv2d adapter); f32 MFMA products in fixed orders, no atomics.",
    'saliency.hip': "Opt-in saliency-masked unlearning (siss_amd/saliency.py, `deletion.saliency`; SalUn, Fan et al., ICLR 2024; no counterpart in the\n * reference, whose runs update every parameter): the exact k-th largest gradient magnitude of the flat buffer by an integer radix select,\n * the packed one-bit-per-weight mask of that threshold, and the two flat passes of optimizer.hip restricted to the weights whose bit is\n * set; integer counts and sums in fixed orders, no atomics on global memory.",
    'ewc.hip': "Opt-in Fisher-weighted anchor of the unlearning update (siss_amd/ewc.py, `deletion.ewc`; elastic weight consolidation as Selective\n * Amnesia uses it, Heng & Soh, NeurIPS 2023, and its uniform case L2-SP; no counterpart in the reference, whose runs have no penalty\n * term): the running empirical Fisher F += g^2 w of the keep gradient, and pass 1 of optimizer.hip with the penalty's gradient\n * strength * F * (p - pstar) folded into the keep-side set before the norms; explicit f32 round-to-nearest operations, f64 sums in\n * fixed orders, no atomics.",
    'surgery.hip': "Opt-in gradient surgery between the keep and forget gradients (siss_amd/surgery.py, `deletion.surgery`; PCGrad, Yu et al.,\n * NeurIPS 2020; gradient-projection unlearning, Hoang et al., WACV 2024; the restricted gradient of Ko et al., NeurIPS 2024; no counterpart\n * in the reference, whose update is g_x - s g_a whatever the sign of <g_x, g_a>): a deterministic segmented reduction of the three sums\n * per group of the flat buffer (the whole buffer, or one parameter tensor), the per-group coefficient table (cx, ca) of the projected\n * pair, and pass 2 of optimizer.hip recombining with it; f64 sums in fixed orders that do not depend on the grid, explicit f32\n * round-to-nearest operations, no atomics.",
    'teacher.hip': "Opt-in teacher-target unlearning (siss_amd/teacher.py, `deletion.loss_fn=teacher_target` with `deletion.teacher`; ESD, Gandikota\n * et al., ICCV 2023, and Concept Ablation, Kumari et al., ICCV 2023; NOT the reference's protocol, whose objectives regress onto the drawn\n * noise): the regression target from a frozen teacher's outputs with the cotangent of the student's stacked rows and the per-row loss sums\n * in one launch, and pass 1 of optimizer.hip with the scaling factor fixed at -weight (a plain weighted sum of the two gradient sets);\n * explicit f32 round-to-nearest operations, f64 sums in fixed orders that do not depend on the grid, no atomics.",
    'ssd.hip': "Opt-in Selective Synaptic Dampening (siss_amd/ssd.py, `deletion.ssd`; Foster, Schoepf & Brintrup, AAAI 2024; no counterpart in\n * the reference, whose runs unlearn by gradient steps only): the ratio of the forget set's empirical Fisher to the keep data's per\n * weight, and ONE streaming pass that selects the weights whose ratio lies above a threshold, scales them by min(lambda / ratio, 1)\n * and reports what it did; explicit f32 round-to-nearest operations, exact counts, f64 sums in fixed orders, no atomics.",
    'uce.hip': "Opt-in Unified Concept Editing of the SD UNet (siss_amd/uce.py, `deletion.uce`; Gandikota, Orgad, Belinkov, Materzynska\\n * & Bau, WACV 2024; no counterpart in the reference, whose runs unlearn by gradient steps only): the closed-form edit W' = W + W dT of\\n * the cross-attention key / value projections, dT ONE X x X matrix for every edited weight (formed in f64 on the host): the increments\\n * of all targets in one launch over a host job table (exact f32 on v_mfma_f32_16x16x4_f32, the tile of sscd_search.hip), and ONE f32\\n * add over the targets' floats that reports what it did; f64 sums in fixed orders, no atomics.",
    'sscd_search.hip': "Dataset-wide SSCD copy search (siss_amd/sscd_search.py, `metrics.sscd_nn`, tools/find_copies.py; notebooks/sscd.ipynb of the\n * reference: embed a directory, form ALL pairwise similarities on the host, list what lies above a threshold): many unit-row queries\n * against a gallery of N unit rows, keeping per query the best k or the rows at or above a threshold; the nq x N matrix is never formed and\n * no similarity travels to the host.  Exact f32 on v_mfma_f32_16x16x4_f32, one value per pair whatever the entry point, no atomics.",
    'feature_sets.hip': "Pairwise work on feature sets (siss_amd/feature_sets.py, `metrics.fid.sets`; torchmetrics' KernelInceptionDistance,\n * Binkowski et al. 2018, and precision / recall / density / coverage, Kynkaanniemi et al. 2019, Naeem et al. 2020, on the [N, 2048]\n * features the FID's Inception-v3 already produces; NOT the reference's protocol, which reports FID only): squared norms, k-th-neighbour\n * radii, ball membership counts with the nearest row, and the cubic polynomial-kernel sums of all subsets in one launch; no N x M matrix\n * is formed.  Exact f32 on v_mfma_f32_16x16x4_f32 (the tile of sscd_search.hip), one distance per pair whatever the entry point,\n * f64 kernel sums in fixed orders, no atomics.",
    'attribution.hip': "Gradient-feature data attribution (siss_amd/attribution.py, tools/attribute.py; TRAK, Park et al., ICML 2023; D-TRAK, Zheng\n * et al., ICLR 2024; NOT the reference's protocol, which has no attribution step): the dense Rademacher projection of the whole flat\n * gradient buffer (or of listed stretches of it) to k dimensions, the n x k sign matrix defined by a counter hash and never in memory;\n * one f32 partial per chunk and column, chunks folded in f64 in a fixed order, no atomics.",
    'timeemb.hip': "Sinusoidal timestep embedding (diffusers Timesteps/get_timestep_embedding), TimestepEmbedding MLP and\n * ResnetBlock2D.time_emb_proj linears (M = batch rows), forward and backward.",
}
ORDER = ['siss_loss.hip', 'gemm_nt.hip', 'gemm_tn.hip', 'groupnorm.hip', 'conv_small.hip', 'attention.hip', 'attn1h.hip', 'flash_attn.hip', 'transformer.hip',
         'timeemb.hip', 'elementwise.hip', 'optimizer.hip', 'train_state.hip', 'likelihood.hip', 'membership.hip', 'mia.hip', 'metric_conv.hip', 'metric_train.hip', 'inception.hip', 'kmeans.hip', 'sscd.hip', 'clip_iqa.hip', 'prompt_grad.hip', 'injection.hip', 'dpm_solver.hip', 'latent_cache.hip', 'image_store.hip', 'lora.hip', 'saliency.hip', 'ewc.hip', 'surgery.hip', 'teacher.hip', 'ssd.hip', 'uce.hip', 'sscd_search.hip', 'feature_sets.hip', 'attribution.hip', 'f32_path.hip']
HEAD = '''/* siss_hip.h -- C ABI of libsiss_hip.so: the MI355X (gfx950) kernels of the SISS unlearning step.
 *
 * GENERATED by tools/gen_header.py from the .hip sources under siss_amd/csrc -- edit the sources, then regenerate.
 *
 * The reference (claserken/SISS) is pure Python and has no FFI of its own; its hot path reaches
 * device code only through torch / diffusers.  These entry points are what a Python-side binding
 * for that path binds instead (ctypes stub: siss_amd/lib.py; see INTEGRATION.md).  Conventions:
 *   - plain C: raw DEVICE pointers + sizes, no torch types; bf16 tensors are `void*` (uint16 storage);
 *   - every launcher takes the HIP stream as its last argument (`void*` = hipStream_t) and only
 *     enqueues work: no allocation, no synchronisation, safe under hipGraph capture;
 *   - return value: 0 = ok, 1 = bad argument (shape / alignment the kernel does not cover),
 *     2 = launch error;  the *_words functions return buffer sizes and take no stream;
 *   - activations: NHWC bf16 with a one-pixel zero halo, flattened to rows (siss_amd/layout.py);
 *     "sets" = the two cotangent / gradient sets (g_x, g_a) of the dual backward.
 */
#ifndef SISS_HIP_H
#define SISS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One problem of siss_gemm_tn_grouped: the argument list of siss_gemm_tn as a struct (shifts / coffs inline). */
typedef struct siss_tn_job {
    const void* Y; long ldy; const void* X; long ldx; float* dW; long set_stride;
    int N, C, npanels, nsets, rows_per_set, row_begin, row_end, nsplits;
    long x_set_rows;
    const void* zero_page; float* dbias; float* dbias2;
    int shifts[9]; int coffs[9];
    long bias_set_stride;       /* floats between the sets of dbias / dbias2; 0 = set_stride */
} siss_tn_job;

/* The `terms` of siss_rk_combine / siss_rk_norm: sum_j c[j] * row[j] over n <= 8 f64 device rows. */
typedef struct siss_rk_terms {
    const double* row[8]; double c[8]; int n;
} siss_rk_terms;
'''


def generate():
    """(text of include/siss_hip.h, entry point names in header order) from the sources; writes nothing."""
    h = [HEAD]
    names = []
    for f in ORDER:
        s = open(os.path.join(ROOT, 'siss_amd', 'csrc', f)).read()
        # every extern "C" block of the file (gemm_nt.hip has two, around its dispatch helper)
        body = "\n".join(blk.split('}  // extern "C"')[0] for blk in s.split('extern "C" {')[1:])
        h.append('/* ---- %s ----\n * %s\n */' % (f, DOCS[f]))
        for m in re.finditer(r'\n((?://[^\n]*\n)*)(int|long) (siss_\w+)\(([^)]*)\)\s*\{', body):
            comment, ret, name, args = m.groups()
            names.append(name)
            args = ' '.join(args.split()) or 'void'
            if comment.strip():
                c = ' '.join(l.strip().lstrip('/').strip() for l in comment.strip().split('\n'))
                h.append('\n   '.join(textwrap.wrap('/* %s */' % c, 110)))
            h.append('\n    '.join(textwrap.wrap(f'{ret} {name}({args});', 110)))
        h.append('')
    h.append('#ifdef __cplusplus\n}\n#endif\n#endif /* SISS_HIP_H */\n')
    return '\n'.join(h), names


def export_sentence(names):
    """The export count DESIGN.md quotes between its <!--exports--> markers: written from the header's names, not by hand."""
    nf32 = sum(n.endswith('_f32') for n in names)
    return f"{len(names)} `extern \"C\"` entry points ({len(names) - nf32} of the bf16 product path and its helpers + {nf32} `_f32` forms for the f32 parity mode)"


def main():
    header, names = generate()
    open(os.path.join(ROOT, 'include', 'siss_hip.h'), 'w').write(header)
    text = export_sentence(names)
    dp = os.path.join(ROOT, 'DESIGN.md')
    d = open(dp).read()
    d2 = re.sub(r'<!--exports-->.*?<!--/exports-->', '<!--exports-->' + text + '<!--/exports-->', d, flags=re.S)
    if d2 != d:
        open(dp, 'w').write(d2)
    print(f"include/siss_hip.h: {len(names)} entry points ({sum(n.endswith('_f32') for n in names)} _f32)")


if __name__ == '__main__':
    main()

// Fisher-weighted anchor of the unlearning update (elastic weight consolidation; siss_amd/ewc.py, `deletion.ewc`; no counterpart in the
// reference, whose runs have no penalty term):
//   siss_fisher_accumulate     F += (g * g) * w: one micro-batch's squared keep gradient into the running empirical Fisher
//   siss_grad_norms_scale_ewc  pass 1 of optimizer.hip with the penalty's gradient strength * F * (p - pstar) folded into g_x first and
//                              written back over it, plus the penalty and the norm of its gradient into two spare slots of the block
// Grid, thread -> granule map, summation order of the three norm sums, the scalar block and scalars_kernel are opt_step.h's: pass 1
// here IS siss_grad_norms_scale on the folded g_x, and pass 2 stays siss_recombine_clip_adamw.  Every f32 operation is an explicit
// round-to-nearest one (no contraction), every fold has a fixed order, no atomics: bitwise repeatable.
#include "opt_step.h"

namespace {

constexpr int kEwcPenaltySlot = 12, kEwcGradNormSlot = 13;      // pad3[0], pad3[1] of StepScalars: scalars_kernel never writes them

__global__ __launch_bounds__(kThreads) void fisher_accumulate_kernel(const float* __restrict__ g, float* __restrict__ F, long n, float w) {
    const long nvec = n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads) {
        const f32x4_t x = reinterpret_cast<const f32x4_t*>(g)[k];
        f32x4_t f = reinterpret_cast<f32x4_t*>(F)[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = __fadd_rn(f[j], __fmul_rn(__fmul_rn(x[j], x[j]), w));
        reinterpret_cast<f32x4_t*>(F)[k] = f;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) F[i] = __fadd_rn(F[i], __fmul_rn(__fmul_rn(g[i], g[i]), w));
}

// one element of the fold: the penalty gradient t = (strength * F) * (p - pstar) and g_x' = g_x + t; the two f64 sums of the log
__device__ __forceinline__ float ewc_fold(float x, float pp, float ps, float f, float strength, double& sfd, double& stt) {
    const float d = __fsub_rn(pp, ps);
    const float t = __fmul_rn(__fmul_rn(strength, f), d);
    sfd += (double)f * (double)d * (double)d;
    stt += (double)t * (double)t;
    return __fadd_rn(x, t);
}

// pass 1 with the fold: 20 B read + 4 B written per element (g_x, g_a, p, pstar, F; g_x' back over g_x -- each thread reads its own
// granule before it writes it, nobody else touches it).  Row b of `partials` / `ewc_partials`: block b's three norm sums / two
// penalty sums.
__global__ __launch_bounds__(kThreads) void norms_ewc_kernel(float* __restrict__ gx, const float* __restrict__ ga,
                                                             const float* __restrict__ p, const float* __restrict__ pstar,
                                                             const float* __restrict__ F, long n, float strength,
                                                             double* __restrict__ partials, double* __restrict__ ewc_partials) {
    __shared__ double she[2 * kThreads / 64];
    double sxx = 0, saa = 0, sxa = 0, sfd = 0, stt = 0;
    const long nvec = n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads) {
        f32x4_t x = reinterpret_cast<const f32x4_t*>(gx)[k];
        const f32x4_t a = reinterpret_cast<const f32x4_t*>(ga)[k];
        const f32x4_t pp = reinterpret_cast<const f32x4_t*>(p)[k], ps = reinterpret_cast<const f32x4_t*>(pstar)[k],
                      f = reinterpret_cast<const f32x4_t*>(F)[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ewc_fold(x[j], pp[j], ps[j], f[j], strength, sfd, stt);
        reinterpret_cast<f32x4_t*>(gx)[k] = x;
        norm_granule(x, a, sxx, saa, sxa);
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) {
            const float x = ewc_fold(gx[i], p[i], pstar[i], F[i], strength, sfd, stt);
            gx[i] = x;
            norm_tail(x, ga[i], sxx, saa, sxa);
        }
    // the two penalty sums: lanes -> waves -> one row per block, fixed order (the three norm sums: norm_block_fold, after it)
    sfd = wave_sum_d(sfd); stt = wave_sum_d(stt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { she[2 * w] = sfd; she[2 * w + 1] = stt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, b = 0;
        for (int i = 0; i < kThreads / 64; ++i) { a += she[2 * i]; b += she[2 * i + 1]; }
        ewc_partials[2 * blockIdx.x] = a; ewc_partials[2 * blockIdx.x + 1] = b;
    }
    norm_block_fold(sxx, saa, sxa, partials);
}

// ONE block folds the per-block penalty rows (fixed lane -> index map, as scalars_kernel does) and writes the two logged values
__global__ __launch_bounds__(kThreads) void ewc_finish_kernel(const double* __restrict__ ewc_partials, int nblk, float strength,
                                                              float* __restrict__ scalars) {
    __shared__ double shs[2 * kThreads / 64];
    double fd = 0, tt = 0;
    for (int i = threadIdx.x; i < nblk; i += kThreads) { fd += ewc_partials[2 * i]; tt += ewc_partials[2 * i + 1]; }
    fd = wave_sum_d(fd); tt = wave_sum_d(tt);
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; shs[2 * w] = fd; shs[2 * w + 1] = tt; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    fd = tt = 0;
    for (int i = 0; i < kThreads / 64; ++i) { fd += shs[2 * i]; tt += shs[2 * i + 1]; }
    scalars[kEwcPenaltySlot] = (float)(0.5 * (double)strength * fd);
    scalars[kEwcGradNormSlot] = (float)sqrt(tt);
}

}  // namespace

extern "C" {

// Words (doubles) of the caller-owned slab `ewc_partials` of siss_grad_norms_scale_ewc: one row of 2 per block.
long siss_ewc_partials_words(void) { return 2L * kMaxBlocks; }

// F[i] = F[i] + (g[i] * g[i]) * w over n floats: three round-to-nearest f32 operations in that order, no contraction.  g and F
// 16-byte aligned.  One launch per micro-batch of the Fisher estimate (siss_amd/ewc.py FisherAnchor.from_batches, w = 1 / batches).
int siss_fisher_accumulate(const float* g, float* F, long n, float w, void* stream) {
    SISS_CHECK_ARG(g && F && n > 0);
    SISS_CHECK_ARG(((uintptr_t)g | (uintptr_t)F) % 16 == 0);
    fisher_accumulate_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(g, F, n, w);
    SISS_LAUNCH_RET();
}

// siss_grad_norms_scale with the gradient of the anchor penalty (strength / 2) sum_i F_i (p_i - pstar_i)^2 folded into the keep-side
// set first: per element d = p - pstar, t = (strength * F) * d, gx' = gx + t (each one f32 round-to-nearest operation), gx' WRITTEN
// BACK over gx; the three norm sums, the scaling factor (all modes), the clip coefficient and the bias corrections are then those of
// siss_grad_norms_scale on (gx', ga) -- same grid, thread -> granule map, summation order and scalars kernel -- and pass 2 is
// siss_recombine_clip_adamw on the same buffers, unchanged.  ga, p, pstar and F are read only; all five 16-byte aligned.  Besides,
// per-block f64 sums of F d^2 and t^2 go to `ewc_partials` (siss_ewc_partials_words doubles) and a one-block kernel writes
// scalars[12] = (float)(0.5 * strength * sum F d^2) (the penalty) and scalars[13] = (float)sqrt(sum t^2) (the norm of its gradient):
// two slots of the 16-float block that no other kernel writes and that travel with the step's one device-to-host copy.
int siss_grad_norms_scale_ewc(float* gx, const float* ga, const float* p, const float* pstar, const float* F, long n, float strength,
                              int mode, float knob, float max_norm, float beta1, float beta2, double* partials, double* ewc_partials,
                              float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && p && pstar && F && partials && ewc_partials && scalars && n > 0 && mode >= 0 && mode <= 2);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga | (uintptr_t)p | (uintptr_t)pstar | (uintptr_t)F) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    norms_ewc_kernel<<<nblk, kThreads, 0, s>>>(gx, ga, p, pstar, F, n, strength, partials, ewc_partials);
    scalars_kernel<<<1, kThreads, 0, s>>>(partials, nblk, mode, knob, max_norm, beta1, beta2, reinterpret_cast<StepScalars*>(scalars));
    ewc_finish_kernel<<<1, kThreads, 0, s>>>(ewc_partials, nblk, strength, scalars);
    SISS_LAUNCH_RET();
}

}  // extern "C"

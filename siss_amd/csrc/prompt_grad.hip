// Prompt-embedding gradients of the SD UNet and the augmented-prompt optimisation built on them (siss_amd/prompt_aug.py;
// reference: data/src/local_sd_pipeline.py:325-445 get_text_cond_grad, :474-663 aug_prompt).
//
//   ctx_dgrad    : one cross-attention site's text gradient  out[rows][X] = dK[rows][C] W_k + dV[rows][C] W_v  from the site's key /
//                  value cotangents and the [X][C] dgrad copies of to_k / to_v: an NT product on MFMA (bf16 operands, or f32 ones
//                  in the f32 parity mode), f32 accumulation, f32 OUTPUT into the site's own slab (overwritten).
//   ctx_reduce   : the sum of the sites' slabs (and, on request, of the samples) in a fixed order -- the store-then-sum form: no float
//                  atomics anywhere, two runs give the same bits; the running sum never passes through bf16.
//   noise_norm_cot: loss = ||p - u||_2 over ALL elements (f64 sum of squares: per-block partials, fixed-order finish) and its cotangent
//                  (p - u) / loss, zero where the norm is zero (torch's subgradient).  The scalar stays on the device.
//   embed_update : the [L][X] embedding's step: optional distance penalty, row-0 gradient mask, torch.optim.AdamW at its defaults.
//
// The context product is latency-bound (rows = n * Sk: a few hundred, X = 768, K = 2C <= 2560: 240 tiles of 32 x 32 at most per site),
// so it is the simplest MFMA kernel that masks its tails: one wave per 16 x 16 tile, operands straight from global memory (both are
// K-contiguous: 16 B per lane per fragment), no LDS, no split-K.
// Built with -ffp-contract=off (build.py EXACT): the AdamW arithmetic is torch's operation by operation.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------- context dgrad
template <typename T> struct Op;
template <> struct Op<bf16_t> {
    static constexpr int kLane = 8;                      // k per lane per step: one 16-B fragment
    typedef bf16x8_t frag;
    static __device__ __forceinline__ frag zero() { return frag{0, 0, 0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ f32x4_t mma(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Op<float> {
    static constexpr int kLane = 4;
    typedef f32x4_t frag;
    static __device__ __forceinline__ frag zero() { return frag{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ f32x4_t mma(frag a, frag b, f32x4_t c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
};

// out[r][x] = sum_c dk[r][c] wk[x][c] + sum_c dv[r][c] wv[x][c].  Block: 4 waves = a 32 x 32 tile, wave w the 16 x 16 tile
// (w >> 1, w & 1).  Lane (li = lane & 15, q = lane >> 4) supplies row li of both operands at k = k0 + kLane q + [0, kLane) (the same
// bijection of the step's k onto MFMA slots on both sides) and receives rows 4 q + [0, 4) of column li.  A row >= rows, a column >= X
// or a k >= C is never read: the lane reads a valid element instead and holds zeros.
template <typename T>
__global__ __launch_bounds__(kThreads) void ctx_dgrad_kernel(const T* __restrict__ dk, const T* __restrict__ dv, long ldd,
                                                             const T* __restrict__ wk, const T* __restrict__ wv,
                                                             float* __restrict__ out, int rows, int C, int X) {
    typedef typename Op<T>::frag frag;
    constexpr int KL = Op<T>::kLane, KS = 4 * KL;
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    const int li = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.y * 32 + (wv_ >> 1) * 16, x0 = blockIdx.x * 32 + (wv_ & 1) * 16;
    if (r0 >= rows || x0 >= X) return;                   // (wave-uniform)
    const int ar = r0 + li, bx = x0 + li;
    const bool aok = ar < rows, bok = bx < X;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    auto panel = [&](const T* __restrict__ A, const T* __restrict__ W) {
        const T* a = A + (long)(aok ? ar : 0) * ldd;
        const T* b = W + (long)(bok ? bx : 0) * C;
        // four k-steps per trip: eight loads in flight before the first MFMA waits (the product is bound by load latency).  Every
        // load is unconditional and in bounds -- a masked lane reads row 0 / k 0 and drops the value; C is a multiple of kLane, so
        // a fragment is inside or outside, and the steps past C of the last trip contribute zeros
        for (int k0 = 0; k0 < C; k0 += 4 * KS) {
            frag fa[4], fb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j * KS + KL * q;
                const bool kok = k < C;
                const int kk = kok ? k : 0;
                fa[j] = *reinterpret_cast<const frag*>(a + kk);
                fb[j] = *reinterpret_cast<const frag*>(b + kk);
                if (!(aok && kok)) fa[j] = Op<T>::zero();
                if (!(bok && kok)) fb[j] = Op<T>::zero();
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = Op<T>::mma(fa[j], fb[j], acc);
        }
    };
    panel(dk, wk);
    panel(dv, wv);
    if (!bok) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * q + r;
        if (row < rows) out[(long)row * X + bx] = acc[r];
    }
}

// out[n][i] = sum_s slabs[s][n][i], s ascending; with reduce: out[i] = sum_n (that), n ascending.  per = L * X.
__global__ __launch_bounds__(kThreads) void ctx_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, int nsites,
                                                              int N, long per, int reduce) {
    const long total = reduce ? per : (long)N * per;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        if (reduce) {
            float acc = 0.f;
            for (int n = 0; n < N; ++n) {
                float a = 0.f;
                for (int s = 0; s < nsites; ++s) a += slabs[((long)s * N + n) * per + i];
                acc += a;
            }
            out[i] = acc;
        } else {
            float a = 0.f;
            for (int s = 0; s < nsites; ++s) a += slabs[(long)s * N * per + i];
            out[i] = a;
        }
    }
}

// ---------------------------------------------------------------- noise norm and its cotangent
constexpr int kNormMaxBlocks = 256;

inline int norm_blocks(long count) {
    long b = (count + 4 * kThreads - 1) / (4 * kThreads);
    return (int)(b < 1 ? 1 : b > kNormMaxBlocks ? kNormMaxBlocks : b);
}

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) t += sh[i];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(kThreads) void sq_diff_partials_kernel(const float* __restrict__ p, const float* __restrict__ u,
                                                                    long count, double* __restrict__ partials) {
    __shared__ double sh[kThreads / 64];
    double acc = 0.0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long)gridDim.x * kThreads) {
        const double d = (double)p[i] - (double)u[i];
        acc += d * d;
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// every block folds the partials left to right (the same sum in every block), block 0 writes the scalar
__global__ __launch_bounds__(kThreads) void norm_cot_kernel(const float* __restrict__ p, const float* __restrict__ u, long count,
                                                            const double* __restrict__ partials, int nblk, float* __restrict__ cot,
                                                            float* __restrict__ loss) {
    __shared__ double nrm_sh;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < nblk; ++i) s += partials[i];
        nrm_sh = sqrt(s);
        if (blockIdx.x == 0) loss[0] = (float)nrm_sh;
    }
    __syncthreads();
    const double nrm = nrm_sh;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long)gridDim.x * kThreads) {
        const double d = (double)p[i] - (double)u[i];
        cot[i] = nrm > 0.0 ? (float)(d / nrm) : 0.f;
    }
}

// ---------------------------------------------------------------- embedding update
// dist[r] = ||e_r - e0_r||_2 (f64 sum in a fixed order): one block per row
__global__ __launch_bounds__(kThreads) void row_dist_kernel(const float* __restrict__ e, const float* __restrict__ e0, int X,
                                                            double* __restrict__ dist) {
    __shared__ double sh[kThreads / 64];
    const int r = blockIdx.x;
    double acc = 0.0;
    for (int x = threadIdx.x; x < X; x += kThreads) {
        const double d = (double)e[(long)r * X + x] - (double)e0[(long)r * X + x];
        acc += d * d;
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) dist[r] = sqrt(acc);
}

// One block per row.  The penalty applies when use_penalty and mean_{r >= 1} dist[r] > optim_epsilon (decided on the device, the same
// in every block): g = alpha g + (1 - alpha) / (L - 1) (e - e0) / dist[r], the second term 0 where dist[r] = 0.  Row 0: g = 0 -- its
// moments stay where they are and the decoupled decay still multiplies it.  Then torch.optim.AdamW's single-tensor update.
__global__ __launch_bounds__(kThreads) void embed_update_kernel(float* __restrict__ e, const float* __restrict__ e0,
                                                                const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, const double* __restrict__ dist, int L, int X,
                                                                float lr, float beta1, float beta2, float eps, float wd, float bc1,
                                                                float bc2s, float alpha, float optim_epsilon, int use_penalty) {
    __shared__ int apply_sh;
    const int r = blockIdx.x;
    if (threadIdx.x == 0) {
        int apply = 0;
        if (use_penalty && L > 1) {
            double s = 0.0;
            for (int i = 1; i < L; ++i) s += dist[i];
            apply = s / (L - 1) > (double)optim_epsilon;
        }
        apply_sh = apply;
    }
    __syncthreads();
    const bool apply = apply_sh != 0;
    const float step_size = lr / bc1;
    const float decay = 1.f - lr * wd;
    const double dr = apply ? dist[r] : 0.0;
    const double pen = (1.0 - (double)alpha) / (double)(L > 1 ? L - 1 : 1);
    for (int x = threadIdx.x; x < X; x += kThreads) {
        const long i = (long)r * X + x;
        float pp = e[i], mm = m[i], vv = v[i];
        float gg = 0.f;
        if (r > 0) {
            gg = g[i];
            if (apply) {                                 // (formed in f64, rounded once: the gradient AdamW is handed)
                double gd = (double)alpha * (double)gg;
                if (dr > 0.0) gd += pen * (((double)pp - (double)e0[i]) / dr);
                gg = (float)gd;
            }
        }
        pp = __fmul_rn(pp, decay);
        mm = __fadd_rn(mm, __fmul_rn(__fsub_rn(gg, mm), 1.f - beta1));           // lerp
        vv = __fadd_rn(__fmul_rn(vv, beta2), __fmul_rn(__fmul_rn(gg, gg), 1.f - beta2));
        const float den = __fadd_rn(sqrtf(vv) / bc2s, eps);
        pp = __fsub_rn(pp, __fmul_rn(step_size, mm / den));
        e[i] = pp; m[i] = mm; v[i] = vv;
    }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" {

// One cross-attention site's text gradient: out[rows][X] (f32, OVERWRITTEN) = dk[rows][C] wk^T + dv[rows][C] wv^T.  dk, dv: the key /
// value cotangents, rows ldd elements apart (the two column halves of a fused [rows][2C] tensor: dv = dk + C, ldd = 2C -- or wider:
// columns past C are never read); wk, wv: the [X][C] dgrad copies of to_k / to_v.  f32_operands 0: bf16 operands (C % 8 == 0,
// ldd % 8 == 0), 1: f32 operands (C % 4 == 0, ldd % 4 == 0); all operand pointers 16-B aligned.  Row and column tails are masked.
int siss_ctx_dgrad(const void* dk, const void* dv, long ldd, const void* wk, const void* wv, float* out, int rows, int C, int X,
                   int f32_operands, void* stream) {
    SISS_CHECK_ARG(dk && dv && wk && wv && out && rows > 0 && C > 0 && X > 0 && ldd >= C);
    SISS_CHECK_ARG(f32_operands == 0 || f32_operands == 1);
    const int lane = f32_operands ? 4 : 8;
    SISS_CHECK_ARG(C % lane == 0 && ldd % lane == 0);
    SISS_CHECK_ARG(aligned16(dk) && aligned16(dv) && aligned16(wk) && aligned16(wv));
    dim3 grid(cdiv(X, 32), cdiv(rows, 32));
    SISS_CHECK_ARG(grid.y <= 65535);
    hipStream_t s = (hipStream_t)stream;
    if (f32_operands)
        ctx_dgrad_kernel<float><<<grid, kThreads, 0, s>>>((const float*)dk, (const float*)dv, ldd, (const float*)wk, (const float*)wv,
                                                          out, rows, C, X);
    else
        ctx_dgrad_kernel<bf16_t><<<grid, kThreads, 0, s>>>((const bf16_t*)dk, (const bf16_t*)dv, ldd, (const bf16_t*)wk,
                                                           (const bf16_t*)wv, out, rows, C, X);
    SISS_LAUNCH_RET();
}

// The finish of the store-then-sum reduction: slabs [nsites][N][per] f32 (per = L * X) -> out [N][per] = the sum over the sites in
// ascending order; reduce = 1: out [per] = the sum over the samples (ascending) of those sums.  No atomics: bitwise reproducible.
int siss_ctx_reduce(const float* slabs, float* out, int nsites, int N, long per, int reduce, void* stream) {
    SISS_CHECK_ARG(slabs && out && nsites > 0 && N > 0 && per > 0 && (reduce == 0 || reduce == 1));
    const long total = reduce ? per : (long)N * per;
    long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 2048) blocks = 2048;
    ctx_reduce_kernel<<<(int)blocks, kThreads, 0, (hipStream_t)stream>>>(slabs, out, nsites, N, per, reduce);
    SISS_LAUNCH_RET();
}

// Number of f64 words siss_noise_norm_cot needs in `partials` for n rows of chw elements.
long siss_noise_norm_partials_words(int n, long chw) { return norm_blocks((long)n * chw); }

// loss[0] = ||p - u||_2 over all n * chw elements (f32; differences and their squares in f64, per-block partial sums folded left to
// right) and cot = (p - u) / that norm -- all zeros when the norm is zero.  p, u, cot: [n][chw] f32 (chw need not be a multiple of 4);
// partials: f64 scratch of siss_noise_norm_partials_words(n, chw) words.
int siss_noise_norm_cot(const float* p, const float* u, int n, long chw, float* cot, float* loss, double* partials, void* stream) {
    SISS_CHECK_ARG(p && u && cot && loss && partials && n > 0 && chw > 0);
    const long count = (long)n * chw;
    const int nblk = norm_blocks(count);
    hipStream_t s = (hipStream_t)stream;
    sq_diff_partials_kernel<<<nblk, kThreads, 0, s>>>(p, u, count, partials);
    norm_cot_kernel<<<nblk, kThreads, 0, s>>>(p, u, count, partials, nblk, cot, loss);
    SISS_LAUNCH_RET();
}

// One step of the augmented-prompt optimisation on the embedding e [L][X] f32 (torch.optim.AdamW at betas / eps / weight decay as
// given, moments m, v; bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) formed in f64 by the caller).  g: d(noise norm) / de.
// dist: f64 [L] scratch, left holding ||e_r - e0_r||_2 of the embedding BEFORE the step.  use_penalty = 1: when the mean of dist over
// rows 1.. exceeds optim_epsilon, row r >= 1 takes alpha g + (1 - alpha) / (L - 1) (e_r - e0_r) / dist[r] (the second term 0 where
// dist[r] = 0) instead of g.  Row 0's gradient is zero: it receives the decoupled weight decay only.  e0 may be null without penalty.
int siss_prompt_embed_update(float* e, const float* e0, const float* g, float* m, float* v, double* dist, int L, int X, float lr,
                             float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt, float alpha,
                             float optim_epsilon, int use_penalty, void* stream) {
    SISS_CHECK_ARG(e && g && m && v && dist && L > 0 && X > 0);
    SISS_CHECK_ARG(use_penalty == 0 || (use_penalty == 1 && e0));
    SISS_CHECK_ARG(bc1 > 0.f && bc2_sqrt > 0.f);
    hipStream_t s = (hipStream_t)stream;
    if (use_penalty) row_dist_kernel<<<L, kThreads, 0, s>>>(e, e0, X, dist);
    embed_update_kernel<<<L, kThreads, 0, s>>>(e, e0, g, m, v, dist, L, X, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, alpha,
                                               optim_epsilon, use_penalty);
    SISS_LAUNCH_RET();
}

}  // extern "C"

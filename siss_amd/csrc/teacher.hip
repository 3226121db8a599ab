// Opt-in teacher-target unlearning (siss_amd/teacher.py, `deletion.loss_fn=teacher_target` + `deletion.teacher`; ESD, Gandikota et al.,
// ICCV 2023; Concept Ablation, Kumari et al., ICCV 2023; no counterpart in the reference, whose objectives regress onto the drawn noise):
//   siss_teacher_seed         the regression target from the frozen teacher's outputs, the cotangent of the student's stacked rows and
//                             the per-row squared-error sums, one streaming launch + a one-thread-per-row fold
//   siss_grad_norms_weighted  pass 1 of optimizer.hip with the scaling factor fixed at s = -weight (g = g_x + weight g_a: a plain
//                             weighted sum, descent on both sets); pass 2 stays siss_recombine_clip_adamw
// Every f32 operation is an explicit round-to-nearest one (no contraction), every fold has a fixed order that does not depend on the
// grid, no atomics: bitwise repeatable.  Grid, thread -> granule map, summation order of the three norm sums and the scalar block of
// pass 1 are opt_step.h's.
#include "opt_step.h"

namespace {

constexpr int kSeedIters = 4;                               // granules per thread and chunk
constexpr long kSeedChunk = 4L * kThreads * kSeedIters;     // floats of a row one block sums at a time (4096)
constexpr int kSeedMaxBlocksX = 64;                         // blocks per row: a block walks its chunks c, c + gridDim.x, ...
constexpr int kSeedMaxRows = 65535;                         // gridDim.y

enum { KEEP_NOISE = 0, KEEP_TEACHER = 1, KEEP_NONE = 2 };
enum { FORGET_ESD = 0, FORGET_ANCHOR = 1 };

inline long seed_chunks(long chw) { return (chw + kSeedChunk - 1) / kSeedChunk; }

template <bool BF16>
__device__ __forceinline__ float noise_at(const void* p, long i) {
    if constexpr (BF16) return bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
    else return reinterpret_cast<const float*>(p)[i];
}
template <bool BF16>
__device__ __forceinline__ f32x4_t noise_at4(const void* p, long i) {        // i: a multiple of 4 of a 16-byte aligned row
    if constexpr (BF16) {
        const u32x2_t r = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const bf16_t*>(p) + i);
        return f32x4_t{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xffff0000u),
                       __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xffff0000u)};
    } else {
        return *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(p) + i);
    }
}

// y = u - eta (k - u): three roundings, in this order
__device__ __forceinline__ float esd_target(float k, float u, float eta) { return __fsub_rn(u, __fmul_rn(eta, __fsub_rn(k, u))); }

// Row r of the student's rows [keep B | forget B] ([forget B] with KEEP_NONE).  Its target reads: the noise row i (keep-noise), the
// teacher row i (keep-teacher), or the teacher's rows koff + i (k) and koff + B + i (u, esd only) with koff = B under keep-teacher.
// A row is cut into chunks of kSeedChunk floats; chunk c of row r is summed by ONE block with a fixed thread -> element map (thread t
// owns granules t, t + 256, ... of the chunk, elements in ascending order) into partials[r * nchunks + c]: the sums do not depend on
// the grid.  VEC: every row starts 16-byte aligned (chw % 4 == 0): 16-byte loads and stores; else the same map element by element.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kThreads) void teacher_seed_kernel(const float* __restrict__ pred, const void* __restrict__ noise,
                                                                const float* __restrict__ teach, int B, long chw, int keep, int forget,
                                                                float eta, float two_scale, float* __restrict__ cot,
                                                                double* __restrict__ partials) {
    __shared__ double sh[kThreads / 64];
    const int r = blockIdx.y;
    const bool keep_row = keep != KEEP_NONE && r < B;
    const int i = keep_row ? r : r - (keep != KEEP_NONE ? B : 0);
    const int koff = keep == KEEP_TEACHER ? B : 0;
    const int src = keep_row ? (keep == KEEP_TEACHER ? 1 : 0) : (forget == FORGET_ESD ? 2 : 1);     // 0 noise, 1 teacher row, 2 esd pair
    const float* p = pred + (long)r * chw;
    float* c_out = cot + (long)r * chw;
    const float* k = teach + (long)(keep_row ? i : koff + i) * chw;        // (read when src != 0)
    const float* u = teach + (long)(koff + B + i) * chw;                   // (read when src == 2)
    const long nrow = (long)i * chw;                                       // (noise: read when src == 0)
    const long nchunks = (chw + kSeedChunk - 1) / kSeedChunk;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double s = 0;
#pragma unroll
        for (int it = 0; it < kSeedIters; ++it) {
            const long e = c * kSeedChunk + 4L * (it * kThreads + threadIdx.x);
            if (e >= chw) continue;
            if constexpr (VEC) {
                const f32x4_t pv = *reinterpret_cast<const f32x4_t*>(p + e);
                f32x4_t y, o;
                if (src == 0) y = noise_at4<BF16>(noise, nrow + e);
                else y = *reinterpret_cast<const f32x4_t*>(k + e);
                if (src == 2) {
                    const f32x4_t uv = *reinterpret_cast<const f32x4_t*>(u + e);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[j] = esd_target(y[j], uv[j], eta);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = __fsub_rn(pv[j], y[j]);
                    o[j] = __fmul_rn(two_scale, d);
                    s += (double)d * (double)d;
                }
                *reinterpret_cast<f32x4_t*>(c_out + e) = o;
            } else {
                for (int j = 0; j < 4 && e + j < chw; ++j) {
                    float y;
                    if (src == 0) y = noise_at<BF16>(noise, nrow + e + j);
                    else y = k[e + j];
                    if (src == 2) y = esd_target(y, u[e + j], eta);
                    const float d = __fsub_rn(p[e + j], y);
                    c_out[e + j] = __fmul_rn(two_scale, d);
                    s += (double)d * (double)d;
                }
            }
        }
        // lanes -> waves -> the chunk's one double, fixed order
        s = wave_sum_d(s);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0;
            for (int w = 0; w < kThreads / 64; ++w) a += sh[w];
            partials[(long)r * nchunks + c] = a;
        }
        __syncthreads();                                                    // (sh is reused by the block's next chunk)
    }
}

// one thread per row: its chunks in ascending order, ONE rounding to f32
__global__ void teacher_fold_kernel(const double* __restrict__ partials, long nchunks, int R, float* __restrict__ sums) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double s = 0;
    for (long c = 0; c < nchunks; ++c) s += partials[(long)r * nchunks + c];
    sums[r] = (float)s;
}

__global__ __launch_bounds__(kThreads) void weighted_norms_kernel(const float* __restrict__ gx, const float* __restrict__ ga, long n,
                                                                  double* __restrict__ partials) {
    double sxx = 0, saa = 0, sxa = 0;
    const long nvec = n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads)
        norm_granule(reinterpret_cast<const f32x4_t*>(gx)[k], reinterpret_cast<const f32x4_t*>(ga)[k], sxx, saa, sxa);
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) norm_tail(gx[i], ga[i], sxx, saa, sxa);
    norm_block_fold(sxx, saa, sxa, partials);
}

// scalars_kernel of opt_step.h with the scaling factor GIVEN: s = -weight (no norm fix, no inf guard, no EraseDiff rule), the same
// fold of the per-block rows, the same pre-clip norm from the f64 sums, the same clip coefficient, step count and bias corrections.
__global__ void weighted_scalars_kernel(const double* __restrict__ partials, int nblk, float weight, float max_norm, float beta1,
                                        float beta2, StepScalars* __restrict__ sc) {
    __shared__ double shs[3 * kThreads / 64];
    double xx = 0, aa = 0, xa = 0;
    for (int i = threadIdx.x; i < nblk; i += kThreads) { xx += partials[3 * i]; aa += partials[3 * i + 1]; xa += partials[3 * i + 2]; }
    xx = wave_sum_d(xx); aa = wave_sum_d(aa); xa = wave_sum_d(xa);
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; shs[3 * w] = xx; shs[3 * w + 1] = aa; shs[3 * w + 2] = xa; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    xx = aa = xa = 0;
    for (int i = 0; i < kThreads / 64; ++i) { xx += shs[3 * i]; aa += shs[3 * i + 1]; xa += shs[3 * i + 2]; }
    const double s = -(double)weight;
    double g2 = xx - 2 * s * xa + s * s * aa;
    if (g2 < 0) g2 = 0;
    const double gn = sqrt(g2);
    double coef = (double)max_norm / (gn + 1e-6);
    if (coef > 1) coef = 1;
    const float step = sc->step + 1.f;
    sc->norm_x = (float)sqrt(xx); sc->norm_a = (float)sqrt(aa); sc->dot = (float)xa; sc->scale = (float)s;
    sc->pre_clip_norm = (float)gn; sc->clip_coef = (float)coef; sc->step = step;
    sc->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    sc->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

}  // namespace

extern "C" {

// Words (doubles) of the caller-owned slab `partials` of siss_teacher_seed for R student rows of chw floats: one per row and chunk.
long siss_teacher_partials_words(int R, long chw) { return R > 0 && chw > 0 ? (long)R * seed_chunks(chw) : 0; }

// Cotangent and loss sums of the teacher-target objective over the student's stacked rows.  pred [R, chw] f32: the student's output,
// R = 2 B rows [keep B | forget B], or B rows [forget B] with keep_mode 2.  teach [teach_rows, chw] f32: the frozen teacher's output
// on its rows [keep B (keep_mode 1 only) | forget under c or c_anchor B | forget under the empty prompt B (forget_mode 0 only)];
// teach_rows must be at least that many.  noise [B, chw], f32 or bf16 (noise_bf16): read with keep_mode 0 only (may be NULL otherwise).
// keep_mode: 0 the drawn noise, 1 the teacher's prediction, 2 no keep rows.  forget_mode: 0 esd, y = u - eta (k - u) with k the
// teacher under c and u under the empty prompt; 1 anchor, y = k.  Per element, each an f32 round-to-nearest operation, no contraction:
// d = pred - y, cot = two_scale * d with two_scale = 2 * scale formed once here in f32.  sums[r] = (float) sum_e d^2 of row r, the
// squares and the sum in f64: a row is cut into chunks of 4096 floats, each summed by one block in a fixed order into `partials`
// (siss_teacher_partials_words doubles), the chunks folded in ascending order -- the same bits whatever the grid, no atomics.  Rows
// of chw % 4 == 0 floats move as 16-byte vectors (bf16 noise as 8-byte ones); any chw >= 1 is accepted.  pred, teach, noise and cot
// 16-byte aligned.  A bad argument returns 1 and nothing is written.
int siss_teacher_seed(const float* pred, const void* noise, int noise_bf16, const float* teach, int teach_rows, int B, long chw,
                      int keep_mode, int forget_mode, float eta, float scale, float* cot, float* sums, double* partials,
                      void* stream) {
    SISS_CHECK_ARG(pred && teach && cot && sums && partials && B > 0 && chw > 0);
    SISS_CHECK_ARG(keep_mode >= KEEP_NOISE && keep_mode <= KEEP_NONE && forget_mode >= FORGET_ESD && forget_mode <= FORGET_ANCHOR);
    SISS_CHECK_ARG(noise || keep_mode != KEEP_NOISE);
    SISS_CHECK_ARG(B <= kSeedMaxRows / 2);
    const int R = keep_mode == KEEP_NONE ? B : 2 * B;
    const int need = (keep_mode == KEEP_TEACHER ? B : 0) + B + (forget_mode == FORGET_ESD ? B : 0);
    SISS_CHECK_ARG(teach_rows >= need);
    SISS_CHECK_ARG(((uintptr_t)pred | (uintptr_t)teach | (uintptr_t)cot | (uintptr_t)noise) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const float two_scale = 2.f * scale;
    const long nchunks = seed_chunks(chw);
    dim3 grid((unsigned)(nchunks < kSeedMaxBlocksX ? nchunks : kSeedMaxBlocksX), R);
    const bool vec = chw % 4 == 0;
#define SISS_TEACHER_SEED(BF, V) \
    teacher_seed_kernel<BF, V><<<grid, kThreads, 0, s>>>(pred, noise, teach, B, chw, keep_mode, forget_mode, eta, two_scale, cot, partials)
    if (noise_bf16) { if (vec) SISS_TEACHER_SEED(true, true); else SISS_TEACHER_SEED(true, false); }
    else { if (vec) SISS_TEACHER_SEED(false, true); else SISS_TEACHER_SEED(false, false); }
#undef SISS_TEACHER_SEED
    teacher_fold_kernel<<<cdiv(R, 64), 64, 0, s>>>(partials, nchunks, R, sums);
    SISS_LAUNCH_RET();
}

// siss_grad_norms_scale with the scaling factor fixed at s = -weight, for g = g_x + weight g_a (weight > 0): the same grid, thread ->
// granule map and summation order of |g_x|^2, |g_a|^2, <g_x, g_a> into the same slab (siss_opt_partials_words), and the same scalar
// block (siss_opt_scalars_words): |g_x|, |g_a|, <g_x, g_a>, s, the pre-clip norm of g_x - s g_a from the f64 sums, the clip
// coefficient, the step count and the two bias corrections.  Pass 2 is siss_recombine_clip_adamw on the same buffers, unchanged.
int siss_grad_norms_weighted(const float* gx, const float* ga, long n, float weight, float max_norm, float beta1, float beta2,
                             double* partials, float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && partials && scalars && n > 0 && weight > 0.f && weight <= 3.0e38f);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    weighted_norms_kernel<<<nblk, kThreads, 0, s>>>(gx, ga, n, partials);
    weighted_scalars_kernel<<<1, kThreads, 0, s>>>(partials, nblk, weight, max_norm, beta1, beta2, reinterpret_cast<StepScalars*>(scalars));
    SISS_LAUNCH_RET();
}

}  // extern "C"

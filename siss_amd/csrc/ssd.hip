// Selective Synaptic Dampening (SSD, Foster, Schoepf & Brintrup, AAAI 2024; siss_amd/ssd.py, `deletion.ssd`; no counterpart in the
// reference, whose runs unlearn by gradient steps only):
//   siss_ssd_ratio    r = F_forget / F_keep per float of the flat buffer, 0 where F_forget is 0 (0/0 -> 0, x/0 -> +inf, never a NaN)
//   siss_ssd_dampen   one streaming pass: select (r > threshold, or r >= threshold), p <- p * min(lambda / r, 1) on the selected,
//                     and eight f64 statistics of what that did (or, apply = 0, of what it would do)
// The threshold of the fraction mode is siss_absf_select (saliency.hip) on r.  Grid, block size and wave sums are opt_step.h's.  Every
// f32 operation is an explicit round-to-nearest one (no contraction), every fold has a fixed order, no atomics: bitwise repeatable.
#include "opt_step.h"

namespace {

constexpr int kSsdStats = 8;             // one row per block, and the result block: 8 doubles
enum { SSD_SELECTED = 0, SSD_DAMPENED, SSD_ZEROED, SSD_SUM_BETA, SSD_SUM_DELTA2, SSD_SUM_P2_SELECTED, SSD_SUM_P2, SSD_SPARE };

// one launch of the dampening pass (the flat C arguments of siss_ssd_dampen, gathered once)
struct SsdDampenCall {
    float* p;
    const float* ratio;
    long n;
    float threshold, lambda;
    int strict, apply;
};

__device__ __forceinline__ float ssd_ratio(float fk, float ff) { return ff == 0.f ? 0.f : __fdiv_rn(ff, fk); }

__global__ __launch_bounds__(kThreads) void ssd_ratio_kernel(const float* __restrict__ fk, const float* __restrict__ ff,
                                                             float* __restrict__ r, long n) {
    const long nvec = n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads) {
        const f32x4_t a = reinterpret_cast<const f32x4_t*>(fk)[k], b = reinterpret_cast<const f32x4_t*>(ff)[k];
        f32x4_t q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = ssd_ratio(a[j], b[j]);
        reinterpret_cast<f32x4_t*>(r)[k] = q;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) r[i] = ssd_ratio(fk[i], ff[i]);
}

// one element: whether it is selected, its new value, and its terms of the seven sums (counts are integers carried in f64: exact)
__device__ __forceinline__ bool ssd_element(const SsdDampenCall& c, float r, float& pp, double* s) {
    const double p2 = (double)pp * (double)pp;
    s[SSD_SUM_P2] += p2;
    if (!(c.strict ? r > c.threshold : r >= c.threshold)) return false;
    const float beta = r > c.lambda ? __fdiv_rn(c.lambda, r) : 1.f;        // min(lambda / r, 1); r = +inf: 0
    const float q = __fmul_rn(pp, beta);
    const double d = (double)q - (double)pp;
    s[SSD_SELECTED] += 1.0;
    s[SSD_DAMPENED] += beta < 1.f ? 1.0 : 0.0;
    s[SSD_ZEROED] += beta == 0.f ? 1.0 : 0.0;
    s[SSD_SUM_BETA] += (double)beta;
    s[SSD_SUM_DELTA2] += d * d;
    s[SSD_SUM_P2_SELECTED] += p2;
    pp = q;
    return true;
}

// 8 B read per float (p, r); a granule is written back (apply) only when one of its four floats is selected: at most 4 B per float.
// Row b of `partials`: block b's sums.
__global__ __launch_bounds__(kThreads) void ssd_dampen_kernel(const SsdDampenCall c, double* __restrict__ partials) {
    __shared__ double sh[kSsdStats * kThreads / 64];
    double s[kSsdStats] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long nvec = c.n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads) {
        f32x4_t pp = reinterpret_cast<const f32x4_t*>(c.p)[k];
        const f32x4_t r = reinterpret_cast<const f32x4_t*>(c.ratio)[k];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) { float v = pp[j]; any |= ssd_element(c, r[j], v, s); pp[j] = v; }
        if (any && c.apply) reinterpret_cast<f32x4_t*>(c.p)[k] = pp;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < c.n; i += kThreads) {
            float v = c.p[i];
            if (ssd_element(c, c.ratio[i], v, s) && c.apply) c.p[i] = v;
        }
    // lanes -> waves -> one row per block, fixed order
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kSsdStats; ++j) {
        const double t = wave_sum_d(s[j]);
        if ((threadIdx.x & 63) == 0) sh[kSsdStats * w + j] = t;
    }
    __syncthreads();
    if (threadIdx.x < kSsdStats) {
        double a = 0;
        for (int i = 0; i < kThreads / 64; ++i) a += sh[kSsdStats * i + threadIdx.x];
        partials[(long)kSsdStats * blockIdx.x + threadIdx.x] = a;
    }
}

// ONE block folds the per-block rows (fixed lane -> index map, as scalars_kernel does) and writes the eight statistics
__global__ __launch_bounds__(kThreads) void ssd_finish_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ stats) {
    __shared__ double sh[kSsdStats * kThreads / 64];
    double s[kSsdStats] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblk; i += kThreads) {
#pragma unroll
        for (int j = 0; j < kSsdStats; ++j) s[j] += partials[(long)kSsdStats * i + j];
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kSsdStats; ++j) {
        const double t = wave_sum_d(s[j]);
        if ((threadIdx.x & 63) == 0) sh[kSsdStats * w + j] = t;
    }
    __syncthreads();
    if (threadIdx.x >= kSsdStats) return;
    double a = 0;
    for (int i = 0; i < kThreads / 64; ++i) a += sh[kSsdStats * i + threadIdx.x];
    stats[threadIdx.x] = threadIdx.x == SSD_SPARE ? 0.0 : a;
}

inline bool ssd_overlap(const float* a, const float* b, long n) { return a < b + n && b < a + n; }

}  // namespace

extern "C" {

// Words (doubles) of the caller-owned slab `partials` of siss_ssd_dampen: one row of 8 per block.
long siss_ssd_partials_words(void) { return (long)kSsdStats * kMaxBlocks; }

// ratio[i] = f_forget[i] == 0 ? 0 : f_forget[i] / f_keep[i] over n floats: one f32 round-to-nearest division, so that 0/0 gives 0,
// x/0 gives +inf and a NaN never arises from importances >= 0.  All three pointers 16-byte aligned; `ratio` may overlap neither input.
int siss_ssd_ratio(const float* f_keep, const float* f_forget, float* ratio, long n, void* stream) {
    SISS_CHECK_ARG(f_keep && f_forget && ratio && n > 0);
    SISS_CHECK_ARG(((uintptr_t)f_keep | (uintptr_t)f_forget | (uintptr_t)ratio) % 16 == 0);
    SISS_CHECK_ARG(!ssd_overlap(ratio, f_keep, n) && !ssd_overlap(ratio, f_forget, n));
    ssd_ratio_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(f_keep, f_forget, ratio, n);
    SISS_LAUNCH_RET();
}

// The dampening pass over n floats: element i is selected iff (strict ? ratio[i] > threshold : ratio[i] >= threshold); a selected
// p[i] becomes p[i] * beta with beta = ratio[i] > lambda ? lambda / ratio[i] : 1 (one f32 division and one f32 multiplication, round
// to nearest, no contraction; ratio = +inf gives beta = 0); an unselected float keeps its bits.  apply = 0: nothing is written to p
// (a dry run with the same statistics).  p and ratio 16-byte aligned; `partials`: siss_ssd_partials_words doubles of scratch.
// `stats` (DEVICE, 8 doubles, all written): [0] selected, [1] selected with beta < 1, [2] selected with beta == 0, [3] the sum of
// beta over the selected, [4] the sum of (p' - p)^2, [5] the sum of p^2 over the selected (before), [6] the sum of p^2 over all n
// (before), [7] 0 -- counts exact, squares formed in f64 from the f32 values, per-block rows folded by one block in a fixed order.
// Refused: lambda not finite or <= 0, threshold NaN or negative (+inf is legal: with strict it selects nothing).
int siss_ssd_dampen(float* p, const float* ratio, long n, float threshold, int strict, float lambda, int apply, double* partials,
                    double* stats, void* stream) {
    SISS_CHECK_ARG(p && ratio && partials && stats && n > 0);
    SISS_CHECK_ARG(((uintptr_t)p | (uintptr_t)ratio) % 16 == 0 && ((uintptr_t)partials | (uintptr_t)stats) % 8 == 0);
    SISS_CHECK_ARG(lambda > 0.f && lambda <= 3.402823466e38f && threshold >= 0.f);      // (a NaN fails every comparison)
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    const SsdDampenCall call{p, ratio, n, threshold, lambda, strict != 0, apply != 0};
    ssd_dampen_kernel<<<nblk, kThreads, 0, s>>>(call, partials);
    ssd_finish_kernel<<<1, kThreads, 0, s>>>(partials, nblk, stats);
    SISS_LAUNCH_RET();
}

}  // extern "C"

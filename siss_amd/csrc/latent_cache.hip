// The latent cache's sampling launch (siss_amd/latent_cache.py LatentCache.latents): the frozen VAE encoder's posterior moments of a
// whole dataset stay resident on the device, and a micro-batch of latents is ONE gather-and-sample launch over the rows its indices
// name -- instead of the encoder's forward per micro-batch (delete_sd.py:879-888 of the reference: vae.encode(x).latent_dist.sample()
// * vae.config.scaling_factor; the moments of an image never change, only the normals of sample() do).
//
//   r = idx[i]
//   out[i] = (mean[r] + exp(0.5 * clamp(logvar[r], -30, 20)) * eps[i]) * scaling          (latent_sample.h posterior_sample)
//
// HBM-bound streaming kernel like latent_inject_kernel (csrc/injection.hip): 16 B per lane per f32 access, a grid-stride loop, no
// reduction, no atomics.  Built with -ffp-contract=off (build.py EXACT).  An index outside [0, rows) is never dereferenced: that
// sample's output row is NaN.
#include "common.h"
#include "latent_sample.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ void store4(float* p, long q, f32x4_t v) { reinterpret_cast<f32x4_t*>(p)[q] = v; }
__device__ __forceinline__ void store4(bf16_t* p, long q, f32x4_t v) {               // RNE, NaN stays NaN (common.h pack_bf2)
    reinterpret_cast<u32x2_t*>(p)[q] = u32x2_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
}

// grid (blocks per sample, n).  VEC: chw % 4 == 0 and cache, eps and out start 16-B aligned (out: 8-B when bf16), which makes every
// row of them aligned: one quad per lane per iteration; else one element per lane.
template <typename OT, bool VEC>
__global__ __launch_bounds__(kThreads) void latent_sample_kernel(const float* __restrict__ cache, const int64_t* __restrict__ idx,
                                                                 const float* __restrict__ eps, OT* __restrict__ out, long rows,
                                                                 long chw, float scaling) {
    const int i = blockIdx.y;
    const long r = idx[i];                                            // block-uniform
    const bool ok = r >= 0 && r < rows;
    const float* mean = cache + (ok ? r : 0) * 2 * chw;               // (never read when !ok)
    const float* logvar = mean + chw;
    const float* ez = eps + (long)i * chw;
    OT* o = out + (long)i * chw;
    const float nan = __builtin_nanf("");
    if constexpr (VEC) {
        const long nq = chw / 4;
        for (long q = (long)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (long)gridDim.x * kThreads) {
            f32x4_t v{nan, nan, nan, nan};
            if (ok) {
                const f32x4_t mu = reinterpret_cast<const f32x4_t*>(mean)[q], lv = reinterpret_cast<const f32x4_t*>(logvar)[q];
                const f32x4_t vz = reinterpret_cast<const f32x4_t*>(ez)[q];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = posterior_sample(mu[k], lv[k], vz[k], scaling);
            }
            store4(o, q, v);
        }
    } else {
        for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads)
            o[k] = from_f<OT>(ok ? posterior_sample(mean[k], logvar[k], ez[k], scaling) : nan);
    }
}

inline bool aligned(const void* p, int bytes) { return (uintptr_t)p % bytes == 0; }

}  // namespace

extern "C" {

// A micro-batch of VAE latents from the cached posterior moments of a dataset: for i < n, r = idx[i],
// out[i] = (mean[r] + exp(0.5 * clamp(logvar[r], -30, 20)) * eps[i]) * scaling, every product and sum rounded to f32 on its own
// (the expression inside siss_latent_inject, from the same header).  cache [rows][2C][hw] f32: the mean in channels 0..C-1, the
// unclamped log-variance in C..2C-1 (VAEEncoder.raw_moments); idx [n] int64 on the device; eps [n][chw] f32; out [n][chw] f32
// (out_bf16 = 0) or bf16 rounded to nearest even (1); chw = C * h * w.  An idx[i] outside [0, rows) is not dereferenced: out[i] is
// filled with NaN.  nblk blocks per sample (1..1024), the rest is grid-strided.  f32x4 lanes when chw % 4 == 0 and cache, eps and
// out are 16-B aligned (8-B for a bf16 out), else one element per lane.
int siss_latent_sample(const float* cache, const int64_t* idx, const float* eps, void* out, int out_bf16, long rows, int n,
                       long chw, float scaling, int nblk, void* stream) {
    SISS_CHECK_ARG(cache && idx && eps && out);
    SISS_CHECK_ARG(n > 0 && n <= 65535 && chw > 0 && rows > 0 && nblk >= 1 && nblk <= 1024);
    SISS_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1);
    const bool vec = chw % 4 == 0 && aligned(cache, 16) && aligned(eps, 16) && aligned(out, out_bf16 ? 8 : 16);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(nblk, n);
    float* of = (float*)out;
    bf16_t* ob = (bf16_t*)out;
    if (out_bf16 && vec) latent_sample_kernel<bf16_t, true><<<grid, kThreads, 0, s>>>(cache, idx, eps, ob, rows, chw, scaling);
    else if (out_bf16) latent_sample_kernel<bf16_t, false><<<grid, kThreads, 0, s>>>(cache, idx, eps, ob, rows, chw, scaling);
    else if (vec) latent_sample_kernel<float, true><<<grid, kThreads, 0, s>>>(cache, idx, eps, of, rows, chw, scaling);
    else latent_sample_kernel<float, false><<<grid, kThreads, 0, s>>>(cache, idx, eps, of, rows, chw, scaling);
    SISS_LAUNCH_RET();
}

}  // extern "C"

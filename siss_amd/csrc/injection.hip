// The inject-then-denoise check's entry into the DDIM loop (siss_amd/sd_sampler.py prepare_latents_img2img; reference:
// data/src/local_sd_pipeline.py:250-323): the VAE encoder's posterior moments of m images -> the n noised starting latents, in ONE
// launch instead of chunk / clamp / exp / sample / scale / cat / add_noise (eight elementwise passes and their temporaries).
//
//   j = i mod m                                                       (torch.cat([init_latents] * (n / m)))
//   z_j = (mean_j + exp(0.5 * clamp(logvar_j, -30, 20)) * eps_z_j) * scaling    (DiagonalGaussianDistribution.sample, * scaling_factor)
//   x_i = a * z_j + b * eps_t_i                                       (DDIMScheduler.add_noise at the first timestep)
//
// HBM-bound streaming kernel: 16 B per lane per f32 access (8 B for bf16 moments), a capped grid with a grid-stride loop, no
// reduction, no atomics.  Built with -ffp-contract=off (build.py EXACT): every product and sum rounded on its own, as torch's chain
// rounds them; libm's expf (not a fast intrinsic).
#include "common.h"
#include "latent_sample.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float inject_one(float mean, float logvar, float ez, float et, float scaling, float a, float b) {
    const float z = posterior_sample(mean, logvar, ez, scaling);          // latent_sample.h: shared with siss_latent_sample
    return __fadd_rn(__fmul_rn(a, z), __fmul_rn(b, et));
}

__device__ __forceinline__ f32x4_t load4(const float* p, long q) { return reinterpret_cast<const f32x4_t*>(p)[q]; }
__device__ __forceinline__ f32x4_t load4(const bf16_t* p, long q) {
    const u32x2_t w = reinterpret_cast<const u32x2_t*>(p)[q];
    return f32x4_t{__builtin_bit_cast(float, w[0] << 16), __builtin_bit_cast(float, w[0] & 0xffff0000u),
                   __builtin_bit_cast(float, w[1] << 16), __builtin_bit_cast(float, w[1] & 0xffff0000u)};
}

// grid (blocks per sample, n).  VEC: every row of every tensor starts 16-B aligned (8-B for bf16 moments) and chw % 4 == 0: one
// quad per lane per iteration; else one element per lane.
template <typename MT, bool VEC>
__global__ __launch_bounds__(kThreads) void latent_inject_kernel(const MT* __restrict__ moments, const float* __restrict__ eps_z,
                                                                 const float* __restrict__ eps_t, float* __restrict__ x, int m,
                                                                 long chw, float scaling, float a, float b) {
    const int i = blockIdx.y;
    const int j = i % m;
    const MT* mean = moments + (long)j * 2 * chw;
    const MT* logvar = mean + chw;
    const float* ez = eps_z + (long)j * chw;
    const float* et = eps_t + (long)i * chw;
    float* out = x + (long)i * chw;
    if constexpr (VEC) {
        const long nq = chw / 4;
        for (long q = (long)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (long)gridDim.x * kThreads) {
            const f32x4_t mu = load4(mean, q), lv = load4(logvar, q), vz = load4(ez, q), vt = load4(et, q);
            f32x4_t o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = inject_one(mu[k], lv[k], vz[k], vt[k], scaling, a, b);
            reinterpret_cast<f32x4_t*>(out)[q] = o;
        }
    } else {
        for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads)
            out[k] = inject_one(to_f(mean[k]), to_f(logvar[k]), ez[k], et[k], scaling, a, b);
    }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" {

// The starting latents of an img2img DDIM loop from the VAE encoder's posterior moments: for i < n, j = i mod m,
// x[i] = a * ((mean[j] + exp(0.5 * clamp(logvar[j], -30, 20)) * eps_z[j]) * scaling) + b * eps_t[i], every product and sum
// rounded to f32 on its own.  moments [m][2C][hw]: the mean in channels 0..C-1, the log-variance in C..2C-1, f32
// (moments_bf16 = 0) or bf16 (1); eps_z [m][chw], eps_t [n][chw], x [n][chw] f32, chw = C * h * w.  n must be a multiple of m.
// a = sqrt(alphas_cumprod[t]), b = sqrt(1 - alphas_cumprod[t]).  nblk blocks per sample (1..1024), the rest is grid-strided.
// f32x4 lanes when chw % 4 == 0 and every pointer is 16-B aligned, else one element per lane.
int siss_latent_inject(const void* moments, int moments_bf16, const float* eps_z, const float* eps_t, float* x, int m, int n,
                       long chw, float scaling, float a, float b, int nblk, void* stream) {
    SISS_CHECK_ARG(moments && eps_z && eps_t && x);
    SISS_CHECK_ARG(m > 0 && n > 0 && n <= 65535 && n % m == 0 && chw > 0 && nblk >= 1 && nblk <= 1024);
    SISS_CHECK_ARG(moments_bf16 == 0 || moments_bf16 == 1);
    const bool vec = chw % 4 == 0 && aligned16(moments) && aligned16(eps_z) && aligned16(eps_t) && aligned16(x);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(nblk, n);
    const float* mf = (const float*)moments;
    const bf16_t* mb = (const bf16_t*)moments;
    if (moments_bf16 && vec) latent_inject_kernel<bf16_t, true><<<grid, kThreads, 0, s>>>(mb, eps_z, eps_t, x, m, chw, scaling, a, b);
    else if (moments_bf16) latent_inject_kernel<bf16_t, false><<<grid, kThreads, 0, s>>>(mb, eps_z, eps_t, x, m, chw, scaling, a, b);
    else if (vec) latent_inject_kernel<float, true><<<grid, kThreads, 0, s>>>(mf, eps_z, eps_t, x, m, chw, scaling, a, b);
    else latent_inject_kernel<float, false><<<grid, kThreads, 0, s>>>(mf, eps_z, eps_t, x, m, chw, scaling, a, b);
    SISS_LAUNCH_RET();
}

}  // extern "C"

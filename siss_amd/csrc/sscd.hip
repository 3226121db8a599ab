// The SD experiment's copy-detection score (delete_sd.py:226-228,:277-283: the SSCD network `sscd_disc_mixup.torchscript.pt`, a
// torchvision-layout ResNet-50 with GeM pooling, a 2048 -> 512 linear layer and L2 normalisation; the score is the cosine of the
// memorized image's embedding and a validation image's).  The trunk and the linear layer run on metric_conv.hip's siss_metric_conv /
// siss_metric_maxpool3; this file holds what is around them, f32 in and out:
//   - preprocess     : the network's input from uint8 images, or straight from the VAE decoder's output (quantised exactly as
//                      kmeans.hip quantises it, decoded_u8.h; the bytes are written too, for the PNG grid):
//                      Normalize(mean, std)(ToTensor(.)) = ((u8 / 255) - mean[c]) / std[c], each operation an IEEE f32 operation as
//                      torch's CPU ToTensor and its subtraction / division round them -- true divisions, no reciprocal, no fma
//                      (build.py EXACT: -ffp-contract=off; the intrinsics below say so again)
//   - gem            : GeM pooling of the NHWC layer4 map: clamp at (float)eps in f32, the power, sum, mean and 1/p root in f64
//   - normalize_score: F.normalize(dim=1) with the norm in f64, and the score against a unit reference row as an f64 dot product
// No atomics; every sum in a fixed order: the same input gives the same bits on every call.
#include "common.h"
#include "decoded_u8.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Norm3 { float mean[3], std[3]; };

__device__ __forceinline__ float normalized(uint8_t q, float mean, float std) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)q, 255.f), mean), std);
}

// One thread per pixel.  FORM 0: src = uint8 [n][h][w][3]; 1 / 2: src = the decoder's output [n][3][h][w] in f32 / bf16.
template <int FORM>
__global__ __launch_bounds__(kThreads) void sscd_preprocess_kernel(const void* __restrict__ src, long hw, long total, Norm3 c,
                                                                   uint8_t* __restrict__ u8_out, float* __restrict__ y) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const long img = e / hw, pix = e - img * hw;
    uint8_t q[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if constexpr (FORM == 0) q[ch] = static_cast<const uint8_t*>(src)[e * 3 + ch];
        else if constexpr (FORM == 1) q[ch] = to_u8(static_cast<const float*>(src)[(img * 3 + ch) * hw + pix]);
        else q[ch] = to_u8(static_cast<const bf16_t*>(src)[(img * 3 + ch) * hw + pix]);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (FORM != 0 && u8_out) u8_out[e * 3 + ch] = q[ch];
        y[(img * 3 + ch) * hw + pix] = normalized(q[ch], c.mean[ch], c.std[ch]);
    }
}

// Block = 64 channels x 4 slices of the pixels: slice s sums pixels s, s + 4, ... in f64, the four slices are added 0..3.
__global__ __launch_bounds__(kThreads) void sscd_gem_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int C, double p,
                                                            float eps) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const long n = blockIdx.y;
    double acc = 0.0;
    if (c < C) {
        const float* row = x + n * HW * (long)C + c;
        const bool cube = p == 3.0;
        for (int i = s; i < HW; i += 4) {
            const double v = (double)fmaxf(row[(long)i * C], eps);
            acc += cube ? v * v * v : pow(v, p);
        }
    }
    sh[s][lane] = acc;
    __syncthreads();
    if (s == 0 && c < C) {
        const double sum = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
        y[n * C + c] = (float)pow(sum / (double)HW, 1.0 / p);
    }
}

// One block per row: ||e||^2 in f64 (lane-strided partials, xor butterfly per wave, the waves left to right), then the quotients
// and, with a reference row, the f64 dot product of the ROUNDED quotients with it, summed the same way.
__global__ __launch_bounds__(kThreads) void sscd_normalize_score_kernel(const float* e, int D, double eps, const float* __restrict__ r,
                                                                        float* out, float* __restrict__ score) {
    __shared__ double sh[kWaves];
    const long n = blockIdx.x;
    const float* row = e + n * D;
    float* dst = out + n * D;                               // (may be the same row: an element is read and written by one thread)
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < D; i += kThreads) {
        const double v = (double)row[i];
        acc += v * v;
    }
    acc = wave_sum_d(acc);
    if ((t & 63) == 0) sh[t >> 6] = acc;
    __syncthreads();
    double ss = sh[0];
    for (int w = 1; w < kWaves; ++w) ss += sh[w];
    const double denom = fmax(sqrt(ss), eps);
    __syncthreads();                                        // (sh is reused for the dot product)
    double dot = 0.0;
    for (int i = t; i < D; i += kThreads) {
        const float q = (float)((double)row[i] / denom);
        dst[i] = q;
        if (r) dot += (double)q * (double)r[i];
    }
    if (!r) return;
    dot = wave_sum_d(dot);
    if ((t & 63) == 0) sh[t >> 6] = dot;
    __syncthreads();
    if (t == 0) {
        double d = sh[0];
        for (int w = 1; w < kWaves; ++w) d += sh[w];
        score[n] = (float)d;
    }
}

}  // namespace

extern "C" {

// The SSCD network's input y[n][3][h][w] (f32 NCHW) = ((u8 / 255) - mean[c]) / std[c], every operation rounded in f32 (true
// divisions).  form 0: src = uint8 [n][h][w][3] (u8_out unused, may be null); form 1 / 2: src = the VAE decoder's output [n][3][h][w]
// in f32 / bf16, first quantised as siss_kmeans_decoded quantises it -- ((img / 2 + 0.5).clamp(0, 1) * 255).round(), each operation
// rounded in src's dtype -- and, when u8_out is not null, those bytes are written to u8_out [n][h][w][3].  Any h, w.
int siss_sscd_preprocess(const void* src, int form, int n, int h, int w, float mean0, float mean1, float mean2, float std0, float std1,
                         float std2, uint8_t* u8_out, float* y, void* stream) {
    SISS_CHECK_ARG(src && y && n > 0 && h > 0 && w > 0 && form >= 0 && form <= 2);
    SISS_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f);
    const long hw = (long)h * w, total = (long)n * hw;
    SISS_CHECK_ARG((total + kThreads - 1) / kThreads < (1L << 31));
    const Norm3 c{{mean0, mean1, mean2}, {std0, std1, std2}};
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    hipStream_t st = (hipStream_t)stream;
    if (form == 0) hipLaunchKernelGGL(sscd_preprocess_kernel<0>, grid, dim3(kThreads), 0, st, src, hw, total, c, u8_out, y);
    else if (form == 1) hipLaunchKernelGGL(sscd_preprocess_kernel<1>, grid, dim3(kThreads), 0, st, src, hw, total, c, u8_out, y);
    else hipLaunchKernelGGL(sscd_preprocess_kernel<2>, grid, dim3(kThreads), 0, st, src, hw, total, c, u8_out, y);
    SISS_LAUNCH_RET();
}

// GeM pooling y[N][C] = mean_hw(max(x, (float)eps)^p)^(1/p) of the NHWC f32 map x[N][HW][C]: the clamp on the f32 value, the power
// (v * v * v when p == 3, pow otherwise), the sum in a fixed order, the mean and the root in f64, rounded once to f32.  eps > 0, p > 0.
int siss_sscd_gem(const float* x, float* y, int N, int HW, int C, double p, double eps, void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && N < 65536 && HW > 0 && C > 0 && p > 0.0 && (float)eps > 0.f);
    hipLaunchKernelGGL(sscd_gem_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, x, y, HW,
                       C, p, (float)eps);
    SISS_LAUNCH_RET();
}

// F.normalize(e, dim=1, eps) of the rows e[N][D] (f32): out[N][D] = e / max(||e||, eps), the norm in f64 and the quotient rounded once
// (out may be e itself); an all-zero row stays zero.  With r (a unit row [D], f32) not null also score[N] = the f64 dot product of
// the written row with r, rounded to f32; with r null score is not touched.
int siss_sscd_normalize_score(const float* e, int N, int D, double eps, const float* r, float* out, float* score, void* stream) {
    SISS_CHECK_ARG(e && out && N > 0 && D > 0 && eps > 0.0 && (!r || score));
    hipLaunchKernelGGL(sscd_normalize_score_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, e, D, eps, r, out, score);
    SISS_LAUNCH_RET();
}

}  // extern "C"

// What the flat-buffer update passes share (optimizer.hip: whole buffer and listed stretches; saliency.hip: under a bit mask): the
// grid, the device scalar block with the kernel that forms it, the order of the three norm sums and the AdamW arithmetic.  One
// statement of each, so that "the masked pass under an all-ones mask IS the whole-buffer pass, bit for bit" holds by construction.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

struct StepScalars {   // lives in device memory; 16 floats
    float norm_x, norm_a, dot, scale;      // 0..3  (scale = s in g = g_x - s*g_a)
    float pre_clip_norm, clip_coef, step, pad0;  // 4..7
    float bc1, bc2_sqrt, pad1, pad2;       // 8..11
    float pad3[4];
};

inline int grid_for(long n) {
    long b = (n / 4 + kThreads - 1) / kThreads;
    if (b < 1) b = 1;
    if (b > kMaxBlocks) b = kMaxBlocks;
    return (int)b;
}

// pass 1, one granule: the three products summed over its four lanes in f32, then added to the thread's f64 sums
__device__ __forceinline__ void norm_granule(const f32x4_t& x, const f32x4_t& a, double& sxx, double& saa, double& sxa) {
    float pxx = 0, paa = 0, pxa = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { pxx += x[j] * x[j]; paa += a[j] * a[j]; pxa += x[j] * a[j]; }
    sxx += pxx; saa += paa; sxa += pxa;
}
// pass 1, one element of the scalar tail (n % 4): products in f64
__device__ __forceinline__ void norm_tail(float x, float a, double& sxx, double& saa, double& sxa) {
    sxx += (double)x * x; saa += (double)a * a; sxa += (double)x * a;
}
// pass 1, end of a block: lanes -> waves -> one row of 3 doubles per block, fixed order
__device__ __forceinline__ void norm_block_fold(double sxx, double saa, double sxa, double* __restrict__ partials) {
    __shared__ double sh[3 * kThreads / 64];
    sxx = wave_sum_d(sxx); saa = wave_sum_d(saa); sxa = wave_sum_d(sxa);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[3 * w] = sxx; sh[3 * w + 1] = saa; sh[3 * w + 2] = sxa; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, b = 0, c = 0;
        for (int i = 0; i < kThreads / 64; ++i) { a += sh[3 * i]; b += sh[3 * i + 1]; c += sh[3 * i + 2]; }
        partials[3 * blockIdx.x] = a; partials[3 * blockIdx.x + 1] = b; partials[3 * blockIdx.x + 2] = c;
    }
}

// mode 0: norm fixing  s = scaling_norm / ||g_a||        (delete_celeb.py:746)
// mode 1: erasediff    s = -max(eta - <gx,ga>/||ga||^2, 0) (:740-742)
// mode 2: like 0 but s = 0 when it would be inf          (delete_tshirt.py:688-690)
__global__ void scalars_kernel(const double* __restrict__ partials, int nblk, int mode, float knob,
                               float max_norm, float beta1, float beta2, StepScalars* __restrict__ sc) {
    // one block folds the per-block partial sums in parallel (a single thread walking 2048 x 3 dependent L2 reads
    // cost 240 us: more than the streaming pass that produced them); fixed lane -> index map: deterministic
    __shared__ double shs[3 * kThreads / 64];
    double xx = 0, aa = 0, xa = 0;
    for (int i = threadIdx.x; i < nblk; i += kThreads) { xx += partials[3 * i]; aa += partials[3 * i + 1]; xa += partials[3 * i + 2]; }
    xx = wave_sum_d(xx); aa = wave_sum_d(aa); xa = wave_sum_d(xa);
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; shs[3 * w] = xx; shs[3 * w + 1] = aa; shs[3 * w + 2] = xa; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    xx = aa = xa = 0;
    for (int i = 0; i < kThreads / 64; ++i) { xx += shs[3 * i]; aa += shs[3 * i + 1]; xa += shs[3 * i + 2]; }
    const double nx = sqrt(xx), na = sqrt(aa);
    double s;
    if (mode == 1) {
        s = (double)knob - xa / aa;
        s = -(s > 0 ? s : 0);
    } else {
        s = (double)knob / na;
        if (mode == 2 && isinf(s)) s = 0;
    }
    double g2 = xx - 2 * s * xa + s * s * aa;
    if (g2 < 0) g2 = 0;
    const double gn = sqrt(g2);
    double coef = (double)max_norm / (gn + 1e-6);   // torch.nn.utils.clip_grad_norm_
    if (coef > 1) coef = 1;
    const float step = sc->step + 1.f;
    sc->norm_x = (float)nx; sc->norm_a = (float)na; sc->dot = (float)xa; sc->scale = (float)s;
    sc->pre_clip_norm = (float)gn; sc->clip_coef = (float)coef; sc->step = step;
    // in double, ONE rounding: 1.f - powf(beta, step) cancels at small step counts (beta2 = 0.999, step 2: an f32 pow's ~3e-8
    // absolute error over 0.002 is 3.5e-6 of the update, where torch's own f32 AdamW is at 2e-7 of it; docs/history.md)
    sc->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    sc->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

// pass 2, one element: g = clip * (g_x - s g_a); torch.optim.AdamW single-tensor update order.  Returns g.
struct AdamWStep {
    float s, clip, bc2s, step_size, decay, beta1, beta2, eps;
    __device__ AdamWStep(const StepScalars* __restrict__ sc, float lr, float beta1_, float beta2_, float eps_, float wd)
        : s(sc->scale), clip(sc->clip_coef), bc2s(sc->bc2_sqrt), step_size(lr / sc->bc1), decay(1.f - lr * wd), beta1(beta1_),
          beta2(beta2_), eps(eps_) {}
    __device__ __forceinline__ float operator()(float x, float a, float& pp, float& mm, float& vv) const {
        const float g = __fmul_rn(__fsub_rn(x, __fmul_rn(s, a)), clip);
        pp = __fmul_rn(pp, decay);
        mm = __fadd_rn(mm, __fmul_rn(__fsub_rn(g, mm), 1.f - beta1));           // lerp
        vv = __fadd_rn(__fmul_rn(vv, beta2), __fmul_rn(__fmul_rn(g, g), 1.f - beta2));
        const float den = __fadd_rn(sqrtf(vv) / bc2s, eps);
        pp = __fsub_rn(pp, __fmul_rn(step_size, mm / den));
        return g;
    }
};

// pass 2, one whole granule i of the buffers: load, four element updates, p / m / v (+ g_out, + the bf16 shadow) stored as vectors
__device__ __forceinline__ void update_granule(const AdamWStep& upd, const float* __restrict__ gx, const float* __restrict__ ga,
                                               float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                               bf16_t* __restrict__ shadow, float* __restrict__ g_out, long i) {
    f32x4_t x = reinterpret_cast<const f32x4_t*>(gx)[i], a = reinterpret_cast<const f32x4_t*>(ga)[i];
    f32x4_t pp = reinterpret_cast<f32x4_t*>(p)[i], mm = reinterpret_cast<f32x4_t*>(m)[i],
            vv = reinterpret_cast<f32x4_t*>(v)[i], gg;
#pragma unroll
    for (int j = 0; j < 4; ++j) { float P = pp[j], M = mm[j], V = vv[j]; gg[j] = upd(x[j], a[j], P, M, V); pp[j] = P; mm[j] = M; vv[j] = V; }
    reinterpret_cast<f32x4_t*>(p)[i] = pp;
    reinterpret_cast<f32x4_t*>(m)[i] = mm;
    reinterpret_cast<f32x4_t*>(v)[i] = vv;
    if (g_out) reinterpret_cast<f32x4_t*>(g_out)[i] = gg;
    if (shadow) reinterpret_cast<u32x2_t*>(shadow)[i] = u32x2_t{pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3])};
}
// pass 2, element i of the scalar tail (n % 4)
__device__ __forceinline__ void update_element(const AdamWStep& upd, const float* __restrict__ gx, const float* __restrict__ ga,
                                               float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                               bf16_t* __restrict__ shadow, float* __restrict__ g_out, long i) {
    float P = p[i], M = m[i], V = v[i];
    const float g = upd(gx[i], ga[i], P, M, V);
    p[i] = P; m[i] = M; v[i] = V;
    if (g_out) g_out[i] = g;
    if (shadow) shadow[i] = f2bf(P);
}

}  // namespace

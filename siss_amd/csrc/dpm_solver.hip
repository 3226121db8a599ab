// DPM-Solver++ multistep (order <= 2, "2M") update behind classifier-free guidance, fused: the opt-in evaluation sampler of
// siss_amd/scheduler.py DPMSolverMultistepScheduler (Lu et al. 2022, "DPM-Solver++", Algorithm 2; diffusers'
// DPMSolverMultistepScheduler with algorithm_type = "dpmsolver++", solver_type = "midpoint").  The reference has no such
// sampler: this is not its protocol.  Per element, each product / sum rounded on its own in this order:
//   d = e_text - e_uncond;  e = e_uncond + g * d                  (CFG only; the order of cfg_ddim_kernel, siss_loss.hip)
//   m  = a * x - b * e                                            (x0-prediction: a = 1 / alpha_s, b = sigma_s / alpha_s)
//   x' = (c_x * x + c_0 * m) + c_1 * m1                           (the last term only when c_1 != 0: m1 is not read otherwise)
// The five coefficients are formed on the host in f64 and rounded once.  Streaming: 4 reads + 2 writes of f32 per element under
// guidance (DDIM: 3 + 1), f32x4 lanes, nblk blocks per sample, grid-strided beyond that.
// CFG: each block also writes its partial sums of e_uncond^2 and d^2 to norms[2][n][gridDim.x] -- the construction of
// cfg_ddim_kernel restated (same lanes, same f64 sums, same order: the two slabs are bitwise equal on the same eps and grid).
#include "common.h"

namespace {

constexpr int kThreads = 256;

template <bool M1>
__device__ __forceinline__ void dpmpp_one(float e, float xv, float m1, float a, float b, float cx, float c0, float c1,
                                          float& xo, float& mo) {
    const float m = __fsub_rn(__fmul_rn(a, xv), __fmul_rn(b, e));
    float o = __fadd_rn(__fmul_rn(cx, xv), __fmul_rn(c0, m));
    if constexpr (M1) o = __fadd_rn(o, __fmul_rn(c1, m1));
    xo = o;
    mo = m;
}

// x_out may alias x, m_out may alias m_prev (no __restrict__ on the four): a lane reads its elements of x and m_prev before it
// writes them, and no other lane touches them.
template <bool CFG, bool VEC, bool M1>
__global__ __launch_bounds__(kThreads) void cfg_dpmpp_kernel(const float* __restrict__ eps, const float* x, const float* m_prev,
                                                             float* x_out, float* m_out, int n, long chw, float g, float a,
                                                             float b, float cx, float c0, float c1, float* __restrict__ norms) {
    __shared__ double sh[2 * kThreads / 64];
    const int s = blockIdx.y;
    const long base = (long)s * chw;
    const float* eu = eps + base;
    const float* et = eps + (long)n * chw + base;            // (read only when CFG)
    double su = 0, sd = 0;
    auto guide = [&](float u, float t, float& e) {
        if constexpr (CFG) {
            const float d = __fsub_rn(t, u);
            e = __fadd_rn(u, __fmul_rn(g, d));
            su += (double)u * (double)u;
            sd += (double)d * (double)d;
        } else {
            e = u;
        }
    };
    auto one = [&](long k) {                                  // one element of this sample
        float e, xo, mo;
        guide(eu[k], CFG ? et[k] : 0.f, e);
        dpmpp_one<M1>(e, x[base + k], M1 ? m_prev[base + k] : 0.f, a, b, cx, c0, c1, xo, mo);
        x_out[base + k] = xo;
        m_out[base + k] = mo;
    };
    if constexpr (VEC) {                                      // every row starts 16-B aligned: one f32x4 per lane
        const long nq = chw / 4;
        for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nq; i += (long)gridDim.x * kThreads) {
            const f32x4_t u = reinterpret_cast<const f32x4_t*>(eu)[i];
            const f32x4_t xv = reinterpret_cast<const f32x4_t*>(x + base)[i];
            f32x4_t t = u, m1 = u, xo, mo;
            if constexpr (CFG) t = reinterpret_cast<const f32x4_t*>(et)[i];
            if constexpr (M1) m1 = reinterpret_cast<const f32x4_t*>(m_prev + base)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e, xj, mj;
                guide(u[j], t[j], e);
                dpmpp_one<M1>(e, xv[j], m1[j], a, b, cx, c0, c1, xj, mj);
                xo[j] = xj;
                mo[j] = mj;
            }
            reinterpret_cast<f32x4_t*>(x_out + base)[i] = xo;
            reinterpret_cast<f32x4_t*>(m_out + base)[i] = mo;
        }
        if (blockIdx.x == 0) {                                // scalar tail (one row, C*H*W not a multiple of 4)
            for (long k = nq * 4 + threadIdx.x; k < chw; k += kThreads) one(k);
        }
    } else {                                                  // rows not 16-B aligned (odd C*H*W): one element per lane
        for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads) one(k);
    }
    if constexpr (CFG) {                                      // (block_reduce2 of siss_loss.hip: waves in f64, then wave 0..3 in order)
        su = wave_sum_d(su);
        sd = wave_sum_d(sd);
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
        if (l == 0) { sh[2 * w] = su; sh[2 * w + 1] = sd; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double pu = 0, pd = 0;
            for (int i = 0; i < kThreads / 64; ++i) { pu += sh[2 * i]; pd += sh[2 * i + 1]; }
            norms[(long)s * gridDim.x + blockIdx.x] = (float)pu;
            norms[((long)n + s) * gridDim.x + blockIdx.x] = (float)pd;
        }
    }
}

template <bool CFG, bool VEC>
void launch(bool m1, dim3 grid, hipStream_t s, const float* eps, const float* x, const float* m_prev, float* x_out, float* m_out,
            int n, long chw, float g, float a, float b, float cx, float c0, float c1, float* norms) {
    if (m1) cfg_dpmpp_kernel<CFG, VEC, true><<<grid, kThreads, 0, s>>>(eps, x, m_prev, x_out, m_out, n, chw, g, a, b, cx, c0, c1, norms);
    else cfg_dpmpp_kernel<CFG, VEC, false><<<grid, kThreads, 0, s>>>(eps, x, m_prev, x_out, m_out, n, chw, g, a, b, cx, c0, c1, norms);
}

}  // namespace

extern "C" {

// Classifier-free guidance + one DPM-Solver++ multistep update (order 1 or 2) over n samples of chw f32 each: eps [2n][chw]
// (uncond rows first) when guidance > 1, else [n][chw] (no guidance, norms unused); x, x_out, m_out [n][chw] (x_out may be x,
// m_out may be m_prev).  e = e_uncond + guidance * (e_text - e_uncond); m_out = inv_alpha * x - sigma_over_alpha * e (the
// x0-prediction); x_out = c_x * x + c_0 * m_out + c_1 * m_prev.  m_prev [n][chw], the previous step's m_out, may be NULL exactly
// when c_1 == 0 (an order-1 or final step) and is not read then.  nblk blocks per sample (1..1024); with guidance,
// norms[2][n][nblk] receives the per-block partial sums of e_uncond^2 and (e_text - e_uncond)^2, the same bits as
// siss_cfg_ddim_step leaves for the same eps, n, chw and nblk.  A bad argument writes nothing.
int siss_cfg_dpmpp_step(const float* eps, const float* x, const float* m_prev, float* x_out, float* m_out, int n, long chw,
                        float guidance, float inv_alpha, float sigma_over_alpha, float c_x, float c_0, float c_1, float* norms,
                        int nblk, void* stream) {
    const bool cfg = guidance > 1.f;
    SISS_CHECK_ARG(eps && x && x_out && m_out && n > 0 && n <= 65535 && chw > 0 && inv_alpha > 0.f && nblk >= 1 && nblk <= 1024);
    SISS_CHECK_ARG(!cfg || norms);
    SISS_CHECK_ARG(m_prev || c_1 == 0.f);
    const bool m1 = c_1 != 0.f;
    // f32x4 lanes when every row starts 16-B aligned (a single row always does; the rest of it is the scalar tail)
    const uintptr_t ptrs = (uintptr_t)eps | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)m_out | (m1 ? (uintptr_t)m_prev : 0);
    const bool vec = (chw % 4 == 0 || (n == 1 && !cfg)) && ptrs % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(nblk, n);
    const float g = guidance, a = inv_alpha, b = sigma_over_alpha;
    if (cfg && vec) launch<true, true>(m1, grid, s, eps, x, m_prev, x_out, m_out, n, chw, g, a, b, c_x, c_0, c_1, norms);
    else if (cfg) launch<true, false>(m1, grid, s, eps, x, m_prev, x_out, m_out, n, chw, g, a, b, c_x, c_0, c_1, norms);
    else if (vec) launch<false, true>(m1, grid, s, eps, x, m_prev, x_out, m_out, n, chw, g, a, b, c_x, c_0, c_1, nullptr);
    else launch<false, false>(m1, grid, s, eps, x, m_prev, x_out, m_out, n, chw, g, a, b, c_x, c_0, c_1, nullptr);
    SISS_LAUNCH_RET();
}

}  // extern "C"

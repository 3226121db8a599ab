// Training of the MNIST ResNet-18 metric classifier (siss_amd/classifier_train.py): what the eval-only f32 metric stack of
// metric_conv.hip lacks -- the convolution's two gradients, batch-statistics BatchNorm forward / backward, the 3 x 3 / 2 max pool's
// backward and softmax cross-entropy.  f32 on NHWC activations, weights in metric_net.pack_conv's layout ([Cout][Kp], (kh, kw, ci)
// order, Kp % 32 == 0, zeros beyond K); the forward convolutions are siss_metric_conv with a zero bias.
//   - cls_dgrad_kernel: dx as an implicit GEMM, M = N H W input pixels, N = Cin, K = KH KW Cout in (kh, kw, co) order; dy gathered
//     with zero fill at the taps where (h + p - kh) / s is exact and in range; the weights read transposed out of the packed layout.
//     K can be split like the forward's (the late layers have a handful of 64 x 64 tiles and K up to 4608).
//   - cls_wgrad_kernel: dW[co][k] as a GEMM over the reduction m = N Ho Wo: both operands staged transposed (dy^T, gathered x^T);
//     the tile covers the pad slots k >= K with zero operands, so they are written as exact zeros.  The reduction can be split:
//     raw partial tiles to a slab, summed by a second launch in split order.
//   - products on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain), the tile and the k-slot scheme of metric_conv_kernel.
//   - BatchNorm: per-channel f64 partial sums over row chunks, a finalize launch that sums them in chunk order, an apply launch.
// No atomics anywhere: the same call gives the same bits.  No launcher synchronises with the host.
#include "common.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32, LDS_LD = BK + 4;      // (metric_conv.hip's tile)
constexpr int kBnChunks = 64;                                  // row chunks of the BatchNorm partial sums, at most
constexpr double kBnEps = 1e-5, kBnMomentum = 0.1;

typedef float Tile[LDS_LD];

// 8 staged floats of thread t as a row piece: S[t / 4][(t % 4) * 8 ..]
__device__ __forceinline__ void stage_row(Tile* S, int lr, int lk, const f32x4_t (&r)[2]) {
    *reinterpret_cast<f32x4_t*>(&S[lr][lk]) = r[0];
    *reinterpret_cast<f32x4_t*>(&S[lr][lk + 4]) = r[1];
}
// ... as a column piece (the operand is read transposed): S[(t % 8) * 8 + j][t / 8]
__device__ __forceinline__ void stage_col(Tile* S, int c8, int kk, const f32x4_t (&r)[2]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) S[c8 + j][kk] = r[j >> 2][j & 3];
}

// The K loop of metric_conv_kernel: the next step's operands are in flight (load) while the current step's 32 MFMAs per wave run
// from LDS.  acc[i][jj][r]: row wm 32 + i 16 + 4 q + r, column wn 32 + jj 16 + li of the 64 x 64 tile.
template <class Load, class Stage>
__device__ __forceinline__ void gemm_loop(int s0, int s1, Tile* As, Tile* Bs, f32x4_t (&acc)[2][2], Load load, Stage stage) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wm = wv & 1, wn = wv >> 1, li = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (s0 >= s1) return;
    load(s0);
    stage();
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        if (s + 1 < s1) load(s + 1);
#pragma unroll
        for (int g = 0; g < BK / 16; ++g) {
            f32x4_t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const f32x4_t*>(&As[wm * 32 + i * 16 + li][g * 16 + 4 * q]);
                b[i] = *reinterpret_cast<const f32x4_t*>(&Bs[wn * 32 + i * 16 + li][g * 16 + 4 * q]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][j], b[jj][j], acc[i][jj], 0, 0, 0);
        }
        if (s + 1 < s1) {
            __syncthreads();
            stage();
            __syncthreads();
        }
    }
}

__device__ __forceinline__ f32x4_t ld4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
constexpr f32x4_t kZero4 = {0.f, 0.f, 0.f, 0.f};

// ---------------------------------------------------------------------------------------------------------------- data gradient
struct DgradP {
    const float* dy; const float* w; const float* add; float* dx; float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, ldy, KH, KW, stride, pad_h, pad_w, Kp, M, steps_per_split;
};

// A K step is 32 output channels of one tap: step s -> tap s / (ldy / 32), channels (s % (ldy / 32)) * 32 ...  Split-K (gridDim.z > 1)
// writes raw partial tiles to the slab that cls_dgrad_reduce_kernel sums in split order.
__global__ __launch_bounds__(256) void cls_dgrad_kernel(const DgradP p) {
    __shared__ float As[BM][LDS_LD];
    __shared__ float Bs[BN][LDS_LD];
    const int t = threadIdx.x;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int cps = p.ldy / BK;

    // A: this thread's input pixel (img, h, w), 8 output channels per step
    const int lr = t >> 2, lk = (t & 3) * 8;
    const long am = m0 + lr;
    const bool arow_ok = am < p.M;
    int img = 0, hy = 0, wx = 0;
    if (arow_ok) {
        const int hw = p.H * p.W;
        img = (int)(am / hw);
        const int rem = (int)(am - (long)img * hw);
        hy = rem / p.W;
        wx = rem - hy * p.W;
    }
    // B: weight row co0 + kk, 8 input channels n0 + c8 ...
    const int kk = t >> 3, c8 = (t & 7) * 8;
    const bool bcol_ok = n0 + c8 < p.Cin;

    f32x4_t ra[2], rb[2];
    auto load = [&](int s) {
        const int tap = s / cps, co0 = (s - tap * cps) * BK;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        ra[0] = ra[1] = kZero4;
        const int ty = hy + p.pad_h - kh, tx = wx + p.pad_w - kw;
        if (arow_ok && ty >= 0 && tx >= 0 && ty % p.stride == 0 && tx % p.stride == 0) {
            const int oy = ty / p.stride, ox = tx / p.stride;
            if (oy < p.Ho && ox < p.Wo) {
                const float* src = p.dy + (((long)img * p.Ho + oy) * p.Wo + ox) * p.ldy + co0 + lk;
                ra[0] = ld4(src);
                ra[1] = ld4(src + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (co0 + lk + j >= p.Cout) ra[j >> 2][j & 3] = 0.f;          // (the carried channels beyond Cout)
            }
        }
        rb[0] = rb[1] = kZero4;
        if (bcol_ok && co0 + kk < p.Cout) {
            const float* src = p.w + (long)(co0 + kk) * p.Kp + (long)tap * p.Cin + n0 + c8;
            rb[0] = ld4(src);
            rb[1] = ld4(src + 4);
        }
    };
    auto stage = [&]() {
        stage_row(As, lr, lk, ra);
        stage_col(Bs, c8, kk, rb);
    };
    f32x4_t acc[2][2];
    const int s0 = blockIdx.z * p.steps_per_split;
    gemm_loop(s0, min(s0 + p.steps_per_split, p.KH * p.KW * cps), As, Bs, acc, load, stage);

    const int lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1, li = lane & 15, q = lane >> 4;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wn * 32 + jj * 16 + li;
        if (n >= p.Cin) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wm * 32 + i * 16 + 4 * q + r;
                if (m >= p.M) continue;
                float v = acc[i][jj][r];
                if (gridDim.z > 1) {
                    p.ws[((long)blockIdx.z * p.M + m) * p.Cin + n] = v;
                    continue;
                }
                if (p.add) v += p.add[m * p.Cin + n];
                p.dx[m * p.Cin + n] = v;
            }
    }
}

// dx = the sum over the splits in split order (+ add; add may be dx: read before the write, by the same thread)
__global__ __launch_bounds__(256) void cls_dgrad_reduce_kernel(const float* __restrict__ ws, const float* add, float* dx, long total,
                                                               int splits) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    float v = ws[e];
    for (int z = 1; z < splits; ++z) v += ws[(long)z * total + e];
    if (add) v += add[e];
    dx[e] = v;
}

// -------------------------------------------------------------------------------------------------------------- weight gradient
struct WgradP {
    const float* x; const float* dy; float* dw; float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, ldy, KH, KW, stride, pad_h, pad_w, Kp, K, M, steps_per_split;
};

enum { NHWC_VEC, NHWC_GATHER, NCHW_GATHER };                    // the input forms, as metric_conv_kernel's

// Rows: 64 output channels; columns: 64 packed k slots; a reduction step: 32 output pixels m.
template <int IN>
__global__ __launch_bounds__(256) void cls_wgrad_kernel(const WgradP p) {
    __shared__ float As[BM][LDS_LD];
    __shared__ float Bs[BN][LDS_LD];
    const int t = threadIdx.x;
    const int co0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int steps = (p.M + BK - 1) / BK;
    const int s0 = blockIdx.z * p.steps_per_split, s1 = min(s0 + p.steps_per_split, steps);
    const int kk = t >> 3, c8 = (t & 7) * 8;                    // output pixel s 32 + kk; 8 channels / k slots from c8
    const bool a_ok = co0 + c8 < p.ldy;
    const int k8 = n0 + c8;
    int kh = 0, kw = 0, ci = 0;
    if (IN == NHWC_VEC && k8 < p.K) {                          // (Cin % 8 == 0: the 8 slots lie in one tap)
        const int tap = k8 / p.Cin;
        ci = k8 - tap * p.Cin;
        kh = tap / p.KW;
        kw = tap - kh * p.KW;
    }

    f32x4_t ra[2], rb[2];
    auto load = [&](int s) {
        const long m = (long)s * BK + kk;
        ra[0] = ra[1] = rb[0] = rb[1] = kZero4;
        if (m >= p.M) return;
        if (a_ok) {
            const float* src = p.dy + m * p.ldy + co0 + c8;
            ra[0] = ld4(src);
            ra[1] = ld4(src + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (co0 + c8 + j >= p.Cout) ra[j >> 2][j & 3] = 0.f;
        }
        const int hw = p.Ho * p.Wo;
        const int img = (int)(m / hw);
        const int rem = (int)(m - (long)img * hw);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        const int iy0 = oy * p.stride - p.pad_h, ix0 = ox * p.stride - p.pad_w;
        if (IN == NHWC_VEC) {
            const int iy = iy0 + kh, ix = ix0 + kw;
            if (k8 < p.K && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                const float* src = p.x + (((long)img * p.H + iy) * p.W + ix) * p.Cin + ci;
                rb[0] = ld4(src);
                rb[1] = ld4(src + 4);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k8 + j;
                if (k >= p.K) continue;
                const int tap = k / p.Cin, c = k - tap * p.Cin;
                const int th = tap / p.KW;
                const int iy = iy0 + th, ix = ix0 + tap - th * p.KW;
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                    rb[j >> 2][j & 3] = IN == NCHW_GATHER ? p.x[(((long)img * p.Cin + c) * p.H + iy) * p.W + ix]
                                                          : p.x[(((long)img * p.H + iy) * p.W + ix) * p.Cin + c];
            }
        }
    };
    auto stage = [&]() {
        stage_col(As, c8, kk, ra);
        stage_col(Bs, c8, kk, rb);
    };
    f32x4_t acc[2][2];
    gemm_loop(s0, s1, As, Bs, acc, load, stage);

    const int lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1, li = lane & 15, q = lane >> 4;
    float* out = gridDim.z > 1 ? p.ws + (long)blockIdx.z * p.Cout * p.Kp : p.dw;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int k = n0 + wn * 32 + jj * 16 + li;
        if (k >= p.Kp) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + wm * 32 + i * 16 + 4 * q + r;
                if (co < p.Cout) out[(long)co * p.Kp + k] = acc[i][jj][r];
            }
    }
}

// dw = the sum over the splits in split order -- one thread per element
__global__ __launch_bounds__(256) void cls_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, long total,
                                                               int splits) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    float v = ws[e];
    for (int z = 1; z < splits; ++z) v += ws[(long)z * total + e];
    dw[e] = v;
}

// db[c] = sum over m of dy[m][c], in m order (f64, rounded once) -- one thread per column
__global__ __launch_bounds__(64) void cls_bias_grad_kernel(const float* __restrict__ dy, float* __restrict__ db, int M, int C, int ldy) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0;
    for (int m = 0; m < M; ++m) s += dy[(long)m * ldy + c];
    db[c] = (float)s;
}

// -------------------------------------------------------------------------------------------------------------------- BatchNorm
// Block = 64 channels x 4 row lanes over one chunk of rows; the four lanes are added in lane order.  BWD: the two sums of the
// backward (g, g xhat with g = dy masked by the saved output's sign) instead of (x, x^2).
template <bool BWD>
__global__ __launch_bounds__(256) void cls_bn_sums_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ y, const double* __restrict__ mean,
                                                          const double* __restrict__ invstd, double* __restrict__ partials, int M,
                                                          int C, int rows_per_chunk) {
    __shared__ double sh[2][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(r0 + rows_per_chunk, M);
    double a = 0, b = 0;
    if (c < C) {
        const double mu = BWD ? mean[c] : 0.0, is = BWD ? invstd[c] : 0.0;
        for (int r = r0 + rl; r < r1; r += 4) {
            const long e = (long)r * C + c;
            if (BWD) {
                float g = dy[e];
                if (y && !(y[e] > 0.f)) g = 0.f;
                a += g;
                b += (double)g * (((double)x[e] - mu) * is);
            } else {
                const double v = x[e];
                a += v;
                b += v * v;
            }
        }
    }
    sh[0][rl][cl] = a;
    sh[1][rl][cl] = b;
    __syncthreads();
    if (rl == 0 && c < C) {
        a = sh[0][0][cl] + sh[0][1][cl] + sh[0][2][cl] + sh[0][3][cl];
        b = sh[1][0][cl] + sh[1][1][cl] + sh[1][2][cl] + sh[1][3][cl];
        partials[((long)blockIdx.y * C + c) * 2] = a;
        partials[((long)blockIdx.y * C + c) * 2 + 1] = b;
    }
}

// Training: mean / biased variance from the chunk sums (in chunk order), the saved mean and 1 / sqrt(var + eps), the running
// statistics with the unbiased variance, and the batch counter.  Eval: the saved pair from the running statistics, nothing updated.
__global__ __launch_bounds__(256) void cls_bn_finalize_kernel(const double* __restrict__ partials, int chunks, int M, int C, int training,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              long* __restrict__ num_batches_tracked, double* __restrict__ save_mean,
                                                              double* __restrict__ save_invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (!training) {
        save_mean[c] = running_mean[c];
        save_invstd[c] = 1.0 / sqrt((double)running_var[c] + kBnEps);
        return;
    }
    double s = 0, ss = 0;
    for (int z = 0; z < chunks; ++z) {
        s += partials[((long)z * C + c) * 2];
        ss += partials[((long)z * C + c) * 2 + 1];
    }
    const double mean = s / M;
    const double var = fmax(ss / M - mean * mean, 0.0);
    save_mean[c] = mean;
    save_invstd[c] = 1.0 / sqrt(var + kBnEps);
    running_mean[c] = (float)((1.0 - kBnMomentum) * running_mean[c] + kBnMomentum * mean);
    running_var[c] = (float)((1.0 - kBnMomentum) * running_var[c] + kBnMomentum * (var * M / (M - 1)));
    if (c == 0) *num_batches_tracked += 1;
}

// y = gamma (x - mean) invstd + beta (+ res) (ReLU), formed in f64 from the f64 statistics and rounded once -- one thread per 4
// channels of a row
__global__ __launch_bounds__(256) void cls_bn_apply_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                           const double* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ res,
                                                           float* __restrict__ y, long total4, int C, int relu) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total4) return;
    const int c = (int)(e % (C / 4)) * 4;
    const f32x4_t v = ld4(x + e * 4), ga = ld4(gamma + c), be = ld4(beta + c);
    f32x4_t r = kZero4;
    if (res) r = ld4(res + e * 4);
    f32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        o[j] = (float)(((double)v[j] - mean[c + j]) * invstd[c + j] * (double)ga[j] + (double)be[j] + (double)r[j]);
    if (relu)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
    *reinterpret_cast<f32x4_t*>(y + e * 4) = o;
}

// dgamma = sum g xhat, dbeta = sum g from the chunk sums, in chunk order
__global__ __launch_bounds__(256) void cls_bn_bwd_finalize_kernel(const double* __restrict__ partials, int chunks, int C,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0, sx = 0;
    for (int z = 0; z < chunks; ++z) {
        s += partials[((long)z * C + c) * 2];
        sx += partials[((long)z * C + c) * 2 + 1];
    }
    dbeta[c] = (float)s;
    dgamma[c] = (float)sx;
}

// dx = gamma invstd (g - dbeta / M - xhat dgamma / M), formed in f64 and rounded once; dres = g (the residual branch's gradient; may be dy itself: each element is
// read before it is written, by the same thread) -- so no __restrict__ on dy / dres
__global__ __launch_bounds__(256) void cls_bn_bwd_apply_kernel(const float* dy, const float* __restrict__ y, const float* __restrict__ x,
                                                               const double* __restrict__ mean, const double* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, float* __restrict__ dx, float* dres,
                                                               long total4, int C, double inv_m) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total4) return;
    const int c = (int)(e % (C / 4)) * 4;
    f32x4_t g = ld4(dy + e * 4);
    if (y) {
        const f32x4_t o = ld4(y + e * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!(o[j] > 0.f)) g[j] = 0.f;
    }
    const f32x4_t v = ld4(x + e * 4), ga = ld4(gamma + c), dg = ld4(dgamma + c), db = ld4(dbeta + c);
    f32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double is = invstd[c + j], xh = ((double)v[j] - mean[c + j]) * is;
        o[j] = (float)((double)ga[j] * is * ((double)g[j] - (double)db[j] * inv_m - xh * (double)dg[j] * inv_m));
    }
    *reinterpret_cast<f32x4_t*>(dx + e * 4) = o;
    if (dres) *reinterpret_cast<f32x4_t*>(dres + e * 4) = g;
}

// --------------------------------------------------------------------------------------------------------------------- max pool
// Gather form of the 3 x 3 / 2 pad 1 pool's backward: an input position sums the dy of the windows whose FIRST maximum (scan order
// (kh, kw) ascending, a later tap wins only when larger or NaN: torch's rule) it is, windows in (oy, ox) order.  One thread per
// (position, 4 channels); the maxima are recomputed from x.
__global__ __launch_bounds__(256) void cls_maxpool3_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ dx, int N, int H, int W, int C, int Ho, int Wo) {
    const int c4 = C / 4;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * H * W * c4) return;
    const int c = (int)(e % c4) * 4;
    const long pix = e / c4;
    const int w = (int)(pix % W), h = (int)((pix / W) % H), img = (int)(pix / ((long)W * H));
    const float* xi = x + (long)img * H * W * C + c;
    const int me = h * W + w;
    f32x4_t acc = kZero4;
    for (int oy = max(0, h / 2); oy <= min(Ho - 1, (h + 1) / 2); ++oy)
        for (int ox = max(0, w / 2); ox <= min(Wo - 1, (w + 1) / 2); ++ox) {
            f32x4_t best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int bi[4] = {-1, -1, -1, -1};
            for (int kh = 0; kh < 3; ++kh) {
                const int iy = oy * 2 - 1 + kh;
                if (iy < 0 || iy >= H) continue;
                for (int kw = 0; kw < 3; ++kw) {
                    const int ix = ox * 2 - 1 + kw;
                    if (ix < 0 || ix >= W) continue;
                    const f32x4_t v = ld4(xi + (long)(iy * W + ix) * C);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (bi[j] < 0 || v[j] > best[j] || v[j] != v[j]) {
                            best[j] = v[j];
                            bi[j] = iy * W + ix;
                        }
                }
            }
            const f32x4_t g = ld4(dy + (((long)img * Ho + oy) * Wo + ox) * C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (bi[j] == me) acc[j] += g[j];
        }
    *reinterpret_cast<f32x4_t*>(dx + pix * C + c) = acc;
}

// ---------------------------------------------------------------------------------------------------------------- cross-entropy
// One block: thread t takes the rows t, t + 256, ...: the row's log-sum-exp shifted by its maximum, in f64, its loss and
// dlogits = (softmax - onehot) / B (zeros on the carried columns C .. ldd); the losses are added per thread in row order, then over
// the threads in thread order, and divided by B.  A label outside [0, C) makes the loss NaN.
__global__ __launch_bounds__(256) void cls_softmax_ce_kernel(const float* __restrict__ logits, const long* __restrict__ labels,
                                                             float* __restrict__ loss, float* __restrict__ dlogits, int B, int C,
                                                             int ldl, int ldd) {
    __shared__ double sh[256];
    double mine = 0;
    for (int r = threadIdx.x; r < B; r += 256) {
        const float* row = logits + (long)r * ldl;
        float* drow = dlogits + (long)r * ldd;
        const long lab = labels[r];
        double mx = row[0];
        for (int j = 1; j < C; ++j) mx = fmax(mx, (double)row[j]);
        double sum = 0;
        for (int j = 0; j < C; ++j) sum += exp((double)row[j] - mx);          // (the differences of f32 values are exact in f64)
        const double lsum = log(sum);
        // softmax - onehot: exp(z) - 1 at the label as expm1 -- a confident row has z there near 0, and the difference would cancel
        for (int j = 0; j < C; ++j) {
            const double z = (double)row[j] - mx - lsum;
            drow[j] = (float)((j == lab ? expm1(z) : exp(z)) / B);
        }
        for (int j = C; j < ldd; ++j) drow[j] = 0.f;
        mine += lab >= 0 && lab < C ? lsum - ((double)row[lab] - mx) : (double)NAN;
    }
    sh[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < 256; ++i) s += sh[i];
        *loss = (float)(s / B);
    }
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
inline bool conv_shape_ok(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_h, int pad_w) {
    return N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad_h >= 0 && pad_w >= 0 && pad_h < KH &&
           pad_w < KW && H + 2 * pad_h >= KH && W + 2 * pad_w >= KW && Ho == (H + 2 * pad_h - KH) / stride + 1 &&
           Wo == (W + 2 * pad_w - KW) / stride + 1 && (long)N * H * W < (1L << 31) && (long)N * Ho * Wo < (1L << 31);
}
inline int bn_chunk_rows(int M) { return max(64, (M + kBnChunks - 1) / kBnChunks); }     // at least 64 rows, at most kBnChunks chunks

}  // namespace

extern "C" {

// Data gradient of one convolution of the classifier: dx[m][ci] (NHWC [N][H][W][Cin], Cin % 32 == 0) = sum over (kh, kw, co) of
// dy[n, (h + pad_h - kh) / stride, (w + pad_w - kw) / stride, co] w[co][(kh, kw, ci)] (+ add[m][ci], rows of Cin floats, when add is
// given; add may be dx).  dy: NHWC [N][Ho][Wo][ldy], ldy % 32 == 0, 0 <= ldy - Cout < 32 (fc: Cout = 10 carried as 32; the carried
// channels are not read as values).  w: the packed [Cout][Kp] weights of siss_metric_conv over the channel stride Cin.  splits > 1:
// the K steps (32 output channels of a tap each) in that many parts over ws (>= splits N H W Cin floats) and a fixed-order reduce launch.
int siss_cls_conv_dgrad(const float* dy, const float* w, const float* add, float* dx, float* ws, long ws_words, int N, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int ldy, int KH, int KW, int stride, int pad_h, int pad_w, int Kp,
                        int splits, void* stream) {
    SISS_CHECK_ARG(dy && w && dx && aligned16(dy, w, add, dx) && aligned16(ws));
    SISS_CHECK_ARG(conv_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w));
    SISS_CHECK_ARG(Cin % BK == 0 && ldy % BK == 0 && ldy >= Cout && ldy - Cout < BK);
    const long K = (long)KH * KW * Cin;
    SISS_CHECK_ARG(Kp % BK == 0 && Kp >= K && Kp - K < BK);
    const long M = (long)N * H * W;
    const int steps = KH * KW * (ldy / BK);
    SISS_CHECK_ARG(splits >= 1 && splits <= steps);
    const int per = (steps + splits - 1) / splits;
    splits = (steps + per - 1) / per;                       // no empty split
    if (splits > 1) SISS_CHECK_ARG(ws && ws_words >= (long)splits * M * Cin);
    DgradP p{dy, w, add, dx, ws, N, H, W, Cin, Ho, Wo, Cout, ldy, KH, KW, stride, pad_h, pad_w, Kp, (int)M, per};
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((Cin + BN - 1) / BN), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cls_dgrad_kernel, grid, dim3(256), 0, st, p);
    if (splits > 1) {
        const long total = M * Cin;
        hipLaunchKernelGGL(cls_dgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, add, dx, total, splits);
    }
    SISS_LAUNCH_RET();
}

// Weight gradient of one convolution of the classifier, in the packed layout: dw[co][k] = sum over the N Ho Wo output pixels m of
// dy[m][co] x[gather(m, kh, kw)][ci] for k = (kh, kw, ci) < K, exactly zero on the pad slots K <= k < Kp.  x: NHWC f32
// [N][H][W][Cin] with Cin % 32 == 0, or an image (Cin <= 4, scalar gathers), NCHW [N][Cin][H][W] when nchw_in; dy: [N][Ho][Wo][ldy]
// (ldy % 32 == 0, 0 <= ldy - Cout < 32).  splits > 1: the reduction in that many parts over ws (>= splits Cout Kp floats) and a
// fixed-order reduce launch.
int siss_cls_conv_wgrad(const float* x, int nchw_in, const float* dy, float* dw, float* ws, long ws_words, int N, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int ldy, int KH, int KW, int stride, int pad_h, int pad_w, int Kp,
                        int splits, void* stream) {
    SISS_CHECK_ARG(x && dy && dw && aligned16(x, dy, dw, ws));
    SISS_CHECK_ARG(conv_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w));
    SISS_CHECK_ARG(ldy % BK == 0 && ldy >= Cout && ldy - Cout < BK);
    const long K = (long)KH * KW * Cin;
    SISS_CHECK_ARG(Kp % BK == 0 && Kp >= K && Kp - K < BK);
    const bool gather = Cin % BK != 0;
    SISS_CHECK_ARG((!gather || Cin <= 4) && (!nchw_in || Cin <= 4));
    const long M = (long)N * Ho * Wo;
    const int steps = (int)((M + BK - 1) / BK);
    SISS_CHECK_ARG(splits >= 1 && splits <= steps);
    const int per = (steps + splits - 1) / splits;
    splits = (steps + per - 1) / per;                       // no empty split
    if (splits > 1) SISS_CHECK_ARG(ws && ws_words >= (long)splits * Cout * Kp);
    WgradP p{x, dy, dw, ws, N, H, W, Cin, Ho, Wo, Cout, ldy, KH, KW, stride, pad_h, pad_w, Kp, (int)K, (int)M, per};
    dim3 grid((unsigned)((Cout + BM - 1) / BM), (unsigned)((Kp + BN - 1) / BN), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    if (nchw_in) hipLaunchKernelGGL(cls_wgrad_kernel<NCHW_GATHER>, grid, dim3(256), 0, st, p);
    else if (gather) hipLaunchKernelGGL(cls_wgrad_kernel<NHWC_GATHER>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(cls_wgrad_kernel<NHWC_VEC>, grid, dim3(256), 0, st, p);
    if (splits > 1) {
        const long total = (long)Cout * Kp;
        hipLaunchKernelGGL(cls_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, dw, total, splits);
    }
    SISS_LAUNCH_RET();
}

// Bias gradient of fc: db[c] = sum over the M rows of dy[m][c], c < C, rows of ldy floats; summed in row order.
int siss_cls_bias_grad(const float* dy, float* db, int M, int C, int ldy, void* stream) {
    SISS_CHECK_ARG(dy && db && M > 0 && C > 0 && ldy >= C);
    hipLaunchKernelGGL(cls_bias_grad_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dy, db, M, C, ldy);
    SISS_LAUNCH_RET();
}

// The f64 words of the BatchNorm launchers' `partials` for C channels (any row count).
long siss_cls_bn_partials_words(int C) { return C > 0 ? 2L * kBnChunks * C : 0; }

// BatchNorm2d (eps 1e-5, momentum 0.1) on NHWC rows x [M][C], C % 4 == 0: y = gamma (x - mean) / sqrt(var + eps) + beta (+ res)
// (ReLU when relu), formed in f64 and rounded once.  training: mean and biased variance of the M rows per channel (f64 sums), M >= 2;
// save_mean / save_invstd (f64 [C]) are written for the backward, running_mean / running_var updated in place with the unbiased variance and *num_batches_tracked (int64)
// incremented.  Otherwise the running statistics are used (and copied to save_mean / save_invstd), nothing is updated and
// num_batches_tracked may be null.  partials: siss_cls_bn_partials_words(C) doubles.  y may be x.
int siss_cls_bn_fwd(const float* x, const float* gamma, const float* beta, const float* res, float* y, float* running_mean,
                    float* running_var, long* num_batches_tracked, double* save_mean, double* save_invstd, double* partials,
                    long partials_words, int M, int C, int relu, int training, void* stream) {
    SISS_CHECK_ARG(x && gamma && beta && y && running_mean && running_var && save_mean && save_invstd && M > 0 && C > 0 && C % 4 == 0);
    SISS_CHECK_ARG(aligned16(x, gamma, beta, res) && aligned16(y, save_mean, save_invstd));
    SISS_CHECK_ARG((long)M * C < (1L << 40));
    hipStream_t st = (hipStream_t)stream;
    int chunks = 0;
    if (training) {
        SISS_CHECK_ARG(M >= 2 && num_batches_tracked && partials && partials_words >= siss_cls_bn_partials_words(C));
        const int rows = bn_chunk_rows(M);
        chunks = (M + rows - 1) / rows;
        hipLaunchKernelGGL(cls_bn_sums_kernel<false>, dim3((unsigned)((C + 63) / 64), (unsigned)chunks), dim3(256), 0, st, x, nullptr,
                           nullptr, nullptr, nullptr, partials, M, C, rows);
    }
    hipLaunchKernelGGL(cls_bn_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, partials, chunks, M, C, training,
                       running_mean, running_var, num_batches_tracked, save_mean, save_invstd);
    const long total4 = (long)M * (C / 4);
    hipLaunchKernelGGL(cls_bn_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, x, save_mean, save_invstd, gamma,
                       beta, res, y, total4, C, relu);
    SISS_LAUNCH_RET();
}

// Backward of siss_cls_bn_fwd in training mode: g = dy where the saved output y > 0 (all of dy when y is null: no ReLU);
// dbeta = sum g, dgamma = sum g xhat (f64 sums over the M rows), dx = gamma invstd (g - dbeta / M - xhat dgamma / M), and
// dres = g when dres is given (the residual branch's gradient; dres may be dy).  x is the forward's input.
int siss_cls_bn_bwd(const float* dy, const float* y, const float* x, const float* gamma, const double* save_mean,
                    const double* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta, double* partials,
                    long partials_words, int M, int C, void* stream) {
    SISS_CHECK_ARG(dy && x && gamma && save_mean && save_invstd && dx && dgamma && dbeta && M > 0 && C > 0 && C % 4 == 0);
    SISS_CHECK_ARG(aligned16(dy, y, x, gamma) && aligned16(save_mean, save_invstd, dx, dres) && aligned16(dgamma, dbeta));
    SISS_CHECK_ARG((long)M * C < (1L << 40) && partials && partials_words >= siss_cls_bn_partials_words(C));
    hipStream_t st = (hipStream_t)stream;
    const int rows = bn_chunk_rows(M), chunks = (M + rows - 1) / rows;
    hipLaunchKernelGGL(cls_bn_sums_kernel<true>, dim3((unsigned)((C + 63) / 64), (unsigned)chunks), dim3(256), 0, st, x, dy, y,
                       save_mean, save_invstd, partials, M, C, rows);
    hipLaunchKernelGGL(cls_bn_bwd_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, partials, chunks, C, dgamma,
                       dbeta);
    const long total4 = (long)M * (C / 4);
    hipLaunchKernelGGL(cls_bn_bwd_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dy, y, x, save_mean,
                       save_invstd, gamma, dgamma, dbeta, dx, dres, total4, C, 1.0 / M);
    SISS_LAUNCH_RET();
}

// Backward of the 3 x 3 max pool with stride 2 and padding 1 on NHWC f32: dx[N][H][W][C] from x (the pool's input) and
// dy[N][Ho][Wo][C], C % 4 == 0; each input position sums the dy of the windows whose first maximum it is (torch's tie rule).
int siss_cls_maxpool3_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo, void* stream) {
    SISS_CHECK_ARG(x && dy && dx && aligned16(x, dy, dx) && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0);
    SISS_CHECK_ARG(Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1 && (long)H * W < (1L << 31));
    const long total = (long)N * H * W * (C / 4);
    SISS_CHECK_ARG((total + 255) / 256 < (1L << 31));
    hipLaunchKernelGGL(cls_maxpool3_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, N,
                       H, W, C, Ho, Wo);
    SISS_LAUNCH_RET();
}

// Softmax cross-entropy with mean reduction: *loss = mean over the B rows of (log sum exp(logits[b]) - logits[b][labels[b]]) and
// dlogits[b][c] = (softmax(logits[b])[c] - (c == labels[b])) / B, zeros on the columns C .. ldd.  logits: rows of ldl floats;
// labels: int64; dlogits: rows of ldd floats.  f64 arithmetic, shifted by the row maximum; sums in a fixed order.
int siss_cls_softmax_ce(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B, int C, int ldl, int ldd,
                        void* stream) {
    SISS_CHECK_ARG(logits && labels && loss && dlogits && B > 0 && C > 0 && ldl >= C && ldd >= C);
    SISS_CHECK_ARG((uintptr_t)labels % 8 == 0 && (uintptr_t)logits % 4 == 0 && (uintptr_t)dlogits % 4 == 0 && (uintptr_t)loss % 4 == 0);
    hipLaunchKernelGGL(cls_softmax_ce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, reinterpret_cast<const long*>(labels),
                       loss, dlogits, B, C, ldl, ldd);
    SISS_LAUNCH_RET();
}

}  // extern "C"

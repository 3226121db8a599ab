// The MNIST ResNet-18 of the reference's quality metrics (metrics/mnist_resnet.py behind metrics/classifier.py: the Inception Score of
// the T-shirt experiment).  f32 end to end: the reference classifier runs in fp32, and the metric takes an argmax and the exponential
// of a KL divergence.  Two kernels:
//   - cls_conv_kernel: ONE implicit-GEMM convolution for every layer (conv1 7x7/2 on the NCHW image, the 3x3 convolutions of the
//     BasicBlocks, the 1x1/2 shortcuts, and fc as a 1x1 convolution on a 1x1 map).  M = N Ho Wo output pixels, N = Cout, K = KH KW
//     Cin in (kh, kw, ci) order; the activations are NHWC f32, gathered with zero fill (no halo rows: at 7x7 .. 1x1 maps a padded
//     layout would cost 65 % .. 800 % extra rows).  Products on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain).
//     Epilogue: the folded-BN bias, an optional residual, ReLU.  Split-K writes raw partial tiles to a slab that a second kernel sums
//     in split order: no atomics, so the same input gives bitwise-equal logits on every call.
//   - cls_maxpool_kernel: nn.MaxPool2d(3, 2, 1) on NHWC; padded positions are never chosen.
#include "common.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32, LDS_LD = BK + 4;      // (row stride 36 floats: the 16 rows of a b128 read start on 16 distinct 4-bank groups)

struct ConvP {
    const float* x; const float* w; const float* bias; const float* res; float* y; float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Kp, K, relu, steps_per_split, M;
};

__device__ __forceinline__ float epi(const ConvP& p, float v, long m, int n) {
    v += p.bias[n];
    if (p.res) v += p.res[m * p.Cout + n];
    return p.relu ? fmaxf(v, 0.f) : v;
}

// Block = 4 waves over a 64 x 64 output tile, wave (wm, wn) owns 32 x 32 = 2 x 2 MFMA tiles.  A K step of 32: thread t stages 8 k of
// A row t / 4 and of W row t / 4 in registers (the next step's load is in flight while the current step's 32 MFMAs per wave run from
// LDS).  MFMA k-slots: in a 16-k group, lane group q takes k = 4 q + j for instruction j on BOTH operands (one b128 LDS read each).
// NCHW_IN: conv1 on the image (Cin 1 or 3, scalar gathers); otherwise NHWC with Cin % 32 == 0, so a K step lies inside one tap.
template <bool NCHW_IN>
__global__ __launch_bounds__(256) void cls_conv_kernel(const ConvP p) {
    __shared__ float As[BM][LDS_LD];
    __shared__ float Bs[BN][LDS_LD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv & 1, wn = wv >> 1;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int s0 = blockIdx.z * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.Kp / BK);

    // this thread's staging row: output pixel (img, oy, ox) and weight row
    const int lr = t >> 2, lk = (t & 3) * 8;
    const long am = m0 + lr;
    const bool arow_ok = am < p.M;
    int img = 0, iy0 = 0, ix0 = 0;
    if (arow_ok) {
        const int hw = p.Ho * p.Wo;
        img = (int)(am / hw);
        const int rem = (int)(am - (long)img * hw);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0 = oy * p.stride - p.pad;
        ix0 = ox * p.stride - p.pad;
    }
    const int bn = n0 + lr;
    const bool brow_ok = bn < p.Cout;
    const float* wrow = p.w + (long)(brow_ok ? bn : 0) * p.Kp + lk;

    f32x4_t ra[2], rb[2];
    auto load = [&](int s) {
        const int k0 = s * BK;
        if (NCHW_IN) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + lk + j;
                float v = 0.f;
                if (arow_ok && k < p.K) {
                    const int ci = k % p.Cin, tap = k / p.Cin;
                    const int kh = tap / p.KW, kw = tap - kh * p.KW;
                    const int iy = iy0 + kh, ix = ix0 + kw;
                    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) v = p.x[(((long)img * p.Cin + ci) * p.H + iy) * p.W + ix];
                }
                ra[j >> 2][j & 3] = v;
            }
        } else {
            const int tap = k0 / p.Cin, ci = k0 - tap * p.Cin + lk;
            const int kh = tap / p.KW, kw = tap - kh * p.KW;
            const int iy = iy0 + kh, ix = ix0 + kw;
            if (arow_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                const float* src = p.x + (((long)img * p.H + iy) * p.W + ix) * p.Cin + ci;
                ra[0] = *reinterpret_cast<const f32x4_t*>(src);
                ra[1] = *reinterpret_cast<const f32x4_t*>(src + 4);
            } else {
                ra[0] = ra[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
        }
        if (brow_ok) {
            rb[0] = *reinterpret_cast<const f32x4_t*>(wrow + k0);
            rb[1] = *reinterpret_cast<const f32x4_t*>(wrow + k0 + 4);
        } else {
            rb[0] = rb[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage = [&]() {
        *reinterpret_cast<f32x4_t*>(&As[lr][lk]) = ra[0];
        *reinterpret_cast<f32x4_t*>(&As[lr][lk + 4]) = ra[1];
        *reinterpret_cast<f32x4_t*>(&Bs[lr][lk]) = rb[0];
        *reinterpret_cast<f32x4_t*>(&Bs[lr][lk + 4]) = rb[1];
    };

    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, q = lane >> 4;
    if (s0 < s1) {
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
    // acc[i][jj][r]: row m0 + wm 32 + i 16 + 4 q + r, column n0 + wn 32 + jj 16 + li
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wn * 32 + jj * 16 + li;
        if (n >= p.Cout) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wm * 32 + i * 16 + 4 * q + r;
                if (m >= p.M) continue;
                if (split) p.ws[((long)blockIdx.z * p.M + m) * p.Cout + n] = acc[i][jj][r];
                else p.y[m * p.Cout + n] = epi(p, acc[i][jj][r], m, n);
            }
    }
}

// y = epi(sum over the splits in split order) -- one thread per output element
__global__ __launch_bounds__(256) void cls_splitk_reduce_kernel(const ConvP p, int splits) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)p.M * p.Cout;
    if (e >= total) return;
    float v = p.ws[e];
    for (int z = 1; z < splits; ++z) v += p.ws[(long)z * total + e];
    const long m = e / p.Cout;
    p.y[e] = epi(p, v, m, (int)(e - m * p.Cout));
}

// nn.MaxPool2d(3, stride 2, padding 1) on NHWC: one thread per (pixel, 4 channels); taps outside the map are skipped (never chosen)
__global__ __launch_bounds__(256) void cls_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C,
                                                          int Ho, int Wo) {
    const int c4 = C / 4;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * Ho * Wo * c4) return;
    const int c = (int)(e % c4) * 4;
    const long pix = e / c4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), img = (int)(pix / ((long)Wo * Ho));
    f32x4_t m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= W) continue;
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + (((long)img * H + iy) * W + ix) * C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
        }
    }
    *reinterpret_cast<f32x4_t*>(y + pix * C + c) = m;
}

}  // namespace

extern "C" {

// One convolution layer of the classifier: y[N][Ho][Wo][Cout] (NHWC f32) = epi(conv(x, w)), epi = + bias[Cout] (+ res, same layout as y)
// (ReLU when relu).  x: NHWC [N][H][W][Cin] (Cin % 32 == 0), or the NCHW image [N][Cin][H][W] when nchw_in.  w: [Cout][Kp] f32 in
// (kh, kw, ci) order, Kp % 32 == 0, zero beyond K = KH KW Cin.  splits > 1: split-K over ws (>= splits N Ho Wo Cout floats) and a
// fixed-order reduce launch.
int siss_cls_conv(const float* x, int nchw_in, const float* w, const float* bias, const float* res, float* y, float* ws, long ws_words,
                  int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int Kp, int relu,
                  int splits, void* stream) {
    SISS_CHECK_ARG(x && w && bias && y && N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0);
    SISS_CHECK_ARG(Ho == (H + 2 * pad - KH) / stride + 1 && Wo == (W + 2 * pad - KW) / stride + 1 && Ho > 0 && Wo > 0);
    const int K = KH * KW * Cin;
    SISS_CHECK_ARG(Kp % BK == 0 && Kp >= K && Kp - K < BK);
    SISS_CHECK_ARG(nchw_in ? Cin <= 4 : Cin % BK == 0);
    const long M = (long)N * Ho * Wo;
    SISS_CHECK_ARG(M < (1L << 31) && (M + BM - 1) / BM < (1L << 31));
    const int steps = Kp / BK;
    SISS_CHECK_ARG(splits >= 1 && splits <= steps);
    const int per = (steps + splits - 1) / splits;
    splits = (steps + per - 1) / per;                       // no empty split
    if (splits > 1) SISS_CHECK_ARG(ws && ws_words >= (long)splits * M * Cout);
    ConvP p{x, w, bias, res, y, ws, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Kp, K, relu, per, (int)M};
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((Cout + BN - 1) / BN), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    if (nchw_in) hipLaunchKernelGGL(cls_conv_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(cls_conv_kernel<false>, grid, dim3(256), 0, st, p);
    if (splits > 1) {
        const long total = M * Cout;
        hipLaunchKernelGGL(cls_splitk_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p, splits);
    }
    SISS_LAUNCH_RET();
}

// nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on NHWC f32 [N][H][W][C] -> [N][Ho][Wo][C], C % 4 == 0
int siss_cls_maxpool(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0);
    SISS_CHECK_ARG(Ho == (H + 2 - 3) / 2 + 1 && Wo == (W + 2 - 3) / 2 + 1);
    const long total = (long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(cls_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C,
                       Ho, Wo);
    SISS_LAUNCH_RET();
}

}  // extern "C"

// The convolution and the 3 x 3 max pool that the four f32, eval-only, BN-folded metric networks share: the MNIST ResNet-18
// (siss_amd/classifier.py), the FID Inception-v3 (siss_amd/fid.py), the SSCD ResNet-50 (siss_amd/sscd.py) and the CLIP RN50
// (siss_amd/clip_iqa.py); siss_amd/metric_net.py is their host side.  f32 end to end, as the reference runs these networks' arithmetic.
//   - metric_conv_kernel: ONE implicit-GEMM convolution for every layer (the stems, the 1x1 / 3x3 / 5x5 / 1x7 / 7x1 / 1x3 / 3x1
//     convolutions, the strided 1x1 shortcuts, and fc / the projections as a 1x1 convolution on a 1x1 map).  M = N Ho Wo output
//     pixels, N = Cout, K = KH KW Cin in (kh, kw, ci) order; KH, KW, pad_h, pad_w independent; the activations are NHWC f32, gathered
//     with zero fill (no halo rows: at 7x7 .. 1x1 maps a padded layout would cost 65 % .. 800 % extra rows).  Cin is the channel
//     STRIDE of x and a multiple of 32 (Inception's 80 and 48 are carried as 96 and 64 with zero channels and zero weights); an image
//     (Cin <= 4) takes a scalar-gather form, NHWC (Inception's stem) or NCHW (the ResNets').  Products on v_mfma_f32_16x16x4_f32
//     (exact f32: a k-ordered fmaf chain).  Epilogue: the folded-BN bias, an optional residual, an optional ReLU, written at
//     y[m * ldy + coff + n]: a branch of a Mixed block lands in its slice of the block's concatenated output, no concat pass.
//     Split-K writes raw partial tiles to a slab that a second kernel sums in split order: no atomics, so the same call gives the
//     same bits.
//   - metric_maxpool3_kernel: 3 x 3 max pool on NHWC, stride 1 or 2, padding 0 or 1, into a channel slice; padded positions are
//     never chosen.
#include "common.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32, LDS_LD = BK + 4;      // (row stride 36 floats: the 16 rows of a b128 read start on 16 distinct 4-bank groups)

struct ConvP {
    const float* x; const float* w; const float* bias; const float* res; float* y; float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w, Kp, K, relu, steps_per_split, M, ldy, coff;
};

enum { NHWC_VEC, NHWC_GATHER, NCHW_GATHER };                    // the input forms of metric_conv_kernel

// (bias = p.bias[n], read by the caller once per column: a read here would be repeated after every store, which it might alias)
__device__ __forceinline__ void epi(const ConvP& p, float v, float bias, long m, int n) {
    v += bias;
    if (p.res) v += p.res[m * p.Cout + n];
    p.y[m * p.ldy + p.coff + n] = p.relu ? fmaxf(v, 0.f) : v;
}

// Block = 4 waves over a 64 x 64 output tile, wave (wm, wn) owns 32 x 32 = 2 x 2 MFMA tiles.  A K step of 32: thread t stages 8 k of
// A row t / 4 and of W row t / 4 in registers (the next step's load is in flight while the current step's 32 MFMAs per wave run from
// LDS).  MFMA k-slots: in a 16-k group, lane group q takes k = 4 q + j for instruction j on BOTH operands (one b128 LDS read each).
// IN: NHWC_VEC with Cin % 32 == 0, so a K step lies inside one tap; the two gather forms (Cin <= 4, scalar gathers over (tap, ci))
// differ in the image's layout alone.
template <int IN>
__global__ __launch_bounds__(256) void metric_conv_kernel(const ConvP p) {
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
        iy0 = oy * p.stride - p.pad_h;
        ix0 = ox * p.stride - p.pad_w;
    }
    const int bn = n0 + lr;
    const bool brow_ok = bn < p.Cout;
    const float* wrow = p.w + (long)(brow_ok ? bn : 0) * p.Kp + lk;

    f32x4_t ra[2], rb[2];
    auto load = [&](int s) {
        const int k0 = s * BK;
        if (IN != NHWC_VEC) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + lk + j;
                float v = 0.f;
                if (arow_ok && k < p.K) {
                    const int tap = k / p.Cin, ci = k - tap * p.Cin;
                    const int kh = tap / p.KW, kw = tap - kh * p.KW;
                    const int iy = iy0 + kh, ix = ix0 + kw;
                    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                        v = IN == NCHW_GATHER ? p.x[(((long)img * p.Cin + ci) * p.H + iy) * p.W + ix]
                                              : p.x[(((long)img * p.H + iy) * p.W + ix) * p.Cin + ci];
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
        const float bias = p.bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wm * 32 + i * 16 + 4 * q + r;
                if (m >= p.M) continue;
                if (split) p.ws[((long)blockIdx.z * p.M + m) * p.Cout + n] = acc[i][jj][r];
                else epi(p, acc[i][jj][r], bias, m, n);
            }
    }
}

// y = epi(sum over the splits in split order) -- one thread per output element
__global__ __launch_bounds__(256) void metric_splitk_reduce_kernel(const ConvP p, int splits) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)p.M * p.Cout;
    if (e >= total) return;
    float v = p.ws[e];
    for (int z = 1; z < splits; ++z) v += p.ws[(long)z * total + e];
    const long m = e / p.Cout;
    const int n = (int)(e - m * p.Cout);
    epi(p, v, p.bias[n], m, n);
}

// 3 x 3 max pool on NHWC, stride / pad given: one thread per (pixel, 4 channels); taps outside the map are skipped (never chosen)
__global__ __launch_bounds__(256) void metric_maxpool3_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W,
                                                              int C, int Ho, int Wo, int stride, int pad, int ldy, int coff) {
    const int c4 = C / 4;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * Ho * Wo * c4) return;
    const int c = (int)(e % c4) * 4;
    const long pix = e / c4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), img = (int)(pix / ((long)Wo * Ho));
    f32x4_t m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * stride - pad + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * stride - pad + dx;
            if (ix < 0 || ix >= W) continue;
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + (((long)img * H + iy) * W + ix) * C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
        }
    }
    *reinterpret_cast<f32x4_t*>(y + pix * ldy + coff + c) = m;
}

}  // namespace

extern "C" {

// One convolution layer of a metric network: y[m][coff + n] (row stride ldy floats, m over the N Ho Wo output pixels) =
// epi(conv(x, w)), n < Cout; epi = + bias[n] (+ res[m][n], rows of Cout floats: only with coff == 0 and ldy == Cout) (ReLU when relu).
// x: NHWC f32 [N][H][W][Cin], Cin % 32 == 0 (channels beyond the layer's own are zero in x or in w) or Cin <= 4 (an image, scalar
// gathers), or the NCHW image [N][Cin][H][W] (Cin <= 4) when nchw_in.  w: [Cout][Kp] f32 in (kh, kw, ci) order, Kp % 32 == 0, zero
// beyond K = KH KW Cin.  splits > 1: split-K over ws (>= splits N Ho Wo Cout floats) and a fixed-order reduce launch.
int siss_metric_conv(const float* x, int nchw_in, const float* w, const float* bias, const float* res, float* y, float* ws,
                     long ws_words, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_h,
                     int pad_w, int Kp, int ldy, int coff, int relu, int splits, void* stream) {
    SISS_CHECK_ARG(x && w && bias && y && N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0);
    SISS_CHECK_ARG(pad_h >= 0 && pad_w >= 0 && pad_h < KH && pad_w < KW);
    SISS_CHECK_ARG(H + 2 * pad_h >= KH && W + 2 * pad_w >= KW);
    SISS_CHECK_ARG(Ho == (H + 2 * pad_h - KH) / stride + 1 && Wo == (W + 2 * pad_w - KW) / stride + 1 && Ho > 0 && Wo > 0);
    SISS_CHECK_ARG(coff >= 0 && (long)coff + Cout <= ldy);
    SISS_CHECK_ARG(!res || (coff == 0 && ldy == Cout));
    const long K = (long)KH * KW * Cin;
    SISS_CHECK_ARG(Kp % BK == 0 && Kp >= K && Kp - K < BK);
    const bool gather = Cin % BK != 0;
    SISS_CHECK_ARG(!gather || Cin <= 4);
    SISS_CHECK_ARG(!nchw_in || Cin <= 4);
    const long M = (long)N * Ho * Wo;
    SISS_CHECK_ARG(M < (1L << 31) && (long)N * H * W < (1L << 31));
    const int steps = Kp / BK;
    SISS_CHECK_ARG(splits >= 1 && splits <= steps);
    const int per = (steps + splits - 1) / splits;
    splits = (steps + per - 1) / per;                       // no empty split
    if (splits > 1) SISS_CHECK_ARG(ws && ws_words >= (long)splits * M * Cout);
    ConvP p{x, w, bias, res, y, ws, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w, Kp, (int)K, relu, per, (int)M, ldy, coff};
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((Cout + BN - 1) / BN), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    if (nchw_in) hipLaunchKernelGGL(metric_conv_kernel<NCHW_GATHER>, grid, dim3(256), 0, st, p);
    else if (gather) hipLaunchKernelGGL(metric_conv_kernel<NHWC_GATHER>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(metric_conv_kernel<NHWC_VEC>, grid, dim3(256), 0, st, p);
    if (splits > 1) {
        const long total = M * Cout;
        hipLaunchKernelGGL(metric_splitk_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p, splits);
    }
    SISS_LAUNCH_RET();
}

// 3 x 3 max pool, stride 1 or 2, padding 0 or 1, on NHWC f32 [N][H][W][C] -> y[m][coff + c] (row stride ldy floats, m over the
// N Ho Wo output pixels); C, ldy, coff multiples of 4.  Padded positions are never chosen.
int siss_metric_maxpool3(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, int stride, int pad, int ldy, int coff,
                         void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldy % 4 == 0 && coff % 4 == 0);
    SISS_CHECK_ARG((stride == 1 || stride == 2) && (pad == 0 || pad == 1) && coff >= 0 && (long)coff + C <= ldy);
    SISS_CHECK_ARG(H + 2 * pad >= 3 && W + 2 * pad >= 3 && Ho == (H + 2 * pad - 3) / stride + 1 && Wo == (W + 2 * pad - 3) / stride + 1);
    const long total = (long)N * Ho * Wo * (C / 4);
    SISS_CHECK_ARG((total + 255) / 256 < (1L << 31));
    hipLaunchKernelGGL(metric_maxpool3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W,
                       C, Ho, Wo, stride, pad, ldy, coff);
    SISS_LAUNCH_RET();
}

}  // extern "C"

// The FID Inception-v3 (pt_inception-2015-12-05 behind torchmetrics' FrechetInceptionDistance / torch-fidelity's
// FeatureExtractorInceptionV3, which metrics/fid.py of the reference holds) up to the 2048-wide global average pool, and the f64
// feature statistics of the Frechet distance.  f32 end to end, as the reference runs it.  Kernels:
//   - inc_conv_kernel: ONE implicit-GEMM convolution for all 94 BasicConv2d layers.  M = N Ho Wo output pixels, N = Cout,
//     K = KH KW Cin in (kh, kw, ci) order; NHWC f32 activations gathered with zero fill; KH, KW, pad_h, pad_w independent (the 1x7 /
//     7x1 / 1x3 / 3x1 taps); products on v_mfma_f32_16x16x4_f32 (exact f32).  Epilogue: folded-BN bias + ReLU, written at
//     y[m * ldy + coff + n]: a branch of a Mixed block lands in its slice of the block's concatenated output, no concat pass.
//     Cin is the channel STRIDE of x and a multiple of 32 (80 and 48 are carried as 96 and 64 with zero channels and zero weights);
//     the 3-channel stem takes the scalar-gather form.  Split-K writes raw partial tiles to a slab that a second kernel sums in
//     split order: no atomics, the same call gives the same bits.
//   - inc_maxpool_kernel (3x3, stride 1 or 2, pad 0 or 1, into a channel slice), inc_avgpool_kernel (3x3 / 1 / 1 divided by the
//     number of in-map taps), inc_global_avg_kernel.
//   - inc_preprocess_kernel: [N, 3, H, W] in [0, 1] -> truncated 0..255 -> TF1 bilinear resize to 299 x 299 -> (x - 128) / 128, NHWC.
//   - fid_cov_kernel / fid_sum_kernel: cov_sum += f^T f, sum += sum_rows f in f64 from f32 features.  Plain f64 FMAs, not
//     v_mfma_f64_16x16x4_f64: an update reads and writes the D x D f64 matrix once (64 MiB at D = 2048) against 2 n D^2 = 0.5 GFLOP
//     at n = 64 -- the FMA form already sits at the memory time, and it keeps the k order of a row walk in plain sight.
#include "common.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32, LDS_LD = BK + 4;      // (row stride 36 floats: the 16 rows of a b128 read start on 16 distinct 4-bank groups)

struct ConvP {
    const float* x; const float* w; const float* bias; float* y; float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w, Kp, K, steps_per_split, M, ldy, coff;
};

__device__ __forceinline__ float epi(const ConvP& p, float v, int n) { return fmaxf(v + p.bias[n], 0.f); }

// Block = 4 waves over a 64 x 64 output tile, wave (wm, wn) owns 32 x 32 = 2 x 2 MFMA tiles.  A K step of 32: thread t stages 8 k of
// A row t / 4 and of W row t / 4 in registers (the next step's load is in flight while the current step's 32 MFMAs per wave run from
// LDS).  MFMA k-slots: in a 16-k group, lane group q takes k = 4 q + j for instruction j on BOTH operands (one b128 LDS read each).
// GATHER: the stem (Cin <= 4, scalar gathers over (tap, ci)); otherwise Cin % 32 == 0, so a K step lies inside one tap.
template <bool GATHER>
__global__ __launch_bounds__(256) void inc_conv_kernel(const ConvP p) {
    __shared__ float As[BM][LDS_LD];
    __shared__ float Bs[BN][LDS_LD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv & 1, wn = wv >> 1;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int s0 = blockIdx.z * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.Kp / BK);

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
        if (GATHER) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + lk + j;
                float v = 0.f;
                if (arow_ok && k < p.K) {
                    const int tap = k / p.Cin, ci = k - tap * p.Cin;
                    const int kh = tap / p.KW, kw = tap - kh * p.KW;
                    const int iy = iy0 + kh, ix = ix0 + kw;
                    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) v = p.x[(((long)img * p.H + iy) * p.W + ix) * p.Cin + ci];
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
                else p.y[m * p.ldy + p.coff + n] = epi(p, acc[i][jj][r], n);
            }
    }
}

// y = epi(sum over the splits in split order) -- one thread per output element
__global__ __launch_bounds__(256) void inc_splitk_reduce_kernel(const ConvP p, int splits) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)p.M * p.Cout;
    if (e >= total) return;
    float v = p.ws[e];
    for (int z = 1; z < splits; ++z) v += p.ws[(long)z * total + e];
    const long m = e / p.Cout;
    const int n = (int)(e - m * p.Cout);
    p.y[m * p.ldy + p.coff + n] = epi(p, v, n);
}

// 3 x 3 max pool on NHWC, stride / pad given: one thread per (pixel, 4 channels); taps outside the map are skipped (never chosen)
__global__ __launch_bounds__(256) void inc_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C,
                                                          int Ho, int Wo, int stride, int pad, int ldy, int coff) {
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

// F.avg_pool2d(3, stride 1, padding 1, count_include_pad=False) on NHWC: the in-map taps summed in (dy, dx) order, divided by their number
__global__ __launch_bounds__(256) void inc_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C) {
    const int c4 = C / 4;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * H * W * c4) return;
    const int c = (int)(e % c4) * 4;
    const long pix = e / c4;
    const int ox = (int)(pix % W), oy = (int)((pix / W) % H), img = (int)(pix / ((long)W * H));
    f32x4_t s = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = oy + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = ox + dx;
            if (ix < 0 || ix >= W) continue;
            s += *reinterpret_cast<const f32x4_t*>(x + (((long)img * H + iy) * W + ix) * C + c);
            ++cnt;
        }
    }
    const float d = (float)cnt;
    *reinterpret_cast<f32x4_t*>(y + pix * C + c) = f32x4_t{s[0] / d, s[1] / d, s[2] / d, s[3] / d};
}

// y[n][c] = mean over the HW pixels of x[n][.][c], pixels in order: one thread per (n, c) (neighbouring threads read neighbouring c)
__global__ __launch_bounds__(256) void inc_global_avg_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int HW, int C) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * C) return;
    const int c = (int)(e % C);
    const long n = e / C;
    const float* src = x + n * HW * C + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += src[(long)i * C];
    y[e] = s / (float)HW;
}

constexpr int INC_SIZE = 299;

// One thread per output (image, oy, ox): the three channels.  Per tap v = float(uint8(trunc(255 x))); TF1 resize (no half-pixel
// centres): src = dst * (in / out), i0 = floor(src), i1 = min(i0 + 1, in - 1), top = tl + (tr - tl) fx, bottom likewise,
// out = top + (bottom - top) fy -- each operation rounded on its own (no fma), as the tensor arithmetic it restates; then (v - 128) / 128.
__global__ __launch_bounds__(256) void inc_preprocess_kernel(const float* __restrict__ img, float* __restrict__ y, int N, int H, int W,
                                                             float sy, float sx) {
#pragma clang fp contract(off)
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * INC_SIZE * INC_SIZE) return;
    const int ox = (int)(e % INC_SIZE), oy = (int)((e / INC_SIZE) % INC_SIZE);
    const long n = e / (INC_SIZE * INC_SIZE);
    const float fy_src = (float)oy * sy, fx_src = (float)ox * sx;
    const float y0f = floorf(fy_src), x0f = floorf(fx_src);
    const int y0 = min((int)y0f, H - 1), x0 = min((int)x0f, W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float fy = fy_src - y0f, fx = fx_src - x0f;
    auto px = [&](int c, int iy, int ix) {
        const float v = img[((n * 3 + c) * H + iy) * (long)W + ix] * 255.f;
        return (float)((int)v & 255);
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tl = px(c, y0, x0), tr = px(c, y0, x1), bl = px(c, y1, x0), br = px(c, y1, x1);
        const float top = tl + (tr - tl) * fx;
        const float bot = bl + (br - bl) * fx;
        const float v = top + (bot - top) * fy;
        y[e * 3 + c] = (v - 128.f) / 128.f;
    }
}

// ---- Frechet statistics ----
constexpr int ST = 64, SK = 16;

// cov[i][j] += sum_r f[r][i] f[r][j] in f64: block = one 64 x 64 tile of cov, thread (ty, tx) 4 x 4 of it; the rows are walked in order,
// 16 at a time through LDS (f32 there: the product of two f32 values is exact in f64).  D % 4 == 0: a float4 is all in or all out.
__global__ __launch_bounds__(256) void fid_cov_kernel(const float* __restrict__ f, int n, int D, double* __restrict__ cov) {
    __shared__ float As[SK][ST];
    __shared__ float Bs[SK][ST];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int ti = blockIdx.y * ST, tj = blockIdx.x * ST;
    const int lrow = t >> 4, lcol = (t & 15) * 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int r0 = 0; r0 < n; r0 += SK) {
        const int r = r0 + lrow;
        f32x4_t va = {0.f, 0.f, 0.f, 0.f}, vb = va;
        if (r < n) {
            if (ti + lcol < D) va = *reinterpret_cast<const f32x4_t*>(f + (long)r * D + ti + lcol);
            if (tj + lcol < D) vb = *reinterpret_cast<const f32x4_t*>(f + (long)r * D + tj + lcol);
        }
        *reinterpret_cast<f32x4_t*>(&As[lrow][lcol]) = va;
        *reinterpret_cast<f32x4_t*>(&Bs[lrow][lcol]) = vb;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SK; ++k) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(&As[k][ty * 4]);
            const f32x4_t b = *reinterpret_cast<const f32x4_t*>(&Bs[k][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma((double)a[i], (double)b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gi = ti + ty * 4 + i;
        if (gi >= D) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gj = tj + tx * 4 + j;
            if (gj < D) cov[(long)gi * D + gj] += acc[i][j];
        }
    }
}

// sum[j] += sum_r f[r][j] in f64, rows in order: one thread per column
__global__ __launch_bounds__(256) void fid_sum_kernel(const float* __restrict__ f, int n, int D, double* __restrict__ sum) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D) return;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += (double)f[(long)r * D + j];
    sum[j] += s;
}

}  // namespace

extern "C" {

// One BasicConv2d of the FID Inception-v3: y[m][coff + n] (row stride ldy floats, m over the N Ho Wo output pixels) =
// relu(conv(x, w) + bias[n]), n < Cout.  x: NHWC f32 [N][H][W][Cin], Cin % 32 == 0 (channels beyond the layer's own are zero in x or
// in w), or Cin <= 4 (the stem, scalar gathers).  w: [Cout][Kp] f32 in (kh, kw, ci) order, Kp % 32 == 0, zero beyond K = KH KW Cin.
// splits > 1: split-K over ws (>= splits N Ho Wo Cout floats) and a fixed-order reduce launch.
int siss_inc_conv(const float* x, const float* w, const float* bias, float* y, float* ws, long ws_words, int N, int H, int W, int Cin,
                  int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int Kp, int ldy, int coff, int splits,
                  void* stream) {
    SISS_CHECK_ARG(x && w && bias && y && N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0);
    SISS_CHECK_ARG(pad_h >= 0 && pad_w >= 0 && pad_h < KH && pad_w < KW);
    SISS_CHECK_ARG(H + 2 * pad_h >= KH && W + 2 * pad_w >= KW);
    SISS_CHECK_ARG(Ho == (H + 2 * pad_h - KH) / stride + 1 && Wo == (W + 2 * pad_w - KW) / stride + 1 && Ho > 0 && Wo > 0);
    SISS_CHECK_ARG(coff >= 0 && (long)coff + Cout <= ldy);
    const long K = (long)KH * KW * Cin;
    SISS_CHECK_ARG(Kp % BK == 0 && Kp >= K && Kp - K < BK);
    const bool gather = Cin % BK != 0;
    SISS_CHECK_ARG(!gather || Cin <= 4);
    const long M = (long)N * Ho * Wo;
    SISS_CHECK_ARG(M < (1L << 31) && (long)N * H * W < (1L << 31));
    const int steps = Kp / BK;
    SISS_CHECK_ARG(splits >= 1 && splits <= steps);
    const int per = (steps + splits - 1) / splits;
    splits = (steps + per - 1) / per;                       // no empty split
    if (splits > 1) SISS_CHECK_ARG(ws && ws_words >= (long)splits * M * Cout);
    ConvP p{x, w, bias, y, ws, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w, Kp, (int)K, per, (int)M, ldy, coff};
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((Cout + BN - 1) / BN), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    if (gather) hipLaunchKernelGGL(inc_conv_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(inc_conv_kernel<false>, grid, dim3(256), 0, st, p);
    if (splits > 1) {
        const long total = M * Cout;
        hipLaunchKernelGGL(inc_splitk_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p, splits);
    }
    SISS_LAUNCH_RET();
}

// 3 x 3 max pool, stride 1 or 2, padding 0 or 1, on NHWC f32 [N][H][W][C] -> y[m][coff + c] (row stride ldy floats, m over the
// N Ho Wo output pixels); C, ldy, coff multiples of 4.  Padded positions are never chosen.
int siss_inc_maxpool(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, int stride, int pad, int ldy, int coff,
                     void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldy % 4 == 0 && coff % 4 == 0);
    SISS_CHECK_ARG((stride == 1 || stride == 2) && (pad == 0 || pad == 1) && coff >= 0 && (long)coff + C <= ldy);
    SISS_CHECK_ARG(H + 2 * pad >= 3 && W + 2 * pad >= 3 && Ho == (H + 2 * pad - 3) / stride + 1 && Wo == (W + 2 * pad - 3) / stride + 1);
    const long total = (long)N * Ho * Wo * (C / 4);
    SISS_CHECK_ARG((total + 255) / 256 < (1L << 31));
    hipLaunchKernelGGL(inc_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C,
                       Ho, Wo, stride, pad, ldy, coff);
    SISS_LAUNCH_RET();
}

// F.avg_pool2d(3, stride 1, padding 1, count_include_pad=False) on NHWC f32 [N][H][W][C] -> the same shape, C % 4 == 0
int siss_inc_avgpool(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    SISS_CHECK_ARG(x && y && x != y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0);
    const long total = (long)N * H * W * (C / 4);
    SISS_CHECK_ARG((total + 255) / 256 < (1L << 31));
    hipLaunchKernelGGL(inc_avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C);
    SISS_LAUNCH_RET();
}

// y[N][C] = the mean over the HW pixels of NHWC f32 x[N][HW][C]
int siss_inc_global_avg(const float* x, float* y, int N, int HW, int C, void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && HW > 0 && C > 0);
    const long total = (long)N * C;
    hipLaunchKernelGGL(inc_global_avg_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, HW, C);
    SISS_LAUNCH_RET();
}

// The FID preprocessing in one launch: img [N][3][H][W] f32 in [0, 1] -> (img * 255) truncated to the 0..255 integer -> bilinear resize
// to 299 x 299 the TF1 way (src = dst * in / 299, no half-pixel centres) -> (x - 128) / 128, written NHWC [N][299][299][3].
int siss_inc_preprocess(const float* img, float* y, int N, int H, int W, void* stream) {
    SISS_CHECK_ARG(img && y && N > 0 && H > 0 && W > 0 && (long)N * 3 * H * W < (1L << 40));
    const long total = (long)N * INC_SIZE * INC_SIZE;
    SISS_CHECK_ARG((total + 255) / 256 < (1L << 31));
    const float sy = (float)H / (float)INC_SIZE, sx = (float)W / (float)INC_SIZE;
    hipLaunchKernelGGL(inc_preprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, y, N, H, W,
                       sy, sx);
    SISS_LAUNCH_RET();
}

// The Frechet statistics of n feature rows f [n][D] f32: sum[D] += sum_r f[r], cov_sum[D][D] += f^T f, both f64 and accumulated in
// place; D % 16 == 0.  Every output element is owned by one thread that walks the rows in order: no atomics, deterministic.
int siss_fid_stats_update(const float* f, int n, int D, double* sum, double* cov_sum, void* stream) {
    SISS_CHECK_ARG(f && sum && cov_sum && n > 0 && D > 0 && D % 16 == 0);
    const unsigned tiles = (unsigned)((D + ST - 1) / ST);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fid_sum_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, f, n, D, sum);
    hipLaunchKernelGGL(fid_cov_kernel, dim3(tiles, tiles), dim3(256), 0, st, f, n, D, cov_sum);
    SISS_LAUNCH_RET();
}

}  // extern "C"

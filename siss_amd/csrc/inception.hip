// The FID Inception-v3 (pt_inception-2015-12-05 behind torchmetrics' FrechetInceptionDistance / torch-fidelity's
// FeatureExtractorInceptionV3, which metrics/fid.py of the reference holds) up to the 2048-wide global average pool, and the f64
// feature statistics of the Frechet distance.  f32 end to end, as the reference runs it.  Kernels:
//   - the 94 BasicConv2d layers and the 3 x 3 max pools run on metric_conv.hip's siss_metric_conv / siss_metric_maxpool3 (a branch
//     of a Mixed block written into its slice of the block's concatenated output); this file holds what is the Inception's own:
//   - inc_avgpool_kernel (3x3 / 1 / 1 divided by the number of in-map taps), inc_global_avg_kernel.
//   - inc_preprocess_kernel: [N, 3, H, W] in [0, 1] -> truncated 0..255 -> TF1 bilinear resize to 299 x 299 -> (x - 128) / 128, NHWC.
//   - fid_cov_kernel / fid_sum_kernel: cov_sum += f^T f, sum += sum_rows f in f64 from f32 features.  Plain f64 FMAs, not
//     v_mfma_f64_16x16x4_f64: an update reads and writes the D x D f64 matrix once (64 MiB at D = 2048) against 2 n D^2 = 0.5 GFLOP
//     at n = 64 -- the FMA form already sits at the memory time, and it keeps the k order of a row walk in plain sight.
#include "common.h"

namespace {

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

// The SD experiment's image-quality score (delete_sd.py:222-223,:264-267: torchmetrics' CLIPImageQualityAssessment with its
// defaults -- the OpenAI CLIP RN50 "ModifiedResNet", its attention pooling, and the softmax over the cosines with the two anchor
// prompts "Good photo." / "Bad photo.").  The convolutions and the three small projections (q, c_proj as 1 x 1 convolutions on a
// 1 x 1 map) run on metric_conv.hip's siss_metric_conv, the preprocessing on sscd.hip's siss_sscd_preprocess; this file holds what is
// around them, f32 in and out:
//   - avgpool     : the anti-aliasing nn.AvgPool2d(k) of the stem, of a Bottleneck's main path and of its shortcut, NHWC, with floor
//   - token_mean  : the mean over the HW positions of the layer4 map: the attention pool's only query and its first token
//   - the attention pool WITHOUT the key and value projections.  One query per head, so with q_h = (W_q m + b_q)_h / sqrt(D):
//         s[h, t]  = (W_{k,h}^T q_h) . x_t + q_h . b_{k,h}                                      (fold_query, then scores)
//         out_h    = W_{v,h} (sum_t softmax_t(s)[h, t] x_t) + b_{v,h}                           (pool, then head_value)
//     which replaces the 2 T E^2 MACs of k_proj / v_proj over every token by 2 E^2 + 2 T E heads.  The tokens are the mean row and
//     the HW rows of the map, read where they lie: no token tensor is built.
//   - score       : f / ||f||, 100 x the dot products with the unit anchor rows, the softmax over each (positive, negative) pair, f64
// No atomics; every sum in a fixed order: the same input gives the same bits on every call.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kImgTile = 8;         // images a block of fold_query / head_value carries through one pass over a weight row
constexpr int kMaxHeads = 256;      // pool: the per-head softmax statistics live in LDS

// One thread per (output pixel, 4 channels): the k x k window summed (kh, then kw ascending) in f64, the mean rounded once.
__global__ __launch_bounds__(kThreads) void clipiqa_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                                   int C4, int Ho, int Wo, int k, long total) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e % C4);
    long r = e / C4;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const long n = r / Ho;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw) {
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + (((n * H + (long)ho * k + kh) * W + (long)wo * k + kw) * C4 + c4) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)v[j];
        }
    const double inv = 1.0 / (double)(k * k);
    f32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (float)(acc[j] * inv);
    *reinterpret_cast<f32x4_t*>(y + e * 4) = o;
}

// Block = 64 channels x 4 slices of the positions: slice s sums positions s, s + 4, ... in f64, the four slices are added 0..3.
__global__ __launch_bounds__(kThreads) void clipiqa_token_mean_kernel(const float* __restrict__ x, float* __restrict__ m, int HW, int C) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const long n = blockIdx.y;
    double acc = 0.0;
    if (c < C) {
        const float* row = x + n * HW * (long)C + c;
        for (int i = s; i < HW; i += 4) acc += (double)row[(long)i * C];
    }
    sh[s][lane] = acc;
    __syncthreads();
    if (s == 0 && c < C) m[n * C + c] = (float)((((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane]) / (double)HW);
}

// Block (column chunk of 256, head h, image tile): thread = one column j of W_k; the D rows of the head are read once, each
// multiplied into up to kImgTile images' queries (LDS).  qt[n][h][j] = scale sum_d q[n][D h + d] W_k[D h + d][j] (d ascending, fmaf);
// the block of column chunk 0 also writes c[n][h] = scale sum_d q[n][D h + d] b_k[D h + d].
__global__ __launch_bounds__(kThreads) void clipiqa_fold_query_kernel(const float* __restrict__ q, const float* __restrict__ wk,
                                                                      const float* __restrict__ bk, float* __restrict__ qt,
                                                                      float* __restrict__ cst, int N, int E, int heads, int D, float scale) {
    extern __shared__ float shq[];                    // [kImgTile][D]
    const int h = blockIdx.y, n0 = blockIdx.z * kImgTile;
    const int nn = min(kImgTile, N - n0);
    for (int i = threadIdx.x; i < kImgTile * D; i += kThreads) {
        const int n = i / D, d = i - n * D;
        shq[i] = n < nn ? q[(long)(n0 + n) * E + h * D + d] : 0.f;
    }
    __syncthreads();
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < E) {
        float acc[kImgTile];
#pragma unroll
        for (int n = 0; n < kImgTile; ++n) acc[n] = 0.f;
        const float* w = wk + (long)h * D * E + j;
        for (int d = 0; d < D; ++d) {
            const float v = w[(long)d * E];
#pragma unroll
            for (int n = 0; n < kImgTile; ++n) acc[n] = fmaf(shq[n * D + d], v, acc[n]);
        }
#pragma unroll
        for (int n = 0; n < kImgTile; ++n)
            if (n < nn) qt[((long)(n0 + n) * heads + h) * E + j] = acc[n] * scale;
    }
    if (blockIdx.x == 0 && threadIdx.x < nn) {
        const int n = threadIdx.x;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(shq[n * D + d], bk[h * D + d], acc);
        cst[(long)(n0 + n) * heads + h] = acc * scale;
    }
}

// Token row t of image n: the mean row for t = 0, else position t - 1 of the map.
__device__ __forceinline__ const float* token_row(const float* __restrict__ x, const float* __restrict__ m, long n, int t, int HW, int E) {
    return t == 0 ? m + n * E : x + (n * HW + (t - 1)) * (long)E;
}

// Block (token tile of 16, head tile of 32, image): the [16 x E] . [E x 32] product on v_mfma_f32_16x16x4_f32.  Wave w takes the K
// range [w E / 4, (w + 1) E / 4) with two independent accumulators (heads 0-15 / 16-31 of the tile); lane (li = lane & 15,
// g = lane >> 4) supplies token row li and head rows li / 16 + li at k = k0 + 4 g + [0, 4) -- the same bijection of the step's k onto
// the MFMA slots on both sides -- and receives tokens 4 g + [0, 4) of head li.  The four partial tiles are added in wave order in
// LDS.  A token >= T or a head >= heads is never read: the lane reads row 0 instead and its results are not written.
__global__ __launch_bounds__(kThreads) void clipiqa_scores_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                                  const float* __restrict__ qt, const float* __restrict__ cst,
                                                                  float* __restrict__ s, int HW, int E, int heads) {
    __shared__ float part[kWaves][2][4][64];
    const int T = HW + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const long n = blockIdx.z;
    const int t0 = blockIdx.x * 16, h0 = blockIdx.y * 32;
    const int t = t0 + li < T ? t0 + li : 0;
    const int ha = h0 + li < heads ? h0 + li : 0, hb = h0 + 16 + li < heads ? h0 + 16 + li : 0;
    const float* a = token_row(x, m, n, t, HW, E) + 4 * g;
    const float* b0 = qt + (n * heads + ha) * (long)E + 4 * g;
    const float* b1 = qt + (n * heads + hb) * (long)E + 4 * g;
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int kq = E / kWaves;
    for (int k = w * kq; k < (w + 1) * kq; k += 16) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + k);
        const f32x4_t bv0 = *reinterpret_cast<const f32x4_t*>(b0 + k);
        const f32x4_t bv1 = *reinterpret_cast<const f32x4_t*>(b1 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv1[j], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        part[w][0][r][lane] = acc0[r];
        part[w][1][r][lane] = acc1[r];
    }
    __syncthreads();
    // thread -> (half, r, lane) of the tile, 512 values over 256 threads
    for (int i = threadIdx.x; i < 512; i += kThreads) {
        const int half = i >> 8, r = (i >> 6) & 3, l = i & 63;
        const float v = ((part[0][half][r][l] + part[1][half][r][l]) + part[2][half][r][l]) + part[3][half][r][l];
        const int tt = t0 + 4 * (l >> 4) + r, hh = h0 + 16 * half + (l & 15);
        if (tt < T && hh < heads) s[(n * heads + hh) * (long)T + tt] = v + cst[n * heads + hh];
    }
}

// Block (channel slab of 64, image).  Phase 1: per head the maximum over t (exact) and the sum of exp(s - max) in f64
// (lane-strided partials, xor butterfly), wave w the heads w, w + 4, ...  Phase 2: 64 tokens at a time, p[h][t] = exp(s - max) / sum
// goes to LDS and thread (channel = lane, wave w) adds p[h][t] x[t][c] for the heads h = hb + w + 4 i, i < 8, t ascending (fmaf).
__global__ __launch_bounds__(kThreads) void clipiqa_pool_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                                const float* __restrict__ s, float* __restrict__ xbar, int HW, int E,
                                                                int heads) {
    __shared__ float smax[kMaxHeads];
    __shared__ double sinv[kMaxHeads];
    __shared__ float p[32][64];
    const int T = HW + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long n = blockIdx.y;
    const int c = blockIdx.x * 64 + lane;
    for (int h = w; h < heads; h += kWaves) {
        const float* row = s + (n * heads + h) * (long)T;
        float mx = -INFINITY;
        for (int t = lane; t < T; t += 64) mx = fmaxf(mx, row[t]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        double sum = 0.0;
        for (int t = lane; t < T; t += 64) sum += (double)expf(row[t] - mx);
        sum = wave_sum_d(sum);
        if (lane == 0) { smax[h] = mx; sinv[h] = 1.0 / sum; }
    }
    __syncthreads();
    for (int hb = 0; hb < heads; hb += 32) {
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int tb = 0; tb < T; tb += 64) {
            for (int i = threadIdx.x; i < 32 * 64; i += kThreads) {
                const int hh = hb + (i >> 6), t = tb + (i & 63);
                p[i >> 6][i & 63] = hh < heads && t < T
                    ? (float)((double)expf(s[(n * heads + hh) * (long)T + t] - smax[hh]) * sinv[hh]) : 0.f;
            }
            __syncthreads();
            const int tn = min(64, T - tb);
            if (c < E)
                for (int tt = 0; tt < tn; ++tt) {
                    const float v = token_row(x, m, n, tb + tt, HW, E)[c];
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] = fmaf(p[w + 4 * i][tt], v, acc[i]);
                }
            __syncthreads();
        }
        if (c < E)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int hh = hb + w + 4 * i;
                if (hh < heads) xbar[(n * heads + hh) * (long)E + c] = acc[i];
            }
    }
}

// One wave per output row r = D h + d of W_v, up to kImgTile images per pass over the row: lane-strided float4 partials (fmaf, k
// ascending per lane), xor butterfly, + b_v.
__global__ __launch_bounds__(kThreads) void clipiqa_head_value_kernel(const float* __restrict__ xbar, const float* __restrict__ wv,
                                                                      const float* __restrict__ bv, float* __restrict__ o, int N, int E,
                                                                      int heads, int D) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= E) return;
    const int h = r / D, n0 = blockIdx.y * kImgTile;
    const int nn = min(kImgTile, N - n0);
    float acc[kImgTile];
#pragma unroll
    for (int n = 0; n < kImgTile; ++n) acc[n] = 0.f;
    const float* wrow = wv + (long)r * E;
    for (int k = lane * 4; k < E; k += 256) {
        const f32x4_t wq = *reinterpret_cast<const f32x4_t*>(wrow + k);
#pragma unroll
        for (int n = 0; n < kImgTile; ++n)
            if (n < nn) {
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xbar + ((long)(n0 + n) * heads + h) * E + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[n] = fmaf(wq[j], v[j], acc[n]);
            }
    }
#pragma unroll
    for (int n = 0; n < kImgTile; ++n) {
        const float t = wave_sum(acc[n]);
        if (lane == 0 && n < nn) o[(long)(n0 + n) * E + r] = t + bv[r];
    }
}

// f64 sum over the block of one value per thread: xor butterfly per wave, the waves left to right; the result in every thread.
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();                                        // (sh may still be read from the call before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
    for (int w = 1; w < kWaves; ++w) t += sh[w];
    return t;
}

// One block per image: ||f||^2 and the 2 P dot products in f64, then per pair the positive's softmax probability.
__global__ __launch_bounds__(kThreads) void clipiqa_score_kernel(const float* __restrict__ f, const float* __restrict__ anchors, int D,
                                                                 int P, float* __restrict__ out) {
    __shared__ double sh[kWaves];
    const long n = blockIdx.x;
    const float* row = f + n * D;
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < D; i += kThreads) {
        const double v = (double)row[i];
        acc += v * v;
    }
    const double norm = sqrt(block_sum_d(acc, sh));
    for (int p = 0; p < P; ++p) {
        double dp = 0.0, dn = 0.0;
        const float* ap = anchors + (long)(2 * p) * D;
        const float* an = ap + D;
        for (int i = t; i < D; i += kThreads) {
            const double v = (double)row[i];
            dp += v * (double)ap[i];
            dn += v * (double)an[i];
        }
        dp = block_sum_d(dp, sh);
        dn = block_sum_d(dn, sh);
        if (t == 0) {
            const double lp = 100.0 * (dp / norm), ln = 100.0 * (dn / norm);
            out[n * P + p] = (float)(1.0 / (1.0 + exp(ln - lp)));
        }
    }
}

}  // namespace

extern "C" {

// nn.AvgPool2d(k) (stride k, no padding, floor: a trailing row / column that does not fill a window is dropped) of the NHWC f32 map
// x[N][H][W][C] -> y[N][H / k][W / k][C]; the window summed in f64 in a fixed order, the mean rounded once.  C % 4 == 0, H, W >= k.
int siss_clipiqa_avgpool(const float* x, float* y, int N, int H, int W, int C, int k, void* stream) {
    SISS_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && k >= 1 && H >= k && W >= k);
    SISS_CHECK_ARG(((uintptr_t)x | (uintptr_t)y) % 16 == 0);
    const int Ho = H / k, Wo = W / k, C4 = C / 4;
    const long total = (long)N * Ho * Wo * C4;
    SISS_CHECK_ARG((total + kThreads - 1) / kThreads < (1L << 31));
    hipLaunchKernelGGL(clipiqa_avgpool_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, x, y, H, W, C4, Ho, Wo, k, total);
    SISS_LAUNCH_RET();
}

// m[N][C] = the mean over the HW positions of the NHWC f32 map x[N][HW][C], summed in f64 in a fixed order, rounded once.
int siss_clipiqa_token_mean(const float* x, float* m, int N, int HW, int C, void* stream) {
    SISS_CHECK_ARG(x && m && N > 0 && N < 65536 && HW > 0 && C > 0);
    hipLaunchKernelGGL(clipiqa_token_mean_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream,
                       x, m, HW, C);
    SISS_LAUNCH_RET();
}

// The query folded into the key projection: qt[N][heads][E] = scale sum_d q[n][D h + d] wk[D h + d][:] and c[N][heads] = scale
// sum_d q[n][D h + d] bk[D h + d], D = E / heads, q[N][E] the projected (unscaled) query, wk[E][E] ([out][in]) and bk[E] the key
// projection.  wk is read once per 8 images.
int siss_clipiqa_fold_query(const float* q, const float* wk, const float* bk, float* qt, float* c, int N, int E, int heads, float scale,
                            void* stream) {
    SISS_CHECK_ARG(q && wk && bk && qt && c && N > 0 && E > 0 && heads > 0 && heads < 65536 && E % heads == 0);
    const int D = E / heads;
    SISS_CHECK_ARG((N + kImgTile - 1) / kImgTile < 65536 && (long)kImgTile * D * 4 <= 48 * 1024);
    hipLaunchKernelGGL(clipiqa_fold_query_kernel, dim3((unsigned)((E + kThreads - 1) / kThreads), (unsigned)heads,
                                                        (unsigned)((N + kImgTile - 1) / kImgTile)),
                       dim3(kThreads), (size_t)kImgTile * D * sizeof(float), (hipStream_t)stream, q, wk, bk, qt, c, N, E, heads, D, scale);
    SISS_LAUNCH_RET();
}

// The attention pool's logits s[N][heads][HW + 1] = qt[n][h][:] . tok[n][t][:] + c[n][h], token 0 the mean row m[N][E], token t >= 1
// position t - 1 of the NHWC f32 map x[N][HW][E] (no token tensor is built).  E % 64 == 0.
int siss_clipiqa_scores(const float* x, const float* m, const float* qt, const float* c, float* s, int N, int HW, int E, int heads,
                        void* stream) {
    SISS_CHECK_ARG(x && m && qt && c && s && N > 0 && N < 65536 && HW > 0 && E > 0 && E % 64 == 0 && heads > 0);
    SISS_CHECK_ARG(((uintptr_t)x | (uintptr_t)m | (uintptr_t)qt) % 16 == 0 && (heads + 31) / 32 < 65536);
    hipLaunchKernelGGL(clipiqa_scores_kernel, dim3((unsigned)((HW + 1 + 15) / 16), (unsigned)((heads + 31) / 32), (unsigned)N),
                       dim3(kThreads), 0, (hipStream_t)stream, x, m, qt, c, s, HW, E, heads);
    SISS_LAUNCH_RET();
}

// xbar[N][heads][E] = sum_t softmax_t(s[n][h][:])[t] tok[n][t][:] over the same HW + 1 tokens, t ascending; the softmax's maximum
// exact, its sum in f64 in a fixed order.  heads <= 256.
int siss_clipiqa_pool(const float* x, const float* m, const float* s, float* xbar, int N, int HW, int E, int heads, void* stream) {
    SISS_CHECK_ARG(x && m && s && xbar && N > 0 && N < 65536 && HW > 0 && E > 0 && heads > 0 && heads <= kMaxHeads);
    hipLaunchKernelGGL(clipiqa_pool_kernel, dim3((unsigned)((E + 63) / 64), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, x, m,
                       s, xbar, HW, E, heads);
    SISS_LAUNCH_RET();
}

// The value projection after the pooling: o[N][E], o[n][D h + d] = wv[D h + d][:] . xbar[n][h][:] + bv[D h + d], D = E / heads,
// wv[E][E] ([out][in]) read once per 8 images.  E % 4 == 0.
int siss_clipiqa_head_value(const float* xbar, const float* wv, const float* bv, float* o, int N, int E, int heads, void* stream) {
    SISS_CHECK_ARG(xbar && wv && bv && o && N > 0 && E > 0 && E % 4 == 0 && heads > 0 && E % heads == 0);
    SISS_CHECK_ARG(((uintptr_t)xbar | (uintptr_t)wv) % 16 == 0 && (N + kImgTile - 1) / kImgTile < 65536);
    hipLaunchKernelGGL(clipiqa_head_value_kernel, dim3((unsigned)((E + kWaves - 1) / kWaves), (unsigned)((N + kImgTile - 1) / kImgTile)),
                       dim3(kThreads), 0, (hipStream_t)stream, xbar, wv, bv, o, N, E, heads, E / heads);
    SISS_LAUNCH_RET();
}

// The CLIP-IQA probabilities out[N][P] of the image rows f[N][D] against the unit anchor rows anchors[2 P][D] (row 2 p the positive
// prompt of pair p, row 2 p + 1 its negative): the norm of f and the dot products in f64 in a fixed order, logits = 100 f . a / ||f||,
// out = the positive's share of the pair's softmax, rounded once to f32.  An all-zero row gives NaN, as the division does in torch.
int siss_clipiqa_score(const float* f, const float* anchors, int N, int D, int P, float* out, void* stream) {
    SISS_CHECK_ARG(f && anchors && out && N > 0 && D > 0 && P >= 1);
    hipLaunchKernelGGL(clipiqa_score_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, f, anchors, D, P, out);
    SISS_LAUNCH_RET();
}

}  // extern "C"

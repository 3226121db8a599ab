// The SD deletion fraction's device side (siss_amd/kmeans.py; reference: delete_sd.py:224-225,:269-275, a scikit-learn KMeans on
// flattened uint8 images): nearest-centre classification of generated images and the Lloyd passes that fit the classifier.
//
//   decoded : VAE decoder output [n,3,H,W] (f32 / bf16) -> uint8 [n,H,W,3], bitwise diffusers' postprocess
//             `((img / 2 + 0.5).clamp(0, 1) * 255).round().to(uint8).permute(0, 2, 3, 1)`, and in the same pass the partial
//             squared distances of those uint8 values to K centres [K, H*W*3] (f32, HWC order)        (1 read + 1/4 write per element)
//   assign  : the same distances over rows that are already uint8 [N, D]                                (1 byte per element)
//   finalize: slab [rows, K, blocks] -> f64 distances, argmin labels, row minima, inertia, count of changed labels
//   update  : per feature and label the INTEGER sum of the rows (exact), centre = f32(sum / count)
//
// Accumulation: each term is (float(u8) - c)^2 with the difference and the square rounded to f32 (relative error <= 3 * 2^-24 of a
// non-negative term), added in f64 per lane, lanes -> wave -> block in fixed orders, blocks summed left to right in f64 by finalize:
// no atomics anywhere, every result bit-reproducible.  Built with -ffp-contract=off (build.py EXACT): the uint8 image is a bitwise claim.
// 1 <= K <= 16; a launch is instantiated for the tile KT in {1, 2, 3, 4, 8, 16} that holds K.
#include "common.h"
#include "decoded_u8.h"      // to_u8: torch's chain on one decoded element, shared with sscd.hip

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 4;      // rows of the uint8 matrix per block pass: the centre slice is fetched once for the four
constexpr int kMaxBlocks = 64;
constexpr int kMaxSegments = 8;

// features per lane per iteration: 16 (one 16-B load of uint8) while the centre slice fits the registers, else 4
template <int KT> struct Lane { static constexpr int F = KT <= 4 ? 16 : 4; };

__device__ __forceinline__ void sq_acc(double& acc, float x, float c) {
    const float d = __fsub_rn(x, c);
    acc += (double)__fmul_rn(d, d);
}

// acc[r][k] of every lane -> slab[(row0 + r) * k + kk][blk]; one barrier.  Wave sums by xor butterfly, the waves left to right.
template <int R, int KT>
__device__ __forceinline__ void block_store(double (&acc)[R][KT], double (*sh)[R][KT], long row0, long n, int k, int nblk, int blk,
                                            double* __restrict__ slab) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            const double s = wave_sum_d(acc[r][kk]);
            if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][r][kk] = s;
        }
    __syncthreads();
    const int r = threadIdx.x / KT, kk = threadIdx.x % KT;
    if (r < R && kk < k && row0 + r < n) {
        double s = sh[0][r][kk];
        for (int w = 1; w < kWaves; ++w) s += sh[w][r][kk];
        slab[((row0 + r) * k + kk) * nblk + blk] = s;
    }
}

// One image per blockIdx.x, pixel chunks over blockIdx.y (grid-strided).  VEC: 4 pixels per lane (H*W % 4 == 0, 16-B aligned bases).
template <int KT, typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void decoded_kernel(const T* __restrict__ img, const float* __restrict__ centres, long hw, int k,
                                                           uint8_t* __restrict__ u8, double* __restrict__ slab) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ double sh[kWaves][1][KT];
    const long row = blockIdx.x, d = 3 * hw;
    const T* src = img + row * d;
    uint8_t* dst = u8 + row * d;
    double acc[1][KT] = {};
    const long nvec = hw / P;
    for (long i = (long)blockIdx.y * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.y * kThreads) {
        uint8_t q[P][3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            T v[P];
            if constexpr (VEC) {
                typedef T vec_t __attribute__((ext_vector_type(4)));
                const vec_t t = *reinterpret_cast<const vec_t*>(src + ch * hw + i * P);
#pragma unroll
                for (int p = 0; p < P; ++p) v[p] = t[p];
            } else {
                v[0] = src[ch * hw + i];
            }
#pragma unroll
            for (int p = 0; p < P; ++p) q[p][ch] = to_u8(v[p]);
        }
        if constexpr (VEC) {
            uint32_t w[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                w[j] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) w[j] |= (uint32_t)q[(4 * j + b) / 3][(4 * j + b) % 3] << (8 * b);
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(dst + i * 12);
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dst[i * 3 + ch] = q[0][ch];
        }
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            if (kk < k) {
                const float* c = centres + kk * d + i * (3 * P);
                float cv[3 * P];
                if constexpr (VEC) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const f32x4_t t = reinterpret_cast<const f32x4_t*>(c)[j];
#pragma unroll
                        for (int b = 0; b < 4; ++b) cv[4 * j + b] = t[b];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j) cv[j] = c[j];
                }
#pragma unroll
                for (int j = 0; j < 3 * P; ++j) sq_acc(acc[0][kk], (float)q[j / 3][j % 3], cv[j]);
            }
        }
    }
    block_store<1, KT>(acc, sh, row, row + 1, k, gridDim.y, blockIdx.y, slab);
}

// kRows rows per blockIdx.x, feature chunks over blockIdx.y (grid-strided).  VEC: Lane<KT>::F features per lane (d % F == 0, rows
// and centres 16-B aligned).
template <int KT, bool VEC>
__global__ __launch_bounds__(kThreads) void assign_kernel(const uint8_t* __restrict__ rows, const float* __restrict__ centres, long n,
                                                          long d, int k, double* __restrict__ slab) {
    constexpr int F = VEC ? Lane<KT>::F : 1;
    __shared__ double sh[kWaves][kRows][KT];
    const long row0 = (long)blockIdx.x * kRows;
    double acc[kRows][KT] = {};
    const long nvec = d / F;
    for (long i = (long)blockIdx.y * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.y * kThreads) {
        float cv[KT][F];
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            if (kk < k) {
                const float* c = centres + kk * d + i * F;
                if constexpr (VEC) {
#pragma unroll
                    for (int j = 0; j < F / 4; ++j) {
                        const f32x4_t t = reinterpret_cast<const f32x4_t*>(c)[j];
#pragma unroll
                        for (int b = 0; b < 4; ++b) cv[kk][4 * j + b] = t[b];
                    }
                } else {
                    cv[kk][0] = c[0];
                }
            } else {
#pragma unroll
                for (int f = 0; f < F; ++f) cv[kk][f] = 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (row0 + r < n) {                                    // (block-uniform)
                const uint8_t* x = rows + (row0 + r) * d + i * F;
                float xv[F];
                if constexpr (VEC) {
                    uint32_t w[F / 4];
                    if constexpr (F == 16) {
                        const u32x4_t t = *reinterpret_cast<const u32x4_t*>(x);
#pragma unroll
                        for (int j = 0; j < 4; ++j) w[j] = t[j];
                    } else {
                        w[0] = *reinterpret_cast<const uint32_t*>(x);
                    }
#pragma unroll
                    for (int f = 0; f < F; ++f) xv[f] = (float)((w[f / 4] >> (8 * (f % 4))) & 0xffu);
                } else {
                    xv[0] = (float)x[0];
                }
#pragma unroll
                for (int kk = 0; kk < KT; ++kk)
                    if (kk < k)
#pragma unroll
                        for (int f = 0; f < F; ++f) sq_acc(acc[r][kk], xv[f], cv[kk][f]);
            }
        }
    }
    block_store<kRows, KT>(acc, sh, row0, n, k, gridDim.y, blockIdx.y, slab);
}

// ONE block: lane t takes rows t, t + 256, ...; every row's K x nblk partials are summed left to right in f64.  labels (when given)
// holds the previous pass's on entry; the count of rows whose label changed and the inertia (sum of the row minima: lanes in row
// order, then a fixed tree over the lanes) leave through single stores.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double* __restrict__ slab, long n, int k, int nblk,
                                                            double* __restrict__ dist, int32_t* __restrict__ labels,
                                                            double* __restrict__ row_min, double* __restrict__ inertia,
                                                            int64_t* __restrict__ status) {
    __shared__ double shd[kThreads];
    __shared__ int shc[kThreads];
    double mine = 0;
    int changed = 0;
    for (long r = threadIdx.x; r < n; r += kThreads) {
        double best = 0;
        int arg = 0;
        for (int kk = 0; kk < k; ++kk) {
            const double* p = slab + (r * k + kk) * nblk;
            double s = 0;
            for (int b = 0; b < nblk; ++b) s += p[b];
            dist[r * k + kk] = s;
            if (kk == 0 || s < best) { best = s; arg = kk; }       // lowest index on ties
        }
        if (labels) {
            changed += labels[r] != arg;
            labels[r] = arg;
        }
        if (row_min) row_min[r] = best;
        mine += best;
    }
    shd[threadIdx.x] = mine;
    shc[threadIdx.x] = changed;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            shd[threadIdx.x] += shd[threadIdx.x + s];
            shc[threadIdx.x] += shc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (inertia) inertia[0] = shd[0];
        if (status) reinterpret_cast<int32_t*>(status)[0] = shc[0];      // low word: labels changed
    }
}

// Row segment blockIdx.y of nseg, one feature group per lane (no grid stride: grid.x covers d).  The label of a row is uniform over
// the launch, so the K-way select is a scalar branch; a label outside [0, k) adds to nothing.
template <int KT, bool VEC>
__global__ __launch_bounds__(kThreads) void update_partial_kernel(const uint8_t* __restrict__ rows, const int32_t* __restrict__ labels,
                                                                  long n, long d, int k, uint32_t* __restrict__ sums,
                                                                  int64_t* __restrict__ cnts) {
    constexpr int F = VEC ? Lane<KT>::F : 1;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < d / F;
    const long per = (n + gridDim.y - 1) / gridDim.y;
    const long r0 = (long)blockIdx.y * per, r1 = r0 + per < n ? r0 + per : n;
    uint32_t acc[KT][F] = {};
    int cnt[KT] = {};
#pragma unroll 4
    for (long r = r0; r < r1; ++r) {
        const int lab = labels[r];
        uint32_t xv[F];
#pragma unroll
        for (int f = 0; f < F; ++f) xv[f] = 0;
        if (live) {
            const uint8_t* x = rows + r * d + i * F;
            if constexpr (VEC) {
                uint32_t w[F / 4];
                if constexpr (F == 16) {
                    const u32x4_t t = *reinterpret_cast<const u32x4_t*>(x);
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = t[j];
                } else {
                    w[0] = *reinterpret_cast<const uint32_t*>(x);
                }
#pragma unroll
                for (int f = 0; f < F; ++f) xv[f] = (w[f / 4] >> (8 * (f % 4))) & 0xffu;
            } else {
                xv[0] = x[0];
            }
        }
#pragma unroll
        for (int kk = 0; kk < KT; ++kk)
            if (lab == kk) {
                ++cnt[kk];
#pragma unroll
                for (int f = 0; f < F; ++f) acc[kk][f] += xv[f];
            }
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk)
        if (kk < k) {
            if (live) {
                uint32_t* o = sums + ((long)blockIdx.y * k + kk) * d + i * F;
#pragma unroll
                for (int f = 0; f < F; ++f) o[f] = acc[kk][f];
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) cnts[(long)blockIdx.y * k + kk] = cnt[kk];
        }
}

// One lane per feature: the segments' sums and counts added left to right (integers: exact), centre = f32(sum / count) with the
// quotient in f64 -- for count < 2^24 a quotient that is not an f32 midpoint is at least 2^-49 (relative) away from one, so the two
// roundings give the correctly rounded f32 mean.  An empty cluster keeps its centre and is counted in the status word.
__global__ __launch_bounds__(kThreads) void update_finalize_kernel(const uint32_t* __restrict__ sums, const int64_t* __restrict__ cnts,
                                                                   int nseg, int k, long d, float* __restrict__ centres,
                                                                   int64_t* __restrict__ counts, int64_t* __restrict__ status) {
    const long j = (long)blockIdx.x * kThreads + threadIdx.x;
    int empty = 0;
    for (int kk = 0; kk < k; ++kk) {
        int64_t cnt = 0;
        for (int s = 0; s < nseg; ++s) cnt += cnts[(long)s * k + kk];
        empty += cnt == 0;
        if (j == 0) counts[kk] = cnt;
        if (j < d && cnt > 0) {
            uint64_t t = 0;
            for (int s = 0; s < nseg; ++s) t += sums[((long)s * k + kk) * d + j];
            centres[kk * d + j] = (float)((double)t / (double)cnt);
        }
    }
    if (j == 0 && status) reinterpret_cast<int32_t*>(status)[1] = empty;   // high word: empty clusters
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline int tile_of(int k) { return k <= 4 ? k : k <= 8 ? 8 : 16; }
inline int lane_features(int k) { return tile_of(k) <= 4 ? 16 : 4; }
inline int clampi(long v, long lo, long hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }
inline int decoded_blocks(long hw) { return clampi(hw / 4 / kThreads, 1, kMaxBlocks); }
inline int assign_blocks(long d, int k) { return clampi(d / lane_features(k) / kThreads, 1, kMaxBlocks); }
inline long update_groups(long d, int k, bool vec) { return (d / (vec ? lane_features(k) : 1) + kThreads - 1) / kThreads; }
inline int update_segments(long n, long d, int k) {
    const long groups = update_groups(d, k, true);                   // (0 for a row shorter than one lane's features)
    const long by_rows = (n + 31) / 32, by_grid = 1024 / (groups > 0 ? groups : 1);
    return clampi(by_rows < by_grid ? by_rows : by_grid, 1, kMaxSegments);
}

#define KM_TILES(k, CALL)          \
    switch (tile_of(k)) {          \
        case 1: CALL(1); break;    \
        case 2: CALL(2); break;    \
        case 3: CALL(3); break;    \
        case 4: CALL(4); break;    \
        case 8: CALL(8); break;    \
        default: CALL(16); break;  \
    }

int launch_assign(const uint8_t* rows, const float* centres, long n, long d, int k, double* slab, int nblk, hipStream_t s) {
    const bool vec = d % lane_features(k) == 0 && aligned16(rows) && aligned16(centres);
    dim3 grid((unsigned)((n + kRows - 1) / kRows), nblk);
#define KM_CALL(KT)                                                                                              \
    if (vec) assign_kernel<KT, true><<<grid, kThreads, 0, s>>>(rows, centres, n, d, k, slab);                    \
    else assign_kernel<KT, false><<<grid, kThreads, 0, s>>>(rows, centres, n, d, k, slab)
    KM_TILES(k, KM_CALL)
#undef KM_CALL
    return SISS_OK;
}

}  // namespace

extern "C" {

// Blocks per image of siss_kmeans_decoded for H * W = hw pixels (the last extent of its slab).
long siss_kmeans_decoded_blocks(long hw) { return hw > 0 ? decoded_blocks(hw) : 0; }

// Blocks per row of siss_kmeans_assign for rows of d features and k centres (the last extent of its slab).
long siss_kmeans_assign_blocks(long d, int k) { return d > 0 && k >= 1 && k <= 16 ? assign_blocks(d, k) : 0; }

// Row segments of siss_kmeans_update for n rows of d features and k centres: sums is uint32 [segments][k][d], cnts int64 [segments][k].
long siss_kmeans_update_segments(long n, long d, int k) { return n > 0 && d > 0 && k >= 1 && k <= 16 ? update_segments(n, d, k) : 0; }

// The VAE decoder's output to the uint8 image and its partial squared distances to k centres, one pass.  img: [n][3][h][w], f32
// or (bf16 != 0) bf16; u8: uint8 [n][h][w][3] = ((img / 2 + 0.5).clamp(0, 1) * 255).round() rounded as torch rounds each operation
// in img's dtype; centres: f32 [k][h * w * 3] in the same HWC order; slab: f64 [n][k][nblk], nblk = siss_kmeans_decoded_blocks(h * w),
// every entry written.  1 <= k <= 16.  siss_kmeans_finalize turns the slab into distances and labels.
int siss_kmeans_decoded(const void* img, int bf16, const float* centres, int n, int h, int w, int k, uint8_t* u8, double* slab,
                        int nblk, void* stream) {
    SISS_CHECK_ARG(img && centres && u8 && slab && n > 0 && h > 0 && w > 0 && k >= 1 && k <= 16);
    const long hw = (long)h * w;
    SISS_CHECK_ARG(nblk == decoded_blocks(hw));
    const bool vec = hw % 4 == 0 && aligned16(img) && aligned16(centres) && aligned16(u8);
    dim3 grid(n, nblk);
    hipStream_t s = (hipStream_t)stream;
#define KM_CALL(KT)                                                                                                            \
    if (bf16) {                                                                                                                \
        if (vec) decoded_kernel<KT, bf16_t, true><<<grid, kThreads, 0, s>>>((const bf16_t*)img, centres, hw, k, u8, slab);     \
        else decoded_kernel<KT, bf16_t, false><<<grid, kThreads, 0, s>>>((const bf16_t*)img, centres, hw, k, u8, slab);        \
    } else {                                                                                                                   \
        if (vec) decoded_kernel<KT, float, true><<<grid, kThreads, 0, s>>>((const float*)img, centres, hw, k, u8, slab);       \
        else decoded_kernel<KT, float, false><<<grid, kThreads, 0, s>>>((const float*)img, centres, hw, k, u8, slab);          \
    }
    KM_TILES(k, KM_CALL)
#undef KM_CALL
    SISS_LAUNCH_RET();
}

// Slab [n][k][nblk] (f64 partial squared distances) to dist f64 [n][k] (partials summed left to right), labels int32 [n] (argmin,
// lowest index on ties), row_min f64 [n], inertia f64 [1] (sum of the row minima in a fixed order) and the LOW 32-bit word of status
// (int64 [1]): the number of rows whose label differs from the one labels held on entry.  labels, row_min, inertia, status may be
// null.  One block: no atomics.
int siss_kmeans_finalize(const double* slab, long n, int k, int nblk, double* dist, int32_t* labels, double* row_min, double* inertia,
                         int64_t* status, void* stream) {
    SISS_CHECK_ARG(slab && dist && n > 0 && k >= 1 && k <= 16 && nblk >= 1);
    finalize_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(slab, n, k, nblk, dist, labels, row_min, inertia, status);
    SISS_LAUNCH_RET();
}

// Squared distances of uint8 rows [n][d] to k f32 centres [k][d] and their labels: the distance pass into slab (f64 [n][k][nblk],
// nblk = siss_kmeans_assign_blocks(d, k)), then siss_kmeans_finalize's outputs.  1 <= k <= 16 (k = 1: the distance to one centre).
int siss_kmeans_assign(const uint8_t* rows, const float* centres, long n, long d, int k, double* slab, int nblk, double* dist,
                       int32_t* labels, double* row_min, double* inertia, int64_t* status, void* stream) {
    SISS_CHECK_ARG(rows && centres && slab && dist && n > 0 && n <= (1L << 31) - 8 && d > 0 && k >= 1 && k <= 16);
    SISS_CHECK_ARG(nblk == assign_blocks(d, k));
    hipStream_t s = (hipStream_t)stream;
    launch_assign(rows, centres, n, d, k, slab, nblk, s);
    finalize_kernel<<<1, kThreads, 0, s>>>(slab, n, k, nblk, dist, labels, row_min, inertia, status);
    SISS_LAUNCH_RET();
}

// The Lloyd update: centres[kk] = mean of the rows with labels[r] == kk, from exact integer sums taken in row order, as the correctly
// rounded f32 of sum / count; counts int64 [k]; the HIGH 32-bit word of status (int64 [1], may be null) = the number of empty
// clusters, whose centres are left as they were.  rows: uint8 [n][d], n < 2^24; labels: int32 [n] (a value outside [0, k) joins no
// cluster); sums / cnts: scratch of siss_kmeans_update_segments(n, d, k) segments, sized for nseg of them.
int siss_kmeans_update(const uint8_t* rows, const int32_t* labels, long n, long d, int k, float* centres, uint32_t* sums, int64_t* cnts,
                       int nseg, int64_t* counts, int64_t* status, void* stream) {
    SISS_CHECK_ARG(rows && labels && centres && sums && cnts && counts && n > 0 && n < (1L << 24) && d > 0 && k >= 1 && k <= 16);
    SISS_CHECK_ARG(nseg == update_segments(n, d, k));
    const bool vec = d % lane_features(k) == 0 && aligned16(rows) && aligned16(sums);
    const long groups = update_groups(d, k, vec);
    SISS_CHECK_ARG(groups < (1L << 31));
    dim3 grid((unsigned)groups, nseg);
    hipStream_t s = (hipStream_t)stream;
#define KM_CALL(KT)                                                                                           \
    if (vec) update_partial_kernel<KT, true><<<grid, kThreads, 0, s>>>(rows, labels, n, d, k, sums, cnts);    \
    else update_partial_kernel<KT, false><<<grid, kThreads, 0, s>>>(rows, labels, n, d, k, sums, cnts)
    KM_TILES(k, KM_CALL)
#undef KM_CALL
    update_finalize_kernel<<<cdiv(d, kThreads), kThreads, 0, s>>>(sums, cnts, nseg, k, d, centres, counts, status);
    SISS_LAUNCH_RET();
}

}  // extern "C"

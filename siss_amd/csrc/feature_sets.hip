// Pairwise work on feature sets (siss_amd/feature_sets.py: the Kernel Inception Distance and precision / recall / density / coverage
// on the [N, 2048] f32 features the FID's Inception-v3 already produces): squared norms, k-th-neighbour radii, "does this row fall
// inside any ball" with the nearest row, and the cubic polynomial-kernel sums of many subsets.  NOT the reference's protocol, which
// reports FID only.  No N x M matrix is formed: one wave owns a 32 x 64 tile of pairs (sscd_tile of sscd_tile.h, eight
// v_mfma_f32_16x16x4_f32 accumulators), walks its piece of the second set and keeps per row what survives; the pieces of a row are
// folded by a second small kernel.  Everything that is not the k loop (distances, selection, the f64 conversions of the kernel sums)
// runs once per tile, after it.
//
// NUMERIC CONTRACT.
//   dot(a, b)  the f32 fmaf chain over k = 0, 1, ..., d - 1 from +0: the value sscd_tile produces, the only place a product is formed.
//   sq(a)      the sum of the squares in f64 over ascending k (each square is exact in f64), rounded ONCE to f32 (siss_feat_sqnorm).
//   d2(a, b)   fmaxf(0, fmaf(-2, dot(a, b), sq(a) + sq(b))): one f32 value that depends on the two rows and d alone -- not on the tile
//              position, the split into pieces, the entry point or the batch -- and d2(a, b) == d2(b, a) bit for bit.
//   k(a, b)    (gamma * dot(a, b) + coef)^3 in f64 from the f32 dot: t = gamma * (double)dot + coef (two roundings), (t * t) * t.
// The self pair is excluded by INDEX (position, in the kernel sums), never by value.  A NaN distance is never selected and never
// counted (a NaN kernel value is summed: it is the caller's data).  This file is built without a * b + c contraction.
//
// ORDER.  Neighbour candidates are ordered (value ascending, index ascending); each piece keeps its exact k smallest values and the
// fold takes the k smallest of the pieces' lists, so a radius does not depend on the number of pieces.  Counts are integers; minima
// are folded under the same total order; the f64 tile sums of the kernel sums are folded lane tree -> tiles in ascending order.  No
// atomics anywhere: results are independent of the grid and bitwise repeatable.
#include "common.h"
#include "sscd_tile.h"

namespace {

constexpr int kMaxK = 16;
constexpr int kMaxPieces = 256;      // pieces of the second set per row (the radius fold gives each lane at most four lists)
constexpr int kTargetWaves = 2048;   // 256 CUs x 4 SIMDs x 2 waves
constexpr int kTilePitch = kGT + 1;
constexpr int kNone = 0x7fffffff;

// How the second set is cut for (nq, ng): `pieces` contiguous runs of `tpp` wave tiles.  Depends on nq and ng only.
struct Split { int pieces; long tpp; };
static inline Split split_for(long nq, long ng, long waves_per_tile_row = 1) {
    const long ntiles = (ng + kGT - 1) / kGT;
    const long nqt = ((nq + kQT - 1) / kQT) * waves_per_tile_row;
    long want = (kTargetWaves + nqt - 1) / nqt;
    if (want > kMaxPieces) want = kMaxPieces;
    if (want > ntiles) want = ntiles;
    if (want < 1) want = 1;
    Split s;
    s.tpp = (ntiles + want - 1) / want;
    s.pieces = (int)((ntiles + s.tpp - 1) / s.tpp);
    return s;
}

// sq[i] = (float) sum_k (double)x[i][k]^2, k ascending: one lane per row walks it in order.
__global__ __launch_bounds__(64) void feat_sqnorm_kernel(const float* __restrict__ x, int n, int d, float* __restrict__ sq) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* p = x + i * d;
    double s = 0.0;
    for (int k = 0; k < d; k += 4) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (double)v[j] * (double)v[j];
    }
    sq[i] = (float)s;
}

// The distance of a pair from its dot product and the two squared norms; false: NaN (never a candidate).  -0 -> +0.
__device__ __forceinline__ bool dist2(float dot, float sa, float sb, float& v) {
    const float t = fmaf(-2.f, dot, sa + sb);
    v = t > 0.f ? t : 0.f;
    return t == t;
}

// a before b in the neighbour order (value ascending, then index ascending; values are never NaN here)
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) { return av < bv || (av == bv && ai < bi); }

// The k smallest d2(i, j), j != i, j in this piece, per row i -> lists[(i * pieces + piece) * k ...] ascending, unused slots +inf.
__global__ __launch_bounds__(64) void feat_knn_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ sq, int k,
                                                      int pieces, long tpp, float* __restrict__ lists) {
    __shared__ float tile[kQT * kTilePitch];
    __shared__ float lv[kQT * kMaxK];
    __shared__ float kth[kQT];
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int q0 = blockIdx.x * kQT, piece = blockIdx.y;
    const long ntiles = ((long)n + kGT - 1) / kGT;
    const long t_begin = piece * tpp, t_end = t_begin + tpp < ntiles ? t_begin + tpp : ntiles;
    const float inf = __builtin_inff();

    for (int i = lane; i < kQT * k; i += 64) lv[i] = inf;
    if (lane < kQT) kth[lane] = inf;
    __syncthreads();
    float sa[kQS][4];
#pragma unroll
    for (int u = 0; u < kQS; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + 16 * u + 4 * h + r;
            sa[u][r] = sq[qi < n ? qi : n - 1];
        }

    for (long tt = t_begin; tt < t_end; ++tt) {
        const long g0 = tt * kGT;
        f32x4_t acc[kQS][4];
        sscd_tile(x, n, x, n, d, q0, g0, c, h, acc);
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long gi = g0 + 16 * t + c;
            const float sb = sq[gi < n ? gi : n - 1];
#pragma unroll
            for (int u = 0; u < kQS; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qi = q0 + 16 * u + 4 * h + r;
                    float v;
                    const bool ok = dist2(acc[u][t][r], sa[u][r], sb, v) && gi < n && qi < n && gi != qi;
                    acc[u][t][r] = ok ? v : inf;
                    any |= ok && v < kth[16 * u + 4 * h + r];
                }
        }
        if (__ballot(any)) {                         // wave-uniform: some row's list changes
#pragma unroll
            for (int u = 0; u < kQS; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tile[(16 * u + 4 * h + r) * kTilePitch + 16 * t + c] = acc[u][t][r];
            __syncthreads();
            if (lane < kQT) {                        // one lane per row walks its 64 columns in ascending index
                float* v_ = lv + lane * k;
                float last = v_[k - 1];
                for (int j = 0; j < kGT; ++j) {
                    const float v = tile[lane * kTilePitch + j];
                    if (v < last) {                  // equal to the k-th with a larger index: stays out
                        int p = k - 1;
                        while (p > 0 && v_[p - 1] > v) { v_[p] = v_[p - 1]; --p; }
                        v_[p] = v;
                        last = v_[k - 1];
                    }
                }
                kth[lane] = last;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = lane; i < kQT * k; i += 64) {
        const int qi = q0 + i / k;
        if (qi < n) lists[((long)qi * pieces + piece) * k + i % k] = lv[i];
    }
}

// radius[i]: the k-th smallest value of row i's `pieces` ascending lists.  One wave per row, lane l reads the lists l, l + 64, ...;
// per slot the wave takes the first head under (value, piece) and the lane that owned it moves on.  +inf slots are padding, so the
// k-th pick is +inf exactly when fewer than k candidates exist.
__global__ __launch_bounds__(64) void feat_knn_fold_kernel(const float* __restrict__ lists, int pieces, int k, float* __restrict__ radius) {
    const int lane = threadIdx.x;
    const long qi = blockIdx.x;
    const float* mine = lists + qi * pieces * k;
    int head[kMaxPieces / 64] = {0, 0, 0, 0};
    const float inf = __builtin_inff();
    float wv = inf;
    for (int slot = 0; slot < k; ++slot) {
        float bv = inf;
        int bp = kNone, bj = -1;
#pragma unroll
        for (int j = 0; j < kMaxPieces / 64; ++j) {
            const int p = lane + 64 * j;
            if (p < pieces && head[j] < k) {
                const float v = mine[(long)p * k + head[j]];
                if (before(v, p, bv, bp)) { bv = v; bp = p; bj = j; }
            }
        }
        wv = bv;
        int wp = bp;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wv, o, 64);
            const int op = __shfl_xor(wp, o, 64);
            if (before(ov, op, wv, wp)) { wv = ov; wp = op; }
        }
#pragma unroll
        for (int j = 0; j < kMaxPieces / 64; ++j)
            if (j == bj && bp == wp && wp != kNone) ++head[j];
    }
    if (lane == 0) radius[qi] = wv;
}

// Per query row and piece: the number of gallery rows j of the piece with d2(i, j) <= rad[j] (rad != null), the smallest d2(i, j) and
// the lowest j attaining it ((+inf, kNone): no candidate).  All in registers: a lane owns eight query rows x its 4 columns per tile.
__global__ __launch_bounds__(64) void feat_ball_kernel(const float* __restrict__ q, int nq, const float* __restrict__ sq_q,
                                                       const float* __restrict__ g, int ng, const float* __restrict__ sq_g,
                                                       const float* __restrict__ rad, int d, long self0, int pieces, long tpp,
                                                       int* __restrict__ pcnt, float* __restrict__ pmin, int* __restrict__ parg) {
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int q0 = blockIdx.x * kQT, piece = blockIdx.y;
    const long ntiles = ((long)ng + kGT - 1) / kGT;
    const long t_begin = piece * tpp, t_end = t_begin + tpp < ntiles ? t_begin + tpp : ntiles;
    const float inf = __builtin_inff();
    float sa[kQS][4], mv[kQS][4];
    int cnt[kQS][4], mi[kQS][4];
#pragma unroll
    for (int u = 0; u < kQS; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + 16 * u + 4 * h + r;
            sa[u][r] = sq_q[qi < nq ? qi : nq - 1];
            mv[u][r] = inf;
            mi[u][r] = kNone;
            cnt[u][r] = 0;
        }

    for (long tt = t_begin; tt < t_end; ++tt) {
        const long g0 = tt * kGT;
        f32x4_t acc[kQS][4];
        sscd_tile(q, nq, g, ng, d, q0, g0, c, h, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long gi = g0 + 16 * t + c;
            const long gc = gi < ng ? gi : (long)ng - 1;
            const float sb = sq_g[gc];
            const float rj = rad ? rad[gc] : 0.f;
#pragma unroll
            for (int u = 0; u < kQS; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qi = q0 + 16 * u + 4 * h + r;
                    float v;
                    const bool ok = dist2(acc[u][t][r], sa[u][r], sb, v) && gi < ng && qi < nq && !(self0 >= 0 && gi == self0 + qi);
                    cnt[u][r] += ok && rad && v <= rj;
                    if (ok && before(v, (int)gi, mv[u][r], mi[u][r])) { mv[u][r] = v; mi[u][r] = (int)gi; }
                }
        }
    }
#pragma unroll
    for (int u = 0; u < kQS; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int n = cnt[u][r], wi = mi[u][r];
            float wv = mv[u][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {       // the 16 lanes of a query row
                n += __shfl_xor(n, o, 64);
                const float ov = __shfl_xor(wv, o, 64);
                const int oi = __shfl_xor(wi, o, 64);
                if (before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
            }
            const int qi = q0 + 16 * u + 4 * h + r;
            if (c == 0 && qi < nq) {
                const long at = (long)qi * pieces + piece;
                pcnt[at] = n;
                pmin[at] = wv;
                parg[at] = wi;
            }
        }
}

// Per query row: the pieces' counts summed and their minima folded in ascending piece order under (value, index).
__global__ void feat_ball_fold_kernel(const int* __restrict__ pcnt, const float* __restrict__ pmin, const int* __restrict__ parg, int nq,
                                      int pieces, int* __restrict__ inside, float* __restrict__ min_d2, int* __restrict__ argmin) {
    const long qi = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    int n = 0, wi = kNone;
    float wv = __builtin_inff();
    for (int p = 0; p < pieces; ++p) {
        const long at = qi * pieces + p;
        n += pcnt[at];
        if (before(pmin[at], parg[at], wv, wi)) { wv = pmin[at]; wi = parg[at]; }
    }
    if (inside) inside[qi] = n;
    min_d2[qi] = wv;
    argmin[qi] = wi == kNone ? -1 : wi;
}

// blockIdx.z = 3 b + type: subset b, type 0: x against x, 1: y against y, 2: x against y, over the POSITIONS 0 .. s - 1 of the subset's
// row tables.  part[((3 b + type) * nit + i-tile) * pieces + piece]: the f64 sum of k over the wave's pairs (type 0 / 1: position
// i == position j left out), lane sums folded by a fixed xor tree.
__global__ __launch_bounds__(64) void kid_sums_kernel(const float* __restrict__ x, const int* __restrict__ idx_x, const float* __restrict__ y,
                                                      const int* __restrict__ idx_y, int d, int s, double gamma, double coef, int pieces,
                                                      long tpp, double* __restrict__ part) {
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int q0 = blockIdx.x * kQT, piece = blockIdx.y, type = blockIdx.z % 3;
    const long b = blockIdx.z / 3;
    const float* A = type == 1 ? y : x;
    const float* B = type == 0 ? x : y;
    const int* ai = (type == 1 ? idx_y : idx_x) + b * s;
    const int* bi = (type == 0 ? idx_x : idx_y) + b * s;
    const long ntiles = ((long)s + kGT - 1) / kGT;
    const long t_begin = piece * tpp, t_end = t_begin + tpp < ntiles ? t_begin + tpp : ntiles;
    double sum = 0.0;
    for (long tt = t_begin; tt < t_end; ++tt) {
        const long g0 = tt * kGT;
        f32x4_t acc[kQS][4];
        sscd_tile<true>(A, s, B, s, d, q0, g0, c, h, acc, ai, bi);
#pragma unroll
        for (int u = 0; u < kQS; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long pj = g0 + 16 * t + c;
                    const int pi = q0 + 16 * u + 4 * h + r;
                    if (pi < s && pj < s && !(type < 2 && pi == pj)) {
                        const double v = gamma * (double)acc[u][t][r] + coef;
                        sum += (v * v) * v;
                    }
                }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) part[((long)blockIdx.z * gridDim.x + blockIdx.x) * pieces + piece] = sum;
}

// out[z] = the partial sums of (subset, type) z in ascending (i-tile, piece) order.
__global__ void kid_fold_kernel(const double* __restrict__ part, int nz, int per, double* __restrict__ out) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= nz) return;
    double s = 0.0;
    for (int i = 0; i < per; ++i) s += part[(long)z * per + i];
    out[z] = s;
}

static inline bool dim_ok(int d) { return d >= 4 && d <= 4096 && d % 4 == 0; }
static inline long round16(long n) { return ((n + 15) / 16) * 16; }
static inline Split kid_split(int S, int s) { return split_for(s, s, 3L * S); }

}  // namespace

extern "C" {

// sq[n] (f32): per row of x[n][d] (contiguous f32, 16-byte aligned, d % 4 == 0, 4 <= d <= 4096) the sum of its squares taken in f64
// over ascending k and rounded once to f32: the sq(a) of the distances below.
int siss_feat_sqnorm(const float* x, int n, int d, float* sq, void* stream) {
    SISS_CHECK_ARG(x && sq && n >= 1 && dim_ok(d) && (uintptr_t)x % 16 == 0 && (uintptr_t)sq % 4 == 0);
    feat_sqnorm_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(x, n, d, sq);
    SISS_LAUNCH_RET();
}

// Bytes of the work buffer of siss_feat_knn_radius for n rows: k f32 values per (row, piece); the set is cut into at most 256 pieces
// whatever n is, so the size grows with n x pieces x k, never with n x n.  -1: bad argument.
long siss_feat_knn_ws_bytes(int n, int k) {
    if (n < 1 || k < 1 || k > kMaxK) return -1;
    return round16((long)n * split_for(n, n).pieces * k * 4);
}

// radius[n] (f32): per row i of x[n][d] the k-th smallest d2(i, j) over j != i (the self pair is left out by index), 1 <= k <= 16,
// +inf when fewer than k candidates exist.  d2(a, b) = fmaxf(0, fmaf(-2, dot(a, b), sq(a) + sq(b))), dot the f32 fmaf chain over
// ascending k on v_mfma_f32_16x16x4_f32, sq from siss_feat_sqnorm; NaN distances are never selected.  ws: siss_feat_knn_ws_bytes(n, k)
// bytes, 4-byte aligned, overwritten.  Two launches, no atomics, independent of the split, bitwise repeatable.
int siss_feat_knn_radius(const float* x, int n, int d, const float* sq, int k, float* radius, void* ws, long ws_bytes, void* stream) {
    SISS_CHECK_ARG(x && sq && radius && ws && n >= 1 && dim_ok(d) && k >= 1 && k <= kMaxK);
    SISS_CHECK_ARG((uintptr_t)x % 16 == 0 && ((uintptr_t)sq | (uintptr_t)radius | (uintptr_t)ws) % 4 == 0);
    const Split s = split_for(n, n);
    SISS_CHECK_ARG(ws_bytes >= (long)n * s.pieces * k * 4);
    hipStream_t st = (hipStream_t)stream;
    float* lists = reinterpret_cast<float*>(ws);
    feat_knn_kernel<<<dim3((n + kQT - 1) / kQT, s.pieces), 64, 0, st>>>(x, n, d, sq, k, s.pieces, s.tpp, lists);
    feat_knn_fold_kernel<<<n, 64, 0, st>>>(lists, s.pieces, k, radius);
    SISS_LAUNCH_RET();
}

// Bytes of the work buffer of siss_feat_ball_stats for nq query rows against ng rows: 12 bytes per (query, piece), at most 256 pieces
// whatever ng is.  -1: bad argument.
long siss_feat_ball_ws_bytes(int nq, int ng) {
    if (nq < 1 || ng < 1) return -1;
    return round16((long)nq * split_for(nq, ng).pieces * 12);
}

// Per query row i of q[nq][d] against the rows j of g[ng][d] (same layout rules and the same d2 as siss_feat_knn_radius; sq_q / sq_g
// their siss_feat_sqnorm): inside[i] (int32) the number of j with d2(i, j) <= radius_g[j] (radius_g null: inside is not written and
// may be null), min_d2[i] the smallest d2(i, j) (+inf: no candidate) and argmin[i] (int32) the lowest j attaining it (-1: none).
// self0 >= 0: query i IS gallery row self0 + i and that pair is skipped (-1: none).  NaN distances are never counted or selected.
// ws: siss_feat_ball_ws_bytes(nq, ng) bytes, 4-byte aligned, overwritten.  Two launches, no atomics, independent of the split.
int siss_feat_ball_stats(const float* q, int nq, const float* sq_q, const float* g, int ng, const float* sq_g, const float* radius_g, int d,
                         long self0, void* inside, float* min_d2, void* argmin, void* ws, long ws_bytes, void* stream) {
    SISS_CHECK_ARG(q && sq_q && g && sq_g && min_d2 && argmin && ws && nq >= 1 && ng >= 1 && dim_ok(d) && (inside || !radius_g));
    SISS_CHECK_ARG(((uintptr_t)q | (uintptr_t)g) % 16 == 0);
    SISS_CHECK_ARG(((uintptr_t)sq_q | (uintptr_t)sq_g | (uintptr_t)radius_g | (uintptr_t)inside | (uintptr_t)min_d2 | (uintptr_t)argmin |
                    (uintptr_t)ws) % 4 == 0);
    const Split s = split_for(nq, ng);
    const long cells = (long)nq * s.pieces;
    SISS_CHECK_ARG(ws_bytes >= cells * 12);
    hipStream_t st = (hipStream_t)stream;
    int* pcnt = reinterpret_cast<int*>(ws);
    float* pmin = reinterpret_cast<float*>(pcnt + cells);
    int* parg = reinterpret_cast<int*>(pmin + cells);
    feat_ball_kernel<<<dim3((nq + kQT - 1) / kQT, s.pieces), 64, 0, st>>>(q, nq, sq_q, g, ng, sq_g, radius_g, d, self0, s.pieces, s.tpp, pcnt,
                                                                        pmin, parg);
    feat_ball_fold_kernel<<<(nq + 255) / 256, 256, 0, st>>>(pcnt, pmin, parg, nq, s.pieces, radius_g ? reinterpret_cast<int*>(inside) : nullptr,
                                                           min_d2, reinterpret_cast<int*>(argmin));
    SISS_LAUNCH_RET();
}

// Bytes of the work buffer of siss_kid_sums for S subsets of s positions: one f64 per (subset, sum, 32-position tile, piece) -- linear in
// S x s x pieces, never s x s.  -1: bad argument.
long siss_kid_ws_bytes(int S, int s) {
    if (S < 1 || S > 21845 || s < 1) return -1;
    return round16(3L * S * ((s + kQT - 1) / kQT) * kid_split(S, s).pieces * 8);
}

// The kernel sums of the Kernel Inception Distance for S subsets in ONE launch (plus the fold): idx_x / idx_y are [S][s] int32 DEVICE
// row tables into x[nx][d] / y[ny][d] (entries in 0 .. nx - 1 / 0 .. ny - 1: the caller's duty, the rows are read where they lie; a row
// may appear in several subsets), and out[S][3] (f64) holds per subset b the sum over positions i != j of k(x[idx_x[b][i]],
// x[idx_x[b][j]]), the same for y, and the sum over all i, j of k(x[idx_x[b][i]], y[idx_y[b][j]]), with k(a, b) = (gamma dot(a, b) +
// coef)^3 evaluated in f64 from the f32 dot.  The diagonal is left out by POSITION; xx and yy are taken as FULL squares (a 32 x 64
// tile straddles the diagonal unevenly, and the doubled triangle would save a quarter of the products for a mask per tile).  1 <= S <=
// 21845.  ws: siss_kid_ws_bytes(S, s) bytes, 8-byte aligned, overwritten.  f64 tile sums folded in a fixed order, no atomics.
int siss_kid_sums(const float* x, int nx, const void* idx_x, const float* y, int ny, const void* idx_y, int d, int S, int s, double gamma,
                  double coef, double* out, void* ws, long ws_bytes, void* stream) {
    SISS_CHECK_ARG(x && y && idx_x && idx_y && out && ws && nx >= 1 && ny >= 1 && dim_ok(d) && S >= 1 && S <= 21845 && s >= 1);
    SISS_CHECK_ARG(((uintptr_t)x | (uintptr_t)y) % 16 == 0 && ((uintptr_t)idx_x | (uintptr_t)idx_y) % 4 == 0 &&
                   ((uintptr_t)out | (uintptr_t)ws) % 8 == 0);
    const Split sp = kid_split(S, s);
    const int nit = (s + kQT - 1) / kQT;
    SISS_CHECK_ARG(ws_bytes >= 3L * S * nit * sp.pieces * 8);
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    kid_sums_kernel<<<dim3(nit, sp.pieces, 3 * S), 64, 0, st>>>(x, reinterpret_cast<const int*>(idx_x), y, reinterpret_cast<const int*>(idx_y), d,
                                                              s, gamma, coef, sp.pieces, sp.tpp, part);
    kid_fold_kernel<<<(3 * S + 63) / 64, 64, 0, st>>>(part, 3 * S, nit * sp.pieces, out);
    SISS_LAUNCH_RET();
}

}  // extern "C"

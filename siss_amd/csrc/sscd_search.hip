// Dataset-wide SSCD copy search (siss_amd/sscd_search.py): many unit-row queries against a gallery of N unit rows, keeping per query
// the k largest dot products or the ones at or above a threshold.  The nq x ng similarity matrix is never formed: one wave owns a
// 32-query x 64-gallery-row tile (eight v_mfma_f32_16x16x4_f32 accumulators), steps along its piece of the gallery and keeps what
// survives; the pieces of one query are folded by a second small kernel.
//
// NUMERIC CONTRACT.  The similarity of a pair is ONE f32 value that depends on the two rows (and d) and on nothing else: the fmaf
// chain over k = 0, 1, ..., d - 1 from +0, which is what the MFMA computes when it is fed four consecutive k per instruction in
// ascending order.  Every entry point, every nq / ng / k / self0, every tile position and every split of the gallery into pieces
// runs that same chain (sscd_tile of sscd_tile.h is the only place a product is formed), so count_above and fill_above agree and a value
// returned by topk is the value fill_above lists.  A NaN similarity is never selected and never counted; -0 is returned as +0.
//
// ORDER.  (value descending, gallery index ascending) is a total order on the candidates of a query, each piece keeps the exact
// best k of its rows under it and the fold picks the best k of the pieces' lists under it: the result does not depend on the number of
// pieces.  No atomics anywhere; the threshold lists are placed by counts -> exclusive scan -> ballot ranks, in ascending index.
#include "common.h"
#include "sscd_tile.h"           // kQS, kQT, kGT, transpose4, load4, sscd_tile: shared with feature_sets.hip

namespace {

constexpr int kMaxK = 32;
constexpr int kMaxPieces = 256;  // pieces of the gallery per query (the fold gives each lane at most four lists)
constexpr int kTargetWaves = 2048;   // 256 CUs x 4 SIMDs x 2 waves
constexpr int kTilePitch = kGT + 1;

struct Entry { float v; int i; };

// How the gallery is cut for (nq, ng): `pieces` contiguous runs of `tpp` wave tiles.  Depends on nq and ng only.
struct Split { int pieces; long tpp; };
static inline Split split_for(long nq, long ng) {
    const long ntiles = (ng + kGT - 1) / kGT;
    const long nqt = (nq + kQT - 1) / kQT;
    long want = (kTargetWaves + nqt - 1) / nqt;
    if (want > kMaxPieces) want = kMaxPieces;
    if (want > ntiles) want = ntiles;
    if (want < 1) want = 1;
    Split s;
    s.tpp = (ntiles + want - 1) / want;
    s.pieces = (int)((ntiles + s.tpp - 1) / s.tpp);
    return s;
}

// a before b in the result order (value descending, then index ascending; values are never NaN here)
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// MODE 0: the best k of this piece per query -> lists[(query * pieces + piece) * k ...], unused slots (-inf, -1).
// MODE 1: the number of rows at or above thr in this piece -> pcount[query * pieces + piece].
// MODE 2: the rows at or above thr, in ascending index, from pbase[query * pieces + piece] on (a negative base: nothing is written).
template <int MODE>
__global__ __launch_bounds__(64) void sscd_search_kernel(const float* __restrict__ q, int nq, const float* __restrict__ g, long ng, int d,
                                                         int k, float thr, long self0, int pieces, long tpp, Entry* __restrict__ lists,
                                                         int* __restrict__ pcount, const long* __restrict__ pbase,
                                                         int* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ float tile[MODE == 0 ? kQT * kTilePitch : 1];
    __shared__ float lv[MODE == 0 ? kQT * kMaxK : 1];
    __shared__ int li[MODE == 0 ? kQT * kMaxK : 1];
    __shared__ float kth[MODE == 0 ? kQT : 1];
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int q0 = blockIdx.x * kQT, piece = blockIdx.y;
    const long ntiles = (ng + kGT - 1) / kGT;
    const long t_begin = piece * tpp, t_end = t_begin + tpp < ntiles ? t_begin + tpp : ntiles;
    const float ninf = -__builtin_inff();

    if (MODE == 0) {
        for (int i = lane; i < kQT * k; i += 64) { lv[i] = ninf; li[i] = -1; }
        if (lane < kQT) kth[lane] = ninf;
        __syncthreads();
    }
    int cnt[kQS][4] = {};
    long base[kQS][4];
#pragma unroll
    for (int u = 0; u < kQS; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + 16 * u + 4 * h + r;
            base[u][r] = MODE == 2 && qi < nq ? pbase[(long)qi * pieces + piece] : -1;
        }

    for (long tt = t_begin; tt < t_end; ++tt) {
        const long g0 = tt * kGT;
        f32x4_t acc[kQS][4];
        sscd_tile(q, nq, g, ng, d, q0, g0, c, h, acc);
        // a candidate: a real pair, not the excluded self pair, not NaN; -0 -> +0
        bool ok[kQS][4][4];
#pragma unroll
        for (int u = 0; u < kQS; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long gi = g0 + 16 * t + c;
                    const int qi = q0 + 16 * u + 4 * h + r;
                    const float v = acc[u][t][r];
                    ok[u][t][r] = gi < ng && qi < nq && v == v && !(self0 >= 0 && gi == self0 + qi);
                    acc[u][t][r] = v + 0.f;
                }
        if (MODE == 0) {
            bool any = false;
#pragma unroll
            for (int u = 0; u < kQS; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float th = kth[16 * u + 4 * h + r];
#pragma unroll
                    for (int t = 0; t < 4; ++t) any |= ok[u][t][r] && acc[u][t][r] > th;
                }
            if (__ballot(any)) {                     // wave-uniform: some query's list changes
#pragma unroll
                for (int u = 0; u < kQS; ++u)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            tile[(16 * u + 4 * h + r) * kTilePitch + 16 * t + c] = ok[u][t][r] ? acc[u][t][r] : ninf;
                __syncthreads();
                if (lane < kQT) {                    // one lane per query walks its 64 columns in ascending index
                    float* v_ = lv + lane * k;
                    int* i_ = li + lane * k;
                    float last = v_[k - 1];
                    for (int j = 0; j < kGT; ++j) {
                        const float v = tile[lane * kTilePitch + j];
                        if (v > last) {              // equal to the k-th with a larger index: stays out
                            int p = k - 1;
                            while (p > 0 && v_[p - 1] < v) { v_[p] = v_[p - 1]; i_[p] = i_[p - 1]; --p; }
                            v_[p] = v;
                            i_[p] = (int)(g0 + j);
                            last = v_[k - 1];
                        }
                    }
                    kth[lane] = last;
                }
                __syncthreads();
            }
        } else {
#pragma unroll
            for (int u = 0; u < kQS; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool pass = ok[u][t][r] && acc[u][t][r] >= thr;
                        if (MODE == 1) {
                            cnt[u][r] += pass;
                        } else {
                            const unsigned grp = (unsigned)(__ballot(pass) >> (16 * h)) & 0xffffu;   // this query's 16 columns
                            if (pass && base[u][r] >= 0) {
                                const long at = base[u][r] + __popc(grp & ((1u << c) - 1u));
                                out_idx[at] = (int)(g0 + 16 * t + c);
                                out_val[at] = acc[u][t][r];
                            }
                            if (base[u][r] >= 0) base[u][r] += __popc(grp);
                        }
                    }
        }
    }

    if (MODE == 0) {
        __syncthreads();
        for (int i = lane; i < kQT * k; i += 64) {
            const int qi = q0 + i / k;
            if (qi < nq) lists[((long)qi * pieces + piece) * k + i % k] = Entry{lv[i], li[i]};
        }
    } else if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < kQS; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int n = cnt[u][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) n += __shfl_xor(n, o, 64);
                const int qi = q0 + 16 * u + 4 * h + r;
                if (c == 0 && qi < nq) pcount[(long)qi * pieces + piece] = n;
            }
    }
}

// The best k of a query's `pieces` lists (each sorted in the result order): one wave per query, lane l reads the lists l, l + 64, ...;
// per output slot the wave takes the first head in the order and the lane that owned it moves on.
__global__ __launch_bounds__(64) void sscd_fold_kernel(const Entry* __restrict__ lists, int pieces, int k, float* __restrict__ val,
                                                       int* __restrict__ idx) {
    const int lane = threadIdx.x;
    const long qi = blockIdx.x;
    const Entry* mine = lists + qi * pieces * k;
    int head[kMaxPieces / 64] = {0, 0, 0, 0};
    const float ninf = -__builtin_inff();
    for (int slot = 0; slot < k; ++slot) {
        float bv = ninf;
        int bi = 0x7fffffff, bj = -1;
#pragma unroll
        for (int j = 0; j < kMaxPieces / 64; ++j) {
            const int p = lane + 64 * j;
            if (p < pieces && head[j] < k) {
                const Entry e = mine[(long)p * k + head[j]];
                if (e.i >= 0 && before(e.v, e.i, bv, bi)) { bv = e.v; bi = e.i; bj = j; }
            }
        }
        float wv = bv;
        int wi = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wv, o, 64);
            const int oi = __shfl_xor(wi, o, 64);
            if (before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
        }
        if (lane == 0) {
            val[qi * k + slot] = wi == 0x7fffffff ? ninf : wv;
            idx[qi * k + slot] = wi == 0x7fffffff ? -1 : wi;
        }
#pragma unroll
        for (int j = 0; j < kMaxPieces / 64; ++j)
            if (j == bj && bi == wi && wi != 0x7fffffff) ++head[j];
    }
}

// Per query: the pieces' counts summed (counts != null: count_above's result), or turned into the pieces' first output slots from
// offsets[query] (a query whose offsets do not span exactly its count gets -1 everywhere: fill writes nothing for it).
__global__ void sscd_scan_kernel(const int* __restrict__ pcount, int nq, int pieces, int* __restrict__ counts,
                                 const long* __restrict__ offsets, long* __restrict__ pbase) {
    const long qi = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    long total = 0;
    for (int p = 0; p < pieces; ++p) total += pcount[qi * pieces + p];
    if (counts) { counts[qi] = (int)total; return; }
    const long first = offsets[qi];
    const bool good = first >= 0 && offsets[qi + 1] - first == total;
    long run = first;
    for (int p = 0; p < pieces; ++p) {
        pbase[qi * pieces + p] = good ? run : -1;
        run += pcount[qi * pieces + p];
    }
}

static inline bool rows_ok(const float* q, int nq, const float* g, long ng, int d) {
    return q && g && nq >= 1 && ng >= 1 && ng <= 2147483647L && d >= 4 && d <= 4096 && d % 4 == 0 &&
           ((uintptr_t)q | (uintptr_t)g) % 16 == 0;
}
// threshold forms: pbase (8 bytes) then pcount (4 bytes) per (query, piece)
static inline long thr_ws_bytes(long nq, int pieces) { return ((nq * pieces * 12 + 15) / 16) * 16; }

}  // namespace

extern "C" {

// Bytes of the caller-owned work buffer of the three searches below for nq queries against ng rows: the per-(query, piece) lists of k
// (value, index) pairs of siss_sscd_topk, or with k = 0 the per-(query, piece) counts and first slots of the threshold forms.  The
// gallery is cut into at most 256 pieces whatever ng is: the size grows with nq x pieces x k, never with nq x ng.  -1: bad argument.
long siss_sscd_search_ws_bytes(int nq, long ng, int k) {
    if (nq < 1 || ng < 1 || ng > 2147483647L || k < 0 || k > kMaxK) return -1;
    const Split s = split_for(nq, ng);
    return k == 0 ? thr_ws_bytes(nq, s.pieces) : (long)nq * s.pieces * k * (long)sizeof(Entry);
}

// Per query row of q[nq][d] the k rows of g[ng][d] (contiguous f32, 16-byte aligned bases, d % 4 == 0, 4 <= d <= 4096, ng < 2^31) of
// largest dot product, 1 <= k <= 32: val[nq][k] descending, idx[nq][k] (int32) ascending among equal values, slots beyond the
// candidates (-inf, -1).  self0 >= 0: query i IS gallery row self0 + i and that pair is skipped (-1: none).  A similarity is the f32
// fmaf chain over ascending k on v_mfma_f32_16x16x4_f32, a function of the two rows alone; NaN is never selected.  ws:
// siss_sscd_search_ws_bytes(nq, ng, k) bytes, 8-byte aligned, overwritten.  Two launches, no atomics, bitwise repeatable.
int siss_sscd_topk(const float* q, int nq, const float* g, long ng, int d, int k, long self0, float* val, void* idx, void* ws,
                   long ws_bytes, void* stream) {
    SISS_CHECK_ARG(rows_ok(q, nq, g, ng, d) && k >= 1 && k <= kMaxK && val && idx && ws);
    SISS_CHECK_ARG(((uintptr_t)val | (uintptr_t)idx) % 4 == 0 && (uintptr_t)ws % 8 == 0);
    const Split s = split_for(nq, ng);
    SISS_CHECK_ARG(ws_bytes >= (long)nq * s.pieces * k * (long)sizeof(Entry));
    hipStream_t st = (hipStream_t)stream;
    Entry* lists = reinterpret_cast<Entry*>(ws);
    sscd_search_kernel<0><<<dim3((nq + kQT - 1) / kQT, s.pieces), 64, 0, st>>>(q, nq, g, ng, d, k, 0.f, self0, s.pieces, s.tpp, lists,
                                                                             nullptr, nullptr, nullptr, nullptr);
    sscd_fold_kernel<<<nq, 64, 0, st>>>(lists, s.pieces, k, val, reinterpret_cast<int*>(idx));
    SISS_LAUNCH_RET();
}

// counts[nq] (int32): per query the number of gallery rows with similarity >= thr (the same values, exclusion and NaN rule as
// siss_sscd_topk).  ws: siss_sscd_search_ws_bytes(nq, ng, 0) bytes, 8-byte aligned, overwritten.
int siss_sscd_count_above(const float* q, int nq, const float* g, long ng, int d, float thr, long self0, void* counts, void* ws,
                          long ws_bytes, void* stream) {
    SISS_CHECK_ARG(rows_ok(q, nq, g, ng, d) && counts && ws && (uintptr_t)counts % 4 == 0 && (uintptr_t)ws % 8 == 0);
    const Split s = split_for(nq, ng);
    SISS_CHECK_ARG(ws_bytes >= thr_ws_bytes(nq, s.pieces));
    hipStream_t st = (hipStream_t)stream;
    long* pbase = reinterpret_cast<long*>(ws);
    int* pcount = reinterpret_cast<int*>(pbase + (long)nq * s.pieces);
    sscd_search_kernel<1><<<dim3((nq + kQT - 1) / kQT, s.pieces), 64, 0, st>>>(q, nq, g, ng, d, 0, thr, self0, s.pieces, s.tpp, nullptr,
                                                                             pcount, nullptr, nullptr, nullptr);
    sscd_scan_kernel<<<(nq + 255) / 256, 256, 0, st>>>(pcount, nq, s.pieces, reinterpret_cast<int*>(counts), nullptr, nullptr);
    SISS_LAUNCH_RET();
}

// The rows siss_sscd_count_above counted: query i's gallery indices (int32, ascending) and similarities in idx / val
// [offsets[i], offsets[i + 1]), offsets[nq + 1] (int64, DEVICE) the exclusive scan of its counts.  The counts are formed again here
// (ws needs no history), so a query whose span in offsets is not its count is left unwritten.  Same ws as siss_sscd_count_above.
int siss_sscd_fill_above(const float* q, int nq, const float* g, long ng, int d, float thr, long self0, const void* offsets, void* idx,
                         float* val, void* ws, long ws_bytes, void* stream) {
    SISS_CHECK_ARG(rows_ok(q, nq, g, ng, d) && offsets && idx && val && ws);
    SISS_CHECK_ARG(((uintptr_t)offsets | (uintptr_t)ws) % 8 == 0 && ((uintptr_t)idx | (uintptr_t)val) % 4 == 0);
    const Split s = split_for(nq, ng);
    SISS_CHECK_ARG(ws_bytes >= thr_ws_bytes(nq, s.pieces));
    hipStream_t st = (hipStream_t)stream;
    long* pbase = reinterpret_cast<long*>(ws);
    int* pcount = reinterpret_cast<int*>(pbase + (long)nq * s.pieces);
    const dim3 grid((nq + kQT - 1) / kQT, s.pieces);
    sscd_search_kernel<1><<<grid, 64, 0, st>>>(q, nq, g, ng, d, 0, thr, self0, s.pieces, s.tpp, nullptr, pcount, nullptr, nullptr, nullptr);
    sscd_scan_kernel<<<(nq + 255) / 256, 256, 0, st>>>(pcount, nq, s.pieces, nullptr, reinterpret_cast<const long*>(offsets), pbase);
    sscd_search_kernel<2><<<grid, 64, 0, st>>>(q, nq, g, ng, d, 0, thr, self0, s.pieces, s.tpp, nullptr, nullptr, pbase,
                                              reinterpret_cast<int*>(idx), val);
    SISS_LAUNCH_RET();
}

}  // extern "C"

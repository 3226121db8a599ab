// Gradient-feature data attribution (siss_amd/attribution.py, tools/attribute.py; TRAK, Park et al., ICML 2023; D-TRAK, Zheng et
// al., ICLR 2024; no counterpart in the reference, which names training images by hand): the random projection of the whole flat
// gradient buffer to k dimensions, out = R^T g / sqrt(k), with the n x k Rademacher matrix R never in memory.
//
// R[i, j] = 1 - 2 * ((w >> (i & 31)) & 1), i the FLAT offset (64-bit), j the column, from a counter hash (mix = lowbias32):
//     h = mix(seed ^ 0x9E3779B9);  h = mix(h ^ lo32(i >> 5));  h = mix(h ^ hi32(i >> 5) ^ 0x85EBCA6B);  w = mix(h + j * 0x9E3779B1)
// The first three rounds depend on (seed, i >> 5): one lane forms them once per 32 floats, while the chunk is staged.  The last round is
// per column and per 32 signs.
//
// Layout: a lane per column (four columns a lane, 256 a wave, one wave a block); a CHUNK of kJlChunk consecutive floats of the flat
// index space, cut at multiples of kJlChunk, is staged in LDS with zeros outside [0, n) and outside the listed stretches, next to the
// packed signs of its floats (a ballot while staging) and the group hashes.  The sign of g[i] * R[i, j] is sign(g[i]) ^ bit: the 32
// signs of a group are XORed into w ONCE, and an element costs a shift, a v_bfi (magnitude of g under that sign) and an add per
// column; g itself is wave-uniform and read from LDS as a broadcast.  Per chunk and column ONE f32 partial, summed in ascending i;
// a block folds the partials of its run of consecutive chunks (a SUPER-CHUNK, a function of n alone) into f64 in ascending order and
// writes one row of `ws`; a second kernel folds the rows in ascending order, divides by sqrt(k) in f64 and rounds once.  A zero adds
// +-0 to a sum that is never -0, so a skipped float, a skipped chunk and a zeroed float give the same bits: a subset's projection IS
// the full projection of the gradient zeroed elsewhere.  No atomics; the grid is a function of (n, k): bitwise repeatable.
#include "common.h"

namespace {

constexpr int kJlChunk = 1024;           // floats whose signed sum is formed in f32
constexpr int kJlGroups = kJlChunk / 32;
constexpr int kJlCols = 4;               // columns a lane
constexpr int kJlTile = 64 * kJlCols;    // columns a block
constexpr long kJlMaxRows = 4096;        // rows of `ws` at the most
constexpr long kJlMaxN = 1L << 40;

__host__ __device__ __forceinline__ uint32_t jl_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the magnitude of `bits` under the top bit of `sign`: (bits & 0x7fffffff) | (sign & 0x80000000) in one v_bfi_b32 (written out, the
// compiler splits it into an AND and an OR per column)
__device__ __forceinline__ float jl_signed(uint32_t bits, uint32_t sign) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(0x7fffffffu), "v"(bits), "v"(sign));
    return __uint_as_float(r);
}

// chunks a super-chunk: 64, doubled until at most kJlMaxRows rows remain
inline long jl_chunks(long n) { return (n + kJlChunk - 1) / kJlChunk; }
inline long jl_super(long n) {
    long sc = 64;
    while ((jl_chunks(n) + sc - 1) / sc > kJlMaxRows) sc *= 2;
    return sc;
}
inline long jl_rows(long n) { const long sc = jl_super(n); return (jl_chunks(n) + sc - 1) / sc; }

struct JlCall {
    const float* g;
    long n;
    const long* tab;       // NULL: [0, n); else n_ranges starts, then n_ranges + 1 prefix sums (granules of 4 floats), ascending
    int n_ranges;
    int k;
    uint32_t seed_hash;    // mix(seed ^ 0x9E3779B9)
    long super;            // chunks a block
    long chunks;
};

// [a, b) of stretch r in floats, clamped to the buffer
__device__ __forceinline__ void jl_stretch(const JlCall& c, int r, long& a, long& b) {
    if (!c.tab) { a = 0; b = c.n; return; }
    a = 4 * c.tab[r];
    b = a + 4 * (c.tab[c.n_ranges + r + 1] - c.tab[c.n_ranges + r]);
    if (a < 0) a = 0;
    if (b > c.n) b = c.n;
}

__global__ __launch_bounds__(64) void jl_project_kernel(const JlCall c, double* __restrict__ ws) {
    __shared__ float sg[kJlChunk];
    __shared__ uint32_t ssign[kJlGroups];
    __shared__ uint32_t shash[kJlGroups];
    const int lane = threadIdx.x;
    const int nr = c.tab ? c.n_ranges : 1;
    uint32_t jm[kJlCols];
    double acc[kJlCols];
#pragma unroll
    for (int q = 0; q < kJlCols; ++q) {
        jm[q] = (uint32_t)(blockIdx.y * kJlTile + q * 64 + lane) * 0x9E3779B1u;
        acc[q] = 0.0;
    }
    const long first = (long)blockIdx.x * c.super;
    long last = first + c.super;
    if (last > c.chunks) last = c.chunks;
    int lo = 0;
    for (int hi = nr; lo < hi;) {                              // the last stretch that starts at or before the block's first float, or 0
        const int mid = (lo + hi) >> 1;
        long a, b;
        jl_stretch(c, mid, a, b);
        if (b > first * kJlChunk) hi = mid; else lo = mid + 1;
    }
    for (long ch = first; ch < last; ++ch) {
        const long c0 = ch * kJlChunk, c1 = c0 + kJlChunk;
        // the first stretch that ends after c0 (the stretches ascend, and so do the chunks): uniform, every lane walks the same steps
        for (long a, b; lo < nr; ++lo) {
            jl_stretch(c, lo, a, b);
            if (b > c0) break;
        }
        long a, b;
        if (lo < nr) jl_stretch(c, lo, a, b);
        if (lo >= nr || a >= c1) continue;                     // no float of this chunk is listed: its partial is +0
        __syncthreads();                                       // (one wave: orders the LDS reads of the last chunk before these writes)
#pragma unroll
        for (int t = 0; t < kJlChunk / 64; ++t) sg[t * 64 + lane] = 0.f;
        __syncthreads();
        for (int r = lo; r < nr; ++r) {
            jl_stretch(c, r, a, b);
            if (a >= c1) break;
            if (a < c0) a = c0;
            if (b > c1) b = c1;
            for (long i = a + lane; i < b; i += 64) sg[i - c0] = c.g[i];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kJlChunk / 64; ++t) {
            const unsigned long long neg = __ballot(__float_as_uint(sg[t * 64 + lane]) >> 31);
            if (lane == 0) { ssign[2 * t] = (uint32_t)neg; ssign[2 * t + 1] = (uint32_t)(neg >> 32); }
        }
        if (lane < kJlGroups) {
            const unsigned long long grp = (unsigned long long)(c0 >> 5) + lane;
            uint32_t h = jl_mix(c.seed_hash ^ (uint32_t)grp);
            shash[lane] = jl_mix(h ^ (uint32_t)(grp >> 32) ^ 0x85EBCA6Bu);
        }
        __syncthreads();
        float part[kJlCols];
#pragma unroll
        for (int q = 0; q < kJlCols; ++q) part[q] = 0.f;
        for (int grp = 0; grp < kJlGroups; ++grp) {
            const uint32_t h = __builtin_amdgcn_readfirstlane(shash[grp]);
            const uint32_t neg = __builtin_amdgcn_readfirstlane(ssign[grp]);
            uint32_t w[kJlCols];
#pragma unroll
            for (int q = 0; q < kJlCols; ++q) w[q] = jl_mix(h + jm[q]) ^ neg;
#pragma unroll
            for (int e = 0; e < 32; e += 4) {
                const f32x4_t g4 = *reinterpret_cast<const f32x4_t*>(&sg[grp * 32 + e]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t bits = __float_as_uint(g4[u]);            // (the same in every lane: a broadcast read)
#pragma unroll
                    for (int q = 0; q < kJlCols; ++q) part[q] += jl_signed(bits, w[q] << (31 - (e + u)));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kJlCols; ++q) acc[q] += (double)part[q];
    }
#pragma unroll
    for (int q = 0; q < kJlCols; ++q) {
        const int j = blockIdx.y * kJlTile + q * 64 + lane;
        if (j < c.k) ws[(long)blockIdx.x * c.k + j] = acc[q];
    }
}

// out[j] = (float)((row 0 + row 1 + ... in f64) / sqrt(k)): one thread a column
__global__ __launch_bounds__(64) void jl_fold_kernel(const double* __restrict__ ws, long rows, int k, double root_k,
                                                      float* __restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= k) return;
    double s = 0.0;
    for (long r = 0; r < rows; ++r) s += ws[r * k + j];
    out[j] = (float)(s / root_k);
}

}  // namespace

extern "C" {

// The number of consecutive floats of the flat buffer whose signed sum siss_jl_project forms in f32 (a chunk; chunks are cut at
// multiples of it in the flat index space).
int siss_jl_chunk(void) { return kJlChunk; }

// Bytes of the caller-owned workspace `ws` of siss_jl_project for a buffer of n floats and k columns (one f64 row of k per
// super-chunk: 64 chunks, doubled until at most 4096 rows remain); 0 for an n or k the projection refuses.
long siss_jl_ws_bytes(long n, int k) {
    if (n <= 0 || n > kJlMaxN || k < 32 || k > 8192 || k % 32) return 0;
    return jl_rows(n) * k * (long)sizeof(double);
}

// out[j] = (float)((sum_i R[i, j] g[i]) / sqrt(k)) for j < k: the Rademacher projection of a flat f32 buffer of n floats, R[i, j] =
// 1 - 2 * ((w >> (i & 31)) & 1) with h = mix(seed ^ 0x9E3779B9); h = mix(h ^ lo32(i >> 5)); h = mix(h ^ hi32(i >> 5) ^ 0x85EBCA6B);
// w = mix(h + j * 0x9E3779B1) in u32 arithmetic, mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
// table == NULL (then n_ranges = 0): the sum runs over [0, n).  Else `table` is a DEVICE table in siss_zero_ranges' form (n_ranges
// starts, then the n_ranges + 1 prefix sums of the lengths; longs, 16-byte granules), ASCENDING and not overlapping; the sum runs
// over the listed stretches only, nothing else is read, and i stays the flat offset: the result is, bit for bit, the projection of the
// buffer zeroed outside the stretches.  Per chunk of siss_jl_chunk() floats one f32 partial per column, summed in ascending i; the
// partials are folded in f64 in ascending order, divided by sqrt(k) in f64 and rounded once.  No atomics; the grid is a function of
// (n, k): bitwise repeatable.  g and out 16-byte aligned, ws 8-byte aligned with ws_bytes >= siss_jl_ws_bytes(n, k); k % 32 == 0,
// 32 <= k <= 8192; 0 < n <= 2^40; 0 <= seed < 2^32.  Only out[0:k] and ws[0:siss_jl_ws_bytes) are written.  Bad arguments return 1
// before any launch.
int siss_jl_project(const float* g, long n, const long* table, int n_ranges, int k, long seed, double* ws, long ws_bytes,
                    float* out, void* stream) {
    SISS_CHECK_ARG(g && ws && out && n > 0 && n <= kJlMaxN);
    SISS_CHECK_ARG(k >= 32 && k <= 8192 && k % 32 == 0);
    SISS_CHECK_ARG(seed >= 0 && seed <= 0xffffffffL);
    SISS_CHECK_ARG(table ? n_ranges > 0 : n_ranges == 0);
    SISS_CHECK_ARG(((uintptr_t)g | (uintptr_t)out) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)table) % 8 == 0);
    SISS_CHECK_ARG(ws_bytes >= siss_jl_ws_bytes(n, k));
    hipStream_t s = (hipStream_t)stream;
    const long rows = jl_rows(n);
    const JlCall call{g, n, table, n_ranges, k, jl_mix((uint32_t)seed ^ 0x9E3779B9u), jl_super(n), jl_chunks(n)};
    jl_project_kernel<<<dim3((unsigned)rows, (unsigned)((k + kJlTile - 1) / kJlTile)), 64, 0, s>>>(call, ws);
    jl_fold_kernel<<<(k + 63) / 64, 64, 0, s>>>(ws, rows, k, sqrt((double)k), out);
    SISS_LAUNCH_RET();
}

}  // extern "C"

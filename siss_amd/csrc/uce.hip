// Unified Concept Editing (UCE, Gandikota, Orgad, Belinkov, Materzynska & Bau, WACV 2024; siss_amd/uce.py, `deletion.uce`; no
// counterpart in the reference, whose runs unlearn by gradient steps only).  The closed-form edit of the cross-attention key / value
// projections is W' = W + W dT with ONE X x X matrix dT shared by every edited weight W [C, X] (siss_amd/uce.py forms it in f64 on the
// host and hands over E = dT^T, rounded once to f32, [X, X] row-major):
//   siss_uce_delta   delta[r, j] = <W[r, :], E[j, :]> for every target of a job table, into a compact buffer [sum rows, X] -- out of
//                    place on purpose: a tile reads whole weight rows that other tiles of the same stripe also read
//   siss_uce_apply   p <- p + delta over the targets' floats only (one f32 add), and four f64 statistics of that (or, apply = 0, of
//                    what it would do)
// NUMERIC CONTRACT.  A delta value is the f32 fmaf chain over k = 0, 1, ..., X - 1 from +0 (sscd_tile of sscd_tile.h, unchanged: the
// only place a product is formed): a function of the two rows and X alone, not of the grid or of how tiles map to jobs.  The add is one
// round-to-nearest f32 addition (this file is built without a * b + c contraction).  The statistics fold in a fixed order (one f64 row
// per chunk of kUceChunk floats, one block folds the rows); no atomics: bitwise repeatable.
// JOB TABLE.  A HOST array of 64-byte rows, one per target tensor: {long w_off (floats into p, a multiple of 4); long row_off (the
// target's first row of delta); int rows; int pad; long reserved[5]}.  The launchers check it, derive the tile / chunk prefix sums and
// pass it to the kernels BY VALUE, kUceBatch targets a launch (SD v1.5 has 32: one launch).
#include "common.h"
#include "sscd_tile.h"

namespace {

constexpr int kUceBatch = 64;            // targets per kernel launch (their device rows travel as kernel arguments: 64 x 24 bytes)
constexpr int kUceThreads = 256;
constexpr int kUceChunk = 4096;          // floats of a target per block of the apply pass: 256 threads x 4 granules of 4
constexpr int kUceStats = 4;             // one row per chunk, and the result block: 4 doubles
enum { UCE_SUM_DELTA2 = 0, UCE_SUM_P2, UCE_MAX_DELTA, UCE_FLOATS };

struct UceJob {                          // siss_amd/uce.py job_table: 64 bytes
    long w_off, row_off;
    int rows, pad;
    long reserved[5];
};
static_assert(sizeof(UceJob) == 64, "job rows");

struct UceDevJob {                       // what a kernel needs of a target; first: its first tile (delta) / chunk (apply) of the launch
    long w_off, row_off;
    int rows, first;
};
struct UceBatch {
    UceDevJob j[kUceBatch];
    int n;
};

__device__ __forceinline__ int uce_find(const UceBatch& b, int unit) {
    int lo = 0, hi = b.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b.j[mid].first <= unit) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One wave per 32 x 64 tile of a target's delta; the column tiles of a row stripe are neighbours (they share the weight rows).
__global__ __launch_bounds__(kUceThreads) void uce_delta_kernel(const float* __restrict__ p, const UceBatch b, int total_tiles,
                                                                const float* __restrict__ E, int X, float* __restrict__ delta) {
    const int tile = blockIdx.x * (kUceThreads / 64) + (threadIdx.x >> 6);
    if (tile >= total_tiles) return;                              // (wave-uniform)
    const UceDevJob jb = b.j[uce_find(b, tile)];
    const int ct = (X + kGT - 1) / kGT, lt = tile - jb.first;
    const int q0 = (lt / ct) * kQT;
    const long g0 = (long)(lt % ct) * kGT;
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    f32x4_t acc[kQS][4];
    sscd_tile(p + jb.w_off, jb.rows, E, (long)X, X, q0, g0, c, h, acc);
    float* out = delta + jb.row_off * X;
#pragma unroll
    for (int u = 0; u < kQS; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = q0 + 16 * u + 4 * h + r;
                const long gi = g0 + 16 * t + c;
                if (qi < jb.rows && gi < X) out[(long)qi * X + gi] = acc[u][t][r];
            }
}

// One block per chunk of kUceChunk floats of a target: p + delta (stored when apply), and the chunk's row of `partials`.
__global__ __launch_bounds__(kUceThreads) void uce_apply_kernel(float* __restrict__ p, const UceBatch b, int X,
                                                                const float* __restrict__ delta, int apply,
                                                                double* __restrict__ partials) {
    __shared__ double sh[3 * kUceThreads / 64];
    const UceDevJob jb = b.j[uce_find(b, blockIdx.x)];
    const long n = (long)jb.rows * X;                             // (a multiple of 4: X is)
    const long i0 = (long)(blockIdx.x - jb.first) * kUceChunk;
    float* w = p + jb.w_off;
    const float* d = delta + jb.row_off * X;
    double sd = 0, sp = 0;
    float mx = 0.f;
#pragma unroll
    for (int g = 0; g < kUceChunk / (4 * kUceThreads); ++g) {
        const long i = i0 + 4l * (g * kUceThreads + threadIdx.x);
        if (i < n) {
            f32x4_t pp = *reinterpret_cast<const f32x4_t*>(w + i);
            const f32x4_t dd = *reinterpret_cast<const f32x4_t*>(d + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sd += (double)dd[j] * (double)dd[j];
                sp += (double)pp[j] * (double)pp[j];
                mx = fmaxf(mx, fabsf(dd[j]));
                pp[j] = __fadd_rn(pp[j], dd[j]);
            }
            if (apply) *reinterpret_cast<f32x4_t*>(w + i) = pp;
        }
    }
    // lanes -> waves -> one row per chunk, fixed order
    sd = wave_sum_d(sd);
    sp = wave_sum_d(sp);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[3 * wv] = sd; sh[3 * wv + 1] = sp; sh[3 * wv + 2] = (double)mx; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double a = 0, c = 0, m = 0;
    for (int i = 0; i < kUceThreads / 64; ++i) { a += sh[3 * i]; c += sh[3 * i + 1]; m = fmax(m, sh[3 * i + 2]); }
    const long left = n - i0;
    double* row = partials + (long)kUceStats * blockIdx.x;
    row[UCE_SUM_DELTA2] = a;
    row[UCE_SUM_P2] = c;
    row[UCE_MAX_DELTA] = m;
    row[UCE_FLOATS] = (double)(left < kUceChunk ? left : kUceChunk);
}

// ONE block folds the chunk rows (fixed lane -> index map, as ssd_finish_kernel does) and writes the four statistics
__global__ __launch_bounds__(kUceThreads) void uce_finish_kernel(const double* __restrict__ partials, long nrows,
                                                                 double* __restrict__ stats) {
    __shared__ double sh[kUceStats * kUceThreads / 64];
    double s[kUceStats] = {0, 0, 0, 0};
    for (long i = threadIdx.x; i < nrows; i += kUceThreads) {
        const double* row = partials + kUceStats * i;
        s[UCE_SUM_DELTA2] += row[UCE_SUM_DELTA2];
        s[UCE_SUM_P2] += row[UCE_SUM_P2];
        s[UCE_MAX_DELTA] = fmax(s[UCE_MAX_DELTA], row[UCE_MAX_DELTA]);
        s[UCE_FLOATS] += row[UCE_FLOATS];
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kUceStats; ++j) {
        double t = s[j];
        if (j == UCE_MAX_DELTA) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t = fmax(t, __shfl_xor(t, o, 64));
        } else {
            t = wave_sum_d(t);
        }
        if ((threadIdx.x & 63) == 0) sh[kUceStats * w + j] = t;
    }
    __syncthreads();
    if (threadIdx.x >= kUceStats) return;
    double a = 0;
    for (int i = 0; i < kUceThreads / 64; ++i) {
        const double t = sh[kUceStats * i + threadIdx.x];
        a = threadIdx.x == UCE_MAX_DELTA ? fmax(a, t) : a + t;
    }
    stats[threadIdx.x] = a;
}

inline bool uce_overlap(const float* a, long na, const float* b, long nb) { return a < b + nb && b < a + na; }

inline long uce_chunks(const UceJob& j, int X) { return ((long)j.rows * X + kUceChunk - 1) / kUceChunk; }

// What both entry points refuse about a job table: a row count <= 0, an offset that is negative or off a 16-byte line, two targets
// that share rows of delta, and `other` (E; nullptr: none) or delta overlapping a target's floats.  The units (tiles or chunks) of
// the whole table must fit an int.
inline bool uce_table_ok(const float* p, const UceJob* jobs, int njobs, int X, const float* delta, const float* other, long other_n) {
    long tiles = 0, chunks = 0;
    for (int i = 0; i < njobs; ++i) {
        const UceJob& a = jobs[i];
        if (a.rows <= 0 || a.w_off < 0 || a.w_off % 4 != 0 || a.row_off < 0) return false;
        const long n = (long)a.rows * X;
        if (uce_overlap(p + a.w_off, n, delta + a.row_off * X, n)) return false;
        if (other && uce_overlap(p + a.w_off, n, other, other_n)) return false;
        for (int k = 0; k < njobs; ++k) {
            const UceJob& o = jobs[k];
            if (k != i && a.row_off < o.row_off + o.rows && o.row_off < a.row_off + a.rows) return false;
            if (o.rows > 0 && uce_overlap(p + a.w_off, n, delta + o.row_off * X, (long)o.rows * X)) return false;
        }
        tiles += (long)((a.rows + kQT - 1) / kQT) * ((X + kGT - 1) / kGT);
        chunks += uce_chunks(a, X);
    }
    return tiles < (1l << 30) && chunks < (1l << 30);
}

}  // namespace

extern "C" {

// Words (doubles) of the caller-owned slab `partials` of siss_uce_apply for targets of `floats` floats in all in `njobs` jobs: one row
// of 4 per chunk of 4096 floats of a target (a target's last chunk may be partial).
long siss_uce_partials_words(long floats, int njobs) {
    if (floats < 0 || njobs < 0) return 0;
    return (long)kUceStats * (floats / kUceChunk + njobs);
}

// delta[row_off_t + r, j] = <p[w_off_t + r X ..], E[j, :]> for every target t of the HOST job table `jobs` (njobs rows of 64 bytes:
// {long w_off, row_off; int rows, pad; long reserved[5]}), r < rows_t, j < X: the f32 fmaf chain over k = 0 .. X - 1 from +0.  p: the
// flat f32 parameter buffer (read only); E [X, X] f32 row-major; delta [sum of rows, X] f32; rows of delta no job names are not
// written.  Refused, writing nothing: X < 4 or X % 4 != 0, p / E / delta off a 16-byte line, njobs <= 0, a job with rows <= 0 or with
// an offset that is negative or (w_off) no multiple of 4, two jobs sharing rows of delta, delta or E overlapping a target's floats.
int siss_uce_delta(const float* p, const void* jobs, int njobs, const float* E, int X, float* delta, void* stream) {
    SISS_CHECK_ARG(p && jobs && E && delta && njobs > 0 && X >= 4 && X % 4 == 0);
    SISS_CHECK_ARG(((uintptr_t)p | (uintptr_t)E | (uintptr_t)delta) % 16 == 0);
    const UceJob* jt = static_cast<const UceJob*>(jobs);
    SISS_CHECK_ARG(uce_table_ok(p, jt, njobs, X, delta, E, (long)X * X));
    for (int i = 0; i < njobs; ++i)                              // (delta's extent is the jobs' rows)
        SISS_CHECK_ARG(!uce_overlap(E, (long)X * X, delta + jt[i].row_off * X, (long)jt[i].rows * X));
    const int ct = (X + kGT - 1) / kGT;
    for (int j0 = 0; j0 < njobs; j0 += kUceBatch) {
        UceBatch b;
        b.n = njobs - j0 < kUceBatch ? njobs - j0 : kUceBatch;
        int tiles = 0;
        for (int i = 0; i < b.n; ++i) {
            const UceJob& a = jt[j0 + i];
            b.j[i] = UceDevJob{a.w_off, a.row_off, a.rows, tiles};
            tiles += ((a.rows + kQT - 1) / kQT) * ct;
        }
        const int wpb = kUceThreads / 64;
        uce_delta_kernel<<<(tiles + wpb - 1) / wpb, kUceThreads, 0, (hipStream_t)stream>>>(p, b, tiles, E, X, delta);
    }
    SISS_LAUNCH_RET();
}

// p[w_off_t + i] += delta[row_off_t X + i] for i < rows_t X of every target t of the HOST job table (siss_uce_delta's): one f32
// round-to-nearest add; every other float of p -- the alignment padding between the targets included -- keeps its bits.  apply = 0:
// nothing is written to p (a dry run with the same statistics).  `partials`: siss_uce_partials_words(sum of rows_t X, njobs) doubles
// of scratch.  `stats` (DEVICE, 4 doubles, all written): [0] the sum of delta^2, [1] the sum of p^2 BEFORE the edit, [2] max |delta|,
// [3] the float count -- all over the targets' floats, squares formed in f64 from the f32 values, one row per chunk of 4096 floats
// folded by one block in a fixed order.  Refused, writing nothing: as siss_uce_delta (there is no E here).
int siss_uce_apply(float* p, const void* jobs, int njobs, int X, const float* delta, int apply, double* partials, double* stats,
                   void* stream) {
    SISS_CHECK_ARG(p && jobs && delta && partials && stats && njobs > 0 && X >= 4 && X % 4 == 0);
    SISS_CHECK_ARG(((uintptr_t)p | (uintptr_t)delta) % 16 == 0 && ((uintptr_t)partials | (uintptr_t)stats) % 8 == 0);
    const UceJob* jt = static_cast<const UceJob*>(jobs);
    SISS_CHECK_ARG(uce_table_ok(p, jt, njobs, X, delta, nullptr, 0));
    hipStream_t s = (hipStream_t)stream;
    long row0 = 0;
    for (int j0 = 0; j0 < njobs; j0 += kUceBatch) {
        UceBatch b;
        b.n = njobs - j0 < kUceBatch ? njobs - j0 : kUceBatch;
        int chunks = 0;
        for (int i = 0; i < b.n; ++i) {
            const UceJob& a = jt[j0 + i];
            b.j[i] = UceDevJob{a.w_off, a.row_off, a.rows, chunks};
            chunks += (int)uce_chunks(a, X);
        }
        uce_apply_kernel<<<chunks, kUceThreads, 0, s>>>(p, b, X, delta, apply != 0, partials + kUceStats * row0);
        row0 += chunks;
    }
    uce_finish_kernel<<<1, kUceThreads, 0, s>>>(partials, row0, stats);
    SISS_LAUNCH_RET();
}

}  // extern "C"

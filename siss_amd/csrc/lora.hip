// LoRA unlearning on the UNet's linear projections and 3x3 convolutions (siss_amd/lora.py): the chain rule through W = W0 + s B A
// and the merge.
//
// The engine runs on the merged weight, so its dual-cotangent backward leaves dW_k [O, I] (f32) of every target in the flat gradient
// buffer.  Both kernels are driven by ONE device job table (a row per target: where its weight, its A [r, I], its B [O, r] and its W0
// lie, O, I, and the first tile it owns in each kernel) and cover every target in one launch:
//   - lora_project_kernel: dB_k = s dW_k A^T and dA_k = s B^T dW_k for both gradient sets.  A target owns ceil(O / 64) ROW tiles (a wave
//     per 16 rows of dW: the whole reduction over I, dB rows written once) followed by ceil(I / 64) COLUMN tiles (a wave per 16 columns:
//     the whole reduction over O, dA columns written once) -- dW is read twice, nothing is summed across blocks, no atomics: the same
//     call gives the same bits.  Outputs are OVERWRITTEN (gradient accumulation has happened in dW).
//   - lora_merge_kernel: W = W0 + s B A on 64 x 64 tiles of every target, written to the f32 master and (bf16 engine) as its
//     round-to-nearest-even cast to the operand shadow; no byte outside the targets' [O, I] stretches is touched.
// Products on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per output), operands straight from global memory in the MFMA
// operand layout (lane = 16 q + li: row / column li, k = 4 q ...): A and B are small and stay in the caches, dW and W0 stream.
// Tails (O, I no multiple of the tile, r no multiple of 16) are zero operands and masked stores.  No launcher synchronises.
//
// A 3x3 convolution (siss_lora_project_conv / siss_lora_merge_conv; peft's Conv2d adapter in the native tap-major layout) is the same
// code with T = 9 taps: W [T, O, I], A [T, r, I], W0 [T, O, I] a tap after the other (tap strides O I resp. r I floats), B [O, r]
// shared by the taps: W[t] = W0[t] + s B A[t].  Its job row is 64 bytes: the 48 bytes of the linear row {long w_off, a_off, b_off,
// w0_off; int O, I, ptile0, mtile0} followed by {int taps; int pad[3]} (pad = 0).  A conv target owns ceil(O / 64) row tiles (dB: ONE
// reduction of length T I, t ascending and within a tap i ascending) followed by T ceil(I / 64) column tiles (dA[t], tap-major) in
// the projection and T ceil(O / 64) ceil(I / 64) tiles (tap-major) in the merge.  The linear kernels are the T = 1 instance.
#include "common.h"

namespace {

constexpr int kTile = 64;          // rows (columns) of a target a block owns; a wave owns 16 of them

struct LoraJob {                   // siss_amd/lora.py job_table: 48 bytes
    long w_off, a_off, b_off, w0_off;          // floats: flat parameter / gradient buffer, LoRA buffer (A, B), packed W0
    int O, I, ptile0, mtile0;                  // first tile of the target in the project / merge launch
};
struct LoraConvJob {               // siss_amd/lora.py conv_job_table: 64 bytes
    long w_off, a_off, b_off, w0_off;
    int O, I, ptile0, mtile0;
    int taps, pad[3];                          // W [taps, O, I], A [taps, r, I], W0 [taps, O, I]; B [O, r] shared
};
static_assert(sizeof(LoraJob) == 48 && sizeof(LoraConvJob) == 64, "job rows");
__device__ __forceinline__ int job_taps(const LoraJob&) { return 1; }
__device__ __forceinline__ int job_taps(const LoraConvJob& j) { return j.taps; }

template <bool MERGE, class Job>
__device__ __forceinline__ int find_job(const Job* jobs, int njobs, int tile) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((MERGE ? jobs[mid].mtile0 : jobs[mid].ptile0) <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

constexpr f32x4_t kZero = {0.f, 0.f, 0.f, 0.f};

// row[k .. k + 3] with zeros past `len` (or for a row that does not exist); vec: len % 4 == 0 and a 16-byte aligned row
__device__ __forceinline__ f32x4_t ld_k4(const float* row, int k, int len, bool ok, bool vec) {
    if (!ok || k >= len) return kZero;
    if (vec) return *reinterpret_cast<const f32x4_t*>(row + k);
    f32x4_t v = kZero;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (k + j < len) v[j] = row[k + j];
    return v;
}

// NT = ceil(r / 16): 16-wide tiles of the rank dimension a wave accumulates
template <int NT, class Job>
__global__ __launch_bounds__(256) void lora_project_kernel(const float* __restrict__ grads, long set_stride, int nsets,
                                                           const float* __restrict__ lora_p, float* __restrict__ lora_g,
                                                           long lora_set_stride, const Job* __restrict__ jobs, int njobs, int r,
                                                           float s) {
    const int tile = blockIdx.x, set = blockIdx.y;
    const Job jb = jobs[find_job<false>(jobs, njobs, tile)];
    const int O = jb.O, I = jb.I, T = job_taps(jb), lt = tile - jb.ptile0, rb = (O + kTile - 1) / kTile;
    const long wts = (long)O * I, ats = (long)r * I;         // tap strides of dW and of A / dA
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, q = lane >> 4;
    const bool live = set < nsets;                   // a set the backward pass did not produce: its LoRA gradients are written as zeros
    const float* dW = grads + (long)set * set_stride + jb.w_off;
    const float* A = lora_p + jb.a_off;
    const float* B = lora_p + jb.b_off;
    f32x4_t acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = kZero;

    if (lt < rb) {
        // ---- dB[o][n] = s sum_t sum_i dW[t][o][i] A[t][n][i]: 16 rows per wave, k = (t, i)
        const int o0 = lt * kTile + wv * 16;
        if (o0 >= O) return;
        if (live) {
            const bool vec = (I & 3) == 0;
            const bool rok = o0 + li < O;
            for (int t = 0; t < T; ++t) {
                const float* wrow = dW + t * wts + (long)(o0 + li) * I;
                const float* At = A + t * ats;
                for (int k0 = 0; k0 < I; k0 += 16) {
                    const int k = k0 + 4 * q;
                    const f32x4_t a = ld_k4(wrow, k, I, rok, vec);
                    f32x4_t b[NT];
#pragma unroll
                    for (int n = 0; n < NT; ++n) b[n] = ld_k4(At + (long)(n * 16 + li) * I, k, I, n * 16 + li < r, vec);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[n][j], acc[n], 0, 0, 0);
                }
            }
        }
        float* dB = lora_g + (long)set * lora_set_stride + jb.b_off;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = o0 + 4 * q + j, col = n * 16 + li;
                if (row < O && col < r) dB[(long)row * r + col] = s * acc[n][j];
            }
    } else {
        // ---- dA[t][m][i] = s sum_o B[o][m] dW[t][o][i]: 16 columns of one tap per wave, k = o
        const int cb = (I + kTile - 1) / kTile, t = T == 1 ? 0 : (lt - rb) / cb;
        const int i0 = (lt - rb - t * cb) * kTile + wv * 16;
        if (i0 >= I || t >= T) return;
        dW += t * wts;
        const int col = i0 + li;
        const bool cok = col < I;
        if (live) {
#pragma unroll 4
            for (int o = 0; o < O; o += 4) {
                const int ko = o + q;
                const bool kok = ko < O;
                const float bv = (kok && cok) ? dW[(long)ko * I + col] : 0.f;
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    const float av = (kok && m * 16 + li < r) ? B[(long)ko * r + m * 16 + li] : 0.f;
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
                }
            }
        }
        float* dA = lora_g + (long)set * lora_set_stride + jb.a_off + t * ats;
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = m * 16 + 4 * q + j;
                if (row < r && cok) dA[(long)row * I + col] = s * acc[m][j];
            }
    }
}

template <class Job>
__global__ __launch_bounds__(256) void lora_merge_kernel(float* __restrict__ flat, bf16_t* __restrict__ shadow,
                                                         const float* __restrict__ w0, const float* __restrict__ lora_p,
                                                         const Job* __restrict__ jobs, int njobs, int r, float s) {
    const int tile = blockIdx.x;
    const Job jb = jobs[find_job<true>(jobs, njobs, tile)];
    const int O = jb.O, I = jb.I, T = job_taps(jb), cb = (I + kTile - 1) / kTile, per = ((O + kTile - 1) / kTile) * cb;
    const int t = T == 1 ? 0 : (tile - jb.mtile0) / per, lt = tile - jb.mtile0 - t * per;      // tap-major
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, q = lane >> 4;
    const int o0 = (lt / cb) * kTile + wv * 16, i0 = (lt % cb) * kTile;
    if (o0 >= O || t >= T) return;
    const float* A = lora_p + jb.a_off + (long)t * r * I;
    const float* B = lora_p + jb.b_off;
    f32x4_t acc[4] = {kZero, kZero, kZero, kZero};
    if (s != 0.f) {
        const bool rok = o0 + li < O;
        for (int k0 = 0; k0 < r; k0 += 4) {                      // k ascending: B[o][k] A[k][i]
            const int k = k0 + q;
            const bool kok = k < r;
            const float av = (kok && rok) ? B[(long)(o0 + li) * r + k] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = i0 + c * 16 + li;
                const float bv = (kok && col < I) ? A[(long)k * I + col] : 0.f;
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = o0 + 4 * q + j, col = i0 + c * 16 + li;
            if (row < O && col < I) {
                const long idx = ((long)t * O + row) * I + col;
                const float base = w0[jb.w0_off + idx];
                const float v = s != 0.f ? fmaf(s, acc[c][j], base) : base;      // (s = 0: W0 bit for bit -- unload)
                flat[jb.w_off + idx] = v;
                if (shadow) shadow[jb.w_off + idx] = f2bf(v);
            }
        }
}

template <class Job>
int launch_project(const float* grads, long set_stride, int nsets, const float* lora_p, float* lora_g, long lora_set_stride,
                   const void* jobs, int njobs, int r, float s, int total_tiles, void* stream) {
    SISS_CHECK_ARG(grads && lora_p && lora_g && jobs && njobs >= 1 && total_tiles >= njobs);
    SISS_CHECK_ARG((nsets == 1 || nsets == 2) && r >= 1 && r <= 64 && set_stride % 4 == 0 && lora_set_stride % 4 == 0);
    SISS_CHECK_ARG(((uintptr_t)grads | (uintptr_t)lora_p | (uintptr_t)lora_g) % 16 == 0);
    const dim3 grid(total_tiles, 2), block(256);
    const Job* jt = static_cast<const Job*>(jobs);
    hipStream_t st = (hipStream_t)stream;
#define SISS_LORA_PROJECT(NT) \
    lora_project_kernel<NT, Job><<<grid, block, 0, st>>>(grads, set_stride, nsets, lora_p, lora_g, lora_set_stride, jt, njobs, r, s)
    switch ((r + 15) / 16) {
        case 1: SISS_LORA_PROJECT(1); break;
        case 2: SISS_LORA_PROJECT(2); break;
        case 3: SISS_LORA_PROJECT(3); break;
        default: SISS_LORA_PROJECT(4); break;
    }
#undef SISS_LORA_PROJECT
    SISS_LAUNCH_RET();
}

}  // namespace

extern "C" {

// Rows (columns) of a target one block of the LoRA kernels owns: a target has ceil(O / tile) + ceil(I / tile) tiles in siss_lora_project
// and ceil(O / tile) * ceil(I / tile) in siss_lora_merge (the prefix sums of the job table, siss_amd/lora.py).
long siss_lora_tile(void) {
    return kTile;
}

// The chain rule through W = W0 + s B A: for every target of the job table and both gradient sets, dB_k = s dW_k A^T and
// dA_k = s B^T dW_k, OVERWRITTEN in lora_g [2, lora_set_stride] (f32; A [r, I] and B [O, r] of a target at the offsets they have in
// lora_p).  grads: the flat weight-gradient buffer (f32, sets set_stride floats apart); nsets = 1: the second set of lora_g is
// written as zeros.  jobs: njobs rows of {long w_off, a_off, b_off, w0_off; int O, I, first project tile, first merge tile} on the
// device; total_tiles: the project tiles of all targets.  1 <= r <= 64, any O, I >= 1.  Deterministic: no atomics, fixed order.
int siss_lora_project(const float* grads, long set_stride, int nsets, const float* lora_p, float* lora_g, long lora_set_stride,
                      const void* jobs, int njobs, int r, float s, int total_tiles, void* stream) {
    return launch_project<LoraJob>(grads, set_stride, nsets, lora_p, lora_g, lora_set_stride, jobs, njobs, r, s, total_tiles, stream);
}

// siss_lora_project for 3x3 convolutions (W = W0 + s B A per tap, B shared: peft's Conv2d adapter): for every target of the job
// table and both gradient sets, dB = s sum_t dW[t] A[t]^T (ONE reduction of length taps * I, t ascending) and dA[t] = s B^T dW[t],
// OVERWRITTEN in lora_g (A [taps, r, I] and B [O, r] of a target at the offsets they have in lora_p).  grads: the flat
// weight-gradient buffer with dW [taps, O, I] tap-major at w_off.  jobs: njobs rows of 64 bytes {long w_off, a_off, b_off, w0_off;
// int O, I, first project tile, first merge tile, taps, pad[3]} on the device; a target owns ceil(O / tile) + taps * ceil(I / tile)
// project tiles; total_tiles: their sum.  Everything else as siss_lora_project (nsets = 1: zeros in the second set; 1 <= r <= 64;
// 16-byte aligned bases; deterministic).
int siss_lora_project_conv(const float* grads, long set_stride, int nsets, const float* lora_p, float* lora_g, long lora_set_stride,
                           const void* jobs, int njobs, int r, float s, int total_tiles, void* stream) {
    return launch_project<LoraConvJob>(grads, set_stride, nsets, lora_p, lora_g, lora_set_stride, jobs, njobs, r, s, total_tiles,
                                       stream);
}

// W[o][i] = W0[o][i] + s sum_k B[o][k] A[k][i] (f32, k ascending) for every target of the job table, written to the f32 master `flat`
// and, when `shadow` is given (bf16 engine; null: the f32 engine, whose operand is the master), to shadow as the round-to-nearest-even
// bf16 of that value.  w0: the packed base weights (w0_off of the table).  s = 0 restores W0 bit for bit.  Touches the targets'
// [O, I] stretches only.  total_tiles: the merge tiles of all targets.
int siss_lora_merge(float* flat, void* shadow, const float* w0, const float* lora_p, const void* jobs, int njobs, int r, float s,
                    int total_tiles, void* stream) {
    SISS_CHECK_ARG(flat && w0 && lora_p && jobs && njobs >= 1 && total_tiles >= njobs && r >= 1 && r <= 64);
    lora_merge_kernel<<<dim3(total_tiles), dim3(256), 0, (hipStream_t)stream>>>(flat, static_cast<bf16_t*>(shadow), w0, lora_p,
                                                                                 static_cast<const LoraJob*>(jobs), njobs, r, s);
    SISS_LAUNCH_RET();
}

// siss_lora_merge for 3x3 convolutions: W[t][o][i] = W0[t][o][i] + s sum_k B[o][k] A[t][k][i] (f32, k ascending) for every target of
// the 64-byte job table of siss_lora_project_conv, written to the f32 master and, when `shadow` is given, to its bf16 shadow (round
// to nearest even).  w0: the packed base weights [taps, O, I] at w0_off.  s = 0 restores W0 bit for bit.  Touches the targets'
// [taps, O, I] stretches only; a target owns taps * ceil(O / tile) * ceil(I / tile) merge tiles; total_tiles: their sum.  The
// bases are 16-byte aligned (the shadow 8-byte).
int siss_lora_merge_conv(float* flat, void* shadow, const float* w0, const float* lora_p, const void* jobs, int njobs, int r, float s,
                         int total_tiles, void* stream) {
    SISS_CHECK_ARG(flat && w0 && lora_p && jobs && njobs >= 1 && total_tiles >= njobs && r >= 1 && r <= 64);
    SISS_CHECK_ARG(((uintptr_t)flat | (uintptr_t)w0 | (uintptr_t)lora_p) % 16 == 0 && (uintptr_t)shadow % 8 == 0);
    lora_merge_kernel<<<dim3(total_tiles), dim3(256), 0, (hipStream_t)stream>>>(flat, static_cast<bf16_t*>(shadow), w0, lora_p,
                                                                                 static_cast<const LoraConvJob*>(jobs), njobs, r, s);
    SISS_LAUNCH_RET();
}

}  // extern "C"

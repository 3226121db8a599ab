// Saliency-masked unlearning (SalUn-style weight mask; siss_amd/saliency.py, `deletion.saliency`; no counterpart in the reference,
// whose runs update every parameter):
//   siss_absf_select         the exact k-th largest |g| of a flat f32 buffer: a radix select over the 31 magnitude bits
//   siss_saliency_mask       one bit per float: |g| at or above that threshold
//   siss_grad_norms_scale_masked / siss_recombine_clip_adamw_masked
//                            the two passes of optimizer.hip under the bit mask (grid, thread -> granule map, summation order, scalar
//                            block and AdamW arithmetic are opt_step.h's: an all-ones mask gives the whole-buffer pair bit for bit)
// Magnitudes are compared as INTEGERS (bits & 0x7fffffff): denormals and -0.0 rank by their bit pattern and no flush mode matters.
// Counting is integer and every fold has a fixed order: no global atomics, bitwise repeatable.
#include "opt_step.h"

namespace {

constexpr int kBins = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSelWords = 8;             // the result block: 8 x u64
enum { SEL_THRESHOLD = 0, SEL_GT, SEL_GE, SEL_NONFINITE, SEL_PREFIX, SEL_RANK };

// the four digits of the 31-bit key, from the top: 8 / 8 / 8 / 7 bits
__device__ __host__ __forceinline__ int digit_shift(int pass) { return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0; }
__device__ __host__ __forceinline__ int digit_bits(int pass) { return pass == 3 ? 7 : 8; }

__device__ __forceinline__ unsigned key_of(float f) { return __builtin_bit_cast(unsigned, f) & 0x7fffffffu; }

// One count per valid lane into THIS WAVE's sub-histogram.  The first digit is the f32 exponent and real gradients pile into a
// handful of bins: up to kPeel times the digit of the first remaining lane is counted for every lane that holds it by ONE LDS add
// (ballot + popcount), so that equal keys do not serialise on one LDS address; what is left takes one LDS add per lane.  The calls
// are wave-uniform (every lane of the wave makes them, `valid` or not).
constexpr int kPeel = 4;
__device__ __forceinline__ void wave_hist_add(unsigned* __restrict__ hist, unsigned digit, bool valid) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    for (int r = 0; r < kPeel && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d = (unsigned)__shfl((int)digit, leader, 64);
        const unsigned long long same = __ballot(valid && digit == d);
        if (lane == leader) atomicAdd(&hist[d], (unsigned)__popcll(same));
        valid = valid && digit != d;
        todo &= ~same;
    }
    if (valid) atomicAdd(&hist[digit], 1u);
}

// One pass of the select: the histogram of digit `pass` over the elements whose higher key bits equal the prefix chosen so far
// (sel[SEL_PREFIX]; pass 0: all).  Grid-stride over granules (block 0 takes the scalar tail); per-wave sub-histograms in LDS, summed
// into ONE row of 256 u32 counts per block.
__global__ __launch_bounds__(kThreads) void select_hist_kernel(const float* __restrict__ g, long n, int pass,
                                                               const unsigned long long* __restrict__ sel, unsigned* __restrict__ rows) {
    __shared__ unsigned hist[kWaves][kBins];
    for (int i = threadIdx.x; i < kWaves * kBins; i += kThreads) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const int shift = digit_shift(pass), hi = shift + digit_bits(pass);
    const unsigned dmask = (1u << digit_bits(pass)) - 1u;
    const unsigned prefix = pass == 0 ? 0u : (unsigned)sel[SEL_PREFIX];
    unsigned* mine = hist[threadIdx.x >> 6];
    const long nvec = n / 4;
    for (long base = (long)blockIdx.x * kThreads; base < nvec; base += (long)gridDim.x * kThreads) {    // (wave-uniform trip count)
        const long k = base + threadIdx.x;
        const bool in = k < nvec;
        u32x4_t x = u32x4_t{0u, 0u, 0u, 0u};
        if (in) x = reinterpret_cast<const u32x4_t*>(g)[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned key = x[j] & 0x7fffffffu;
            wave_hist_add(mine, (key >> shift) & dmask, in && (key >> hi) == prefix);
        }
    }
    if (blockIdx.x == 0) {                                   // n % 4 < 4 elements: one round of the block covers them
        const long i = nvec * 4 + threadIdx.x;
        const bool in = i < n;
        const unsigned key = in ? key_of(g[i]) : 0u;
        wave_hist_add(mine, (key >> shift) & dmask, in && (key >> hi) == prefix);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kThreads) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += hist[w][b];
        rows[(long)blockIdx.x * kBins + b] = c;
    }
}

// The fold of a pass (ONE block): thread b sums column b of the rows in 64-bit integers (fixed lane -> index map), thread 0 walks
// the bins from the top until the running count reaches the remaining rank and writes the chosen digit and the new remaining rank.
// After pass 3 the block holds the threshold, count_gt, count_ge; nonfinite (keys >= 0x7f800000: exponent digit 255) comes from pass 0.
__global__ __launch_bounds__(kBins) void select_fold_kernel(const unsigned* __restrict__ rows, int nblk, int pass, long k,
                                                            unsigned long long* __restrict__ sel) {
    __shared__ unsigned long long cnt[kBins];
    unsigned long long c = 0;
    for (int r = 0; r < nblk; ++r) c += rows[(long)r * kBins + threadIdx.x];
    cnt[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long rank = pass == 0 ? (unsigned long long)k : sel[SEL_RANK];
    unsigned long long gt = pass == 0 ? 0ull : sel[SEL_GT];
    const unsigned prefix = pass == 0 ? 0u : (unsigned)sel[SEL_PREFIX];
    int b = (1 << digit_bits(pass)) - 1;
    unsigned long long above = 0;
    while (b > 0 && above + cnt[b] < rank) { above += cnt[b]; --b; }      // (1 <= rank <= matching elements: the walk ends inside)
    const unsigned chosen = (prefix << digit_bits(pass)) | (unsigned)b;
    sel[SEL_PREFIX] = chosen;
    sel[SEL_RANK] = rank - above;
    sel[SEL_GT] = gt + above;
    if (pass == 0) sel[SEL_NONFINITE] = cnt[kBins - 1];
    if (pass == 3) {
        sel[SEL_THRESHOLD] = chosen;
        sel[SEL_GE] = gt + above + cnt[b];
        for (int i = SEL_RANK + 1; i < kSelWords; ++i) sel[i] = 0;      // (the spare words: the block is written entirely)
    }
}

// bits[i >> 5] bit (i & 31) = key(g[i]) >= threshold: a wave takes 64 consecutive floats per step, the ballot is two words, two lanes
// store one each (plain vector stores).  Bits beyond n are zero (their lanes vote false).
__global__ __launch_bounds__(kThreads) void mask_kernel(const float* __restrict__ g, long n, unsigned threshold,
                                                        unsigned* __restrict__ bits, long nwords) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6), nwave = (long)gridDim.x * kWaves;
    for (long base = wave * 64; base < n; base += nwave * 64) {
        const long i = base + lane;
        const bool in = i < n && key_of(g[i]) >= threshold;
        const unsigned long long b = __ballot(in);
        const long w = (base >> 5) + lane;
        if (lane < 2 && w < nwords) bits[w] = lane == 0 ? (unsigned)b : (unsigned)(b >> 32);
    }
}

// the four mask bits of granule k (floats 4k .. 4k + 3)
__device__ __forceinline__ unsigned nibble_of(const unsigned* __restrict__ bits, long k) { return (bits[k >> 3] >> ((int)(k & 7) * 4)) & 0xfu; }
__device__ __forceinline__ bool bit_of(const unsigned* __restrict__ bits, long i) { return (bits[i >> 5] >> (int)(i & 31)) & 1u; }

// pass 1 under the mask: a masked-out element enters the three sums as +0, a granule without a set bit is not loaded
__global__ __launch_bounds__(kThreads) void norms_masked_kernel(const float* __restrict__ gx, const float* __restrict__ ga, long n,
                                                                const unsigned* __restrict__ bits, double* __restrict__ partials) {
    double sxx = 0, saa = 0, sxa = 0;
    const long nvec = n / 4;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < nvec; k += (long)gridDim.x * kThreads) {
        const unsigned nib = nibble_of(bits, k);
        f32x4_t x = f32x4_t{0.f, 0.f, 0.f, 0.f}, a = x;
        if (nib) {
            x = reinterpret_cast<const f32x4_t*>(gx)[k];
            a = reinterpret_cast<const f32x4_t*>(ga)[k];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((nib >> j) & 1u)) { x[j] = 0.f; a[j] = 0.f; }
        }
        norm_granule(x, a, sxx, saa, sxa);
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) {
            const bool on = bit_of(bits, i);
            norm_tail(on ? gx[i] : 0.f, on ? ga[i] : 0.f, sxx, saa, sxa);
        }
    norm_block_fold(sxx, saa, sxa, partials);
}

// pass 2 under the mask: a granule without a set bit is neither loaded nor stored; in a partly masked granule the masked-out lanes
// keep their old p / m / v / shadow / g_out bytes; the scalar tail honours the mask too
__global__ __launch_bounds__(kThreads) void recombine_adamw_masked_kernel(
    const float* __restrict__ gx, const float* __restrict__ ga, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
    bf16_t* __restrict__ shadow, float* __restrict__ g_out, long n, const unsigned* __restrict__ bits, float lr, float beta1,
    float beta2, float eps, float wd, const StepScalars* __restrict__ sc) {
    const AdamWStep upd(sc, lr, beta1, beta2, eps, wd);
    const long nvec = n / 4;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        const unsigned nib = nibble_of(bits, i);
        if (!nib) continue;
        if (nib == 0xfu) { update_granule(upd, gx, ga, p, m, v, shadow, g_out, i); continue; }      // (the whole-buffer pass's granule)
        f32x4_t x = reinterpret_cast<const f32x4_t*>(gx)[i], a = reinterpret_cast<const f32x4_t*>(ga)[i];
        f32x4_t pp = reinterpret_cast<f32x4_t*>(p)[i], mm = reinterpret_cast<f32x4_t*>(m)[i],
                vv = reinterpret_cast<f32x4_t*>(v)[i], gg;
        if (g_out) gg = reinterpret_cast<f32x4_t*>(g_out)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((nib >> j) & 1u) { float P = pp[j], M = mm[j], V = vv[j]; gg[j] = upd(x[j], a[j], P, M, V); pp[j] = P; mm[j] = M; vv[j] = V; }
        reinterpret_cast<f32x4_t*>(p)[i] = pp;
        reinterpret_cast<f32x4_t*>(m)[i] = mm;
        reinterpret_cast<f32x4_t*>(v)[i] = vv;
        if (g_out) reinterpret_cast<f32x4_t*>(g_out)[i] = gg;
        if (shadow) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((nib >> j) & 1u) shadow[4 * i + j] = f2bf(pp[j]);
        }
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) {
            if (bit_of(bits, i)) update_element(upd, gx, ga, p, m, v, shadow, g_out, i);
        }
}

}  // namespace

extern "C" {

// Bytes of the caller-owned work buffer of siss_absf_select (one row of 256 u32 counts per block of the histogram passes).
long siss_absf_select_work_bytes(void) { return (long)kMaxBlocks * kBins * (long)sizeof(unsigned); }
// Words (8-byte integers) of siss_absf_select's result block: threshold_bits, count_gt, count_ge, nonfinite, then the select's own
// running state (prefix, remaining rank) and two spare words.
long siss_absf_select_result_words(void) { return kSelWords; }

// The exact k-th largest magnitude of g[0 .. n), 1 <= k <= n, by the integer key bits(g) & 0x7fffffff: a radix select from the top
// over digits of 8 / 8 / 8 / 7 bits -- per digit one grid-stride histogram launch (per-block rows in `work`, siss_absf_select_work_bytes)
// and one one-block fold that picks the digit: eight launches, no host read, no global atomics, bitwise repeatable.  Afterwards
// `result` (DEVICE, siss_absf_select_result_words 8-byte integers, written entirely) holds [0] threshold_bits, [1] count_gt and
// [2] count_ge (elements strictly above / at or above the threshold), [3] nonfinite (keys >= 0x7f800000: inf and NaN rank on top).
int siss_absf_select(const float* g, long n, long k, void* work, long* result, void* stream) {
    SISS_CHECK_ARG(g && work && result && n > 0 && k >= 1 && k <= n);
    SISS_CHECK_ARG(((uintptr_t)g | (uintptr_t)work) % 16 == 0 && (uintptr_t)result % 8 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    unsigned long long* sel = reinterpret_cast<unsigned long long*>(result);
    for (int pass = 0; pass < 4; ++pass) {
        select_hist_kernel<<<nblk, kThreads, 0, s>>>(g, n, pass, sel, reinterpret_cast<unsigned*>(work));
        select_fold_kernel<<<1, kBins, 0, s>>>(reinterpret_cast<const unsigned*>(work), nblk, pass, k, sel);
    }
    SISS_LAUNCH_RET();
}

// The packed mask of a threshold: bits[i >> 5] bit (i & 31) = (bits(g[i]) & 0x7fffffff) >= threshold_bits for i < n, one 32-bit word
// per 32 floats, ceil(n / 32) words, the bits beyond n zero.
int siss_saliency_mask(const float* g, long n, int threshold_bits, void* bits, void* stream) {
    SISS_CHECK_ARG(g && bits && n > 0 && threshold_bits >= 0);
    SISS_CHECK_ARG((uintptr_t)g % 16 == 0 && (uintptr_t)bits % 4 == 0);
    const long nwords = (n + 31) / 32;
    long blocks = (n + 64L * kWaves - 1) / (64L * kWaves);
    if (blocks > 4 * kMaxBlocks) blocks = 4 * kMaxBlocks;
    mask_kernel<<<(int)blocks, kThreads, 0, (hipStream_t)stream>>>(g, n, (unsigned)threshold_bits, reinterpret_cast<unsigned*>(bits), nwords);
    SISS_LAUNCH_RET();
}

// siss_grad_norms_scale under a bit mask (`bits`: siss_saliency_mask's words over the same n floats, 16-byte aligned): an element
// whose bit is clear enters the three sums as +0 and a granule of four clear bits is not read (a NaN in a masked-out gradient reaches
// no scalar).  Same slabs, scalar block and modes; grid, thread -> granule map and summation order are the whole-buffer pass's: an
// all-ones mask gives its result bit for bit, any mask the result of that pass on gradients multiplied by the mask.
int siss_grad_norms_scale_masked(const float* gx, const float* ga, long n, const unsigned* bits, int mode, float knob, float max_norm,
                                 float beta1, float beta2, double* partials, float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && bits && partials && scalars && n > 0 && mode >= 0 && mode <= 2);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga | (uintptr_t)bits) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    norms_masked_kernel<<<nblk, kThreads, 0, s>>>(gx, ga, n, bits, partials);
    scalars_kernel<<<1, kThreads, 0, s>>>(partials, nblk, mode, knob, max_norm, beta1, beta2, reinterpret_cast<StepScalars*>(scalars));
    SISS_LAUNCH_RET();
}

// siss_recombine_clip_adamw under the same mask: the update on the elements whose bit is set; every other byte of p, m, v, shadow
// and g_out keeps its value (a granule of four clear bits is neither read nor written).
int siss_recombine_clip_adamw_masked(const float* gx, const float* ga, float* p, float* m, float* v, void* shadow, float* g_out,
                                     long n, const unsigned* bits, float lr, float beta1, float beta2, float eps, float wd,
                                     const float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && p && m && v && bits && scalars && n > 0);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)bits) % 16 == 0);
    SISS_CHECK_ARG((!shadow || (uintptr_t)shadow % 8 == 0) && (!g_out || (uintptr_t)g_out % 16 == 0));
    recombine_adamw_masked_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(
        gx, ga, p, m, v, reinterpret_cast<bf16_t*>(shadow), g_out, n, bits, lr, beta1, beta2, eps, wd,
        reinterpret_cast<const StepScalars*>(scalars));
    SISS_LAUNCH_RET();
}

}  // extern "C"

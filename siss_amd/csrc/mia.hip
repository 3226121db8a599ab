// The membership inference attacks' device side (siss_amd/mia.py; SecMI, Duan et al., ICML 2023; PIA, Kong et al., ICLR 2024; no
// counterpart in the reference, whose only membership evidence is the mean eps-MSE of metrics/class_membership.py): the element-wise
// passes between the UNet forwards of a deterministic DDIM chain.
//
//   The N images of an evaluation lie in one [N][chw] f32 pool; a chain works on the b rows starting at *offset (a device scalar: one
//   captured graph serves every batch).  A row past the pool reads the pool's last row (clamped) and writes no sum.
//
//   gather         : out[r] = pool[offset + r]
//   transfer       : y[r] = cx * x[r] + ce * e[r]            (x: b chain rows, or the pool rows at offset; optionally keeps a copy of e)
//   transfer_sqerr : sums[offset + r] = sum_chw ((cx * x[r] + ce * e[r]) - ref[r])^2     -- the last transfer of SecMI, never stored
//   powdiff        : sums[offset + r] = sum_chw |e0[r] - e1[r]|^p, p in {2, 4}            -- PIA's score
//
// f32 tensors, f64 sums.  HBM-bound, 16 B per lane per access where the rows allow it; per-row reductions wave -> block -> one f64
// partial per (row, block) -> folded in index order: no atomics, bit-reproducible.  Built with -ffp-contract=off (build.py EXACT):
// the transfer is bitwise torch's `cx * x + ce * e`.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// The pool row chain row r reads (clamped into the pool), and whether it is a row of the pool at all.
__device__ __forceinline__ long pool_row(const int64_t* __restrict__ offset, long n, int r, bool& live) {
    const long index = offset[0] + r;
    live = index >= 0 && index < n;
    return index < 0 ? 0 : (index >= n ? n - 1 : index);
}

// one deterministic DDIM transfer, each product and the sum rounded on its own
__device__ __forceinline__ float ddim(float cx, float ce, float x, float e) { return __fadd_rn(__fmul_rn(cx, x), __fmul_rn(ce, e)); }

__device__ __forceinline__ double sq_term(float a, float b) {
    const float d = __fsub_rn(a, b);
    return (double)__fmul_rn(d, d);
}

template <int P>
__device__ __forceinline__ double pow_term(float a, float b) {
    const float d = __fsub_rn(a, b);
    const float d2 = __fmul_rn(d, d);
    return (double)(P == 2 ? d2 : __fmul_rn(d2, d2));
}

// VEC: every row starts 16-B aligned and chw % 4 == 0: four elements per lane per access, no tail.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void gather_kernel(const float* __restrict__ pool, const int64_t* __restrict__ offset, long n,
                                                          long chw, float* __restrict__ out) {
    const int r = blockIdx.y;
    bool live;
    const float* src = pool + pool_row(offset, n, r, live) * chw;
    float* dst = out + (long)r * chw;
    const long first = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    if (VEC) {
        for (long i = first; i < chw / 4; i += step) reinterpret_cast<f32x4_t*>(dst)[i] = reinterpret_cast<const f32x4_t*>(src)[i];
    } else {
        for (long k = first; k < chw; k += step) dst[k] = src[k];
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void transfer_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                            const int64_t* __restrict__ offset, long n, long chw, float cx, float ce,
                                                            float* __restrict__ y, float* __restrict__ e_keep) {
    const int r = blockIdx.y;
    bool live;
    const float* xr = x + (offset ? pool_row(offset, n, r, live) : (long)r) * chw;
    const float* er = e + (long)r * chw;
    float* yr = y + (long)r * chw;
    float* kr = e_keep ? e_keep + (long)r * chw : nullptr;
    const long first = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    if (VEC) {
        for (long i = first; i < chw / 4; i += step) {
            const f32x4_t a = reinterpret_cast<const f32x4_t*>(xr)[i], b = reinterpret_cast<const f32x4_t*>(er)[i];
            f32x4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ddim(cx, ce, a[j], b[j]);
            reinterpret_cast<f32x4_t*>(yr)[i] = o;
            if (kr) reinterpret_cast<f32x4_t*>(kr)[i] = b;
        }
    } else {
        for (long k = first; k < chw; k += step) {
            const float b = er[k];
            yr[k] = ddim(cx, ce, xr[k], b);
            if (kr) kr[k] = b;
        }
    }
}

// The block's f64 sum into its slot of the partial slab (every thread of the block calls this).
__device__ __forceinline__ void block_partial(double acc, double* __restrict__ partials, int r) {
    __shared__ double sh[kThreads / 64];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < kThreads / 64; ++i) s += sh[i];
        partials[(long)r * gridDim.x + blockIdx.x] = s;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void transfer_sqerr_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                                  const float* __restrict__ ref, const int64_t* __restrict__ offset,
                                                                  long n, long chw, float cx, float ce, double* __restrict__ partials) {
    const int r = blockIdx.y;
    bool live;
    pool_row(offset, n, r, live);
    if (!live) return;                                                                               // (block-uniform)
    const float* xr = x + (long)r * chw;
    const float* er = e + (long)r * chw;
    const float* rr = ref + (long)r * chw;
    double acc = 0;
    const long first = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    if (VEC) {
        for (long i = first; i < chw / 4; i += step) {
            const f32x4_t a = reinterpret_cast<const f32x4_t*>(xr)[i], b = reinterpret_cast<const f32x4_t*>(er)[i],
                          c = reinterpret_cast<const f32x4_t*>(rr)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += sq_term(ddim(cx, ce, a[j], b[j]), c[j]);
        }
    } else {
        for (long k = first; k < chw; k += step) acc += sq_term(ddim(cx, ce, xr[k], er[k]), rr[k]);
    }
    block_partial(acc, partials, r);
}

template <bool VEC, int P>
__global__ __launch_bounds__(kThreads) void powdiff_kernel(const float* __restrict__ e0, const float* __restrict__ e1,
                                                           const int64_t* __restrict__ offset, long n, long chw,
                                                           double* __restrict__ partials) {
    const int r = blockIdx.y;
    bool live;
    pool_row(offset, n, r, live);
    if (!live) return;                                                                               // (block-uniform)
    const float* ar = e0 + (long)r * chw;
    const float* br = e1 + (long)r * chw;
    double acc = 0;
    const long first = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    if (VEC) {
        for (long i = first; i < chw / 4; i += step) {
            const f32x4_t a = reinterpret_cast<const f32x4_t*>(ar)[i], b = reinterpret_cast<const f32x4_t*>(br)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += pow_term<P>(a[j], b[j]);
        }
    } else {
        for (long k = first; k < chw; k += step) acc += pow_term<P>(ar[k], br[k]);
    }
    block_partial(acc, partials, r);
}

// One thread per row: fold the row's partials left to right into the image's entry of `sums`; rows past the pool write nothing.
__global__ void row_fold_kernel(const double* __restrict__ partials, int nblk, int b, const int64_t* __restrict__ offset, long n,
                                double* __restrict__ sums) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b) return;
    bool live;
    const long index = pool_row(offset, n, r, live);
    if (!live) return;
    double s = 0;
    for (int i = 0; i < nblk; ++i) s += partials[(long)r * nblk + i];
    sums[index] = s;
}

inline int blocks_for(long chw) {
    long v = chw / 4 / kThreads;
    if (v < 1) v = 1;
    if (v > 64) v = 64;
    return (int)v;
}

inline bool aligned(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }
inline bool shape_ok(long n, int b, long chw) { return n > 0 && b > 0 && b <= 65535 && chw > 0; }

}  // namespace

extern "C" {

// Number of f64 words siss_mia_transfer_sqerr / siss_mia_powdiff need in `partials` for b rows of chw elements.
long siss_mia_partials_words(int b, long chw) { return (long)b * blocks_for(chw); }

// The first input of a chain: out[r] = pool[min(offset[0] + r, n - 1)] for r < b.  pool: [n][chw] f32; offset[1] (int64, device): the
// batch's first pool row; out: [b][chw] f32.  A row past the pool is a copy of the pool's last row (it is computed and never scored).
int siss_mia_gather(const float* pool, const int64_t* offset, long n, int b, long chw, float* out, void* stream) {
    SISS_CHECK_ARG(pool && offset && out);
    SISS_CHECK_ARG(aligned(pool, 4) && aligned(out, 4) && aligned(offset, 8));
    SISS_CHECK_ARG(shape_ok(n, b, chw));
    const bool vec = chw % 4 == 0 && aligned(pool, 16) && aligned(out, 16);
    dim3 grid(blocks_for(chw), b);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        gather_kernel<true><<<grid, kThreads, 0, s>>>(pool, offset, n, chw, out);
    else
        gather_kernel<false><<<grid, kThreads, 0, s>>>(pool, offset, n, chw, out);
    SISS_LAUNCH_RET();
}

// One deterministic DDIM transfer: y[r] = cx * x[r'] + ce * e[r] for r < b, in f32 with each product and the sum rounded on its own
// (bitwise torch's `cx * x + ce * e`).  offset == NULL: x is [b][chw] and r' = r; else x is the pool [n][chw] and
// r' = min(offset[0] + r, n - 1) (PIA noises the pool's rows with the network's own prediction).  e, y: [b][chw] f32; e_keep: NULL,
// or [b][chw] f32 that receives a copy of e (the prediction buffer is the engine's and the next forward overwrites it).  y and e_keep
// must not overlap x or e.
int siss_mia_transfer(const float* x, const float* e, const int64_t* offset, long n, int b, long chw, float cx, float ce, float* y,
                      float* e_keep, void* stream) {
    SISS_CHECK_ARG(x && e && y);
    SISS_CHECK_ARG(aligned(x, 4) && aligned(e, 4) && aligned(y, 4) && aligned(e_keep, 4) && aligned(offset, 8));
    SISS_CHECK_ARG(shape_ok(n, b, chw));
    const bool vec = chw % 4 == 0 && aligned(x, 16) && aligned(e, 16) && aligned(y, 16) && aligned(e_keep, 16);
    dim3 grid(blocks_for(chw), b);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        transfer_kernel<true><<<grid, kThreads, 0, s>>>(x, e, offset, n, chw, cx, ce, y, e_keep);
    else
        transfer_kernel<false><<<grid, kThreads, 0, s>>>(x, e, offset, n, chw, cx, ce, y, e_keep);
    SISS_LAUNCH_RET();
}

// SecMI's t-error: the last transfer of the round trip with its squared distance from x_t, the transferred value never stored.  For
// r < b with offset[0] + r inside the pool of n images, sums[offset[0] + r] = sum over chw of ((cx * x[r] + ce * e[r]) - ref[r])^2:
// the transfer as siss_mia_transfer forms it, difference and square rounded to f32, the sum in f64 in a fixed order.  Rows past the
// pool write nothing.  x, e, ref: [b][chw] f32; sums: f64 [n]; partials: f64 scratch of siss_mia_partials_words(b, chw) words.
int siss_mia_transfer_sqerr(const float* x, const float* e, const float* ref, const int64_t* offset, long n, int b, long chw,
                            float cx, float ce, double* sums, double* partials, void* stream) {
    SISS_CHECK_ARG(x && e && ref && offset && sums && partials);
    SISS_CHECK_ARG(aligned(x, 4) && aligned(e, 4) && aligned(ref, 4) && aligned(offset, 8) && aligned(sums, 8) && aligned(partials, 8));
    SISS_CHECK_ARG(shape_ok(n, b, chw));
    const bool vec = chw % 4 == 0 && aligned(x, 16) && aligned(e, 16) && aligned(ref, 16);
    const int nblk = blocks_for(chw);
    dim3 grid(nblk, b);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        transfer_sqerr_kernel<true><<<grid, kThreads, 0, s>>>(x, e, ref, offset, n, chw, cx, ce, partials);
    else
        transfer_sqerr_kernel<false><<<grid, kThreads, 0, s>>>(x, e, ref, offset, n, chw, cx, ce, partials);
    row_fold_kernel<<<cdiv(b, 64), 64, 0, s>>>(partials, nblk, b, offset, n, sums);
    SISS_LAUNCH_RET();
}

// PIA's score: for r < b with offset[0] + r inside the pool of n images, sums[offset[0] + r] = sum over chw of |e0[r] - e1[r]|^p,
// p = 2 or 4 (anything else is refused): the difference, its square and (p = 4) the square's square rounded to f32, the sum in f64 in
// a fixed order.  Rows past the pool write nothing.  e0, e1: [b][chw] f32; sums: f64 [n]; partials: as above.
int siss_mia_powdiff(const float* e0, const float* e1, const int64_t* offset, long n, int b, long chw, int p, double* sums,
                     double* partials, void* stream) {
    SISS_CHECK_ARG(e0 && e1 && offset && sums && partials);
    SISS_CHECK_ARG(aligned(e0, 4) && aligned(e1, 4) && aligned(offset, 8) && aligned(sums, 8) && aligned(partials, 8));
    SISS_CHECK_ARG(shape_ok(n, b, chw) && (p == 2 || p == 4));
    const bool vec = chw % 4 == 0 && aligned(e0, 16) && aligned(e1, 16);
    const int nblk = blocks_for(chw);
    dim3 grid(nblk, b);
    hipStream_t s = (hipStream_t)stream;
    if (vec && p == 2)
        powdiff_kernel<true, 2><<<grid, kThreads, 0, s>>>(e0, e1, offset, n, chw, partials);
    else if (vec)
        powdiff_kernel<true, 4><<<grid, kThreads, 0, s>>>(e0, e1, offset, n, chw, partials);
    else if (p == 2)
        powdiff_kernel<false, 2><<<grid, kThreads, 0, s>>>(e0, e1, offset, n, chw, partials);
    else
        powdiff_kernel<false, 4><<<grid, kThreads, 0, s>>>(e0, e1, offset, n, chw, partials);
    row_fold_kernel<<<cdiv(b, 64), 64, 0, s>>>(partials, nblk, b, offset, n, sums);
    SISS_LAUNCH_RET();
}

}  // extern "C"

// The membership-loss metric's device side (siss_amd/membership.py; reference: metrics/class_membership.py:68-130): the two
// streaming passes either side of the UNet forward, driven by an index table so that no (image x noise) expansion ever exists.
//
//   work item = (image row, noise row, timestep): int64 triples, the whole evaluation is one flat device table `items[n_items][3]`;
//   one forward consumes the `b` items starting at *offset (a device scalar: one captured graph serves every forward).
//
//   pair_noise : xs[r] = add_noise(imgs[item.image], noise[item.noise], item.t), ts[r] = item.t     (2 reads + 1 write per element)
//   pair_sqerr : sums[item] = sum_chw (pred[r] - noise[item.noise])^2                                (2 reads per element)
//
// f32 / index tensors only (the engines take an f32 NCHW sample and return an f32 NCHW prediction in both modes).  HBM-bound, 16 B
// per lane per access, per-row reductions wave -> block -> f64 partial slab -> fixed-order sum: no atomics, bit-reproducible.
// Built with -ffp-contract=off (build.py EXACT): the noised value is bitwise torch's `sa * x + sb * n`.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 8;  // elements per lane per iteration

// The item row r of this forward reads, or false for a row past the end of the table (last, partly filled batch).  An index
// outside its tensor also counts as past the end: the host builds the table, the kernel never follows it out of bounds.
struct Item { long image, noise, t; };
__device__ __forceinline__ bool fetch_item(const int64_t* __restrict__ items, const int64_t* __restrict__ offset, long n_items, int r,
                                           long n_images, long n_noises, long n_timesteps, Item& it, long& index) {
    index = offset[0] + r;
    if (index < 0 || index >= n_items) return false;
    it.image = items[3 * index];
    it.noise = items[3 * index + 1];
    it.t = items[3 * index + 2];
    return it.image >= 0 && it.image < n_images && it.noise >= 0 && it.noise < n_noises && it.t >= 0 && it.t < n_timesteps;
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4_t a = reinterpret_cast<const f32x4_t*>(p)[0], b = reinterpret_cast<const f32x4_t*>(p)[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    reinterpret_cast<f32x4_t*>(p)[0] = f32x4_t{v[0], v[1], v[2], v[3]};
    reinterpret_cast<f32x4_t*>(p)[1] = f32x4_t{v[4], v[5], v[6], v[7]};
}

// DDPMScheduler.add_noise in f32: (ac ** 0.5) * x + ((1 - ac) ** 0.5) * n, each product and the sum rounded on its own
__device__ __forceinline__ float q_sample(float a, float b, float x, float n) {
    return __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, n));
}

// VEC: every row of every tensor starts 16-B aligned (chw % 4 == 0): 8 elements per lane, the ragged tail (chw % 8) by block 0.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void pair_noise_kernel(const float* __restrict__ imgs, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ items, const int64_t* __restrict__ offset,
                                                              long n_items, long n_images, long n_noises,
                                                              const float* __restrict__ ac_tab, long n_timesteps, long chw,
                                                              float* __restrict__ xs, int64_t* __restrict__ ts) {
    const int r = blockIdx.y;
    Item it;
    long index;
    const bool live = fetch_item(items, offset, n_items, r, n_images, n_noises, n_timesteps, it, index);   // (block-uniform)
    float* out = xs + (long)r * chw;
    if (blockIdx.x == 0 && threadIdx.x == 0) ts[r] = live ? it.t : 0;
    float ca = 0.f, cb = 0.f;
    const float* x = imgs;
    const float* nz = noise;
    if (live) {
        const float ac = ac_tab[it.t];
        ca = sqrtf(ac);
        cb = sqrtf(1.f - ac);
        x = imgs + it.image * chw;
        nz = noise + it.noise * chw;
    }
    const long nvec = VEC ? chw / kVec : 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        float vo[8] = {};
        if (live) {
            float vx[8], vn[8];
            load8(x + i * kVec, vx);
            load8(nz + i * kVec, vn);
#pragma unroll
            for (int j = 0; j < 8; ++j) vo[j] = q_sample(ca, cb, vx[j], vn[j]);
        }
        store8(out + i * kVec, vo);
    }
    if (VEC) {
        if (blockIdx.x == 0)
            for (long k = nvec * kVec + threadIdx.x; k < chw; k += kThreads) out[k] = live ? q_sample(ca, cb, x[k], nz[k]) : 0.f;
    } else {
        for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads)
            out[k] = live ? q_sample(ca, cb, x[k], nz[k]) : 0.f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void pair_sqerr_kernel(const float* __restrict__ pred, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ items, const int64_t* __restrict__ offset,
                                                              long n_items, long n_noises, long chw, double* __restrict__ partials) {
    __shared__ double sh[kThreads / 64];
    const int r = blockIdx.y;
    Item it;
    long index;
    if (!fetch_item(items, offset, n_items, r, 1L << 62, n_noises, 1L << 62, it, index)) return;   // (block-uniform)
    const float* p = pred + (long)r * chw;
    const float* nz = noise + it.noise * chw;
    double acc = 0;
    auto one = [&](float a, float b) {
        const float d = __fsub_rn(a, b);
        acc += (double)__fmul_rn(d, d);
    };
    const long nvec = VEC ? chw / kVec : 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        float vp[8], vn[8];
        load8(p + i * kVec, vp);
        load8(nz + i * kVec, vn);
#pragma unroll
        for (int j = 0; j < 8; ++j) one(vp[j], vn[j]);
    }
    if (VEC) {
        if (blockIdx.x == 0)
            for (long k = nvec * kVec + threadIdx.x; k < chw; k += kThreads) one(p[k], nz[k]);
    } else {
        for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads) one(p[k], nz[k]);
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < kThreads / 64; ++i) s += sh[i];
        partials[(long)r * gridDim.x + blockIdx.x] = s;
    }
}

// One thread per row: fold the row's partials left to right into the item's entry of `sums`; rows past the table write nothing.
__global__ void pair_fold_kernel(const double* __restrict__ partials, int nblk, int b, const int64_t* __restrict__ items,
                                 const int64_t* __restrict__ offset, long n_items, long n_noises, double* __restrict__ sums) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b) return;
    Item it;
    long index;
    if (!fetch_item(items, offset, n_items, r, 1L << 62, n_noises, 1L << 62, it, index)) return;
    double s = 0;
    for (int i = 0; i < nblk; ++i) s += partials[(long)r * nblk + i];
    sums[index] = s;
}

inline int blocks_for(long chw) {
    long v = chw / kVec / kThreads;
    if (v < 1) v = 1;
    if (v > 64) v = 64;
    return (int)v;
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" {

// Number of f64 words siss_pair_sqerr needs in `partials` for b rows of chw elements.
long siss_pair_partials_words(int b, long chw) { return (long)b * blocks_for(chw); }

// The model input of one forward of the membership metric.  items[n_items][3] (int64, device): (image row, noise row, timestep)
// per work item; offset[1] (int64, device): the first item of this forward.  For r < b: xs[r] = sqrt(ac[t]) * imgs[image] +
// sqrt(1 - ac[t]) * noise[noise_row] (f32, bitwise DDPMScheduler.add_noise) and ts[r] = t; a row past the end of the table (or
// whose item points outside imgs[n_images] / noise[n_noises] / alphas_cumprod[n_timesteps]) is written as zeros with ts = 0.
// imgs, noise, xs: rows of chw f32.
int siss_pair_noise(const float* imgs, const float* noise, const int64_t* items, const int64_t* offset, long n_items,
                    long n_images, long n_noises, const float* alphas_cumprod, long n_timesteps, int b, long chw, float* xs,
                    int64_t* ts, void* stream) {
    SISS_CHECK_ARG(imgs && noise && items && offset && alphas_cumprod && xs && ts);
    SISS_CHECK_ARG(n_items > 0 && n_images > 0 && n_noises > 0 && n_timesteps > 0 && b > 0 && b <= 65535 && chw > 0);
    const bool vec = chw % 4 == 0 && aligned16(imgs) && aligned16(noise) && aligned16(xs);
    dim3 grid(blocks_for(chw), b);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        pair_noise_kernel<true><<<grid, kThreads, 0, s>>>(imgs, noise, items, offset, n_items, n_images, n_noises, alphas_cumprod, n_timesteps, chw, xs, ts);
    else
        pair_noise_kernel<false><<<grid, kThreads, 0, s>>>(imgs, noise, items, offset, n_items, n_images, n_noises, alphas_cumprod, n_timesteps, chw, xs, ts);
    SISS_LAUNCH_RET();
}

// The per-pair squared error of the same forward: for r < b with item = offset[0] + r inside the table,
// sums[item] = sum over chw of (pred[r] - noise[items[item].noise])^2 -- difference and square rounded to f32 as torch's
// `(out - noise) ** 2`, the sum in f64 in a fixed order.  Rows past the end of the table write nothing.  pred: [b][chw] f32;
// sums: f64 [n_items]; partials: f64 scratch of siss_pair_partials_words(b, chw) words.
int siss_pair_sqerr(const float* pred, const float* noise, const int64_t* items, const int64_t* offset, long n_items,
                    long n_noises, int b, long chw, double* sums, double* partials, void* stream) {
    SISS_CHECK_ARG(pred && noise && items && offset && sums && partials);
    SISS_CHECK_ARG(n_items > 0 && n_noises > 0 && b > 0 && b <= 65535 && chw > 0);
    const bool vec = chw % 4 == 0 && aligned16(pred) && aligned16(noise);
    const int nblk = blocks_for(chw);
    dim3 grid(nblk, b);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        pair_sqerr_kernel<true><<<grid, kThreads, 0, s>>>(pred, noise, items, offset, n_items, n_noises, chw, partials);
    else
        pair_sqerr_kernel<false><<<grid, kThreads, 0, s>>>(pred, noise, items, offset, n_items, n_noises, chw, partials);
    pair_fold_kernel<<<cdiv(b, 64), 64, 0, s>>>(partials, nblk, b, items, offset, n_items, n_noises, sums);
    SISS_LAUNCH_RET();
}

}  // extern "C"

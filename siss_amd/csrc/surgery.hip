// Gradient surgery between the keep and forget gradients of the unlearning update (siss_amd/surgery.py, `deletion.surgery`; PCGrad, Yu
// et al., NeurIPS 2020; gradient-projection unlearning, Hoang et al., WACV 2024; the restricted gradient of Ko et al., NeurIPS 2024; no
// counterpart in the reference, whose update is g = g_x - s g_a whatever the sign of <g_x, g_a>).  Per GROUP G of the flat buffer (the
// whole buffer, or one parameter tensor with the alignment padding behind it) the three sums xx_G, aa_G, xa_G; a group CONFLICTS when
// xa_G > 0 (strictly; xx_G = 0 or aa_G = 0 never conflicts), and there the forget set loses its component along the keep set
// (mode 0, forget), the keep set its component along the forget set (mode 1, keep), or both, each taken from the original pair (mode 2,
// mutual).  The update direction is g = clip (cx_G x - ca_G a) with one coefficient pair per group:
//   siss_grad_norms_scale_surgery      the gram pass, the group sums, the scalar block and the coefficient table
//   siss_recombine_clip_adamw_surgery  pass 2 of optimizer.hip with (cx_G, ca_G) in place of (1, s)
// Grid helpers, the granule sums, the block fold, the scalar block's layout and the AdamW arithmetic are opt_step.h's: with no
// conflicting group cx = 1.0f and ca = (float)s, and pass 2 here IS siss_recombine_clip_adamw, bit for bit.
//
// THE ORDER OF EVERY SUM (tests/surgery_ref.py restates it; no atomics, nothing depends on the grid size):
//   jobs    each group is cut into jobs of C floats (siss_surgery_chunk) from its start, the last one shorter; job j of the plan is
//           row j of `partials`.
//   a row   thread t of 256 owns granules t, t + 256, ... of the job (norm_granule: four f32 products, their f32 sum ((0 + t0) + t1) +
//           t2) + t3, added to the thread's three f64 sums in ascending granule order), then element 4 * granules + t of the scalar
//           tail (n % 4: the buffer's last job alone; norm_tail, f64 products); norm_block_fold: the xor butterfly over the 64 lanes
//           (32, 16, 8, 4, 2, 1), then the four waves added in ascending order from 0.
//   a group one wave per group: lane l adds rows first + l, first + l + 64, ... in ascending order from 0, then the same butterfly.
//   global  one block: thread t adds the per-group terms of groups t, t + 256, ... in ascending order from 0, the butterfly, the four
//           waves in ascending order from 0 -- for the three sums, for |a'|^2 and |x'|^2, and (a second fold, once s is known) for the
//           pre-clip norm.
// The f64 expressions of the scalar block stand in scalars_coef_kernel as tests/surgery_ref.py writes them; every f64 value is rounded
// to f32 once.  Pass 2: every f32 operation is an explicit round-to-nearest one (the file is built without contraction).
#include "opt_step.h"

namespace {

constexpr long kDefaultChunk = 16384;          // floats per job: 16 granules per thread (profiles/surgery.json lists the others tried)
constexpr int kSlotConflicts = 12, kSlotCos = 13, kSlotRemovedA = 14, kSlotRemovedX = 15;   // pad3[0..3] of StepScalars

// process-local test configuration (siss_surgery_test_config): the chunk length and the cap of the persistent grids
long g_chunk = kDefaultChunk;
int g_max_blocks = kMaxBlocks;

// The device plan (int64): [jobs] start of the job (floats), [jobs] its group, [T + 1] first job of each group, [T + 1] the group
// offsets.  A job whose entries do not describe the buffer is skipped (its row is zero, no byte of its stretch is touched).
struct Plan {
    const long* start; const long* grp; const long* first; const long* off;
    long jobs, n, chunk; int T;
    __device__ Plan(const long* plan, long jobs_, int T_, long n_, long chunk_)
        : start(plan), grp(plan + jobs_), first(plan + 2 * jobs_), off(plan + 2 * jobs_ + T_ + 1), jobs(jobs_), n(n_), chunk(chunk_), T(T_) {}
    // job j: its group (or -1), its first float and its length
    __device__ __forceinline__ long job(long j, long& st, long& len) const {
        const long g = grp[j];
        st = start[j]; len = 0;
        if (g < 0 || g >= T || st < 0 || (st & 3) != 0 || st >= n) return -1;
        long end = off[g + 1];
        if (end > n) end = n;
        len = end - st;
        if (len > chunk) len = chunk;
        return len > 0 ? g : -1;
    }
};

__global__ __launch_bounds__(kThreads) void gram_kernel(const float* __restrict__ gx, const float* __restrict__ ga,
                                                        const long* __restrict__ plan, long jobs, int T, long n, long chunk,
                                                        double* __restrict__ rows) {
    const Plan pl(plan, jobs, T, n, chunk);
    for (long j = blockIdx.x; j < jobs; j += gridDim.x) {
        double sxx = 0, saa = 0, sxa = 0;
        long st, len;
        if (pl.job(j, st, len) >= 0) {
            const long nvec = len / 4;
            const f32x4_t* X = reinterpret_cast<const f32x4_t*>(gx + st);
            const f32x4_t* A = reinterpret_cast<const f32x4_t*>(ga + st);
            for (long k = threadIdx.x; k < nvec; k += kThreads) norm_granule(X[k], A[k], sxx, saa, sxa);
            for (long i = nvec * 4 + threadIdx.x; i < len; i += kThreads) norm_tail(gx[st + i], ga[st + i], sxx, saa, sxa);
        }
        norm_block_fold(sxx, saa, sxa, rows + 3 * (j - blockIdx.x));       // (the fold writes row blockIdx.x of what it is given: row j)
        __syncthreads();                                                    // (its LDS words are rewritten by the next job)
    }
}

// one wave per group: the group's rows -> gsum[g][3]
__global__ __launch_bounds__(kThreads) void group_fold_kernel(const double* __restrict__ rows, const long* __restrict__ plan, long jobs,
                                                              int T, double* __restrict__ gsum) {
    const int g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= T) return;                                                     // (wave-uniform)
    const long* first = plan + 2 * jobs;
    long r0 = first[g], r1 = first[g + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > jobs) r1 = jobs;
    double xx = 0, aa = 0, xa = 0;
    for (long r = r0 + lane; r < r1; r += 64) { xx += rows[3 * r]; aa += rows[3 * r + 1]; xa += rows[3 * r + 2]; }
    xx = wave_sum_d(xx); aa = wave_sum_d(aa); xa = wave_sum_d(xa);
    if (lane == 0) { gsum[3 * g] = xx; gsum[3 * g + 1] = aa; gsum[3 * g + 2] = xa; }
}

// the sum of one f64 value per thread over the block, in every thread: butterfly, then the four waves in ascending order
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();                                                        // (sh is reused from one sum to the next)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0;
    for (int i = 0; i < kThreads / 64; ++i) t += sh[i];
    return t;
}

// ONE block: the global sums, s from the PROJECTED forget set's norm, the coefficient table, the pre-clip norm from the unrounded
// coefficients, and the scalar block (slots 0-6, 8, 9 as scalars_kernel fills them; 12-15 the surgery's own; 7, 10, 11 not written).
// smode: 0 forget, 1 keep, 2 mutual.  mode: 0 | 2 of scalars_kernel.
__global__ __launch_bounds__(kThreads) void scalars_coef_kernel(const double* __restrict__ gsum, int T, int smode, int mode, float knob,
                                                                float max_norm, float beta1, float beta2, float* __restrict__ coef,
                                                                float* __restrict__ scalars) {
    __shared__ double sh[kThreads / 64];
    const bool proj_a = smode != 1, proj_x = smode != 0;
    double xx = 0, aa = 0, xa = 0, na2 = 0, nx2 = 0, cnt = 0;
    for (int g = threadIdx.x; g < T; g += kThreads) {
        const double gxx = gsum[3 * g], gaa = gsum[3 * g + 1], gxa = gsum[3 * g + 2];
        const bool phi = gxa > 0 && gxx > 0 && gaa > 0;
        xx += gxx; aa += gaa; xa += gxa;
        na2 += (phi && proj_a) ? gaa - gxa * gxa / gxx : gaa;
        nx2 += (phi && proj_x) ? gxx - gxa * gxa / gaa : gxx;
        cnt += phi ? 1.0 : 0.0;
    }
    xx = block_sum_d(xx, sh); aa = block_sum_d(aa, sh); xa = block_sum_d(xa, sh);
    na2 = block_sum_d(na2, sh); nx2 = block_sum_d(nx2, sh); cnt = block_sum_d(cnt, sh);
    if (na2 < 0) na2 = 0;
    if (nx2 < 0) nx2 = 0;
    double s = (double)knob / sqrt(na2);
    if (mode == 2 && isinf(s)) s = 0;
    double g2 = 0;
    for (int g = threadIdx.x; g < T; g += kThreads) {
        const double gxx = gsum[3 * g], gaa = gsum[3 * g + 1], gxa = gsum[3 * g + 2];
        const bool phi = gxa > 0 && gxx > 0 && gaa > 0;
        const double ca = (phi && proj_x) ? s + gxa / gaa : s;
        const double cx = (phi && proj_a) ? 1.0 + s * gxa / gxx : 1.0;
        coef[2 * g] = (float)cx; coef[2 * g + 1] = (float)ca;
        g2 += cx * cx * gxx - 2 * cx * ca * gxa + ca * ca * gaa;
    }
    g2 = block_sum_d(g2, sh);
    if (threadIdx.x != 0) return;
    if (g2 < 0) g2 = 0;
    const double gn = sqrt(g2), nx = sqrt(xx), na = sqrt(aa);
    double clip = (double)max_norm / (gn + 1e-6);   // torch.nn.utils.clip_grad_norm_
    if (clip > 1) clip = 1;
    StepScalars* sc = reinterpret_cast<StepScalars*>(scalars);
    const float step = sc->step + 1.f;
    sc->norm_x = (float)nx; sc->norm_a = (float)na; sc->dot = (float)xa; sc->scale = (float)s;
    sc->pre_clip_norm = (float)gn; sc->clip_coef = (float)clip; sc->step = step;
    sc->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    sc->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    scalars[kSlotConflicts] = (float)cnt;
    scalars[kSlotCos] = (nx > 0 && na > 0) ? (float)(xa / (nx * na)) : 0.f;
    scalars[kSlotRemovedA] = aa > 0 ? (float)(1.0 - na2 / aa) : 0.f;
    scalars[kSlotRemovedX] = xx > 0 ? (float)(1.0 - nx2 / xx) : 0.f;
}

// pass 2 over the same jobs: x' = cx x (one rounding; exact where cx = 1), then AdamWStep with ca in the place of s
__global__ __launch_bounds__(kThreads) void recombine_surgery_kernel(
    const float* __restrict__ gx, const float* __restrict__ ga, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
    bf16_t* __restrict__ shadow, float* __restrict__ g_out, const long* __restrict__ plan, long jobs, int T, long n, long chunk,
    const float* __restrict__ coef, float lr, float beta1, float beta2, float eps, float wd, const StepScalars* __restrict__ sc) {
    const Plan pl(plan, jobs, T, n, chunk);
    AdamWStep upd(sc, lr, beta1, beta2, eps, wd);
    for (long j = blockIdx.x; j < jobs; j += gridDim.x) {
        long st, len;
        const long g = pl.job(j, st, len);
        if (g < 0) continue;
        const float cx = coef[2 * g];
        upd.s = coef[2 * g + 1];
        const long nvec = len / 4, v0 = st / 4;
        for (long k = threadIdx.x; k < nvec; k += kThreads) {
            const long i = v0 + k;
            f32x4_t x = reinterpret_cast<const f32x4_t*>(gx)[i];
            const f32x4_t a = reinterpret_cast<const f32x4_t*>(ga)[i];
            f32x4_t pp = reinterpret_cast<f32x4_t*>(p)[i], mm = reinterpret_cast<f32x4_t*>(m)[i], vv = reinterpret_cast<f32x4_t*>(v)[i], gg;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float P = pp[e], M = mm[e], V = vv[e];
                gg[e] = upd(__fmul_rn(cx, x[e]), a[e], P, M, V);
                pp[e] = P; mm[e] = M; vv[e] = V;
            }
            reinterpret_cast<f32x4_t*>(p)[i] = pp;
            reinterpret_cast<f32x4_t*>(m)[i] = mm;
            reinterpret_cast<f32x4_t*>(v)[i] = vv;
            if (g_out) reinterpret_cast<f32x4_t*>(g_out)[i] = gg;
            if (shadow) reinterpret_cast<u32x2_t*>(shadow)[i] = u32x2_t{pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3])};
        }
        for (long i = st + nvec * 4 + threadIdx.x; i < st + len; i += kThreads) {
            float P = p[i], M = m[i], V = v[i];
            const float gv = upd(__fmul_rn(cx, gx[i]), ga[i], P, M, V);
            p[i] = P; m[i] = M; v[i] = V;
            if (g_out) g_out[i] = gv;
            if (shadow) shadow[i] = f2bf(P);
        }
    }
}

// The HOST group table: T + 1 ascending offsets (floats), groups[0] = 0, groups[T] = n, every inner offset a multiple of 4.  Returns
// the job count of the table at chunk length C, or -1.
long jobs_of(const long* groups, int T, long n, long C) {
    if (!groups || T < 1 || n < 1 || groups[0] != 0 || groups[T] != n) return -1;
    long jobs = 0;
    for (int g = 0; g < T; ++g) {
        const long len = groups[g + 1] - groups[g];
        if (len <= 0 || (g > 0 && groups[g] % 4 != 0)) return -1;
        jobs += (len + C - 1) / C;
    }
    return jobs;
}

inline int persistent_grid(long jobs) { return (int)(jobs < g_max_blocks ? jobs : g_max_blocks); }

}  // namespace

extern "C" {

// Floats per job of the surgery passes: a multiple of 1024.  Each group of the buffer is cut into jobs of this length from its start.
long siss_surgery_chunk(void) { return g_chunk; }
// Words (doubles) of the caller-owned slab `partials` of siss_grad_norms_scale_surgery for a plan of `jobs` jobs: one row of 3 per job.
long siss_surgery_partials_words(long jobs) { return 3L * (jobs > 0 ? jobs : 0); }
// Words (floats) of the coefficient table of `groups` groups: (cx, ca) per group.  The slab of the f64 group sums holds 3 doubles
// per group.
long siss_surgery_coef_words(long groups) { return 2L * (groups > 0 ? groups : 0); }
// Process-local TEST configuration: the chunk length (a positive multiple of 1024; 0: the default) and the cap of the persistent
// grids (1 .. 2048; 0: the default).  A plan belongs to the chunk length it was built with.  The results do not depend on the cap.
int siss_surgery_test_config(long chunk, int max_blocks) {
    SISS_CHECK_ARG(chunk >= 0 && chunk % 1024 == 0 && max_blocks >= 0 && max_blocks <= kMaxBlocks);
    g_chunk = chunk ? chunk : kDefaultChunk;
    g_max_blocks = max_blocks ? max_blocks : kMaxBlocks;
    return SISS_OK;
}

// Pass 1 of the update with gradient surgery, per group of the flat pair (gx, ga) of n floats.  groups: T + 1 ascending offsets in
// HOST memory (floats; groups[0] = 0, groups[T] = n, every inner offset a multiple of 4, no empty group) -- read here, on the host,
// so that a table that does not describe the buffer is refused without a synchronisation.  plan: the DEVICE table of 2 * jobs + 2 *
// (T + 1) longs: the first float of every job, its group, the first job of every group (T + 1 prefix counts) and the T + 1 offsets
// again; a group is cut into jobs of siss_surgery_chunk() floats from its start, and `jobs` must be the count that follows from
// `groups`.  smode: 0 forget (a' = a - (xa / xx) x on the groups with xa > 0), 1 keep (x' = x - (xa / aa) a there), 2 mutual (both,
// each from the original pair).  mode: 0 (s = knob / |a'|) or 2 (the same, 0 where it would be inf); EraseDiff's mode 1 is refused.
// Writes: partials (siss_surgery_partials_words(jobs) doubles: one row of the three sums per job), group_sums (3 doubles per group),
// coef (siss_surgery_coef_words(T) floats: cx = (float)(1 + s xa / xx) where a is projected, else 1; ca = (float)(s + xa / aa) where
// x is projected, else (float)s) and the 16-float block `scalars`: slots 0-2 |x|, |a|, <x, a> of the ORIGINAL pair, 3 s, 4 the
// pre-clip norm of cx x - ca a from the unrounded coefficients, 5, 6, 8, 9 as siss_grad_norms_scale, 12 the number of conflicting
// groups, 13 the cosine of the pair, 14 1 - |a'|^2 / |a|^2, 15 1 - |x'|^2 / |x|^2 (0 where the denominator is 0); 7, 10, 11 are not
// written.  gx, ga 16-byte aligned.  No atomics, no dependence on the grid: bitwise repeatable.
int siss_grad_norms_scale_surgery(const float* gx, const float* ga, long n, const long* groups, int T, const long* plan, long jobs,
                                  int smode, int mode, float knob, float max_norm, float beta1, float beta2, double* partials,
                                  double* group_sums, float* coef, float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && groups && plan && partials && group_sums && coef && scalars && n > 0 && T >= 1);
    SISS_CHECK_ARG((mode == 0 || mode == 2) && smode >= 0 && smode <= 2);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga) % 16 == 0 && ((uintptr_t)plan | (uintptr_t)partials | (uintptr_t)group_sums) % 8 == 0);
    SISS_CHECK_ARG(jobs > 0 && jobs_of(groups, T, n, g_chunk) == jobs);
    hipStream_t s = (hipStream_t)stream;
    gram_kernel<<<persistent_grid(jobs), kThreads, 0, s>>>(gx, ga, plan, jobs, T, n, g_chunk, partials);
    group_fold_kernel<<<cdiv(T, kThreads / 64), kThreads, 0, s>>>(partials, plan, jobs, T, group_sums);
    scalars_coef_kernel<<<1, kThreads, 0, s>>>(group_sums, T, smode, mode, knob, max_norm, beta1, beta2, coef, scalars);
    SISS_LAUNCH_RET();
}

// Pass 2 on the same plan: g = clip * (cx_G x - ca_G a) -- cx x, ca a, the difference and the product with clip each one f32
// round-to-nearest operation -- then the AdamW update of siss_recombine_clip_adamw on p, m, v, the optional bf16 shadow and the
// optional g_out; every float of [0, n) belongs to exactly one job.  coef and scalars: what siss_grad_norms_scale_surgery wrote.
int siss_recombine_clip_adamw_surgery(const float* gx, const float* ga, float* p, float* m, float* v, void* shadow, float* g_out,
                                      long n, const long* groups, int T, const long* plan, long jobs, const float* coef, float lr,
                                      float beta1, float beta2, float eps, float wd, const float* scalars, void* stream) {
    SISS_CHECK_ARG(gx && ga && p && m && v && groups && plan && coef && scalars && n > 0 && T >= 1);
    SISS_CHECK_ARG(((uintptr_t)gx | (uintptr_t)ga | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) % 16 == 0 && (uintptr_t)plan % 8 == 0);
    SISS_CHECK_ARG((!shadow || (uintptr_t)shadow % 8 == 0) && (!g_out || (uintptr_t)g_out % 16 == 0));
    SISS_CHECK_ARG(jobs > 0 && jobs_of(groups, T, n, g_chunk) == jobs);
    recombine_surgery_kernel<<<persistent_grid(jobs), kThreads, 0, (hipStream_t)stream>>>(
        gx, ga, p, m, v, reinterpret_cast<bf16_t*>(shadow), g_out, plan, jobs, T, n, g_chunk, coef, lr, beta1, beta2, eps, wd,
        reinterpret_cast<const StepScalars*>(scalars));
    SISS_LAUNCH_RET();
}

}  // extern "C"

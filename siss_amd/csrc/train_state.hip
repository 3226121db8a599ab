// The training state of the DDPM pre-training task: single-set clip + AdamW with the EMA of the weights, and the swap that puts the
// EMA weights under the engine for an evaluation.
//
// Reference semantics: train_unconditional.py:366-415 (F.mse_loss -> accelerator.backward -> clip_grad_norm_(1.0) -> AdamW.step ->
// ema_model.step(model.parameters())) with diffusers 0.27.2 training_utils.EMAModel (get_decay / step).  The delete tasks' update
// (optimizer.hip) streams two gradient sets; a plain MSE step has one, and the EMA line reads the parameter the update just wrote:
//   pass 1  reads g                          -> ||g||^2 (f64 slabs) -> the step's scalar block (clip, bias corrections, EMA decay)
//   pass 2  reads g, p, m, v, ema; writes p, m, v, ema (+ bf16 shadow of p, + the clipped gradient)
// All scalars stay on the device: no host sync.  The sums, the element-wise update and the scalar block use the constructions of
// norms_kernel / scalars_kernel / recombine_adamw_kernel::upd operation for operation, so that with a zero second set the two
// pairs of launches agree bit for bit (tests/test_hip_train_state.py).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

struct TrainScalars {   // lives in device memory; 16 floats
    float grad_norm, clip_coef, step, bc1;                 // 0..3  (step = optimizer steps taken, counted in f32)
    float bc2_sqrt, ema_step, one_minus_decay, ema_decay;  // 4..7  (ema_step = EMAModel.optimization_step)
    float pad[8];
};

inline int grid_for(long n) {
    long b = (n / 4 + kThreads - 1) / kThreads;
    if (b < 1) b = 1;
    if (b > kMaxBlocks) b = kMaxBlocks;
    return (int)b;
}

struct EmaSchedule { double max_decay, min_decay, inv_gamma, power; int use_warmup, update_after; };

// EMAModel.step's bookkeeping: optimization_step += 1, decay = get_decay(optimization_step); everything in double, 1 - decay
// rounded ONCE (an f32 `1.f - decay` at decay = 0.9999 is off by 6e-4 of the EMA's step size).
__device__ void ema_advance(TrainScalars* sc, const EmaSchedule& e) {
    const float k = sc->ema_step + 1.f;
    double s = (double)k - (double)e.update_after - 1.0;
    if (s < 0) s = 0;
    double decay = 0.0;
    if (s > 0) {
        decay = e.use_warmup ? 1.0 - pow(1.0 + s / e.inv_gamma, -e.power) : (1.0 + s) / (10.0 + s);
        decay = decay < e.max_decay ? decay : e.max_decay;
        decay = decay > e.min_decay ? decay : e.min_decay;
    }
    sc->ema_step = k;
    sc->one_minus_decay = (float)(1.0 - decay);
    sc->ema_decay = (float)decay;
}

__global__ __launch_bounds__(kThreads) void norm_single_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
    __shared__ double sh[kThreads / 64];
    double sxx = 0;
    const long nvec = n / 4;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        f32x4_t x = reinterpret_cast<const f32x4_t*>(g)[i];
        float pxx = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) pxx += x[j] * x[j];
        sxx += pxx;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) sxx += (double)g[i] * g[i];
    sxx = wave_sum_d(sxx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sxx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0;
        for (int i = 0; i < kThreads / 64; ++i) a += sh[i];
        partials[blockIdx.x] = a;
    }
}

// one block folds the per-block sums (fixed lane -> index map: deterministic) and writes the step's scalars
__global__ void train_scalars_kernel(const double* __restrict__ partials, int nblk, float max_norm, float beta1, float beta2,
                                     EmaSchedule ema, TrainScalars* __restrict__ sc) {
    __shared__ double shs[kThreads / 64];
    double xx = 0;
    for (int i = threadIdx.x; i < nblk; i += kThreads) xx += partials[i];
    xx = wave_sum_d(xx);
    if ((threadIdx.x & 63) == 0) shs[threadIdx.x >> 6] = xx;
    __syncthreads();
    if (threadIdx.x != 0) return;
    xx = 0;
    for (int i = 0; i < kThreads / 64; ++i) xx += shs[i];
    const double gn = sqrt(xx);
    double coef = (double)max_norm / (gn + 1e-6);   // torch.nn.utils.clip_grad_norm_
    if (coef > 1) coef = 1;
    const float step = sc->step + 1.f;
    sc->grad_norm = (float)gn; sc->clip_coef = (float)coef; sc->step = step;
    // in double, ONE rounding (scalars_kernel of optimizer.hip)
    sc->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    sc->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    ema_advance(sc, ema);
}

__global__ void ema_advance_kernel(EmaSchedule ema, TrainScalars* __restrict__ sc) { ema_advance(sc, ema); }

// s_param.sub_(one_minus_decay * (s_param - param))
__device__ __forceinline__ float ema_line(float e, float p, float omd) { return __fsub_rn(e, __fmul_rn(omd, __fsub_rn(e, p))); }

// pass 2: g' = clip * g; torch.optim.AdamW single-tensor update order (recombine_adamw_kernel::upd); the EMA line on the NEW p.
__global__ __launch_bounds__(kThreads) void clip_adamw_ema_kernel(
    const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
    bf16_t* __restrict__ shadow, float* __restrict__ g_out, long n, float lr, float beta1, float beta2, float eps, float wd,
    const TrainScalars* __restrict__ sc) {
    const float clip = sc->clip_coef, bc1 = sc->bc1, bc2s = sc->bc2_sqrt, omd = sc->one_minus_decay;
    const float step_size = lr / bc1;
    const float decay = 1.f - lr * wd;
    const long nvec = n / 4;
    auto upd = [&](float x, float& pp, float& mm, float& vv) -> float {
        const float gg = __fmul_rn(x, clip);
        pp = __fmul_rn(pp, decay);
        mm = __fadd_rn(mm, __fmul_rn(__fsub_rn(gg, mm), 1.f - beta1));           // lerp
        vv = __fadd_rn(__fmul_rn(vv, beta2), __fmul_rn(__fmul_rn(gg, gg), 1.f - beta2));
        const float den = __fadd_rn(sqrtf(vv) / bc2s, eps);
        pp = __fsub_rn(pp, __fmul_rn(step_size, mm / den));
        return gg;
    };
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        f32x4_t x = reinterpret_cast<const f32x4_t*>(g)[i];
        f32x4_t pp = reinterpret_cast<f32x4_t*>(p)[i], mm = reinterpret_cast<f32x4_t*>(m)[i],
                vv = reinterpret_cast<f32x4_t*>(v)[i], gg;
#pragma unroll
        for (int j = 0; j < 4; ++j) { float P = pp[j], M = mm[j], V = vv[j]; gg[j] = upd(x[j], P, M, V); pp[j] = P; mm[j] = M; vv[j] = V; }
        reinterpret_cast<f32x4_t*>(p)[i] = pp;
        reinterpret_cast<f32x4_t*>(m)[i] = mm;
        reinterpret_cast<f32x4_t*>(v)[i] = vv;
        if (ema) {
            f32x4_t ee = reinterpret_cast<f32x4_t*>(ema)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) ee[j] = ema_line(ee[j], pp[j], omd);
            reinterpret_cast<f32x4_t*>(ema)[i] = ee;
        }
        if (g_out) reinterpret_cast<f32x4_t*>(g_out)[i] = gg;
        if (shadow) reinterpret_cast<u32x2_t*>(shadow)[i] = u32x2_t{pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3])};
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) {
            float P = p[i], M = m[i], V = v[i];
            const float gg = upd(g[i], P, M, V);
            p[i] = P; m[i] = M; v[i] = V;
            if (ema) ema[i] = ema_line(ema[i], P, omd);
            if (g_out) g_out[i] = gg;
            if (shadow) shadow[i] = f2bf(P);
        }
}

__global__ __launch_bounds__(kThreads) void ema_step_kernel(const float* __restrict__ p, float* __restrict__ ema, long n,
                                                            const TrainScalars* __restrict__ sc) {
    const float omd = sc->one_minus_decay;
    const long nvec = n / 4;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        f32x4_t pp = reinterpret_cast<const f32x4_t*>(p)[i], ee = reinterpret_cast<f32x4_t*>(ema)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = ema_line(ee[j], pp[j], omd);
        reinterpret_cast<f32x4_t*>(ema)[i] = ee;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) ema[i] = ema_line(ema[i], p[i], omd);
}

__global__ __launch_bounds__(kThreads) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, bf16_t* __restrict__ shadow, long n) {
    const long nvec = n / 4;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
        f32x4_t x = reinterpret_cast<f32x4_t*>(a)[i], y = reinterpret_cast<f32x4_t*>(b)[i];
        reinterpret_cast<f32x4_t*>(a)[i] = y;
        reinterpret_cast<f32x4_t*>(b)[i] = x;
        if (shadow) reinterpret_cast<u32x2_t*>(shadow)[i] = u32x2_t{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3])};
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < n; i += kThreads) {
            const float x = a[i], y = b[i];
            a[i] = y; b[i] = x;
            if (shadow) shadow[i] = f2bf(y);
        }
}

inline bool schedule_ok(double max_decay, double min_decay, double inv_gamma, double power, int update_after) {
    return max_decay >= 0 && max_decay <= 1 && min_decay >= 0 && min_decay <= 1 && inv_gamma > 0 && power > 0 && update_after >= 0;
}

}  // namespace

extern "C" {

long siss_train_partials_words(void) { return kMaxBlocks; }
// The scalar block of the single-set update, 16 floats: 0 pre-clip ||g||, 1 clip coefficient, 2 optimizer step count, 3 bc1,
// 4 bc2_sqrt, 5 the EMA's optimization_step, 6 one_minus_decay, 7 decay (as logged); 8..15 unused.
long siss_train_scalars_words(void) { return sizeof(TrainScalars) / sizeof(float); }

// pass 1 of the single-set update + on-device scalars.  `scalars` (siss_train_scalars_words floats, zero-initialised once) holds
// both step counts; this call increments them.  EMA decay: diffusers EMAModel.get_decay (warmup: 1 - (1 + s / inv_gamma)^-power,
// else (1 + s) / (10 + s), s = max(0, step - update_after - 1); clamped to [min_decay, max_decay]; 0 while s = 0).
int siss_grad_norm_single(const float* g, long n, float max_norm, float beta1, float beta2, double ema_max_decay,
                          double ema_min_decay, double ema_inv_gamma, double ema_power, int ema_use_warmup, int ema_update_after,
                          double* partials, float* scalars, void* stream) {
    SISS_CHECK_ARG(g && partials && scalars && n > 0 && (uintptr_t)g % 16 == 0);
    SISS_CHECK_ARG(schedule_ok(ema_max_decay, ema_min_decay, ema_inv_gamma, ema_power, ema_update_after));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = grid_for(n);
    norm_single_kernel<<<nblk, kThreads, 0, s>>>(g, n, partials);
    train_scalars_kernel<<<1, kThreads, 0, s>>>(partials, nblk, max_norm, beta1, beta2,
                                                EmaSchedule{ema_max_decay, ema_min_decay, ema_inv_gamma, ema_power, ema_use_warmup, ema_update_after},
                                                reinterpret_cast<TrainScalars*>(scalars));
    SISS_LAUNCH_RET();
}

// pass 2 of the single-set update: g' = clip * g, AdamW on (p, m, v), then ema -= one_minus_decay * (ema - p) on the NEW p.
// ema, shadow (bf16 copy of the updated parameters) and g_out (the clipped gradient) are optional.
int siss_clip_adamw_ema(const float* g, float* p, float* m, float* v, float* ema, void* shadow, float* g_out, long n,
                        float lr, float beta1, float beta2, float eps, float wd, const float* scalars, void* stream) {
    SISS_CHECK_ARG(g && p && m && v && scalars && n > 0);
    SISS_CHECK_ARG(((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)g_out) % 16 == 0);
    SISS_CHECK_ARG(!shadow || (uintptr_t)shadow % 8 == 0);
    clip_adamw_ema_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(
        g, p, m, v, ema, reinterpret_cast<bf16_t*>(shadow), g_out, n, lr, beta1, beta2, eps, wd,
        reinterpret_cast<const TrainScalars*>(scalars));
    SISS_LAUNCH_RET();
}

// EMAModel.step's bookkeeping alone: increments the block's optimization_step and forms one_minus_decay (one thread).
int siss_ema_advance(double ema_max_decay, double ema_min_decay, double ema_inv_gamma, double ema_power, int ema_use_warmup,
                     int ema_update_after, float* scalars, void* stream) {
    SISS_CHECK_ARG(scalars && schedule_ok(ema_max_decay, ema_min_decay, ema_inv_gamma, ema_power, ema_update_after));
    ema_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(
        EmaSchedule{ema_max_decay, ema_min_decay, ema_inv_gamma, ema_power, ema_use_warmup, ema_update_after},
        reinterpret_cast<TrainScalars*>(scalars));
    SISS_LAUNCH_RET();
}

// The EMA line alone, ema -= one_minus_decay * (ema - p) with the block's one_minus_decay: EMAModel.step() after an update that
// something else made (siss_ema_advance first).
int siss_ema_step(const float* p, float* ema, long n, const float* scalars, void* stream) {
    SISS_CHECK_ARG(p && ema && scalars && n > 0 && ((uintptr_t)p | (uintptr_t)ema) % 16 == 0);
    ema_step_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(p, ema, n, reinterpret_cast<const TrainScalars*>(scalars));
    SISS_LAUNCH_RET();
}

// a <-> b in one pass; shadow (optional) receives the bf16 rounding of the new a.
int siss_swap_f32(float* a, float* b, void* shadow, long n, void* stream) {
    SISS_CHECK_ARG(a && b && a != b && n > 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0);
    SISS_CHECK_ARG(!shadow || (uintptr_t)shadow % 8 == 0);
    swap_f32_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(a, b, reinterpret_cast<bf16_t*>(shadow), n);
    SISS_LAUNCH_RET();
}

}  // extern "C"

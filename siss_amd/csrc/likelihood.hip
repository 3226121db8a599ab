// The likelihood metric's device side (siss_amd/likelihood.py): the probability-flow drift of the VP-SDE with its Hutchinson
// divergence, and the f64 Runge-Kutta arithmetic of an RK45 integration over the joint state [x ; delta log p].
//
// Built with -ffp-contract=off (build.py EXACT): the drift is bitwise torch's f32 expression, and the f64 stage sums keep the
// product-then-sum rounding of the numpy integrator they restate.  Per-block partial sums go to slabs that a consumer sums in a
// fixed order -- no atomics, so every number here is reproducible run to run.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTerms = 8;

struct RkTerms {                  // siss_rk_terms of include/siss_hip.h
    const double* row[kMaxTerms];
    double c[kMaxTerms];
    int n;
};

// sum over the block in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kThreads / 64; ++i) s += sh[i];
    return s;
}

// The reverse-SDE drift of the probability-flow ODE (metrics/song_likelihood: rsde.sde(x, t)[0] with the discrete-time VP score
// -pred / std), in torch's f32 order:  (-0.5 * beta) * x  -  ((sqrt(beta) ** 2) * (-pred / std)) * 0.5.
// The divergence of that drift along the Hutchinson probe e, in f64, given v = J^T e (J = d pred / d x):
//   e . (-0.5 beta e)  +  e . (0.5 beta / std v)
// par = [beta(t), std(t), sqrt(beta(t)) ** 2] (f32, device: one captured graph serves every t; the squared root is formed by the host
// with IEEE f32 sqrt, as torch's sqrt rounds it).  blockIdx.y = sample.
__global__ __launch_bounds__(kThreads) void pflow_drift_div_kernel(const float* __restrict__ x, const float* __restrict__ pred,
                                                                   const float* __restrict__ v, const float* __restrict__ eps,
                                                                   const float* __restrict__ par, double* __restrict__ drift,
                                                                   double* __restrict__ partials, long chw) {
    __shared__ double sh[kThreads / 64];
    const long base = (long)blockIdx.y * chw;
    const float beta = par[0], sd = par[1], g2 = par[2];
    const float hb = __fmul_rn(-0.5f, beta);
    const double cb = -0.5 * (double)beta, cv = 0.5 * (double)beta / (double)sd;
    double acc = 0;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < chw; k += (long)gridDim.x * kThreads) {
        const long i = base + k;
        const float score = __fdiv_rn(-pred[i], sd);
        drift[i] = (double)__fsub_rn(__fmul_rn(hb, x[i]), __fmul_rn(__fmul_rn(g2, score), 0.5f));
        const double e = eps[i];
        acc += e * (cb * e) + e * (cv * (double)v[i]);
    }
    const double s = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// out[r] = sum of slab row r, left to right
__global__ void slab_rowsum_kernel(const double* __restrict__ slab, double* __restrict__ out, int rows, int cols) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s = 0;
    for (int c = 0; c < cols; ++c) s += slab[(long)r * cols + c];
    out[r] = s;
}

// out = y + (sum_j c_j row_j) * h   (numpy's `y + np.dot(K[:s].T, a[:s]) * h`), and its f32 cast over the first n32 entries
__global__ __launch_bounds__(kThreads) void rk_combine_kernel(RkTerms T, const double* __restrict__ y, double h, double* __restrict__ out,
                                                              float* __restrict__ out32, long n32, long n) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        double acc = 0;
        for (int j = 0; j < T.n; ++j) acc += T.c[j] * T.row[j][i];
        const double r = y[i] + acc * h;
        if (out) out[i] = r;
        if (i < n32) out32[i] = (float)r;
    }
}

// per-block partials of sum_i (((sum_j c_j row_j[i]) * h) / (atol + max(|y[i]|, |y2[i]|) * rtol))^2   (y2 may be null)
__global__ __launch_bounds__(kThreads) void rk_norm_kernel(RkTerms T, double h, const double* __restrict__ y, const double* __restrict__ y2,
                                                           double rtol, double atol, long n, double* __restrict__ partials) {
    __shared__ double sh[kThreads / 64];
    double acc = 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        double v = 0;
        for (int j = 0; j < T.n; ++j) v += T.c[j] * T.row[j][i];
        v = v * h;
        double a = fabs(y[i]);
        if (y2) a = fmax(a, fabs(y2[i]));
        const double q = v / (atol + a * rtol);
        acc += q * q;
    }
    const double s = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

bool terms_ok(const RkTerms* t) {
    if (!t || t->n < 0 || t->n > kMaxTerms) return false;
    for (int j = 0; j < t->n; ++j)
        if (!t->row[j]) return false;
    return true;
}

}  // namespace

extern "C" {

// Probability-flow drift + Hutchinson divergence of the VP-SDE, one launch per function evaluation.  x, pred (the UNet's eps
// prediction), v (= J^T eps, UNetEngine.input_vjp) and eps (the probe): [B][chw] f32; par = [beta(t), std(t), sqrt(beta(t)) ** 2] f32
// on the device.
// drift[B * chw] (f64) receives the drift; partials[B][nblk] (f64) the per-block divergence sums (the caller sums a sample's nblk
// partials in order: siss_slab_rowsum_f64).  nblk blocks per sample, 1..1024.
int siss_pflow_drift_div(const float* x, const float* pred, const float* v, const float* eps, const float* par, double* drift,
                         double* partials, int B, long chw, int nblk, void* stream) {
    SISS_CHECK_ARG(x && pred && v && eps && par && drift && partials && B > 0 && B <= 65535 && chw > 0 && nblk >= 1 && nblk <= 1024);
    pflow_drift_div_kernel<<<dim3(nblk, B), kThreads, 0, (hipStream_t)stream>>>(x, pred, v, eps, par, drift, partials, chw);
    SISS_LAUNCH_RET();
}

// out[r] = sum_{c < cols} slab[r][cols] in order (f64), r < rows
int siss_slab_rowsum_f64(const double* slab, double* out, int rows, int cols, void* stream) {
    SISS_CHECK_ARG(slab && out && rows > 0 && cols > 0);
    slab_rowsum_kernel<<<cdiv(rows, 64), 64, 0, (hipStream_t)stream>>>(slab, out, rows, cols);
    SISS_LAUNCH_RET();
}

// One Runge-Kutta stage input over n f64 entries: out = y + (sum_j terms.c[j] * terms.row[j]) * h (out may be null), and
// out32[i] = (float) that value for i < n32 (out32 may be null when n32 = 0): the next model input.  terms: host struct, <= 8 rows.
int siss_rk_combine(const void* terms, const double* y, double h, double* out, float* out32, long n32, long n, void* stream) {
    const RkTerms* t = (const RkTerms*)terms;
    SISS_CHECK_ARG(terms_ok(t) && y && n > 0 && n32 >= 0 && n32 <= n && (out || out32) && (n32 == 0 || out32));
    long nb = (n + kThreads - 1) / kThreads;
    if (nb > 2048) nb = 2048;
    rk_combine_kernel<<<(int)nb, kThreads, 0, (hipStream_t)stream>>>(*t, y, h, out, out32, n32, n);
    SISS_LAUNCH_RET();
}

// Weighted RMS-norm partials of the RK45 controller: partials[b] (b < nblk) = the block's share of
// sum_i ((sum_j c_j row_j[i]) * h / (atol + max(|y[i]|, |y2[i]|) * rtol))^2 over n entries (y2 may be null).  The caller sums the
// nblk partials in order.
int siss_rk_norm(const void* terms, double h, const double* y, const double* y2, double rtol, double atol, long n, double* partials,
                 int nblk, void* stream) {
    const RkTerms* t = (const RkTerms*)terms;
    SISS_CHECK_ARG(terms_ok(t) && y && n > 0 && partials && nblk >= 1 && nblk <= 1024);
    rk_norm_kernel<<<nblk, kThreads, 0, (hipStream_t)stream>>>(*t, h, y, y2, rtol, atol, n, partials);
    SISS_LAUNCH_RET();
}

}  // extern "C"

// Host side of a GroupNorm backward: one struct describes a call to groupnorm.hip's launchers, groupnorm_slab.hip's one-launch
// kernels and f32_path.hip's instrument (the comments above siss_groupnorm_bwd_ld / _ld_s2d / _sc say what the fields mean).
#pragma once
struct GNBwdCall {
    const void *dy, *x; const float *gamma, *beta, *mean, *rstd; void* dx; const void *accum, *accum2; void* dx2;
    int split_c, accumulate2; float *dgamma, *dbeta, *colsum; long colsum_ld; float* partial; int n2, nx, set_images; long set_stride;
    int H, W, C, G, silu, dy_compact, ldx; void* stream;
};
// siss_groupnorm_bwd_ld's argument list (and its _s2d / _f32 siblings') as a call
inline GNBwdCall gn_bwd_call(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                             void* dx, const void* accum, const void* accum2, void* dx2, int split_c, int accumulate2, float* dgamma,
                             float* dbeta, float* colsum, long colsum_ld, float* partial, int n2, int nx, int set_images, long set_stride,
                             int H, int W, int C, int G, int silu, int dy_compact, int ldx, void* stream) {
    GNBwdCall c = {};
    c.dy = dy; c.x = x; c.gamma = gamma; c.beta = beta; c.mean = mean; c.rstd = rstd; c.dx = dx; c.accum = accum; c.accum2 = accum2;
    c.dx2 = dx2; c.split_c = split_c; c.accumulate2 = accumulate2; c.dgamma = dgamma; c.dbeta = dbeta; c.colsum = colsum;
    c.colsum_ld = colsum_ld; c.partial = partial; c.n2 = n2; c.nx = nx; c.set_images = set_images; c.set_stride = set_stride;
    c.H = H; c.W = W; c.C = C; c.G = G; c.silu = silu; c.dy_compact = dy_compact; c.ldx = ldx; c.stream = stream;
    return c;
}
// The slab kernels (small sites): SISS_OK / error, or -1 when the site is not covered.
int siss_gn_slab_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int N, int H,
                     int W, int C, int G, float eps, int silu, int out_compact, int ldx, void* stream);
int siss_gn_slab_bwd(const GNBwdCall& c);

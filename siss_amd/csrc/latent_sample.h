// latent_dist.sample() * scaling_factor of diffusers' DiagonalGaussianDistribution, one element: the ONE statement of it that
// csrc/injection.hip (siss_latent_inject) and csrc/latent_cache.hip (siss_latent_sample) both compile, so the two cannot drift.
// Every product and sum rounded to f32 on its own (both files are built with -ffp-contract=off, build.py EXACT, and the roundings are
// spelled out besides), libm's expf (not a fast intrinsic) -- as torch's chain clamp / mul / exp / mul / add / mul rounds them.
#pragma once
#include "common.h"

//   z = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scaling
__device__ __forceinline__ float posterior_sample(float mean, float logvar, float eps, float scaling) {
    const float lv = fminf(fmaxf(logvar, -30.f), 20.f);
    const float sd = expf(__fmul_rn(0.5f, lv));
    return __fmul_rn(__fadd_rn(mean, __fmul_rn(sd, eps)), scaling);
}

// The VAE decoder's output as bytes: diffusers' postprocess `((img / 2 + 0.5).clamp(0, 1) * 255).round()` on one element, every
// operation rounded where torch rounds it in the tensor's dtype.  ONE definition for the kernels that turn decoded images into
// uint8 (kmeans.hip's fused classifier pass, sscd.hip's preprocessing): the PNG grid, the k-means features and the SSCD input are
// the same bytes.
#pragma once
#include "common.h"

// f32: /2 is exact, +0.5, clamp, *255, rint
__device__ __forceinline__ uint8_t to_u8(float x) {
    float a = __fadd_rn(__fmul_rn(x, 0.5f), 0.5f);
    a = fminf(fmaxf(a, 0.f), 1.f);                       // (a NaN pixel becomes 0 here; torch leaves its uint8 cast undefined)
    return (uint8_t)rintf(__fmul_rn(a, 255.f));
}
// bf16: each torch operation computes in f32 and rounds its result to bf16
__device__ __forceinline__ uint8_t to_u8(bf16_t xb) {
    float a = bfround(__fmul_rn(bf2f(xb), 0.5f));
    a = bfround(__fadd_rn(a, 0.5f));
    a = fminf(fmaxf(a, 0.f), 1.f);
    a = bfround(__fmul_rn(a, 255.f));
    return (uint8_t)bfround(rintf(a));
}

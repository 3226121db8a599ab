// The wave tile of the exact f32 row-set kernels (sscd_search.hip, feature_sets.hip): the 32 x 64 dot products of 32 "query" rows
// against 64 "gallery" rows on eight v_mfma_f32_16x16x4_f32 accumulators.  sscd_tile is the ONLY place either file forms a product:
// the dot product of a pair is the f32 fmaf chain over k = 0, 1, ..., d - 1 from +0, a function of the two rows and d alone.
#pragma once
#include "common.h"

namespace {

constexpr int kQS = 2;           // 16-row query sub-tiles per wave tile: each gallery operand feeds both (5 -> 3 operand loads per 16 MFMAs)
constexpr int kQT = 16 * kQS;    // queries per wave tile
constexpr int kGT = 64;          // gallery rows per wave tile: four 16-column MFMA tiles; 2 x 4 independent accumulators

// lanes (c, h), c = lane & 15, h = lane >> 4, hold x[j] = row_c[k0 + 4 h + j]; afterwards x[s] = row_c[k0 + 4 s + h]: the operand of
// the MFMA step s (A[c][k = h] / B[k = h][c]).  A 4 x 4 transpose between the lane bits 4, 5 and the register index: v_permlane16_swap
// exchanges the odd 16-lane rows of its first operand with the even rows of its second, v_permlane32_swap the upper half of the first
// with the lower half of the second.  Inline asm with its wait states inside (a VALU write needs two before a permlane swap reads it):
// written with __builtin_amdgcn_permlane{16,32}_swap, hipcc 7.2 fed two MFMA steps of a trip the SAME register and loaded one dword
// of the tail's four (seen in the ISA; the exact-data test fails on it).
__device__ __forceinline__ void transpose4(f32x4_t& x) {
    float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    asm volatile("s_nop 1\n\t"
                 "v_permlane16_swap_b32 %0, %1\n\t"
                 "v_permlane16_swap_b32 %2, %3\n\t"
                 "s_nop 1\n\t"
                 "v_permlane32_swap_b32 %0, %2\n\t"
                 "v_permlane32_swap_b32 %1, %3\n\t"
                 "s_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
    x = f32x4_t{x0, x1, x2, x3};
}

__device__ __forceinline__ f32x4_t load4(const float* p, bool on) {
    return on ? *reinterpret_cast<const f32x4_t*>(p) : f32x4_t{0.f, 0.f, 0.f, 0.f};
}

// The 32 x 64 similarities of queries [q0, q0 + 32) against gallery rows [g0, g0 + 64):
// acc[u][t][r] = <q[q0 + 16 u + 4 h + r], g[g0 + 16 t + c]>.  Rows past the end are read as the last row (their results are discarded by
// the caller).  k runs in ascending order, 16 per trip (one 16-byte load per lane and operand, transposed in registers), the d % 16
// tail by the lane groups that own it.  GATHER: nq / ng count the POSITIONS of two int32 row tables and position p stands for row
// qidx[p] of q (gidx[p] of g) -- the rows are read where they lie, no gathered copy is made; the arithmetic is the same.
template <bool GATHER = false>
__device__ __forceinline__ void sscd_tile(const float* __restrict__ q, int nq, const float* __restrict__ g, long ng, int d,
                                          int q0, long g0, int c, int h, f32x4_t (&acc)[kQS][4],
                                          const int* __restrict__ qidx = nullptr, const int* __restrict__ gidx = nullptr) {
    const float* qp[kQS];
    const float* gp[4];
#pragma unroll
    for (int u = 0; u < kQS; ++u) {
        long qr = (long)q0 + 16 * u + c < nq ? (long)q0 + 16 * u + c : (long)nq - 1;
        if (GATHER) qr = qidx[qr];
        qp[u] = q + qr * d + 4 * h;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        long gr = g0 + 16 * t + c < ng ? g0 + 16 * t + c : ng - 1;
        if (GATHER) gr = gidx[gr];
        gp[t] = g + gr * d + 4 * h;
#pragma unroll
        for (int u = 0; u < kQS; ++u) acc[u][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const int dfull = d & ~15;
    f32x4_t a[kQS], b[4];
    if (dfull) {
#pragma unroll
        for (int u = 0; u < kQS; ++u) a[u] = load4(qp[u], true);
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = load4(gp[t], true);
    }
    for (int k0 = 0; k0 < dfull; k0 += 16) {
        f32x4_t an[kQS], bn[4];
#pragma unroll
        for (int u = 0; u < kQS; ++u) an[u] = a[u];
#pragma unroll
        for (int t = 0; t < 4; ++t) bn[t] = b[t];
        if (k0 + 16 < dfull) {                       // the next trip's operands travel under this trip's MFMAs
#pragma unroll
            for (int u = 0; u < kQS; ++u) an[u] = load4(qp[u] + k0 + 16, true);
#pragma unroll
            for (int t = 0; t < 4; ++t) bn[t] = load4(gp[t] + k0 + 16, true);
        }
#pragma unroll
        for (int u = 0; u < kQS; ++u) transpose4(a[u]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            transpose4(b[t]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int u = 0; u < kQS; ++u) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], b[t][s], acc[u][t], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kQS; ++u) a[u] = an[u];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = bn[t];
    }
    const int steps = (d - dfull) >> 2;              // 0 .. 3 MFMA steps of four k each
    if (steps) {
        const bool on = h < steps;                   // lane group h holds the k of step h after the transpose
#pragma unroll
        for (int u = 0; u < kQS; ++u) {
            a[u] = load4(qp[u] + dfull, on);
            transpose4(a[u]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            b[t] = load4(gp[t] + dfull, on);
            transpose4(b[t]);
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s < steps) {
#pragma unroll
                    for (int u = 0; u < kQS; ++u) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], b[t][s], acc[u][t], 0, 0, 0);
                }
        }
    }
}

}  // namespace

// The image store's gather launch (siss_amd/image_store.py ImageStore.images): a pixel-space dataset stays resident on the device as
// uint8, planar, one row per image, and a micro-batch of training images is ONE launch over the rows its indices name -- instead of
// a decode, ToTensor / Normalize in numpy / torch, a stack of f32 images and a host-to-device copy of 4 bytes per sub-pixel, per
// micro-batch (delete_celeb.py:571-580 and train_unconditional.py:366-372 of the reference: a DataLoader in front of the step).
//
//   r = idx[i]
//   out[i, c, y, x] = table[c][ store[r, c, y, x] ]
//
// The transform of these datasets is a fixed per-channel map of a byte, and the table holds its 256 values per channel as the
// dataset's own transform object computed them on the host (image_store.byte_table): the kernel divides nothing and rounds nothing
// in f32, so the batch has the bits of torch.stack([dataset[j] for j in idx]) by construction.  A bf16 out is the table value
// rounded to nearest even.
//
// Streaming kernel, write-bound: 1 byte in, 4 (2) bytes out.  The table sits in LDS (C * 1 KB, filled once per block); a lane reads
// 4 store bytes as one dword and writes one f32x4 -- 256 B in and 1 KiB out per wave instruction, both contiguous.  16 bytes per lane
// on the read side would split the lane's output into four 16-B stores 64 B apart, and the stores are 4/5 of the traffic: the read
// stays narrow so that the write is the wide, coalesced one.  No reduction, no atomics, no scratch.  Built with -ffp-contract=off
// (build.py EXACT), though nothing here could contract.  An index outside [0, rows) is never dereferenced: that sample's output row
// is NaN.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 32;                     // 32 KB of table: under the 64 KB a block has without asking

__device__ __forceinline__ void store4(float* p, long q, f32x4_t v) { reinterpret_cast<f32x4_t*>(p)[q] = v; }
__device__ __forceinline__ void store4(bf16_t* p, long q, f32x4_t v) {               // RNE, NaN stays NaN (common.h pack_bf2)
    reinterpret_cast<u32x2_t*>(p)[q] = u32x2_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
}

// grid (blocks per sample, n); dynamic LDS C * 256 floats.  VEC: chw % 4 == 0, store 4-B aligned and out 16-B aligned (8-B when
// bf16), which makes every row of them aligned: one quad per lane per iteration; else one element per lane.  chw <= 2^30: the
// position inside a row is an int, and the channel of a quad's first byte costs one 32-bit division per quad (a quad may straddle
// two channels when hw % 4 != 0: the channel moves on inside the quad).
template <typename OT, bool VEC>
__global__ __launch_bounds__(kThreads) void image_gather_kernel(const uint8_t* __restrict__ store, const int64_t* __restrict__ idx,
                                                                const float* __restrict__ table, OT* __restrict__ out, long rows,
                                                                int C, int hw) {
    extern __shared__ float tab[];
    for (int k = threadIdx.x; k < C * 256; k += kThreads) tab[k] = table[k];
    __syncthreads();
    const int i = blockIdx.y;
    const int chw = C * hw;
    const long r = idx[i];                                            // block-uniform
    const bool ok = r >= 0 && r < rows;
    const uint8_t* src = store + (ok ? r : 0) * (long)chw;            // (never read when !ok)
    OT* o = out + (long)i * chw;
    const float nan = __builtin_nanf("");
    const int stride = gridDim.x * kThreads;
    if constexpr (VEC) {
        const int nq = chw / 4;
        for (int q = blockIdx.x * kThreads + threadIdx.x; q < nq; q += stride) {
            f32x4_t v{nan, nan, nan, nan};
            if (ok) {
                const uint32_t b = reinterpret_cast<const uint32_t*>(src)[q];
                int c = (4 * q) / hw;
                int left = (c + 1) * hw - 4 * q;                      // elements of channel c from this quad's first on (>= 1)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (left == 0) { ++c; left = hw; }
                    v[k] = tab[c * 256 + ((b >> (8 * k)) & 0xffu)];
                    --left;
                }
            }
            store4(o, q, v);
        }
    } else {
        for (int k = blockIdx.x * kThreads + threadIdx.x; k < chw; k += stride)
            o[k] = from_f<OT>(ok ? tab[(k / hw) * 256 + src[k]] : nan);
    }
}

inline bool aligned(const void* p, int bytes) { return (uintptr_t)p % bytes == 0; }

}  // namespace

extern "C" {

// A micro-batch of training images from a dataset kept on the device as uint8: for i < n, r = idx[i],
// out[i][c][p] = table[c][store[r][c][p]], p < hw.  store [rows][C][hw] uint8, planar (an image is permuted from HWC once, when its
// row is filled); idx [n] int64 on the device; table [C][256] f32: the dataset's transform of every byte value, per channel
// (image_store.byte_table); out [n][C][hw] f32 (out_bf16 = 0) or bf16, the table value rounded to nearest even (1).  An idx[i]
// outside [0, rows) is not dereferenced: out[i] is filled with NaN.  C in 1..32 (the table is held in LDS, C KB), C * hw <= 2^30,
// n in 1..65535; nblk blocks per sample (1..1024), the rest is grid-strided, the result does not depend on it.  One dword of four
// bytes in and one f32x4 (bf16: 8 B) out per lane when C * hw % 4 == 0, store is 4-B and out 16-B (bf16: 8-B) aligned, else one
// element per lane; out must be aligned to its element and table to 4 B, idx to 8 B.  A refused call (status 1) launches nothing.
int siss_image_gather(const void* store, const int64_t* idx, const float* table, void* out, int out_bf16, long rows, int n, int C,
                      long hw, int nblk, void* stream) {
    SISS_CHECK_ARG(store && idx && table && out);
    SISS_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1);
    SISS_CHECK_ARG(n > 0 && n <= 65535 && rows > 0 && nblk >= 1 && nblk <= 1024);
    SISS_CHECK_ARG(C >= 1 && C <= kMaxC && hw > 0 && hw <= (1L << 30) / C);
    SISS_CHECK_ARG(aligned(idx, 8) && aligned(table, 4) && aligned(out, out_bf16 ? 2 : 4));
    const long chw = (long)C * hw;
    const bool vec = chw % 4 == 0 && aligned(store, 4) && aligned(out, out_bf16 ? 8 : 16);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nblk, n);
    const size_t lds = (size_t)C * 256 * sizeof(float);
    const uint8_t* st = (const uint8_t*)store;
    float* of = (float*)out;
    bf16_t* ob = (bf16_t*)out;
    const int ihw = (int)hw;
    if (out_bf16 && vec) image_gather_kernel<bf16_t, true><<<grid, kThreads, lds, s>>>(st, idx, table, ob, rows, C, ihw);
    else if (out_bf16) image_gather_kernel<bf16_t, false><<<grid, kThreads, lds, s>>>(st, idx, table, ob, rows, C, ihw);
    else if (vec) image_gather_kernel<float, true><<<grid, kThreads, lds, s>>>(st, idx, table, of, rows, C, ihw);
    else image_gather_kernel<float, false><<<grid, kThreads, lds, s>>>(st, idx, table, of, rows, C, ihw);
    SISS_LAUNCH_RET();
}

}  // extern "C"

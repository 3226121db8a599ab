// Host side of the two flash-attention families: flash_attn.hip's 16x16x32-MFMA kernels (every shape; the entry points live there) and
// flash_attn32.hip's 32x32x16-MFMA kernels (narrow heads, whole 128-query blocks; round 6).  One args struct per direction serves both.
#pragma once
struct FABwdArgs {
    const void *q, *k, *v, *o, *d_o;                        // o may be null (head-split layout: delta is given, not formed)
    void *dq, *dk, *dv;
    long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;      // row strides in elements (merged layout: head h at column h * D)
    const float* lse2;                                      // [Bf * H][Sq] base-2 log-sum-exp of the forward
    float* delta;                                           // [nB * H][Sq] scratch: rowsum(dO o O), written by the dQ kernel
    int nB, Bf, H, D, Sq, Sk;                               // cotangent batch entries against Bf forward ones (entry b uses b % Bf)
    float scale;
    int pre;                                                // q holds scale * log2(e) * Q
};
bool siss_fa32_bwd_takes(const FABwdArgs& a);
int siss_fa32_bwd(const FABwdArgs& a, void* stream);
struct FAFwdArgs {
    const void *q, *k, *v;
    void* o;
    long ldq, ldk, ldv, ldo;
    float* lse2;                                            // [B * H][Sq]
    int B, H, D, Sq, Sk;
    float scale;
    int pre;
};
bool siss_fa32_fwd_takes(const FAFwdArgs& a);
int siss_fa32_fwd(const FAFwdArgs& a, void* stream);
// Both families' rule for cutting the dK / dV queries into chunks (flash_attn.hip): with fewer than 512 blocks in the grid (kblocks),
// chunks of at least four of the qtiles 64-row query tiles, as many as bring the grid to ~1024 blocks and fit the library workspace at
// chunk_bytes of partial tiles each (a reduce kernel sums them: deterministic, no atomics).  Returns the workspace and sets nch /
// qchunk (rows) when the launch is to be cut; returns null and leaves them alone when it is not.
float* siss_fa_qchunks(long kblocks, int qtiles, long chunk_bytes, int& nch, int& qchunk);

// One weight-gradient product: the argument list of siss_gemm_tn / siss_gemm_tn_bs as a struct, shifts / coffs inline.  The one definition
// for the library's sources; include/siss_hip.h declares the same layout for the callers of siss_gemm_tn_grouped / siss_gemm_tn_pair.
#pragma once
struct siss_tn_job {
    const void* Y; long ldy; const void* X; long ldx; float* dW; long set_stride;
    int N, C, npanels, nsets, rows_per_set, row_begin, row_end, nsplits;
    long x_set_rows;
    const void* zero_page; float* dbias; float* dbias2;
    int shifts[9]; int coffs[9];
    long bias_set_stride;                 // floats between the sets of dbias / dbias2; 0 = set_stride (siss_gemm_tn_bs's extra argument)
};

// Launchers of the FP8 quantisers and the FP8 GEMM (fp8_gemm.hip). Tile
// geometry, shape preconditions and the FP8_FMT_* operand formats are the
// FP8_* constants of common.h; fp8 bytes travel as unsigned char.
#pragma once

#include "common.h"

// x [M, K] bf16 -> q [M, K] fp8 of format fmt, scale [M] fp32 powers of two.
void launch_fp8_quant_rows(const __hip_bfloat16* x, unsigned char* q, float* scale, long M,
                           int K, int fmt, hipStream_t stream);

// Partial rows of the pass-1 workspaces of launch_fp8_quant_cols_t.
int fp8_cols_partials(long R, int C);

// x [R, C] bf16 -> q [C, Rp] fp8, scale [C], colsum [C] fp32.
// q, scale: may both be null (column sums only). colsum: may be null.
// part_amax / part_sum: [fp8_cols_partials(R, C), C] fp32 workspaces (part_sum
// only with colsum).
void launch_fp8_quant_cols_t(const __hip_bfloat16* x, unsigned char* q, float* scale,
                             float* colsum, float* part_amax, float* part_sum, long R, int C,
                             int fmt, hipStream_t stream);

// y [M, N] = bf16((xq . wq^T) sx[m] sw[n] + bias[n]); xq [M, K] of format fmt_x,
// wq [N, K] e4m3; bias may be null and must be with an e5m2 xq.
void launch_fp8_gemm_nt(const unsigned char* xq, const float* sx, const unsigned char* wq,
                        const float* sw, const __hip_bfloat16* bias, __hip_bfloat16* y, long M,
                        int N, int K, int fmt_x, hipStream_t stream);

// One wave: C [16, 16] fp32 = A [16, 128] . Bt [16, 128]^T on fp8 bytes.
void launch_probe_mfma_fp8(const unsigned char* A, const unsigned char* Bt, float* C, int fmt_a,
                           int fmt_b, hipStream_t stream);

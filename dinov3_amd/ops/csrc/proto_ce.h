// Launchers of the prototype-score cross-entropy and Sinkhorn-Knopp kernels
// (proto_ce.hip).
//
// x (student) and xt (teacher) are bf16 prototype scores with K columns; every
// other pointer is fp32. DINO: x [S, B, K], t or xt [T, B, K], lse / st [S B].
// iBOT: x, t or xt [M, K], w / lse / st [M]. The *_fact_* variants rebuild the
// teacher probabilities from xt and the Sinkhorn factors u (rows) and v
// (columns) instead of reading them. inv_temp = 1 / student temperature,
// inv_tt = 1 / teacher temperature; g is the upstream gradient of the scalar
// loss and loss_sum a zeroed accumulator.
#pragma once

#include "common.h"

void launch_dino_ce_fwd(const __hip_bfloat16* x, const float* t, float* lse, float* st,
                        float* loss_sum, int S, int T, int B, long K, float inv_temp,
                        bool ignore_diag, hipStream_t stream);
void launch_dino_ce_bwd(const __hip_bfloat16* x, const float* t, const float* lse,
                        const float* st, const float* g, __hip_bfloat16* dx, int S, int T,
                        int B, long K, float inv_temp, bool ignore_diag,
                        hipStream_t stream);
void launch_ibot_ce_fwd(const __hip_bfloat16* x, const float* t, const float* w,
                        float* lse, float* st, float* loss_sum, int M, long K,
                        float inv_temp, hipStream_t stream);
void launch_ibot_ce_bwd(const __hip_bfloat16* x, const float* t, const float* w,
                        const float* lse, const float* st, const float* g,
                        __hip_bfloat16* dx, int M, long K, float inv_temp,
                        hipStream_t stream);

// A [K] = column sums of exp(x inv_temp) u (u nullptr: ones); u [M] = 1 / row
// sums of exp(x inv_temp) v.
void launch_sinkhorn_fact_colsum(const __hip_bfloat16* x, const float* u, float* A,
                                 int M, long K, float inv_temp, hipStream_t stream);
void launch_sinkhorn_fact_rowsum(const __hip_bfloat16* x, const float* v, float* u,
                                 int M, long K, float inv_temp, hipStream_t stream);

void launch_ibot_ce_fact_fwd(const __hip_bfloat16* x, const __hip_bfloat16* xt,
                             const float* u, const float* v, const float* w, float* lse,
                             float* st, float* loss_sum, int M, long K, float inv_temp,
                             float inv_tt, hipStream_t stream);
void launch_ibot_ce_fact_bwd(const __hip_bfloat16* x, const __hip_bfloat16* xt,
                             const float* u, const float* v, const float* w,
                             const float* lse, const float* st, const float* g,
                             __hip_bfloat16* dx, int M, long K, float inv_temp,
                             float inv_tt, hipStream_t stream);
void launch_dino_ce_fact_fwd(const __hip_bfloat16* x, const __hip_bfloat16* xt,
                             const float* u, const float* v, float* lse, float* st,
                             float* loss_sum, int S, int T, int B, long K, float inv_temp,
                             float inv_tt, bool ignore_diag, hipStream_t stream);
void launch_dino_ce_fact_bwd(const __hip_bfloat16* x, const __hip_bfloat16* xt,
                             const float* u, const float* v, const float* lse,
                             const float* st, const float* g, __hip_bfloat16* dx, int S,
                             int T, int B, long K, float inv_temp, float inv_tt,
                             bool ignore_diag, hipStream_t stream);

// The materialised Sinkhorn: Q [M, K] fp32 = exp(x inv_temp) over n elements
// with their sum added to the zeroed `total`, then column sums and row scaling.
void launch_sinkhorn_exp(const __hip_bfloat16* x, float* Q, float* total, long n,
                         float inv_temp, hipStream_t stream);
void launch_sinkhorn_colsum(const float* Q, float* out, int M, long K,
                            const float* divisor, hipStream_t stream);
void launch_sinkhorn_div_row(float* Q, const float* col, int M, long K, float k_div,
                             const float* B, bool scale_back, hipStream_t stream);

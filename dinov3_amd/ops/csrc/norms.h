// Launchers of the row-wise normalization kernels (norms.hip).
//
// x is [rows, D] contiguous, T is float or __hip_bfloat16; mean, rstd and s
// are fp32 [rows]. Instantiated for both element types.
#pragma once

#include "common.h"

template <typename T>
void launch_layernorm_fwd(const T* x, const T* w, const T* b, T* y, float* mean,
                          float* rstd, long rows, int D, float eps, hipStream_t stream);

// y[r] = LayerNorm(flat[idx[r]]) and sub[r] = flat[idx[r]] in one kernel
// (D % 8 == 0). Grid and block are those of launch_layernorm_fwd.
template <typename T>
void launch_gather_layernorm_fwd(const T* flat, const long* idx, const T* w, const T* b,
                                 T* y, T* sub, float* mean, float* rstd, long rows, int D,
                                 float eps, hipStream_t stream);

// dw / db come out in T; `ws` is an fp32 workspace of 2 * COLRED_MAX_PARTIALS
// rows of D (dgamma partials, then dbeta partials).
template <typename T>
void launch_layernorm_bwd(const T* dy, const T* x, const T* w, const float* mean,
                          const float* rstd, T* dx, float* ws, T* dw, T* db, long rows,
                          int D, hipStream_t stream);

// dacc[idx[r]] += dx[r] of the LayerNorm backward; wave kernel widths only
// (D % 8 == 0, D <= 1536 — the caller checks). dw / db / ws as above.
template <typename T>
void launch_layernorm_bwd_scatter_acc(const T* dy, const T* x, const T* w, const float* mean,
                                      const float* rstd, T* dacc, const long* idx, float* ws,
                                      T* dw, T* db, long rows, int D, hipStream_t stream);

template <typename T>
void launch_rmsnorm_fwd(const T* x, const T* w, T* y, float* rstd, long rows, int D,
                        float eps, hipStream_t stream);
// `ws`: COLRED_MAX_PARTIALS rows of D (dgamma partials).
template <typename T>
void launch_rmsnorm_bwd(const T* dy, const T* x, const T* w, const float* rstd, T* dx,
                        float* ws, T* dw, long rows, int D, hipStream_t stream);

template <typename T>
void launch_l2norm_fwd(const T* x, T* y, float* s, long rows, int D, float eps,
                       hipStream_t stream);
template <typename T>
void launch_l2norm_bwd(const T* dy, const T* y, const float* s, T* dx, long rows, int D,
                       float eps, hipStream_t stream);

// Launchers of the fused elementwise and row kernels (elementwise.hip):
// bias+GELU, LayerScale axpy, row gather / scatter, SwiGLU, RoPE.
//
// T is float or __hip_bfloat16 (instantiated for both); rows are contiguous
// and their width is a multiple of 8 where the binding says so. gamma, bias
// and scale of the ls_scatter_* launchers may be nullptr, as may scale of the
// row_* ones.
#pragma once

#include "common.h"

template <typename T>
void launch_bias_gelu_fwd(const T* x, const T* bias, T* y, long rows, int H,
                          hipStream_t stream);

// The *_bwd launchers below take `ws`, an fp32 workspace of COLRED_MAX_PARTIALS
// rows of D per parameter gradient, and write each gradient in T.
template <typename T>
void launch_bias_gelu_bwd(const T* dy, const T* x, const T* bias, T* dx, float* ws,
                          T* dbias, long rows, int H, hipStream_t stream);

template <typename T>
void launch_ls_axpy_fwd(const T* x, const T* res, const T* gamma, T* out, long rows,
                        int D, hipStream_t stream);
template <typename T>
void launch_ls_axpy_bwd(const T* dout, const T* res, const T* gamma, T* dres, float* ws,
                        T* dgamma, long rows, int D, hipStream_t stream);
template <typename T>
void launch_ls_axpy_bias_fwd(const T* x, const T* res, const T* gamma, const T* bias,
                             T* out, long rows, int D, hipStream_t stream);
template <typename T>
void launch_ls_axpy_bias_bwd(const T* dout, const T* res, const T* gamma, const T* bias,
                             T* dres, float* ws, T* dgamma, T* dbias, long rows, int D,
                             hipStream_t stream);

template <typename T>
void launch_ls_scatter_add(T* dst, const long* idx, const T* src, const T* gamma,
                           const T* bias, const float* scale, long M, int D,
                           hipStream_t stream);
template <typename T>
void launch_ls_scatter_bwd(const T* dy, const long* idx, const T* src, const T* gamma,
                           const T* bias, const float* scale, T* dres, float* ws, T* dgamma,
                           T* dbias, long M, int D, hipStream_t stream);

template <typename T>
void launch_row_gather(const T* src, const long* idx, T* out, long M, int D,
                       hipStream_t stream);
template <typename T>
void launch_row_scatter_add(T* dst, const long* idx, const T* src, const float* scale,
                            long M, int D, hipStream_t stream);
template <typename T>
void launch_row_gather_scaled(const T* src, const long* idx, const float* scale, T* out,
                              long M, int D, hipStream_t stream);

template <typename T>
void launch_swiglu_fwd(const T* x12, T* y, long rows, int H, hipStream_t stream);
template <typename T>
void launch_swiglu_bwd(const T* dy, const T* x12, T* dx12, long rows, int H,
                       hipStream_t stream);

// x [BH, N, hd]; sin_t / cos_t fp32 [P, hd] for the last P rows of each head.
template <typename T>
void launch_rope_fwd(const T* x, const float* sin_t, const float* cos_t, T* y, long BH,
                     int N, int P, int hd, hipStream_t stream);

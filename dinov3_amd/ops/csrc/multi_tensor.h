// Launchers of the multi-tensor update kernels (multi_tensor.hip).
//
// Every launcher takes the tables of a plan (ops/mt_plan.py), all in device
// memory: one pointer table of n_tensors addresses per tensor list, sizes
// [n_tensors] (elements), and the chunk tables chunk_tensor / chunk_offset
// [n_chunks], which cut tensor t into pieces of MT_CHUNK elements (the last
// one ragged). Per-tensor tables are [n_tensors].
#pragma once

#include "common.h"

#define MT_CHUNK 65536  // elements per chunk; equals CHUNK of ops/mt_plan.py

// t = m t + (1 - m) s in place, T float or __hip_bfloat16 on both sides.
template <typename T>
void launch_multi_tensor_ema(T* const* t_ptrs, const T* const* s_ptrs, const long* sizes,
                             const int* chunk_tensor, const long* chunk_offset,
                             int n_chunks, float m, hipStream_t stream);

// AdamW with decoupled weight decay over params p (T), grads g (GT) and fp32
// moments m, v; with has_master the update runs on the fp32 masters w and p is
// re-quantised from them (w is not read otherwise). Per tensor t:
// lr = (is_last[t] != 0 ? last_lr : lr) * lr_mult[t], wd = wd * wd_mult[t],
// grads are scaled by clip[sub_id[t]]. Instantiated for <T, GT> = <float,
// float>, <bf16, bf16>, <bf16, float>.
template <typename T, typename GT>
void launch_multi_tensor_adamw_planned(
    T* const* p, const GT* const* g, float* const* m, float* const* v, float* const* w,
    const long* sizes, const int* chunk_tensor, const long* chunk_offset, int n_chunks,
    const float* lr_mult, const float* wd_mult, const float* is_last, const int* sub_id,
    const float* clip, float lr, float last_lr, float wd, float beta1, float beta2,
    float eps, float bc1, float bc2, bool has_master, hipStream_t stream);

// out[sub_id[t]] += sum of g_t^2 (float atomics; out zeroed by the caller).
template <typename T>
void launch_multi_tensor_l2norm_planned(const T* const* g, const long* sizes,
                                        const int* chunk_tensor, const long* chunk_offset,
                                        int n_chunks, const int* sub_id, float* out,
                                        hipStream_t stream);

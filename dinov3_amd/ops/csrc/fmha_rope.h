// Memory-layout policies and launchers of the attention kernels (fmha_rope.hip).
//
// A policy names the kernels' tensor arguments (Qkv: inputs, DQkv: gradients)
// and, as a per-(b, h) view, turns (row n, which, column d) into an address.
// o / dO and the gradients follow the layout of their inputs; lse and D are
// [B, H, N] fp32 in both.
#pragma once

#include "common.h"

namespace fmha_rope {

// qkv [B, N, 3, H, hd] (the raw qkv GEMM output), o / dO token-major
// [B, N, H, hd], dq/dk/dv in ONE dqkv buffer shaped like qkv.
struct PackedLayout {
  struct Qkv { const __hip_bfloat16* qkv; };
  struct DQkv { __hip_bfloat16* dqkv; };
  // DINOV3_FMHA_DKV64=1 selects the 64-row dkv staging for this layout only
  static constexpr bool DKV64_OPTION = true;

  int b, h, H, N, HD;
  long qkv_off;       // (b, h) folded: (b*N*3*H + h)*hd
  long row_stride;    // 3*H*hd
  long which_stride;  // H*hd, also the o / dO row stride
  long o_off;         // (b*N*H + h)*hd

  DEV_INLINE PackedLayout(int b_, int h_, int H_, int N_, int HD_)
      : b(b_), h(h_), H(H_), N(N_), HD(HD_) {
    qkv_off = ((long)b * N * 3 * H + h) * HD;
    row_stride = (long)3 * H * HD;
    which_stride = (long)H * HD;
    o_off = ((long)b * N * H + h) * HD;
  }
  // element (n, which, d) of q (which 0), k (1) or v (2)
  DEV_INLINE const __hip_bfloat16* at(const Qkv& a, int n, int which, int d) const {
    return (a.qkv + qkv_off) + (long)n * row_stride + which * which_stride + d;
  }
  // row n of o or dO
  template <typename T> DEV_INLINE T* o_row(T* o, int n) const {
    return (o + o_off) + (long)n * which_stride;
  }
  // row n of dq / dk / dv
  DEV_INLINE __hip_bfloat16* grad_row(const DQkv& g, int which, int n) const {
    return g.dqkv + ((((long)b * N + n) * 3 + which) * H + h) * HD;
  }
};

// q, k, v, o, dO, dq, dk, dv each [B, H, N, hd] behind its own pointer.
struct PlainLayout {
  struct Qkv { const __hip_bfloat16 *q, *k, *v; };
  struct DQkv { __hip_bfloat16 *dq, *dk, *dv; };
  static constexpr bool DKV64_OPTION = false;

  long bh_off;  // (b*H + h)*N*hd
  int HD;

  DEV_INLINE PlainLayout(int b, int h, int H, int N, int HD_) : HD(HD_) {
    bh_off = ((long)b * H + h) * N * HD;
  }
  DEV_INLINE const __hip_bfloat16* at(const Qkv& a, int n, int which, int d) const {
    return o_row(which == 0 ? a.q : which == 1 ? a.k : a.v, n) + d;
  }
  template <typename T> DEV_INLINE T* o_row(T* o, int n) const {
    return (o + bh_off) + (long)n * HD;
  }
  DEV_INLINE __hip_bfloat16* grad_row(const DQkv& g, int which, int n) const {
    return o_row(which == 0 ? g.dq : which == 1 ? g.dk : g.dv, n);
  }
};

// sin_t / cos_t: fp32 [P, hd] rotate-half tables for the last P rows, or both
// nullptr for no RoPE. HD is 64 or 128. Instantiated for both layouts.
template <class L>
void launch_fwd(typename L::Qkv in, const float* sin_t, const float* cos_t,
                __hip_bfloat16* o, float* lse, int B, int H, int N, int P, int HD,
                float scale, hipStream_t stream);
template <class L>
void launch_bwd_pre(const __hip_bfloat16* dout, const __hip_bfloat16* o, float* D, int B,
                    int H, int N, int HD, hipStream_t stream);
template <class L>
void launch_bwd_dq(typename L::Qkv in, const __hip_bfloat16* dout, const float* sin_t,
                   const float* cos_t, const float* lse, const float* D,
                   typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                   hipStream_t stream);
template <class L>
void launch_bwd_dkv(typename L::Qkv in, const __hip_bfloat16* dout, const float* sin_t,
                    const float* cos_t, const float* lse, const float* D,
                    typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                    hipStream_t stream);

// Single-pass backward (pre + dq + dkv in one launch, D computed inside from
// dO and o) for the shapes fused_bwd_supported(N, HD) names; every other shape
// takes the three launches above. fused_bwd_enabled() is false while
// DINOV3_FMHA_FUSED_BWD=0 is set.
bool fused_bwd_supported(int N, int HD);
bool fused_bwd_enabled();
template <class L>
void launch_bwd_fused(typename L::Qkv in, const __hip_bfloat16* dout, const __hip_bfloat16* o,
                      const float* sin_t, const float* cos_t, const float* lse,
                      typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                      hipStream_t stream);

}  // namespace fmha_rope

void launch_probe_mfma(const __hip_bfloat16* A, const __hip_bfloat16* B, float* C,
                       hipStream_t stream);

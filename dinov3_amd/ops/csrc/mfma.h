// v_mfma_f32_32x32x16_bf16 fragment helpers shared by the MFMA kernels
// (fmha_rope.hip, knn_topk.hip, patch_embed.hip).
//
// Fragment layouts (verified on-device by probe_mfma_kernel in fmha_rope.hip):
//   A[i][k]: lane l holds A[i=l&31][k=(l>>5)*8 + idx], idx=0..7
//   B[k][j]: lane l holds B[k=(l>>5)*8 + idx][j=l&31]
//   C[r][c]: lane l reg r holds C[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31]
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

// row index of C reg r for this lane's half h
DEV_INLINE int c_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

DEV_INLINE bf16x8 load8(const __hip_bfloat16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

DEV_INLINE unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// exchange: lanes>=32 of a swap with lanes<32 of b
DEV_INLINE void permlane32_swap(unsigned& a, unsigned& b) {
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}

// Pack 8 fp32 accumulator regs (reg base..base+7 of a C-tile) into one MFMA
// bf16 operand fragment for the NEXT mfma whose k-dim runs over this tile's
// rows. After the swap, (r01, r23) holds k=(h*8)+0..7 for this lane.
DEV_INLINE bf16x8 pack_fragment(const float* s, int base) {
  unsigned r01 = cvt_pk_bf16(s[base + 0], s[base + 1]);
  unsigned r23 = cvt_pk_bf16(s[base + 2], s[base + 3]);
  unsigned r45 = cvt_pk_bf16(s[base + 4], s[base + 5]);
  unsigned r67 = cvt_pk_bf16(s[base + 6], s[base + 7]);
  permlane32_swap(r01, r45);
  permlane32_swap(r23, r67);
  union {
    unsigned u[4];
    bf16x8 v;
  } out;
  out.u[0] = r01;
  out.u[1] = r23;
  out.u[2] = r45;
  out.u[3] = r67;
  return out.v;
}

// Common helpers for the dinov3_amd CDNA4 (gfx950) kernels.
// Wave size is 64 on CDNA; block size is a multiple of 64 everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#define WAVE_SIZE 64
#define DEV_INLINE __device__ __forceinline__

// 16-byte vector of 8 bf16 values (guideline 13: always vectorize bf16 I/O).
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(4))) float float4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int uint4_t;

DEV_INLINE float bf16_to_f32(short u) {
  union { float f; unsigned int i; } v;
  v.i = ((unsigned int)(unsigned short)u) << 16;
  return v.f;
}

// Two fp32 -> one dword of two bf16 (lo in bits 0..15), round-to-nearest-even.
// The vector conversion selects gfx950's packed v_cvt_pk_bf16_f32: one
// instruction per pair instead of the bfe/add3/perm software rounding.
typedef __attribute__((ext_vector_type(2))) float float2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

DEV_INLINE unsigned int pack2_bf16(float lo, float hi) {
  const float2_t f = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(f, bf16x2_t));
}

DEV_INLINE short f32_to_bf16(float f) { return (short)(pack2_bf16(f, 0.0f) & 0xFFFFu); }

// ---- type traits: load/store element at fp32 compute precision ----
template <typename T> struct ScalarOps;

template <> struct ScalarOps<float> {
  DEV_INLINE static float load(const float* p) { return *p; }
  DEV_INLINE static void store(float* p, float v) { *p = v; }
};

template <> struct ScalarOps<__hip_bfloat16> {
  DEV_INLINE static float load(const __hip_bfloat16* p) {
    return bf16_to_f32(*reinterpret_cast<const short*>(p));
  }
  DEV_INLINE static void store(__hip_bfloat16* p, float v) {
    *reinterpret_cast<short*>(p) = f32_to_bf16(v);
  }
};

template <> struct ScalarOps<_Float16> {
  DEV_INLINE static float load(const _Float16* p) { return (float)(*p); }
  DEV_INLINE static void store(_Float16* p, float v) { *p = (_Float16)v; }
};

// ---- 8-element vectorized load/store (16B for bf16/fp16, 2x16B for f32) ----
template <typename T> struct Vec8 {
  DEV_INLINE static void load(T* dst, const T* src) {
    reinterpret_cast<float4_t*>(dst)[0] = reinterpret_cast<const float4_t*>(src)[0];
    reinterpret_cast<float4_t*>(dst)[1] = reinterpret_cast<const float4_t*>(src)[1];
  }
  DEV_INLINE static void store(T* dst, const T* src) {
    reinterpret_cast<float4_t*>(dst)[0] = reinterpret_cast<const float4_t*>(src)[0];
    reinterpret_cast<float4_t*>(dst)[1] = reinterpret_cast<const float4_t*>(src)[1];
  }
};

template <> struct Vec8<__hip_bfloat16> {
  DEV_INLINE static void load(__hip_bfloat16* dst, const __hip_bfloat16* src) {
    *reinterpret_cast<float4_t*>(dst) = *reinterpret_cast<const float4_t*>(src);
  }
  DEV_INLINE static void store(__hip_bfloat16* dst, const __hip_bfloat16* src) {
    *reinterpret_cast<float4_t*>(dst) = *reinterpret_cast<const float4_t*>(src);
  }
};

// ---- 8 fp32 values -> 8 elements of T at dst (16-byte aligned), one store ----
template <typename T> struct Pack8 {
  DEV_INLINE static void store(T* dst, const float* v) {
    T buf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ScalarOps<T>::store(buf + e, v[e]);
    Vec8<T>::store(dst, buf);
  }
};

template <> struct Pack8<__hip_bfloat16> {
  DEV_INLINE static void store(__hip_bfloat16* dst, const float* v) {
    uint4_t u;
    u.x = pack2_bf16(v[0], v[1]);
    u.y = pack2_bf16(v[2], v[3]);
    u.z = pack2_bf16(v[4], v[5]);
    u.w = pack2_bf16(v[6], v[7]);
    *reinterpret_cast<uint4_t*>(dst) = u;
  }
};

// ---- wave + block reductions ----
DEV_INLINE float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE_SIZE);
  return v;  // valid in lane 0 of the wave
}

DEV_INLINE float wave_reduce_max(float v) {
#pragma unroll
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, WAVE_SIZE));
  return v;
}

// Block-wide sum for blockDim.x <= 1024 (<=16 waves). `lds` needs >= 16 floats.
DEV_INLINE float block_reduce_sum(float v, float* lds) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  v = wave_reduce_sum(v);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  const int nw = (blockDim.x + WAVE_SIZE - 1) / WAVE_SIZE;
  v = (threadIdx.x < nw) ? lds[threadIdx.x] : 0.0f;
  if (wid == 0) v = wave_reduce_sum(v);
  if (threadIdx.x == 0) lds[0] = v;
  __syncthreads();
  return lds[0];
}

DEV_INLINE float block_reduce_max(float v, float* lds) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  v = wave_reduce_max(v);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  const int nw = (blockDim.x + WAVE_SIZE - 1) / WAVE_SIZE;
  v = (threadIdx.x < nw) ? lds[threadIdx.x] : -INFINITY;
  if (wid == 0) v = wave_reduce_max(v);
  if (threadIdx.x == 0) lds[0] = v;
  __syncthreads();
  return lds[0];
}

// ---- two-stage column reduction (dgamma / dbias of the backward kernels) ----
// Stage 1: every block of a backward kernel stores its partial column sums as
// row blockIdx.x of a [n_partials, D] fp32 workspace: plain contiguous vector
// stores, no zero fill, no atomics. Stage 2: colreduce_finalize_kernel sums
// the rows down each column in a fixed order and writes the gradient in the
// parameter dtype, up to two accumulators (dgamma and dbias) per launch.
// The result is bit-reproducible from run to run. No launcher uses more than
// COLRED_MAX_PARTIALS partial rows; the bindings size the workspace with it.
#define COLRED_MAX_PARTIALS 1024
#define COLRED_COLS 64    // columns per finalize block (256 B per wave load)
#define COLRED_SLICES 16  // row slices per finalize block, merged through LDS

// Grid of a row-strided walk over `groups` row groups: at most `cap` blocks,
// and every block runs the same number of iterations (no ragged last round).
static inline int even_row_grid(long groups, int cap) {
  if (groups <= cap) return groups > 0 ? (int)groups : 1;
  const long iters = (groups + cap - 1) / cap;
  return (int)((groups + iters - 1) / iters);
}

template <typename T>
__global__ __launch_bounds__(COLRED_COLS * COLRED_SLICES) void colreduce_finalize_kernel(
    const float* __restrict__ part0, T* __restrict__ out0,
    const float* __restrict__ part1, T* __restrict__ out1, int n_partials, int D) {
  __shared__ float acc[COLRED_SLICES][COLRED_COLS];
  const float* __restrict__ part = blockIdx.y == 0 ? part0 : part1;
  T* __restrict__ out = blockIdx.y == 0 ? out0 : out1;
  const int c = threadIdx.x & (COLRED_COLS - 1);
  const int s = threadIdx.x / COLRED_COLS;
  const int col = blockIdx.x * COLRED_COLS + c;
  float sum = 0.f;
  if (col < D) {
#pragma unroll 8
    for (int r = s; r < n_partials; r += COLRED_SLICES) sum += part[(long)r * D + col];
  }
  acc[s][c] = sum;
  __syncthreads();
  if (s == 0 && col < D) {
    float t = acc[0][c];
#pragma unroll
    for (int k = 1; k < COLRED_SLICES; ++k) t += acc[k][c];
    ScalarOps<T>::store(out + col, t);
  }
}

// out0 = colsum(part0) and, when part1 != nullptr, out1 = colsum(part1);
// partials are [n_partials, D] fp32.
template <typename T>
static inline void launch_colreduce_finalize(const float* part0, T* out0, const float* part1,
                                             T* out1, int n_partials, int D,
                                             hipStream_t stream) {
  if (part0 == nullptr) {
    part0 = part1;
    out0 = out1;
    part1 = nullptr;
  }
  if (part0 == nullptr) return;
  dim3 grid((D + COLRED_COLS - 1) / COLRED_COLS, part1 != nullptr ? 2 : 1);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(colreduce_finalize_kernel<T>), grid,
                     dim3(COLRED_COLS * COLRED_SLICES), 0, stream, part0, out0, part1, out1,
                     n_partials, D);
}

// ---- FP8 forward GEMM (fp8_gemm.hip) ----
// Tile geometry and shape preconditions, shared by the kernels, their
// launchers and the bindings' TORCH_CHECKs.
#define FP8_GEMM_BM 128       // output rows per block
#define FP8_GEMM_BN 128       // output columns per block
#define FP8_GEMM_BK 128       // e4m3 bytes of K per stage (one scaled MFMA deep)
#define FP8_GEMM_THREADS 256  // 4 waves, 2 (M) x 2 (N), 64x64 outputs each
#define FP8_GEMM_N_ALIGN 16   // N must be a multiple of one MFMA tile
#define FP8_QUANT_VEC 8       // bf16 elements per 16-byte quantiser load

// Operand formats; the values are the cbsz / blgp immediates of the scaled MFMA.
#define FP8_FMT_E4M3 0
#define FP8_FMT_E5M2 1

// ---- FP8 transposing column quantiser (fp8_gemm.hip) ----
#define FP8_COLS_THREADS 256
#define FP8_COLS_TC 64             // columns per block, both passes (8 threads x 8 columns)
#define FP8_COLS_TR 128            // rows per pass-2 tile = row padding unit = FP8_GEMM_BK
#define FP8_COLS_SLICES 32         // pass 1: row slices per block
#define FP8_COLS_MAX_PARTIALS 256  // pass 1: partial rows of the [partials, C] workspace

// ---- segmentation probe (seg_probe.hip) ----
#define SEG_MAX_CLASSES 255  // labels are uint8 and 255 marks an ignored pixel
#define SEG_MAX_CP 256       // padded class count: four classes per lane
#define SEG_MAX_SCALE 32     // label pixels per cell along an axis

#define HIP_CHECK_LAUNCH()                                                   \
  do {                                                                        \
    hipError_t e = hipGetLastError();                                         \
    if (e != hipSuccess) {                                                    \
      printf("HIP launch error: %s at %s:%d\n", hipGetErrorString(e),         \
             __FILE__, __LINE__);                                             \
    }                                                                         \
  } while (0)

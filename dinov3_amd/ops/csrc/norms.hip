// Row-wise normalization kernels: LayerNorm / RMSNorm / L2-norm, fwd + bwd.
// (SURVEY K2/K3 + the DINO-head bottleneck normalize of K15.)
//
// x is [rows, D] contiguous, bf16 or fp32 I/O, fp32 math. One 256-thread
// block per row (grid-stride over rows). V8=true takes the 8-wide vector
// path (16 B/lane bf16 loads — guideline 13); weight grads accumulate per
// fixed column slice inside a block and leave through the two-stage column
// reduction of common.h: one partial row per block, no atomics.

#include "norms.h"

#define NORM_BLOCK 256
// row-grid caps of the backward kernels (one workspace row per block)
#define LN_BWD_GRID 1024
static_assert(LN_BWD_GRID <= COLRED_MAX_PARTIALS, "workspace holds one row per block");

// block size matched to the row width so no lanes idle in the 8-wide loops
static inline int norm_block_for(int D) {
  if (D >= 2048) return 256;
  if (D >= 1024) return 128;
  return 64;
}

template <typename T, bool V8>
DEV_INLINE void row_load8(const T* p, int i, float* out) {
  if constexpr (V8) {
    T buf[8];
    Vec8<T>::load(buf, p + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = ScalarOps<T>::load(buf + e);
  } else {
    out[0] = ScalarOps<T>::load(p + i);
  }
}

template <typename T, bool V8>
DEV_INLINE void row_store8(T* p, int i, const float* in) {
  if constexpr (V8) {
    Pack8<T>::store(p + i, in);
  } else {
    ScalarOps<T>::store(p + i, in[0]);
  }
}

#define ROW_LOOP(i) \
  for (int i = threadIdx.x * EW; i < D; i += blockDim.x * EW)

// ------------------------------ LayerNorm ------------------------------

// GATHER: row r of the problem is x[idx[r]] (drop-path subset of the flat
// residual buffer); the second pass also writes the compact copy sub[r] that
// backward reads, so the gathered rows cross HBM once. Same block size, loops
// and reduction order as the plain kernel: y / mean / rstd are bit-equal to
// row_gather followed by layernorm_fwd.
template <typename T, bool V8, bool GATHER = false>
__global__ void layernorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ b,
    T* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    long rows, int D, float eps, const long* __restrict__ idx = nullptr,
    T* __restrict__ sub = nullptr) {
  static_assert(V8 || !GATHER, "the gathered forward is 8-wide only");
  constexpr int EW = V8 ? 8 : 1;
  __shared__ float red[16];
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + (GATHER ? idx[row] : row) * (long)D;
    T* yr = y + row * (long)D;
    float s = 0.f, s2 = 0.f;
    ROW_LOOP(i) {
      float v[EW];
      row_load8<T, V8>(xr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) {
        s += v[e];
        s2 += v[e] * v[e];
      }
    }
    s = block_reduce_sum(s, red);
    __syncthreads();
    s2 = block_reduce_sum(s2, red);
    float mean = s / D;
    float var = s2 / D - mean * mean;
    float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    if (threadIdx.x == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    ROW_LOOP(i) {
      float v[EW], wv[EW], bv[EW], o[EW];
      if constexpr (GATHER) {
        T raw[8];
        Vec8<T>::load(raw, xr + i);
        Vec8<T>::store(sub + row * (long)D + i, raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ScalarOps<T>::load(raw + e);
      } else {
        row_load8<T, V8>(xr, i, v);
      }
      row_load8<T, V8>(w, i, wv);
      row_load8<T, V8>(b, i, bv);
#pragma unroll
      for (int e = 0; e < EW; ++e) o[e] = (v[e] - mean) * rstd * wv[e] + bv[e];
      row_store8<T, V8>(yr, i, o);
    }
    __syncthreads();
  }
}

template <typename T, bool V8>
__global__ void layernorm_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    T* __restrict__ dx, float* __restrict__ dw_ws, float* __restrict__ db_ws,
    long rows, int D) {
  constexpr int EW = V8 ? 8 : 1;
  extern __shared__ float smem[];  // [16 red] + [D dw] + [D db]
  float* red = smem;
  float* dw_acc = smem + 16;
  float* db_acc = dw_acc + D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    dw_acc[i] = 0.f;
    db_acc[i] = 0.f;
  }
  __syncthreads();
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + row * (long)D;
    const T* xr = x + row * (long)D;
    T* dxr = dx + row * (long)D;
    const float m = mean[row], r = rstd[row];
    float sum_dyw = 0.f, sum_dyw_xhat = 0.f;
    ROW_LOOP(i) {
      float g[EW], v[EW], wv[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(xr, i, v);
      row_load8<T, V8>(w, i, wv);
#pragma unroll
      for (int e = 0; e < EW; ++e) {
        const float xhat = (v[e] - m) * r;
        const float gw = g[e] * wv[e];
        sum_dyw += gw;
        sum_dyw_xhat += gw * xhat;
        dw_acc[i + e] += g[e] * xhat;
        db_acc[i + e] += g[e];
      }
    }
    sum_dyw = block_reduce_sum(sum_dyw, red);
    __syncthreads();
    sum_dyw_xhat = block_reduce_sum(sum_dyw_xhat, red);
    const float inv_d = 1.0f / D;
    ROW_LOOP(i) {
      float g[EW], v[EW], wv[EW], o[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(xr, i, v);
      row_load8<T, V8>(w, i, wv);
#pragma unroll
      for (int e = 0; e < EW; ++e) {
        const float xhat = (v[e] - m) * r;
        o[e] = (g[e] * wv[e] - (sum_dyw + xhat * sum_dyw_xhat) * inv_d) * r;
      }
      row_store8<T, V8>(dxr, i, o);
    }
    __syncthreads();
  }
  // this block's partial row (the row loop ends on a barrier)
  float* dw_row = dw_ws + (long)blockIdx.x * D;
  float* db_row = db_ws + (long)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    dw_row[i] = dw_acc[i];
    db_row[i] = db_acc[i];
  }
}

// dx of one element of the wave-per-row backward,
//   (g * w - (sum_dyw + xhat * sum_dyw_xhat) / D) * rstd,
// with the fused multiply-adds spelled out: left to the compiler, the plain
// and the accumulating instantiation of one width contracted it differently
// and their dx differed in the last bit. This is the form the compiler chose
// for D = 1024 and 1536.
DEV_INLINE float ln_dx(float g, float w, float xhat, float sum_dyw, float sum_dyw_xhat,
                       float inv_d, float r) {
#pragma clang fp contract(off)
  const float s = __builtin_fmaf(sum_dyw_xhat, xhat, sum_dyw);
  return __builtin_fmaf(g, w, -(s * inv_d)) * r;
}

// Wave-per-row LayerNorm backward: each 64-lane wave owns a row, the row's
// dy/x values stay register-cached between the reduction and the dx pass
// (ONE read of dy and x instead of two), and the row loop has no block
// barriers — wave-level __shfl_xor reductions only. A lane owns the same
// columns for every row, so w is loaded once and dgamma/dbeta accumulate in
// registers across the row loop (2 x CHUNKS x 8 floats). LDS serves only the
// one cross-wave merge at block end, one accumulator at a time, after which
// the block stores its partial row. CHUNKS = ceil(D/512) (1: D<=512, 2: 1024,
// 3: 1536).
// SCATTER: `dx` is a gradient accumulator of the buffer the rows were
// gathered from; the last phase does dx[idx[row]] += dx_row (fp32 add, one
// rounding) instead of storing the row to its own buffer. idx rows are
// disjoint, so the read-modify-write needs no atomics. Row->wave assignment,
// grid and the dgamma/dbeta reduction do not depend on the flag.
// The accumulator loads cost registers; the SCATTER form is held to the plain
// kernel's occupancy at D = 1024 and 1536 (4 and 3 waves per SIMD) through
// the second launch bound, which is 1 (no constraint) for the plain kernel
// and for fp32 I/O, where holding it would spill.
template <typename T, int CHUNKS, bool SCATTER = false>
__global__ __launch_bounds__(256, SCATTER && sizeof(T) == 2
                                      ? (CHUNKS == 1 ? 5 : CHUNKS == 2 ? 4 : 3) : 1)
void layernorm_bwd_wave_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    T* __restrict__ dx, float* __restrict__ dw_ws, float* __restrict__ db_ws,
    long rows, int D, const long* __restrict__ idx = nullptr) {
  constexpr int NW = 4;  // waves per 256-thread block
  const int wid = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  extern __shared__ float smem[];  // [NW][D] merge buffer
  float wv[CHUNKS][8], dw_acc[CHUNKS][8], db_acc[CHUNKS][8];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = (c * 64 + lane) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wv[c][e] = 0.f;
      dw_acc[c][e] = 0.f;
      db_acc[c][e] = 0.f;
    }
    if (i < D) row_load8<T, true>(w, i, wv[c]);
  }
  const float inv_d = 1.0f / D;
  for (long row = (long)blockIdx.x * NW + wid; row < rows; row += (long)gridDim.x * NW) {
    const T* dyr = dy + row * (long)D;
    const T* xr = x + row * (long)D;
    const float m = mean[row], r = rstd[row];
    float g[CHUNKS][8], xhat[CHUNKS][8];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < D) {
        row_load8<T, true>(dyr, i, g[c]);
        row_load8<T, true>(xr, i, xhat[c]);
      }
    }
    float sum_dyw = 0.f, sum_dyw_xhat = 0.f;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < D) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xhat[c][e] = (xhat[c][e] - m) * r;
          const float gw = g[c][e] * wv[c][e];
          sum_dyw += gw;
          sum_dyw_xhat += gw * xhat[c][e];
          dw_acc[c][e] += g[c][e] * xhat[c][e];
          db_acc[c][e] += g[c][e];
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum_dyw += __shfl_xor(sum_dyw, off, 64);
      sum_dyw_xhat += __shfl_xor(sum_dyw_xhat, off, 64);
    }
    T* dxr = dx + (SCATTER ? idx[row] : row) * (long)D;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < D) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          o[e] = ln_dx(g[c][e], wv[c][e], xhat[c][e], sum_dyw, sum_dyw_xhat, inv_d, r);
        if constexpr (SCATTER) {
          float acc[8];
          row_load8<T, true>(dxr, i, acc);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += acc[e];
        }
        row_store8<T, true>(dxr, i, o);
      }
    }
  }
  // cross-wave merge in a fixed order, dgamma then dbeta through one buffer
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) __syncthreads();  // dgamma's merge has been read
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < D) {
        const float* a = pass == 0 ? dw_acc[c] : db_acc[c];
        float4_t* s4 = reinterpret_cast<float4_t*>(smem + (long)wid * D + i);
        s4[0] = float4_t{a[0], a[1], a[2], a[3]};
        s4[1] = float4_t{a[4], a[5], a[6], a[7]};
      }
    }
    __syncthreads();
    float* out_row = (pass == 0 ? dw_ws : db_ws) + (long)blockIdx.x * D;
    for (int i = threadIdx.x * 4; i < D; i += 256 * 4) {
      float4_t a = *reinterpret_cast<const float4_t*>(smem + i);
#pragma unroll
      for (int w2 = 1; w2 < NW; ++w2)
        a += *reinterpret_cast<const float4_t*>(smem + (long)w2 * D + i);
      *reinterpret_cast<float4_t*>(out_row + i) = a;
    }
  }
}

// ------------------------------ RMSNorm --------------------------------

template <typename T, bool V8>
__global__ void rmsnorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
    float* __restrict__ rstd_out, long rows, int D, float eps) {
  constexpr int EW = V8 ? 8 : 1;
  __shared__ float red[16];
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * (long)D;
    T* yr = y + row * (long)D;
    float s2 = 0.f;
    ROW_LOOP(i) {
      float v[EW];
      row_load8<T, V8>(xr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) s2 += v[e] * v[e];
    }
    s2 = block_reduce_sum(s2, red);
    float rstd = rsqrtf(s2 / D + eps);
    if (threadIdx.x == 0) rstd_out[row] = rstd;
    ROW_LOOP(i) {
      float v[EW], wv[EW], o[EW];
      row_load8<T, V8>(xr, i, v);
      row_load8<T, V8>(w, i, wv);
#pragma unroll
      for (int e = 0; e < EW; ++e) o[e] = v[e] * rstd * wv[e];
      row_store8<T, V8>(yr, i, o);
    }
    __syncthreads();
  }
}

template <typename T, bool V8>
__global__ void rmsnorm_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ rstd, T* __restrict__ dx, float* __restrict__ dw_ws,
    long rows, int D) {
  constexpr int EW = V8 ? 8 : 1;
  extern __shared__ float smem[];
  float* red = smem;
  float* dw_acc = smem + 16;
  for (int i = threadIdx.x; i < D; i += blockDim.x) dw_acc[i] = 0.f;
  __syncthreads();
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + row * (long)D;
    const T* xr = x + row * (long)D;
    T* dxr = dx + row * (long)D;
    const float r = rstd[row];
    float sum_gxw = 0.f;
    ROW_LOOP(i) {
      float g[EW], v[EW], wv[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(xr, i, v);
      row_load8<T, V8>(w, i, wv);
#pragma unroll
      for (int e = 0; e < EW; ++e) {
        sum_gxw += g[e] * wv[e] * v[e];
        dw_acc[i + e] += g[e] * v[e] * r;
      }
    }
    sum_gxw = block_reduce_sum(sum_gxw, red);
    const float c = sum_gxw * r * r * r / D;
    ROW_LOOP(i) {
      float g[EW], v[EW], wv[EW], o[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(xr, i, v);
      row_load8<T, V8>(w, i, wv);
#pragma unroll
      for (int e = 0; e < EW; ++e) o[e] = g[e] * wv[e] * r - v[e] * c;
      row_store8<T, V8>(dxr, i, o);
    }
    __syncthreads();
  }
  float* dw_row = dw_ws + (long)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) dw_row[i] = dw_acc[i];
}

// ------------------------------ L2 norm --------------------------------
// y = x / (||x|| + eps); saves s = 1/(||x|| + eps). ||x|| = 1/s - eps.

template <typename T, bool V8>
__global__ void l2norm_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, float* __restrict__ s_out,
    long rows, int D, float eps) {
  constexpr int EW = V8 ? 8 : 1;
  __shared__ float red[16];
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * (long)D;
    T* yr = y + row * (long)D;
    float s2 = 0.f;
    ROW_LOOP(i) {
      float v[EW];
      row_load8<T, V8>(xr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) s2 += v[e] * v[e];
    }
    s2 = block_reduce_sum(s2, red);
    float s = 1.0f / (sqrtf(s2) + eps);
    if (threadIdx.x == 0) s_out[row] = s;
    ROW_LOOP(i) {
      float v[EW], o[EW];
      row_load8<T, V8>(xr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) o[e] = v[e] * s;
      row_store8<T, V8>(yr, i, o);
    }
    __syncthreads();
  }
}

template <typename T, bool V8>
__global__ void l2norm_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ y, const float* __restrict__ s_in,
    T* __restrict__ dx, long rows, int D, float eps) {
  constexpr int EW = V8 ? 8 : 1;
  __shared__ float red[16];
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + row * (long)D;
    const T* yr = y + row * (long)D;
    T* dxr = dx + row * (long)D;
    const float s = s_in[row];
    const float n = 1.0f / s - eps;
    float dot = 0.f;
    ROW_LOOP(i) {
      float g[EW], v[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(yr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) dot += g[e] * v[e];
    }
    dot = block_reduce_sum(dot, red);
    // y = x * s, s = 1/(n+eps)  =>  dx = s*dy - (dot(dy,y)/n) * y
    const float c = dot / fmaxf(n, 1e-20f);
    ROW_LOOP(i) {
      float g[EW], v[EW], o[EW];
      row_load8<T, V8>(dyr, i, g);
      row_load8<T, V8>(yr, i, v);
#pragma unroll
      for (int e = 0; e < EW; ++e) o[e] = s * g[e] - c * v[e];
      row_store8<T, V8>(dxr, i, o);
    }
    __syncthreads();
  }
}

// ------------------------------ C wrappers -----------------------------

#define DISPATCH_V8(D, ...)            \
  if ((D) % 8 == 0) {                  \
    constexpr bool V8 = true;          \
    __VA_ARGS__;                       \
  } else {                             \
    constexpr bool V8 = false;         \
    __VA_ARGS__;                       \
  }

template <typename T>
void launch_layernorm_fwd(const T* x, const T* w, const T* b, T* y, float* mean,
                          float* rstd, long rows, int D, float eps, hipStream_t stream) {
  int grid = (int)min(rows, (long)8192);
  DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_fwd_kernel<T, V8>), dim3(grid),
                                     dim3(norm_block_for(D)), 0, stream, x, w, b, y, mean, rstd,
                                     rows, D, eps));
}

template <typename T>
void launch_gather_layernorm_fwd(const T* flat, const long* idx, const T* w, const T* b,
                                 T* y, T* sub, float* mean, float* rstd, long rows, int D,
                                 float eps, hipStream_t stream) {
  int grid = (int)min(rows, (long)8192);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_fwd_kernel<T, true, true>), dim3(grid),
                     dim3(norm_block_for(D)), 0, stream, flat, w, b, y, mean, rstd, rows, D,
                     eps, idx, sub);
}

// The wave-per-row backward. SCATTER = false stores dx[row]; SCATTER = true
// accumulates the row into dx[idx[row]]. Returns the grid (= partial rows).
template <typename T, bool SCATTER>
static int launch_layernorm_bwd_wave(const T* dy, const T* x, const T* w, const float* mean,
                                     const float* rstd, T* dx, const long* idx, float* dw_ws,
                                     float* db_ws, long rows, int D, hipStream_t stream) {
  // One read of dy/x, no block barriers in the row loop. Four blocks per CU
  // (four waves per SIMD at the 120 VGPRs of D = 1024; three at the 166
  // VGPRs of D = 1536), every block the same number of row rounds.
  const int grid =
      even_row_grid((rows + 3) / 4, D <= 1024 ? LN_BWD_GRID : LN_BWD_GRID * 3 / 4);
  const size_t shmem = 4 * (size_t)D * sizeof(float);
  if (D <= 512)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_bwd_wave_kernel<T, 1, SCATTER>), dim3(grid),
                       dim3(256), shmem, stream, dy, x, w, mean, rstd, dx, dw_ws, db_ws,
                       rows, D, idx);
  else if (D <= 1024)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_bwd_wave_kernel<T, 2, SCATTER>), dim3(grid),
                       dim3(256), shmem, stream, dy, x, w, mean, rstd, dx, dw_ws, db_ws,
                       rows, D, idx);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_bwd_wave_kernel<T, 3, SCATTER>), dim3(grid),
                       dim3(256), shmem, stream, dy, x, w, mean, rstd, dx, dw_ws, db_ws,
                       rows, D, idx);
  return grid;
}

template <typename T>
void launch_layernorm_bwd_scatter_acc(const T* dy, const T* x, const T* w, const float* mean,
                                      const float* rstd, T* dacc, const long* idx, float* ws,
                                      T* dw, T* db, long rows, int D, hipStream_t stream) {
  float* dw_ws = ws;
  float* db_ws = ws + (long)COLRED_MAX_PARTIALS * D;
  const int grid = launch_layernorm_bwd_wave<T, true>(dy, x, w, mean, rstd, dacc, idx, dw_ws,
                                                      db_ws, rows, D, stream);
  launch_colreduce_finalize<T>(dw_ws, dw, db_ws, db, grid, D, stream);
}

template <typename T>
void launch_layernorm_bwd(const T* dy, const T* x, const T* w, const float* mean,
                          const float* rstd, T* dx, float* ws, T* dw, T* db, long rows,
                          int D, hipStream_t stream) {
  float* dw_ws = ws;
  float* db_ws = ws + (long)COLRED_MAX_PARTIALS * D;
  int grid;
  if (D % 8 == 0 && D <= 1536) {
    grid = launch_layernorm_bwd_wave<T, false>(dy, x, w, mean, rstd, dx, nullptr, dw_ws,
                                               db_ws, rows, D, stream);
  } else {
    grid = even_row_grid(rows, LN_BWD_GRID);
    size_t shmem = (16 + 2 * (size_t)D) * sizeof(float);
    DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(layernorm_bwd_kernel<T, V8>), dim3(grid),
                                       dim3(norm_block_for(D)), shmem, stream, dy, x, w, mean,
                                       rstd, dx, dw_ws, db_ws, rows, D));
  }
  launch_colreduce_finalize<T>(dw_ws, dw, db_ws, db, grid, D, stream);
}

template <typename T>
void launch_rmsnorm_fwd(const T* x, const T* w, T* y, float* rstd, long rows, int D,
                        float eps, hipStream_t stream) {
  int grid = (int)min(rows, (long)8192);
  DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(rmsnorm_fwd_kernel<T, V8>), dim3(grid),
                                     dim3(norm_block_for(D)), 0, stream, x, w, y, rstd, rows, D,
                                     eps));
}

template <typename T>
void launch_rmsnorm_bwd(const T* dy, const T* x, const T* w, const float* rstd, T* dx,
                        float* ws, T* dw, long rows, int D, hipStream_t stream) {
  int grid = even_row_grid(rows, LN_BWD_GRID);
  size_t shmem = (16 + (size_t)D) * sizeof(float);
  DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(rmsnorm_bwd_kernel<T, V8>), dim3(grid),
                                     dim3(norm_block_for(D)), shmem, stream, dy, x, w, rstd, dx,
                                     ws, rows, D));
  launch_colreduce_finalize<T>(ws, dw, nullptr, nullptr, grid, D, stream);
}

template <typename T>
void launch_l2norm_fwd(const T* x, T* y, float* s, long rows, int D, float eps,
                       hipStream_t stream) {
  int grid = (int)min(rows, (long)8192);
  DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(l2norm_fwd_kernel<T, V8>), dim3(grid),
                                     dim3(norm_block_for(D)), 0, stream, x, y, s, rows, D, eps));
}

template <typename T>
void launch_l2norm_bwd(const T* dy, const T* y, const float* s, T* dx, long rows, int D,
                       float eps, hipStream_t stream) {
  int grid = (int)min(rows, (long)8192);
  DISPATCH_V8(D, hipLaunchKernelGGL(HIP_KERNEL_NAME(l2norm_bwd_kernel<T, V8>), dim3(grid),
                                     dim3(norm_block_for(D)), 0, stream, dy, y, s, dx, rows, D,
                                     eps));
}

// explicit instantiations of the launchers declared in norms.h
#define INSTANTIATE_NORMS(T)                                                              \
  template void launch_layernorm_fwd<T>(const T*, const T*, const T*, T*, float*, float*, \
                                        long, int, float, hipStream_t);                   \
  template void launch_layernorm_bwd<T>(const T*, const T*, const T*, const float*,       \
                                        const float*, T*, float*, T*, T*, long, int,      \
                                        hipStream_t);                                     \
  template void launch_gather_layernorm_fwd<T>(const T*, const long*, const T*, const T*, \
                                               T*, T*, float*, float*, long, int, float,  \
                                               hipStream_t);                              \
  template void launch_layernorm_bwd_scatter_acc<T>(const T*, const T*, const T*,         \
                                                    const float*, const float*, T*,       \
                                                    const long*, float*, T*, T*, long,    \
                                                    int, hipStream_t);                    \
  template void launch_rmsnorm_fwd<T>(const T*, const T*, T*, float*, long, int, float,   \
                                      hipStream_t);                                       \
  template void launch_rmsnorm_bwd<T>(const T*, const T*, const T*, const float*, T*,     \
                                      float*, T*, long, int, hipStream_t);                \
  template void launch_l2norm_fwd<T>(const T*, T*, float*, long, int, float, hipStream_t);\
  template void launch_l2norm_bwd<T>(const T*, const T*, const float*, T*, long, int,     \
                                     float, hipStream_t);

INSTANTIATE_NORMS(float)
INSTANTIATE_NORMS(__hip_bfloat16)

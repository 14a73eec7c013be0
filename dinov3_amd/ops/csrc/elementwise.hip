// Fused elementwise kernels: bias+GELU (K8 epilogue), SwiGLU gate (K9),
// RoPE rotate-half application (K5).

#include "elementwise.h"

#define EW_BLOCK 256
// The column-reduction backward kernels (bias_gelu_bwd, ls_*_bwd) run
// 512-thread blocks on a grid of at most EW_RED_GRID blocks: two blocks per
// CU, four waves per SIMD, all resident in a single round (their launch bounds
// hold them to the 128 VGPRs that takes). Each block leaves one row of
// partial column sums (common.h, two-stage column reduction).
#define EW_RED_BLOCK 512
#define EW_RED_GRID 512
// bias_gelu_fwd: 256-thread blocks, eight per CU (58 VGPRs in bf16: all resident)
#define EW_FWD_GRID 2048
static_assert(EW_RED_GRID <= COLRED_MAX_PARTIALS, "workspace holds one row per block");

// sigmoid through the hardware exp and reciprocal pipes (v_exp_f32 +
// v_rcp_f32): no IEEE division sequence. exp overflow gives rcp(inf) = 0.
DEV_INLINE float fast_sigmoid(float z) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-z));
}

// tanh-approximation GELU (matches torch F.gelu(approximate="tanh")) in its
// sigmoid form: 0.5*x*(1 + tanh(u)) = x * sigmoid(2u) with
// 2u = 2*sqrt(2/pi) * (x + 0.044715 x^3). Unlike 1 - 2/(1 + e^2u) this does
// not cancel for negative x.
DEV_INLINE float gelu_tanh(float x) {
  const float x2 = x * x;
  return x * fast_sigmoid(x * (1.5957691216f + 0.07135481627f * x2));
}

// d/dx [x * s(2u)] = s + x * s * (1 - s) * (2u)' = s * (1 + q * (1 - s)),
// q = x * (2u)' = x * (1.5957691216 + 3 * 0.07135481627 x^2)
DEV_INLINE float gelu_tanh_grad(float x) {
  const float x2 = x * x;
  const float s = fast_sigmoid(x * (1.5957691216f + 0.07135481627f * x2));
  const float q = x * (1.5957691216f + 0.21406444881f * x2);
  return s * (1.0f + q * (1.0f - s));
}

// 8 elements of T at p (16-byte aligned) as fp32
template <typename T>
DEV_INLINE void load8_f32(const T* p, float* out) {
  T buf[8];
  Vec8<T>::load(buf, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = ScalarOps<T>::load(buf + e);
}

// Thread layout of the fixed-column kernels: `tpr` threads span a tile of a
// row, 8 columns each (blockIdx.y tiles wider rows), and the block's other
// threads take further rows of the same columns ("row lanes"). A thread keeps
// its columns for the whole walk, so per-column sums stay in registers.
struct ColLane {
  int col8;     // first of this thread's 8 columns
  int c;        // column slot inside the tile
  int lr;       // this thread's row lane
  int rl;       // row lanes per block
  bool active;  // false: past the last row lane or the last column
};

DEV_INLINE ColLane col_lane(int tpr, int D) {
  ColLane t;
  t.rl = blockDim.x / tpr;
  t.lr = threadIdx.x / tpr;
  t.c = threadIdx.x - t.lr * tpr;
  t.col8 = (blockIdx.y * tpr + t.c) * 8;
  t.active = t.lr < t.rl && t.col8 < D;
  return t;
}

// Stage 1 of the column reduction: merge the row lanes' sums of 8 columns
// through LDS in a fixed order, then store the block's partial as two float4
// into workspace row blockIdx.x. `red` holds EW_RED_BLOCK * 8 floats. Every
// thread of the block must call this (it has barriers).
DEV_INLINE void colred_block_store(float* red, const float* acc, float* __restrict__ ws,
                                   int D, int tpr, const ColLane& t) {
  if (t.rl > 1) {
    __syncthreads();  // a previous accumulator's merge has been read
    if (t.active && t.lr > 0) {
      float4_t* r4 = reinterpret_cast<float4_t*>(red + threadIdx.x * 8);
      r4[0] = float4_t{acc[0], acc[1], acc[2], acc[3]};
      r4[1] = float4_t{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
  }
  if (t.active && t.lr == 0) {
    float4_t lo = {acc[0], acc[1], acc[2], acc[3]};
    float4_t hi = {acc[4], acc[5], acc[6], acc[7]};
    for (int k = 1; k < t.rl; ++k) {
      const float4_t* r4 = reinterpret_cast<const float4_t*>(red + (k * tpr + t.c) * 8);
      lo += r4[0];
      hi += r4[1];
    }
    float4_t* w4 = reinterpret_cast<float4_t*>(ws + (long)blockIdx.x * D + t.col8);
    w4[0] = lo;
    w4[1] = hi;
  }
}

// ---------------------------- bias + gelu ------------------------------
// Vectorized 8-wide (H % 8 == 0 — every FFN hidden dim). Forward and backward
// give each thread a FIXED 8-column slice (no per-element index arithmetic,
// bias stays in registers) and walk rows, RR rows in flight per iteration:
// all 16-byte loads of an iteration are issued before the first use. Backward
// accumulates dbias in registers and leaves it through the two-stage column
// reduction.

template <typename T, int RR = 4>
__global__ __launch_bounds__(EW_BLOCK) void bias_gelu_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ bias, T* __restrict__ y, long rows, int H,
    int tpr) {
  const ColLane t = col_lane(tpr, H);
  if (!t.active) return;
  float bb[8];
  load8_f32(bias + t.col8, bb);
  long row = ((long)blockIdx.x * t.rl + t.lr) * RR;
  const long rstep = (long)gridDim.x * t.rl * RR;
  for (; row + RR - 1 < rows; row += rstep) {
    T xb[RR][8];
#pragma unroll
    for (int rr = 0; rr < RR; ++rr) Vec8<T>::load(xb[rr], x + (row + rr) * (long)H + t.col8);
#pragma unroll
    for (int rr = 0; rr < RR; ++rr) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = gelu_tanh(ScalarOps<T>::load(xb[rr] + e) + bb[e]);
      Pack8<T>::store(y + (row + rr) * (long)H + t.col8, o);
    }
  }
  for (; row < rows; ++row) {
    const long off = row * (long)H + t.col8;
    float v[8], o[8];
    load8_f32(x + off, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = gelu_tanh(v[e] + bb[e]);
    Pack8<T>::store(y + off, o);
  }
}

template <typename T, int RR = 4>
__global__ __launch_bounds__(EW_RED_BLOCK, 4) void bias_gelu_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ bias,
    T* __restrict__ dx, float* __restrict__ dbias_ws, long rows, int H, int tpr) {
  __shared__ float red[EW_RED_BLOCK * 8];
  const ColLane t = col_lane(tpr, H);
  float db[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (t.active) {
    float bb[8];
    load8_f32(bias + t.col8, bb);
    long row = ((long)blockIdx.x * t.rl + t.lr) * RR;
    const long rstep = (long)gridDim.x * t.rl * RR;
    for (; row + RR - 1 < rows; row += rstep) {
      T xb[RR][8], gb[RR][8];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        const long off = (row + rr) * (long)H + t.col8;
        Vec8<T>::load(xb[rr], x + off);
        Vec8<T>::load(gb[rr], dy + off);
      }
      // keep the scheduler from sinking the loads to their uses (it does, to
      // save registers, and then waits for each in turn)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = ScalarOps<T>::load(xb[rr] + e) + bb[e];
          o[e] = ScalarOps<T>::load(gb[rr] + e) * gelu_tanh_grad(v);
          db[e] += o[e];
        }
        Pack8<T>::store(dx + (row + rr) * (long)H + t.col8, o);
      }
    }
    for (; row < rows; ++row) {
      const long off = row * (long)H + t.col8;
      float v[8], g[8], o[8];
      load8_f32(x + off, v);
      load8_f32(dy + off, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        o[e] = g[e] * gelu_tanh_grad(v[e] + bb[e]);
        db[e] += o[e];
      }
      Pack8<T>::store(dx + off, o);
    }
  }
  colred_block_store(red, db, dbias_ws, H, tpr, t);
}

// -------------------- LayerScale + residual add (K10) -------------------
// out = x + gamma * res ; bwd: dx = dout (aliased), dres = dout * gamma,
// dgamma = colsum(dout * res). 8-wide. The backward is ls_bwd_kernel below,
// shared with the bias-fused and scatter forms.

template <typename T>
__global__ void ls_axpy_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                   const T* __restrict__ gamma, T* __restrict__ out,
                                   long rows, int D) {
  const long total8 = rows * (long)(D / 8);
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total8;
       idx += (long)gridDim.x * blockDim.x) {
    const int col8 = (int)(idx % (D / 8)) * 8;
    T xb[8], rb[8], gb[8], ob[8];
    Vec8<T>::load(xb, x + idx * 8);
    Vec8<T>::load(rb, res + idx * 8);
    Vec8<T>::load(gb, gamma + col8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = ScalarOps<T>::load(xb + e) +
                ScalarOps<T>::load(gb + e) * ScalarOps<T>::load(rb + e);
      ScalarOps<T>::store(ob + e, v);
    }
    Vec8<T>::store(out + idx * 8, ob);
  }
}

// ---- bias-fused variant (DINOV3_FUSED_RESIDUAL): out = x + gamma*(res+bias).

template <typename T>
__global__ void ls_axpy_bias_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                        const T* __restrict__ gamma,
                                        const T* __restrict__ bias, T* __restrict__ out,
                                        long rows, int D) {
  const long total8 = rows * (long)(D / 8);
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total8;
       idx += (long)gridDim.x * blockDim.x) {
    const int col8 = (int)(idx % (D / 8)) * 8;
    T xb[8], rb[8], gb[8], bb[8], ob[8];
    Vec8<T>::load(xb, x + idx * 8);
    Vec8<T>::load(rb, res + idx * 8);
    Vec8<T>::load(gb, gamma + col8);
    Vec8<T>::load(bb, bias + col8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = ScalarOps<T>::load(xb + e) +
                ScalarOps<T>::load(gb + e) *
                    (ScalarOps<T>::load(rb + e) + ScalarOps<T>::load(bb + e));
      ScalarOps<T>::store(ob + e, v);
    }
    Vec8<T>::store(out + idx * 8, ob);
  }
}

// ---------------- fused LayerScale scatter-add (K10 + K11) ----------------
// Stochastic-depth residual with the LayerScale gamma and the producing
// GEMM's bias folded in (kills the standalone gamma multiply and the bias
// epilogue + bias-grad reduction of the proj/fc2 Linears):
//   dst[idx[r], c] += scale[r] * gamma[c] * (src[r, c] + bias[c])
// Rows are disjoint (drop-path subsets), so no atomics on dst.

template <typename T>
__global__ void ls_scatter_add_kernel(T* __restrict__ dst, const long* __restrict__ idx,
                                      const T* __restrict__ src,
                                      const T* __restrict__ gamma,
                                      const T* __restrict__ bias,
                                      const float* __restrict__ scale, long M, int D) {
  const int d8 = D / 8;
  long total = M * (long)d8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / d8;
    const int c8 = (int)(i % d8) * 8;
    const long drow = idx[r];
    const float s = scale != nullptr ? scale[r] : 1.0f;
    T sb[8], db[8], gb[8], bb[8];
    Vec8<T>::load(sb, src + r * (long)D + c8);
    Vec8<T>::load(db, dst + drow * (long)D + c8);
    if (gamma != nullptr) Vec8<T>::load(gb, gamma + c8);
    if (bias != nullptr) Vec8<T>::load(bb, bias + c8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float g = gamma != nullptr ? ScalarOps<T>::load(gb + e) : 1.0f;
      const float bv = bias != nullptr ? ScalarOps<T>::load(bb + e) : 0.0f;
      ScalarOps<T>::store(
          db + e, ScalarOps<T>::load(db + e) + s * g * (ScalarOps<T>::load(sb + e) + bv));
    }
    Vec8<T>::store(dst + drow * (long)D + c8, db);
  }
}

// Backward of all three LayerScale residual forms (ls_axpy, ls_axpy_bias,
// ls_scatter_add), one kernel:
//   dres[r,c] = dy[row(r),c] * gamma[c] * scale[r]
//   dgamma[c] = sum_r dy[row(r),c] * (src[r,c] + bias[c]) * scale[r]
//   dbias[c]  = sum_r dy[row(r),c] * gamma[c] * scale[r]
// row(r) = idx[r] for the scatter form (INDEXED) and r otherwise. Null gamma /
// bias / scale read as 1 / 0 / 1; a null workspace skips that sum. Same
// fixed-column walk and two-stage column reduction as bias_gelu_bwd.
template <typename T, bool INDEXED, int RR = 4>
__global__ __launch_bounds__(EW_RED_BLOCK, 4) void ls_bwd_kernel(
    const T* __restrict__ dy, const long* __restrict__ idx, const T* __restrict__ src,
    const T* __restrict__ gamma, const T* __restrict__ bias, const float* __restrict__ scale,
    T* __restrict__ dres, float* __restrict__ dgamma_ws, float* __restrict__ dbias_ws, long M,
    int D, int tpr) {
  __shared__ float red[EW_RED_BLOCK * 8];
  const ColLane t = col_lane(tpr, D);
  float dg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float db[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (t.active) {
    float gm[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gm[e] = 1.0f;
      bv[e] = 0.0f;
    }
    if (gamma != nullptr) load8_f32(gamma + t.col8, gm);
    if (bias != nullptr) load8_f32(bias + t.col8, bv);
    long r = ((long)blockIdx.x * t.rl + t.lr) * RR;
    const long rstep = (long)gridDim.x * t.rl * RR;
    for (; r + RR - 1 < M; r += rstep) {
      long srow[RR];
      float sc[RR];
      T dyb[RR][8], rb[RR][8];
      // all row indices first: a wait for idx[] between the 16-byte loads
      // would also wait for every load issued before it
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        srow[rr] = INDEXED ? idx[r + rr] : r + rr;
        sc[rr] = scale != nullptr ? scale[r + rr] : 1.0f;
      }
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        Vec8<T>::load(dyb[rr], dy + srow[rr] * (long)D + t.col8);
        Vec8<T>::load(rb[rr], src + (r + rr) * (long)D + t.col8);
      }
      // keep the scheduler from sinking the loads to their uses (it does, to
      // save registers, and then waits for each in turn)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float gv = ScalarOps<T>::load(dyb[rr] + e) * sc[rr];
          dg[e] += gv * (ScalarOps<T>::load(rb[rr] + e) + bv[e]);
          o[e] = gv * gm[e];
          db[e] += o[e];
        }
        Pack8<T>::store(dres + (r + rr) * (long)D + t.col8, o);
      }
    }
    for (; r < M; ++r) {
      const long srow = INDEXED ? idx[r] : r;
      const float s = scale != nullptr ? scale[r] : 1.0f;
      float g[8], v[8], o[8];
      load8_f32(dy + srow * (long)D + t.col8, g);
      load8_f32(src + r * (long)D + t.col8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gv = g[e] * s;
        dg[e] += gv * (v[e] + bv[e]);
        o[e] = gv * gm[e];
        db[e] += o[e];
      }
      Pack8<T>::store(dres + r * (long)D + t.col8, o);
    }
  }
  if (dgamma_ws != nullptr) colred_block_store(red, dg, dgamma_ws, D, tpr, t);
  if (dbias_ws != nullptr) colred_block_store(red, db, dbias_ws, D, tpr, t);
}

// ------------------------------ swiglu ---------------------------------
// x12 = [rows, 2H] as [x1 | x2]; y = silu(x1) * x2.

template <typename T>
__global__ void swiglu_fwd_kernel(const T* __restrict__ x12, T* __restrict__ y,
                                  long rows, int H) {
  long total = rows * (long)H;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    long row = idx / H;
    int col = (int)(idx % H);
    const T* xr = x12 + row * (long)(2 * H);
    float x1 = ScalarOps<T>::load(xr + col);
    float x2 = ScalarOps<T>::load(xr + H + col);
    float sig = __builtin_amdgcn_rcpf(1.0f + expf(-x1));
    ScalarOps<T>::store(y + idx, x1 * sig * x2);
  }
}

template <typename T>
__global__ void swiglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x12,
                                  T* __restrict__ dx12, long rows, int H) {
  long total = rows * (long)H;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    long row = idx / H;
    int col = (int)(idx % H);
    const T* xr = x12 + row * (long)(2 * H);
    T* dxr = dx12 + row * (long)(2 * H);
    float x1 = ScalarOps<T>::load(xr + col);
    float x2 = ScalarOps<T>::load(xr + H + col);
    float g = ScalarOps<T>::load(dy + idx);
    float sig = __builtin_amdgcn_rcpf(1.0f + expf(-x1));
    float silu = x1 * sig;
    float dsilu = sig * (1.0f + x1 * (1.0f - sig));
    ScalarOps<T>::store(dxr + col, g * x2 * dsilu);
    ScalarOps<T>::store(dxr + H + col, g * silu);
  }
}

// -------------------- row gather / scatter-add (K11) --------------------
// Stochastic-depth subset compute: gather kept samples' token rows, compute,
// scatter-add the scaled residual back. Rows are disjoint (no atomics).

template <typename T>
__global__ void row_gather_kernel(const T* __restrict__ src, const long* __restrict__ idx,
                                  T* __restrict__ out, long M, int D) {
  const int d8 = D / 8;
  long total = M * (long)d8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / d8;
    const int c8 = (int)(i % d8) * 8;
    const long srow = idx[r];
    T buf[8];
    Vec8<T>::load(buf, src + srow * (long)D + c8);
    Vec8<T>::store(out + r * (long)D + c8, buf);
  }
}

template <typename T>
__global__ void row_scatter_add_kernel(T* __restrict__ dst, const long* __restrict__ idx,
                                       const T* __restrict__ src,
                                       const float* __restrict__ scale, long M, int D) {
  const int d8 = D / 8;
  long total = M * (long)d8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / d8;
    const int c8 = (int)(i % d8) * 8;
    const long drow = idx[r];
    const float s = scale != nullptr ? scale[r] : 1.0f;
    T sb[8], db[8];
    Vec8<T>::load(sb, src + r * (long)D + c8);
    Vec8<T>::load(db, dst + drow * (long)D + c8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ScalarOps<T>::store(db + e,
                          ScalarOps<T>::load(db + e) + s * ScalarOps<T>::load(sb + e));
    }
    Vec8<T>::store(dst + drow * (long)D + c8, db);
  }
}

// gather with per-row scale (backward of scatter-add)
template <typename T>
__global__ void row_gather_scaled_kernel(const T* __restrict__ src,
                                         const long* __restrict__ idx,
                                         const float* __restrict__ scale,
                                         T* __restrict__ out, long M, int D) {
  const int d8 = D / 8;
  long total = M * (long)d8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / d8;
    const int c8 = (int)(i % d8) * 8;
    const long srow = idx[r];
    const float s = scale != nullptr ? scale[r] : 1.0f;
    T buf[8];
    Vec8<T>::load(buf, src + srow * (long)D + c8);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      ScalarOps<T>::store(buf + e, s * ScalarOps<T>::load(buf + e));
    Vec8<T>::store(out + r * (long)D + c8, buf);
  }
}

// ------------------------------- RoPE ----------------------------------
// x: [B, Hh, N, hd] contiguous; sin/cos: [P, hd] fp32 with P = N - prefix.
// rotate-half: out[j] = x[j]*cos[j] - x[j+hd/2]*sin[j]          (j < hd/2)
//              out[j] = x[j]*cos[j] + x[j-hd/2]*sin[j]          (j >= hd/2)
// Tokens [0, prefix) pass through unchanged (cls + storage tokens).
// One thread per pair (j < hd/2) handles both halves: 2 loads, 2 stores.

template <typename T>
__global__ void rope_fwd_kernel(const T* __restrict__ x, const float* __restrict__ sin_t,
                                const float* __restrict__ cos_t, T* __restrict__ y,
                                long BH, int N, int P, int hd) {
  const int half = hd / 2;
  long total = BH * (long)N * half;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    int j = (int)(idx % half);
    long t = idx / half;          // BH*N token index
    int n = (int)(t % N);
    long base = t * (long)hd;
    int p = n - (N - P);          // patch index (negative for prefix tokens)
    float lo = ScalarOps<T>::load(x + base + j);
    float hi = ScalarOps<T>::load(x + base + half + j);
    if (p < 0) {
      ScalarOps<T>::store(y + base + j, lo);
      ScalarOps<T>::store(y + base + half + j, hi);
    } else {
      const float* srow = sin_t + (long)p * hd;
      const float* crow = cos_t + (long)p * hd;
      float s_lo = srow[j], c_lo = crow[j];
      float s_hi = srow[half + j], c_hi = crow[half + j];
      ScalarOps<T>::store(y + base + j, lo * c_lo - hi * s_lo);
      ScalarOps<T>::store(y + base + half + j, hi * c_hi + lo * s_hi);
    }
  }
}

// ---------------------------- C wrappers -------------------------------

// Launch geometry of the fixed-column kernels (ColLane): threads per row
// tile, column tiles (grid.y) and an even row grid (grid.x) of at most
// max_blocks blocks in all, `rr` rows in flight per row lane.
struct ColGrid {
  int tpr, col_tiles, row_grid;
};

static ColGrid col_grid(long rows, int D, int block, int max_blocks, int rr) {
  ColGrid g;
  const int d8 = D / 8;
  g.tpr = d8 < block ? d8 : block;
  g.col_tiles = (d8 + g.tpr - 1) / g.tpr;
  const long rows_per_iter = (long)(block / g.tpr) * rr;
  const int cap = max_blocks / g.col_tiles > 0 ? max_blocks / g.col_tiles : 1;
  g.row_grid = even_row_grid((rows + rows_per_iter - 1) / rows_per_iter, cap);
  return g;
}

template <typename T>
void launch_bias_gelu_fwd(const T* x, const T* bias, T* y, long rows, int H,
                          hipStream_t stream) {
  const ColGrid g = col_grid(rows, H, EW_BLOCK, EW_FWD_GRID, 4);
  hipLaunchKernelGGL((bias_gelu_fwd_kernel<T, 4>), dim3(g.row_grid, g.col_tiles),
                     dim3(EW_BLOCK), 0, stream, x, bias, y, rows, H, g.tpr);
}

template <typename T>
void launch_bias_gelu_bwd(const T* dy, const T* x, const T* bias, T* dx, float* ws,
                          T* dbias, long rows, int H, hipStream_t stream) {
  const ColGrid g = col_grid(rows, H, EW_RED_BLOCK, EW_RED_GRID, 4);
  hipLaunchKernelGGL((bias_gelu_bwd_kernel<T, 4>), dim3(g.row_grid, g.col_tiles),
                     dim3(EW_RED_BLOCK), 0, stream, dy, x, bias, dx, ws, rows, H, g.tpr);
  launch_colreduce_finalize<T>(ws, dbias, nullptr, nullptr, g.row_grid, H, stream);
}

// all three LayerScale backward forms; a null dgamma / dbias is not computed
template <typename T>
static void launch_ls_bwd(const T* dy, const long* idx, const T* src, const T* gamma,
                          const T* bias, const float* scale, T* dres, float* ws, T* dgamma,
                          T* dbias, long M, int D, hipStream_t stream) {
  const ColGrid g = col_grid(M, D, EW_RED_BLOCK, EW_RED_GRID, 4);
  float* ws_g = dgamma != nullptr ? ws : nullptr;
  float* ws_b = dbias != nullptr ? ws + (long)COLRED_MAX_PARTIALS * D : nullptr;
  if (idx != nullptr)
    hipLaunchKernelGGL((ls_bwd_kernel<T, true, 4>), dim3(g.row_grid, g.col_tiles),
                       dim3(EW_RED_BLOCK), 0, stream, dy, idx, src, gamma, bias, scale, dres,
                       ws_g, ws_b, M, D, g.tpr);
  else
    hipLaunchKernelGGL((ls_bwd_kernel<T, false, 4>), dim3(g.row_grid, g.col_tiles),
                       dim3(EW_RED_BLOCK), 0, stream, dy, idx, src, gamma, bias, scale, dres,
                       ws_g, ws_b, M, D, g.tpr);
  launch_colreduce_finalize<T>(ws_g, dgamma, ws_b, dbias, g.row_grid, D, stream);
}

template <typename T>
void launch_ls_axpy_fwd(const T* x, const T* res, const T* gamma, T* out, long rows,
                        int D, hipStream_t stream) {
  long total8 = rows * (long)(D / 8);
  int grid = (int)min((total8 + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  hipLaunchKernelGGL((ls_axpy_fwd_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream, x,
                     res, gamma, out, rows, D);
}

template <typename T>
void launch_ls_axpy_bwd(const T* dout, const T* res, const T* gamma, T* dres, float* ws,
                        T* dgamma, long rows, int D, hipStream_t stream) {
  launch_ls_bwd<T>(dout, nullptr, res, gamma, nullptr, nullptr, dres, ws, dgamma, nullptr,
                   rows, D, stream);
}

template <typename T>
void launch_ls_axpy_bias_fwd(const T* x, const T* res, const T* gamma, const T* bias,
                             T* out, long rows, int D, hipStream_t stream) {
  long total8 = rows * (long)(D / 8);
  int grid = (int)min((total8 + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  hipLaunchKernelGGL((ls_axpy_bias_fwd_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     x, res, gamma, bias, out, rows, D);
}

template <typename T>
void launch_ls_axpy_bias_bwd(const T* dout, const T* res, const T* gamma, const T* bias,
                             T* dres, float* ws, T* dgamma, T* dbias, long rows, int D,
                             hipStream_t stream) {
  launch_ls_bwd<T>(dout, nullptr, res, gamma, bias, nullptr, dres, ws, dgamma, dbias, rows,
                   D, stream);
}

template <typename T>
void launch_ls_scatter_add(T* dst, const long* idx, const T* src, const T* gamma,
                           const T* bias, const float* scale, long M, int D,
                           hipStream_t stream) {
  long total = M * (long)(D / 8);
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  if (grid == 0) return;
  hipLaunchKernelGGL((ls_scatter_add_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     dst, idx, src, gamma, bias, scale, M, D);
}

template <typename T>
void launch_ls_scatter_bwd(const T* dy, const long* idx, const T* src, const T* gamma,
                           const T* bias, const float* scale, T* dres, float* ws, T* dgamma,
                           T* dbias, long M, int D, hipStream_t stream) {
  launch_ls_bwd<T>(dy, idx, src, gamma, bias, scale, dres, ws, dgamma, dbias, M, D, stream);
}

template <typename T>
void launch_row_gather(const T* src, const long* idx, T* out, long M, int D,
                       hipStream_t stream) {
  long total = M * (long)(D / 8);
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  if (grid == 0) return;
  hipLaunchKernelGGL((row_gather_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream, src,
                     idx, out, M, D);
}

template <typename T>
void launch_row_scatter_add(T* dst, const long* idx, const T* src, const float* scale,
                            long M, int D, hipStream_t stream) {
  long total = M * (long)(D / 8);
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  if (grid == 0) return;
  hipLaunchKernelGGL((row_scatter_add_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     dst, idx, src, scale, M, D);
}

template <typename T>
void launch_row_gather_scaled(const T* src, const long* idx, const float* scale, T* out,
                              long M, int D, hipStream_t stream) {
  long total = M * (long)(D / 8);
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  if (grid == 0) return;
  hipLaunchKernelGGL((row_gather_scaled_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     src, idx, scale, out, M, D);
}

template <typename T>
void launch_swiglu_fwd(const T* x12, T* y, long rows, int H, hipStream_t stream) {
  long total = rows * (long)H;
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  hipLaunchKernelGGL((swiglu_fwd_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     x12, y, rows, H);
}

template <typename T>
void launch_swiglu_bwd(const T* dy, const T* x12, T* dx12, long rows, int H,
                       hipStream_t stream) {
  long total = rows * (long)H;
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)2048);
  hipLaunchKernelGGL((swiglu_bwd_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     dy, x12, dx12, rows, H);
}

template <typename T>
void launch_rope_fwd(const T* x, const float* sin_t, const float* cos_t, T* y, long BH,
                     int N, int P, int hd, hipStream_t stream) {
  long total = BH * (long)N * (hd / 2);
  int grid = (int)min((total + EW_BLOCK - 1) / EW_BLOCK, (long)4096);
  hipLaunchKernelGGL((rope_fwd_kernel<T>), dim3(grid), dim3(EW_BLOCK), 0, stream,
                     x, sin_t, cos_t, y, BH, N, P, hd);
}

#define INSTANTIATE_EW(T)                                                            \
  template void launch_bias_gelu_fwd<T>(const T*, const T*, T*, long, int,           \
                                        hipStream_t);                                \
  template void launch_ls_axpy_fwd<T>(const T*, const T*, const T*, T*, long, int,   \
                                      hipStream_t);                                  \
  template void launch_ls_axpy_bwd<T>(const T*, const T*, const T*, T*, float*, T*,  \
                                      long, int, hipStream_t);                       \
  template void launch_ls_axpy_bias_fwd<T>(const T*, const T*, const T*, const T*,   \
                                           T*, long, int, hipStream_t);              \
  template void launch_ls_axpy_bias_bwd<T>(const T*, const T*, const T*, const T*,   \
                                           T*, float*, T*, T*, long, int,            \
                                           hipStream_t);                             \
  template void launch_ls_scatter_add<T>(T*, const long*, const T*, const T*,        \
                                         const T*, const float*, long, int,          \
                                         hipStream_t);                               \
  template void launch_ls_scatter_bwd<T>(const T*, const long*, const T*, const T*,  \
                                         const T*, const float*, T*, float*, T*, T*, \
                                         long, int, hipStream_t);                    \
  template void launch_row_gather<T>(const T*, const long*, T*, long, int,           \
                                     hipStream_t);                                   \
  template void launch_row_scatter_add<T>(T*, const long*, const T*, const float*,   \
                                          long, int, hipStream_t);                   \
  template void launch_row_gather_scaled<T>(const T*, const long*, const float*, T*, \
                                            long, int, hipStream_t);                 \
  template void launch_bias_gelu_bwd<T>(const T*, const T*, const T*, T*, float*,    \
                                        T*, long, int, hipStream_t);                 \
  template void launch_swiglu_fwd<T>(const T*, T*, long, int, hipStream_t);          \
  template void launch_swiglu_bwd<T>(const T*, const T*, T*, long, int, hipStream_t);\
  template void launch_rope_fwd<T>(const T*, const float*, const float*, T*, long,   \
                                   int, int, int, hipStream_t);

INSTANTIATE_EW(float)
INSTANTIATE_EW(__hip_bfloat16)

// Linear-probe training step, the two non-GEMM parts (docs/KERNELS.md "Linear
// probe"): softmax cross-entropy over a grid of heads with the gradient written
// in place, and the SGD-momentum update with the fused bf16 copy of the weights.
#include "linear_probe.h"

#include <climits>

#define PROBE_CE_WAVES 4          // waves (= rows in flight) per 256-thread block
#define PROBE_CE_MAX_BLOCKS 1024  // blocks of one launch, all heads together
#define PROBE_SGD_TILE 512        // 8-element vectors per block and loop round

static_assert(PROBE_CE_MAX_BLOCKS <= COLRED_MAX_PARTIALS, "workspace holds one row per block");

template <typename T> struct Load8;

template <> struct Load8<float> {
  DEV_INLINE static void load(const float* p, float* o) {
    const float4_t a = reinterpret_cast<const float4_t*>(p)[0];
    const float4_t b = reinterpret_cast<const float4_t*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
};

template <> struct Load8<__hip_bfloat16> {
  DEV_INLINE static void load(const __hip_bfloat16* p, float* o) {
    const short8_t v = *reinterpret_cast<const short8_t*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bf16_to_f32(v[e]);
  }
};

// ------------------------------ probe_ce --------------------------------
// logits [B, G, Cp], grid (row blocks, G). One wave per row; lane `l` owns the
// columns 512 c + 8 l .. + 7 of every row it visits, c < CHUNKS = ceil(Cp/512).
// The row is read once with 16-byte loads and lives in registers as fp32; the
// bias is re-read per row (an L2 hit) instead of held, which keeps Cp = 1024 at
// four waves per SIMD. Max/argmax, the exp sum and z[label] go through wave
// shuffles; the xor butterfly leaves every lane with the same bits, so the
// per-wave loss and count need no broadcast. Columns C..Cp-1 enter as -inf and
// leave as 0. The lowest index among equal maxima wins: lanes scan their
// columns in ascending order with a strict compare, the butterfly prefers the
// lower index on equal values.
// A block's partial sums (dbias when WRITE_GRAD, then loss and count, one
// float each per head) go to row blockIdx.x of the [gridDim.x, ws_cols]
// workspace: columns g Cp .. for dbias, then `tail` + g for the loss and
// `tail` + G + g for the count. colreduce_finalize_kernel sums the rows.
template <typename T, int CHUNKS, bool WRITE_GRAD>
__global__ __launch_bounds__(PROBE_CE_WAVES * 64, CHUNKS == 2 ? 4 : 1)
void probe_ce_kernel(T* __restrict__ logits, const float* __restrict__ bias,
                     const long* __restrict__ labels, float* __restrict__ ws, long B, int G,
                     int Cp, int C, float grad_scale, int ws_cols, int tail) {
  const int wid = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.y;
  // all LDS is dynamic, so that its base stays 16-byte aligned: loss and count
  // per wave, then the [PROBE_CE_WAVES][Cp] dbias merge buffer (WRITE_GRAD only)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float (*red)[PROBE_CE_WAVES] = reinterpret_cast<float (*)[PROBE_CE_WAVES]>(lds);
  float* smem = lds + 2 * PROBE_CE_WAVES;
  const float* __restrict__ bg = bias != nullptr ? bias + (long)g * Cp : nullptr;
  float db[CHUNKS][8];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) db[c][e] = 0.f;
  float loss_acc = 0.f;
  int hit_acc = 0;

  for (long b = (long)blockIdx.x * PROBE_CE_WAVES + wid; b < B;
       b += (long)gridDim.x * PROBE_CE_WAVES) {
    T* row = logits + (b * G + g) * (long)Cp;
    const long lab = labels[b];
    float v[CHUNKS][8];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < Cp) Load8<T>::load(row + i, v[c]);
    }
    float m = -INFINITY, zl = 0.f;
    int am = INT_MAX;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < Cp) {
        if (bg != nullptr) {
          float bv[8];
          Load8<float>::load(bg + i, bv);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[c][e] += bv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (i + e >= C) v[c][e] = -INFINITY;
          if (v[c][e] > m) {
            m = v[c][e];
            am = i + e;
          }
          zl += (long)(i + e) == lab ? v[c][e] : 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[c][e] = -INFINITY;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_xor(m, off, 64);
      const int oa = __shfl_xor(am, off, 64);
      if (om > m || (om == m && oa < am)) {
        m = om;
        am = oa;
      }
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[c][e] = __expf(v[c][e] - m);  // -inf -> 0
        s += v[c][e];
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      zl += __shfl_xor(zl, off, 64);  // one lane holds z[label], the others 0
    }
    const bool counted = lab >= 0;  // -1: the row is ignored
    if (counted) {
      loss_acc += __logf(s) + m - zl;
      hit_acc += (long)am == lab ? 1 : 0;
    }
    if constexpr (WRITE_GRAD) {
      const float r = 1.0f / s;
#pragma unroll
      for (int c = 0; c < CHUNKS; ++c) {
        const int i = (c * 64 + lane) * 8;
        if (i < Cp) {
          float d[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float onehot = (long)(i + e) == lab ? 1.f : 0.f;
            d[e] = counted && i + e < C ? (v[c][e] * r - onehot) * grad_scale : 0.f;
            db[c][e] += d[e];
          }
          Pack8<T>::store(row + i, d);
        }
      }
    }
  }

  // cross-wave merge in a fixed order, then the block's partial row
  float* out_row = ws + (long)blockIdx.x * ws_cols;
  if constexpr (WRITE_GRAD) {
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = (c * 64 + lane) * 8;
      if (i < Cp) {
        float4_t* s4 = reinterpret_cast<float4_t*>(smem + (long)wid * Cp + i);
        s4[0] = float4_t{db[c][0], db[c][1], db[c][2], db[c][3]};
        s4[1] = float4_t{db[c][4], db[c][5], db[c][6], db[c][7]};
      }
    }
  }
  if (lane == 0) {
    red[0][wid] = loss_acc;
    red[1][wid] = (float)hit_acc;
  }
  __syncthreads();
  if constexpr (WRITE_GRAD) {
    for (int i = threadIdx.x * 4; i < Cp; i += PROBE_CE_WAVES * 64 * 4) {
      float4_t a = *reinterpret_cast<const float4_t*>(smem + i);
#pragma unroll
      for (int w2 = 1; w2 < PROBE_CE_WAVES; ++w2)
        a += *reinterpret_cast<const float4_t*>(smem + (long)w2 * Cp + i);
      *reinterpret_cast<float4_t*>(out_row + (long)g * Cp + i) = a;
    }
  }
  if (threadIdx.x < 2) {
    float t = red[threadIdx.x][0];
#pragma unroll
    for (int w2 = 1; w2 < PROBE_CE_WAVES; ++w2) t += red[threadIdx.x][w2];
    out_row[tail + threadIdx.x * G + g] = t;
  }
}

int probe_ce_row_blocks(long B, int G, int row_blocks) {
  const long groups = (B + PROBE_CE_WAVES - 1) / PROBE_CE_WAVES;
  int cap = PROBE_CE_MAX_BLOCKS / G;
  if (cap < 1) cap = 1;
  if (row_blocks > 0) cap = row_blocks < PROBE_CE_MAX_BLOCKS ? row_blocks : PROBE_CE_MAX_BLOCKS;
  return even_row_grid(groups, cap);
}

void probe_ce_layout(int G, int Cp, bool write_grad, int* ws_cols, int* tail) {
  *tail = write_grad ? G * Cp : 0;
  *ws_cols = *tail + (2 * G + 3) / 4 * 4;
}

template <typename T>
void launch_probe_ce(T* logits, const float* bias, const long* labels, float* ws, float* out,
                     long B, int G, int Cp, int C, float grad_scale, bool write_grad, int nblk,
                     hipStream_t stream) {
  int ws_cols, tail;
  probe_ce_layout(G, Cp, write_grad, &ws_cols, &tail);
  const dim3 grid(nblk, G), block(PROBE_CE_WAVES * 64);
  const size_t shmem =
      (2 * PROBE_CE_WAVES + (write_grad ? PROBE_CE_WAVES * (size_t)Cp : 0)) * sizeof(float);
#define PROBE_CE_LAUNCH(CHUNKS, WG)                                                           \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_ce_kernel<T, CHUNKS, WG>), grid, block, shmem,     \
                     stream, logits, bias, labels, ws, B, G, Cp, C, grad_scale, ws_cols, tail)
#define PROBE_CE_CHUNKS(WG)             \
  do {                                  \
    if (Cp <= 512) {                    \
      PROBE_CE_LAUNCH(1, WG);           \
    } else if (Cp <= 1024) {            \
      PROBE_CE_LAUNCH(2, WG);           \
    } else {                            \
      PROBE_CE_LAUNCH(4, WG);           \
    }                                   \
  } while (0)
  if (write_grad)
    PROBE_CE_CHUNKS(true);
  else
    PROBE_CE_CHUNKS(false);
#undef PROBE_CE_CHUNKS
#undef PROBE_CE_LAUNCH
  launch_colreduce_finalize<float>(ws, out, nullptr, nullptr, nblk, ws_cols, stream);
}

template void launch_probe_ce<float>(float*, const float*, const long*, float*, float*, long,
                                     int, int, int, float, bool, int, hipStream_t);
template void launch_probe_ce<__hip_bfloat16>(__hip_bfloat16*, const float*, const long*, float*,
                                              float*, long, int, int, int, float, bool, int,
                                              hipStream_t);

// ------------------------------ probe_sgd_ -------------------------------
// w, mom [G, R] fp32, grad [G, R]; grid (tiles, G), head g reads lr[g], wd[g]:
//   g' = grad + wd w;  mom = momentum mom + g';  w = w - lr lr_scale mom
// and, with w_lp, w_lp = bf16(w). A thread moves two 8-element vectors per
// round, all of their loads issued before the first use; offsets are 64-bit.
template <typename GT>
__global__ __launch_bounds__(256)
void probe_sgd_kernel(float* __restrict__ w, float* __restrict__ mom,
                      const GT* __restrict__ grad, const float* __restrict__ lr,
                      const float* __restrict__ wd, __hip_bfloat16* __restrict__ w_lp, long R,
                      float lr_scale, float momentum) {
  const int g = blockIdx.y;
  const float step = lr[g] * lr_scale;
  const float decay = wd != nullptr ? wd[g] : 0.f;
  const long base = (long)g * R;
  const long nvec = R / 8;
  for (long t = (long)blockIdx.x * PROBE_SGD_TILE + threadIdx.x; t < nvec;
       t += (long)gridDim.x * PROBE_SGD_TILE) {
    float wv[2][8], mv[2][8], gv[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long vec = t + u * (PROBE_SGD_TILE / 2);
      if (vec < nvec) {
        const long off = base + vec * 8;
        Load8<float>::load(w + off, wv[u]);
        Load8<float>::load(mom + off, mv[u]);
        Load8<GT>::load(grad + off, gv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long vec = t + u * (PROBE_SGD_TILE / 2);
      if (vec < nvec) {
        const long off = base + vec * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          mv[u][e] = momentum * mv[u][e] + (gv[u][e] + decay * wv[u][e]);
          wv[u][e] -= step * mv[u][e];
        }
        Pack8<float>::store(mom + off, mv[u]);
        Pack8<float>::store(w + off, wv[u]);
        if (w_lp != nullptr) Pack8<__hip_bfloat16>::store(w_lp + off, wv[u]);
      }
    }
  }
}

template <typename GT>
void launch_probe_sgd(float* w, float* mom, const GT* grad, const float* lr, const float* wd,
                      __hip_bfloat16* w_lp, int G, long R, float lr_scale, float momentum,
                      hipStream_t stream) {
  const long tiles = (R / 8 + PROBE_SGD_TILE - 1) / PROBE_SGD_TILE;
  long cap = 4096 / G;
  if (cap < 1) cap = 1;
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap), G);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_sgd_kernel<GT>), grid, dim3(256), 0, stream, w, mom,
                     grad, lr, wd, w_lp, R, lr_scale, momentum);
}

template void launch_probe_sgd<float>(float*, float*, const float*, const float*, const float*,
                                      __hip_bfloat16*, int, long, float, float, hipStream_t);
template void launch_probe_sgd<__hip_bfloat16>(float*, float*, const __hip_bfloat16*,
                                               const float*, const float*, __hip_bfloat16*, int,
                                               long, float, float, hipStream_t);

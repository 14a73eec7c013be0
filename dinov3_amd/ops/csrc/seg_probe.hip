// Linear segmentation probe, the non-GEMM part of a training step
// (docs/KERNELS.md "Segmentation probe"): bilinear upsampling of patch-resolution
// logits to the label resolution, per-pixel softmax cross-entropy, the IoU
// counts, and the gradient folded back to patch resolution, without ever
// holding the upsampled logits in memory.
#include "seg_probe.h"

#include <climits>

// Grid and LDS sizes of the three kernels, shared by kernels and launchers.
struct SegCeTraits {
  static constexpr int kWaves = 4;  // quads in flight per block
  static constexpr int kThreads = kWaves * 64;
  static constexpr int kMaxBlocks = 1024;  // blocks of one launch, all heads together
  // finalize: a block is kFinVecs 8-column vectors wide and kFinCells cells deep
  static constexpr int kFinVecs = 32;
  static constexpr int kFinCells = 8;
  static constexpr int kFinMaxRows = 128;  // grid.y: kFinCells partial dbias rows each

  // blocks that share a head's quads; every block runs the same number of rounds
  static int quad_blocks(long quads, int G) {
    int cap = kMaxBlocks / G;
    if (cap < 1) cap = 1;
    return even_row_grid((quads + kWaves - 1) / kWaves, cap);
  }
  // per wave: the loss (padded to 16 bytes for all waves together), then [3, Cp] counts
  static size_t lds_bytes(int Cp) { return (kWaves + (size_t)kWaves * 3 * Cp) * sizeof(float); }
  static int fin_rows(long cells) {
    const long r = (cells + kFinCells - 1) / kFinCells;
    return (int)(r < kFinMaxRows ? r : kFinMaxRows);
  }
  static int fin_col_blocks(long NC) { return (int)((NC / 8 + kFinVecs - 1) / kFinVecs); }
};

template <typename T> struct Load8;  // linear_probe.hip

template <> struct Load8<float> {
  DEV_INLINE static void load(const float* p, float* o) {
    const float4_t a = reinterpret_cast<const float4_t*>(p)[0];
    const float4_t b = reinterpret_cast<const float4_t*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
};

DEV_INLINE float readlane_f32(float v, int lane) {
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ------------------------------ seg_ce ----------------------------------
// logits [M, h, w, G, Cp], labels [M, H, W] uint8 with H = s h, W = s w; grid
// (quad blocks, G). Along an axis the pixels with the tap pair (q, min(q+1, h-1))
// are the rows [a(q), b(q)), a(0) = 0, a(q) = q s + s/2, b(q) = (q+1) s + s/2,
// b(h-1) = H; an image is h x w such quads, and every pixel of a quad reads the
// same four cells. One wave walks a quad for one head with lane = class: lane l
// owns the classes l + 64 k, k < CPL, and keeps their four corner logits, their
// four per-tap gradient sums and their three counts in registers. Per pixel:
// four FMAs per class for z, the max/argmax and the exp sum through xor
// butterflies (the lowest index wins among equal maxima: a lane scans its
// classes in ascending order with a strict compare, the butterfly prefers the
// lower index), then g[tap][c] += w_tap (p_c - onehot), which needs no
// cross-lane step. Label, weights and the loop bounds are wave-uniform: a row of
// labels is read by the lanes (one byte each, the next row in flight) and handed
// out with v_readlane, so is the x weight; no address depends on a label.
// A quad's four gradient vectors go to ws [M, h, w, 4, G, Cp] fp32, tap
// 2 dy + dx; a block's loss and counts go to row blockIdx.x of part_loss
// [blocks, G] and part_area [blocks, G, 3, Cp].
template <typename T, int CPL, bool WRITE_GRAD>
__global__ __launch_bounds__(SegCeTraits::kThreads)
void seg_ce_kernel(const T* __restrict__ logits, const float* __restrict__ bias,
                   const unsigned char* __restrict__ labels, float* __restrict__ ws,
                   float* __restrict__ part_loss, int* __restrict__ part_area,
                   const float* __restrict__ scale_ptr, long quads, int h, int w, int s, int G,
                   int Cp, int C, float grad_scale) {
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red = lds;
  int* merge = reinterpret_cast<int*>(lds + SegCeTraits::kWaves);
  const int H = h * s, W = w * s;
  const float two_s = (float)(2 * s);

  float bv[CPL];
  int a_int[CPL], a_pred[CPL], a_lab[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = lane + 64 * k;
    bv[k] = bias != nullptr && c < C ? bias[(long)g * Cp + c] : 0.f;
    a_int[k] = a_pred[k] = a_lab[k] = 0;
  }
  float loss_acc = 0.f;
  float gs = grad_scale;
  if constexpr (WRITE_GRAD) {
    if (scale_ptr != nullptr) gs *= scale_ptr[0];
  }

  for (long q = (long)blockIdx.x * SegCeTraits::kWaves + wid; q < quads;
       q += (long)gridDim.x * SegCeTraits::kWaves) {
    const int qj = (int)(q % w);
    const long qr = q / w;
    const int qi = (int)(qr % h);
    const long m = qr / h;
    const int i1 = qi + 1 < h ? qi + 1 : h - 1;
    const int j1 = qj + 1 < w ? qj + 1 : w - 1;
    const long cell[4] = {(m * h + qi) * w + qj, (m * h + qi) * w + j1, (m * h + i1) * w + qj,
                          (m * h + i1) * w + j1};
    float L[4][CPL], acc[4][CPL];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = lane + 64 * k;
        L[t][k] = c < C ? ScalarOps<T>::load(logits + (cell[t] * G + g) * (long)Cp + c) : 0.f;
        acc[t][k] = 0.f;
      }

    const int ya = qi == 0 ? 0 : qi * s + s / 2;
    const int yb = qi == h - 1 ? H : (qi + 1) * s + s / 2;
    const int xa = qj == 0 ? 0 : qj * s + s / 2;
    const int xb = qj == w - 1 ? W : (qj + 1) * s + s / 2;
    const int nw = xb - xa;  // <= 3 s / 2 <= 48: one lane per pixel of a row
    // wx of the lane's pixel: sx - x0 = (2 x + 1 - s - 2 s qj) / (2 s), 0 left of the first centre
    const int nx = 2 * (xa + lane) + 1 - s - 2 * s * qj;
    const float wx_lane = nx > 0 ? (float)nx / two_s : 0.f;
    const unsigned char* lrow = labels + (m * H + ya) * (long)W + xa;
    int cur = lane < nw ? (int)lrow[lane] : 255;

    for (int y = ya; y < yb; ++y) {
      int nxt = 255;
      if (y + 1 < yb && lane < nw) nxt = (int)lrow[(long)(y + 1 - ya) * W + lane];
      const int ny = 2 * y + 1 - s - 2 * s * qi;
      const float wy = ny > 0 ? (float)ny / two_s : 0.f;
      for (int px = 0; px < nw; ++px) {
        const int lab = __builtin_amdgcn_readlane(cur, px);
        if (lab == 255) continue;
        const float wx = readlane_f32(wx_lane, px);
        const float w00 = (1.f - wy) * (1.f - wx), w01 = (1.f - wy) * wx;
        const float w10 = wy * (1.f - wx), w11 = wy * wx;
        float z[CPL];
        float mx = -INFINITY;
        int am = INT_MAX;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = lane + 64 * k;
          const float v =
              fmaf(w11, L[3][k], fmaf(w10, L[2][k], fmaf(w01, L[1][k], w00 * L[0][k]))) + bv[k];
          z[k] = c < C ? v : -INFINITY;
          if (z[k] > mx) {
            mx = z[k];
            am = c;
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const float om = __shfl_xor(mx, off, 64);
          const int oa = __shfl_xor(am, off, 64);
          if (om > mx || (om == mx && oa < am)) {
            mx = om;
            am = oa;
          }
        }
        float e[CPL];
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          e[k] = __expf(z[k] - mx);  // -inf -> 0
          sum += e[k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        // z[label]: the owner's register, picked by k and read from its lane
        float zsel = z[0];
#pragma unroll
        for (int k = 1; k < CPL; ++k) zsel = (lab >> 6) == k ? z[k] : zsel;
        const float zl = readlane_f32(zsel, lab & 63);
        loss_acc += __logf(sum) + mx - zl;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = lane + 64 * k;
          const int is_pred = am == c ? 1 : 0, is_lab = lab == c ? 1 : 0;
          a_pred[k] += is_pred;
          a_lab[k] += is_lab;
          a_int[k] += is_pred & is_lab;
        }
        if constexpr (WRITE_GRAD) {
          const float r = 1.0f / sum;
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            const int c = lane + 64 * k;
            const float d = e[k] * r - (lab == c ? 1.f : 0.f);  // 0 in the columns >= C
            acc[0][k] = fmaf(w00, d, acc[0][k]);
            acc[1][k] = fmaf(w01, d, acc[1][k]);
            acc[2][k] = fmaf(w10, d, acc[2][k]);
            acc[3][k] = fmaf(w11, d, acc[3][k]);
          }
        }
      }
      cur = nxt;
    }
    if constexpr (WRITE_GRAD) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = lane + 64 * k;
          if (c < Cp) ws[((q * 4 + t) * G + g) * (long)Cp + c] = acc[t][k] * gs;
        }
    }
  }

  // cross-wave merge in a fixed order, then the block's partial rows
  int* mine = merge + (long)wid * 3 * Cp;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < Cp) {
      mine[c] = a_int[k];
      mine[Cp + c] = a_pred[k];
      mine[2 * Cp + c] = a_lab[k];
    }
  }
  if (lane == 0) red[wid] = loss_acc;  // the butterflies left every lane the same sum
  __syncthreads();
  int* out_area = part_area + ((long)blockIdx.x * G + g) * 3 * Cp;
  for (int i = threadIdx.x; i < 3 * Cp; i += SegCeTraits::kThreads) {
    int t = merge[i];
#pragma unroll
    for (int w2 = 1; w2 < SegCeTraits::kWaves; ++w2) t += merge[(long)w2 * 3 * Cp + i];
    out_area[i] = t;
  }
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int w2 = 1; w2 < SegCeTraits::kWaves; ++w2) t += red[w2];
    part_loss[(long)blockIdx.x * G + g] = t;
  }
}

// ------------------------- gradient finalize ----------------------------
// A later launch, so every read of the logits has finished. Cell (i, j) of
// image m sums what the quads around it stored for it, in a fixed order: quads
// (qi, qj) in lexicographic order, taps 0..3 inside a quad, tap 2 dy + dx
// reaching cell (min(qi + dy, h-1), min(qj + dx, w-1)); at most nine terms, at
// the image's last corner. The sum replaces the cell's logits in their dtype,
// and, unrounded, feeds the dbias partial row of this (blockIdx.y, threadIdx.y).
// Block (kFinVecs, kFinCells): x walks NC = G Cp columns eight at a time.
template <typename T>
__global__ __launch_bounds__(SegCeTraits::kFinVecs * SegCeTraits::kFinCells)
void seg_grad_finalize_kernel(const float* __restrict__ ws, T* __restrict__ logits,
                              float* __restrict__ part_db, long cells, int h, int w, long NC) {
  const long vec = (long)blockIdx.x * SegCeTraits::kFinVecs + threadIdx.x;
  if (vec >= NC / 8) return;
  const long col = vec * 8;
  float db[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) db[e] = 0.f;
  for (long cell = (long)blockIdx.y * SegCeTraits::kFinCells + threadIdx.y; cell < cells;
       cell += (long)gridDim.y * SegCeTraits::kFinCells) {
    const int j = (int)(cell % w);
    const long cr = cell / w;
    const int i = (int)(cr % h);
    const long m = cr / h;
    float sum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = 0.f;
    for (int qi = i > 0 ? i - 1 : 0; qi <= i; ++qi)
      for (int qj = j > 0 ? j - 1 : 0; qj <= j; ++qj) {
        const long quad = (m * h + qi) * w + qj;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int ti = qi + (t >> 1) < h ? qi + (t >> 1) : h - 1;
          const int tj = qj + (t & 1) < w ? qj + (t & 1) : w - 1;
          if (ti == i && tj == j) {
            float v[8];
            Load8<float>::load(ws + (quad * 4 + t) * NC + col, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum[e] += v[e];
          }
        }
      }
#pragma unroll
    for (int e = 0; e < 8; ++e) db[e] += sum[e];
    Pack8<T>::store(logits + cell * NC + col, sum);
  }
  Pack8<float>::store(
      part_db + ((long)blockIdx.y * SegCeTraits::kFinCells + threadIdx.y) * NC + col, db);
}

// loss [G] and areas [G, 3, Cp] from the blocks' partial rows, one thread per
// column, rows in ascending order. The counts are summed as integers: a float
// sum, as colreduce_finalize_kernel would form it, is exact only below 2^24
// pixels.
__global__ __launch_bounds__(256)
void seg_sums_finalize_kernel(const float* __restrict__ part_loss,
                              const int* __restrict__ part_area, float* __restrict__ loss,
                              long* __restrict__ areas, int nblk, int G, long acols) {
  const long col = (long)blockIdx.x * 256 + threadIdx.x;
  if (col < acols) {
    long t = 0;
    for (int b = 0; b < nblk; ++b) t += part_area[(long)b * acols + col];
    areas[col] = t;
  } else if (col < acols + G) {
    const int g = (int)(col - acols);
    float t = 0.f;
    for (int b = 0; b < nblk; ++b) t += part_loss[(long)b * G + g];
    loss[g] = t;
  }
}

int seg_ce_quad_blocks(long quads, int G) { return SegCeTraits::quad_blocks(quads, G); }
int seg_ce_fin_rows(long cells) { return SegCeTraits::fin_rows(cells) * SegCeTraits::kFinCells; }

template <typename T>
void launch_seg_ce(T* logits, const float* bias, const unsigned char* labels, float* ws,
                   float* part_loss, int* part_area, float* part_db, float* loss, long* areas,
                   float* dbias, const float* scale, long M, int h, int w, int s, int G, int Cp,
                   int C, float grad_scale, bool write_grad, int nblk, hipStream_t stream) {
  const long quads = M * h * w;
  const dim3 grid(nblk, G), block(SegCeTraits::kThreads);
  const size_t shmem = SegCeTraits::lds_bytes(Cp);
#define SEG_CE_LAUNCH(CPL, WG)                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_ce_kernel<T, CPL, WG>), grid, block, shmem, stream,    \
                     logits, bias, labels, ws, part_loss, part_area, scale, quads, h, w, s, G,  \
                     Cp, C, grad_scale)
#define SEG_CE_CPL(WG)           \
  do {                           \
    if (Cp <= 64) {              \
      SEG_CE_LAUNCH(1, WG);      \
    } else if (Cp <= 128) {      \
      SEG_CE_LAUNCH(2, WG);      \
    } else if (Cp <= 192) {      \
      SEG_CE_LAUNCH(3, WG);      \
    } else {                     \
      SEG_CE_LAUNCH(4, WG);      \
    }                            \
  } while (0)
  if (write_grad)
    SEG_CE_CPL(true);
  else
    SEG_CE_CPL(false);
#undef SEG_CE_CPL
#undef SEG_CE_LAUNCH
  const long acols = (long)G * 3 * Cp;
  hipLaunchKernelGGL(seg_sums_finalize_kernel, dim3((unsigned)((acols + G + 255) / 256)),
                     dim3(256), 0, stream, part_loss, part_area, loss, areas, nblk, G, acols);
  if (write_grad) {
    const long NC = (long)G * Cp;
    const int rows = SegCeTraits::fin_rows(quads);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_grad_finalize_kernel<T>),
                       dim3(SegCeTraits::fin_col_blocks(NC), rows),
                       dim3(SegCeTraits::kFinVecs, SegCeTraits::kFinCells), 0, stream, ws, logits,
                       part_db, quads, h, w, NC);
    launch_colreduce_finalize<float>(part_db, dbias, nullptr, nullptr,
                                     rows * SegCeTraits::kFinCells, (int)NC, stream);
  }
}

template void launch_seg_ce<float>(float*, const float*, const unsigned char*, float*, float*,
                                   int*, float*, float*, long*, float*, const float*, long, int,
                                   int, int, int, int, int, float, bool, int, hipStream_t);
template void launch_seg_ce<__hip_bfloat16>(__hip_bfloat16*, const float*, const unsigned char*,
                                            float*, float*, int*, float*, float*, long*, float*,
                                            const float*, long, int, int, int, int, int, int,
                                            float, bool, int, hipStream_t);

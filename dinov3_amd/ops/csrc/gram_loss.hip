// Gram-anchoring loss and its student gradient without fp32 M x M matrices
// (docs/KERNELS.md "Gram loss").
//
//   loss = 1 / (G M^2) * sum_{g,i,j} (a_ij - b_ij)^2
//   A = s^ s^T, B = t^ t^T per matrix g, s^_i = r_i S_i with r_i = rsqrt(|S_i|^2)
//   (r_i = 1 without apply_norm), a and b the clamped A and B:
//     mode 0: a = A, b = B                                    mask = 1
//     mode 1: a = max(A, 0), b = max(B, 0)   (remove_neg)     mask = A >= 0
//     mode 2: a = A unless A < 0 and B < 0, then 0;           mask = not both < 0
//             b = max(B, 0)   (remove_only_teacher_neg)
//   mask is the derivative of a with respect to A.
//
// Gradient. With e = a - b and E = e * mask (symmetric, because A and B are),
//   dL/dA_ij = 2 / (G M^2) * E_ij,
// and A_ij = s^_i . s^_j holds s^_i twice (as row of (i, j) and as column of
// (j, i)), so
//   dL/ds^_i = 2 * 2 / (G M^2) * sum_j E_ij s^_j = c * Draw_i,
//   c = 4 / (G M^2),  Draw = P @ S,  P_ij = E_ij r_j     (P in bf16).
// The normalisation s^_i = r_i S_i has the Jacobian r_i (I - s^_i s^_i^T):
//   dS_i = c r_i (Draw_i - s^_i (s^_i . Draw_i)),  dS_i = c Draw_i without it.
// P @ S is a plain bf16 GEMM and is left to the library; P exists one row panel
// at a time (the host loop is in ops/gram_loss.py).
//
// Kernels.
//   rnorm_kernel      r for the rows of S and T, one wave per row.
//   tile_kernel       the hot path. A block of 4 waves owns one 128 x 128 tile
//                     of one matrix. The four operand panels S_i, S_j, T_i, T_j
//                     stream through LDS in chunks of GRAM_BK = 64 columns,
//                     double buffered: the global loads of chunk k + 1 are in
//                     flight in registers while chunk k is multiplied (issue
//                     early, write late, one barrier per chunk). Wave w owns
//                     the 64 x 64 quadrant (w >> 1, w & 1) of the tile as 2 x 2
//                     MFMA tiles for each of the two products: 128 accumulator
//                     registers. The operands are the raw bf16 inputs: products
//                     are exact, nothing is rounded before the fp32 epilogue.
//                     The product is taken swapped (C = S_j . S_i^T), so that a
//                     lane holds 16 columns j of ONE row i = lane & 31 and
//                     pack_fragment turns them into 16-byte row-major stores.
//   finish_kernel     sum of the tile partials in a fixed order, over G M^2.
//   norm_bwd_kernel   dS from Draw, one wave per row.
//
// LDS: 2 buffers x 4 panels x 128 rows x (64 + 8) bf16 = 144 KiB, plus 1 KiB
// of r_j. Rows of 144 bytes and ds_read_b128 fragments: the bank argument of
// knn_topk.hip applies unchanged.
//
// Rows and columns past M and columns past D come from clamped addresses and
// are replaced by zeros on the way to LDS (no branch around a load); r_j is 0
// past M. Such entries have A = B = 0, add 0 to the loss and write P = 0, so
// the P panel is written in whole tiles and padded to a multiple of 128
// columns. No float atomics: loss and gradient are bit-identical from run to
// run and for every panel height.

#include "gram_loss.h"
#include "mfma.h"

#define GRAM_TILE 128     // rows and columns of an output tile
#define GRAM_BK 64        // feature columns per staged chunk
#define GRAM_THREADS 256  // 4 waves, 2 x 2 quadrants of 64 x 64
#define GRAM_STRIDE (GRAM_BK + 8)  // bf16 elements per LDS row
#define GRAM_ROW_THREADS 256       // row kernels: one wave per row, 4 rows per block
#define GRAM_FIN_THREADS 256

namespace gram {

// r[0, row] for S and r[1, row] for T; rows = G M.
__global__ __launch_bounds__(GRAM_ROW_THREADS) void rnorm_kernel(
    const __hip_bfloat16* __restrict__ s, const __hip_bfloat16* __restrict__ t,
    float* __restrict__ r, long rows, int D, int apply_norm) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const long row = (long)blockIdx.x * (GRAM_ROW_THREADS / WAVE_SIZE) + threadIdx.x / WAVE_SIZE;
  if (row >= rows) return;  // wave-uniform
  const __hip_bfloat16* __restrict__ x = (blockIdx.y == 0 ? s : t) + row * (long)D;
  float sum = 0.f;
  for (int c = lane * 8; c < D; c += WAVE_SIZE * 8) {
    const short8_t v = *reinterpret_cast<const short8_t*>(x + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = bf16_to_f32(v[e]);
      sum += f * f;
    }
  }
  sum = wave_reduce_sum(sum);
  if (lane == 0) r[(long)blockIdx.y * rows + row] = apply_norm ? rsqrtf(sum) : 1.0f;
}

// grid = (column tiles, row tiles of the panel). Row tile tile0 + blockIdx.y of
// the G * nT row tiles of all matrices; P row blockIdx.y * 128 + local row.
template <int MODE, bool GRAD>
__global__ __launch_bounds__(GRAM_THREADS) void tile_kernel(
    const __hip_bfloat16* __restrict__ S, const __hip_bfloat16* __restrict__ T,
    const float* __restrict__ rs, const float* __restrict__ rt, __hip_bfloat16* __restrict__ P,
    float* __restrict__ partials, int M, int D, int nT, long tile0, long Mpad) {
  __shared__ __attribute__((aligned(16))) __hip_bfloat16 lds[2][4][GRAM_TILE * GRAM_STRIDE];
  __shared__ float rj_lds[2][GRAM_TILE];
  __shared__ float red_lds[GRAM_THREADS / WAVE_SIZE];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int l31 = lane & 31;
  const int hhalf = lane >> 5;
  const int wr = wave >> 1;  // row half of the tile
  const int wc = wave & 1;   // column half
  const long tile = tile0 + blockIdx.y;
  const long g = tile / nT;
  const int i0 = (int)(tile - g * nT) * GRAM_TILE;
  const int j0 = (int)blockIdx.x * GRAM_TILE;
  const long base = g * (long)M;  // first row of matrix g
  const int nkc = (D + GRAM_BK - 1) / GRAM_BK;

  {
    const int which = tid >> 7;  // 0: student, 1: teacher
    const int j = j0 + (tid & (GRAM_TILE - 1));
    const float v = (which ? rt : rs)[base + (j < M ? j : M - 1)];
    rj_lds[which][tid & (GRAM_TILE - 1)] = j < M ? v : 0.f;
  }

  // ---- staging: thread t owns 16-byte chunk t & 7 of rows (t >> 3) + 32 q of
  //      every panel; panels 0..3 = S_i, S_j, T_i, T_j ----
  const int srow = tid >> 3;
  const int scol = (tid & 7) * 8;
  bf16x8 reg[4][4];
  unsigned in_range = 0;  // bit q: row i0 + srow + 32 q and the column are inside; bit 4 + q: row j0 + ...
  auto issue_loads = [&](int kc) {
    const int col = kc * GRAM_BK + scol;
    const bool col_ok = col < D;
    const int ccol = col_ok ? col : 0;
    unsigned ok = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ri = i0 + srow + 32 * q;
      const int rj = j0 + srow + 32 * q;
      const long ai = (base + (ri < M ? ri : M - 1)) * (long)D + ccol;
      const long aj = (base + (rj < M ? rj : M - 1)) * (long)D + ccol;
      reg[0][q] = load8(S + ai);
      reg[1][q] = load8(S + aj);
      reg[2][q] = load8(T + ai);
      reg[3][q] = load8(T + aj);
      ok |= (col_ok && ri < M) ? 1u << q : 0u;
      ok |= (col_ok && rj < M) ? 16u << q : 0u;
    }
    in_range = ok;
  };
  auto write_stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = (in_range >> ((p & 1) * 4 + q)) & 1;
        *reinterpret_cast<bf16x8*>(&lds[buf][p][(srow + 32 * q) * GRAM_STRIDE + scol]) =
            ok ? reg[p][q] : bf16x8{};
      }
    }
  };

  // acc[product][jb][ib]: C[row = column j of the tile][col = row i of the tile]
  f32x16 acc[2][2][2] = {};

  issue_loads(0);
  write_stage(0);
  __syncthreads();
  for (int kc = 0; kc < nkc; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nkc) issue_loads(kc + 1);  // block-uniform

    const int frag = l31 * GRAM_STRIDE + hhalf * 8;
    const __hip_bfloat16* si = &lds[buf][0][(wr * 64) * GRAM_STRIDE + frag];
    const __hip_bfloat16* sj = &lds[buf][1][(wc * 64) * GRAM_STRIDE + frag];
    const __hip_bfloat16* ti = &lds[buf][2][(wr * 64) * GRAM_STRIDE + frag];
    const __hip_bfloat16* tj = &lds[buf][3][(wc * 64) * GRAM_STRIDE + frag];
#pragma unroll
    for (int s = 0; s < GRAM_BK / 16; ++s) {
      bf16x8 fi[2][2], fj[2][2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        fi[0][b] = load8(si + b * 32 * GRAM_STRIDE + s * 16);
        fj[0][b] = load8(sj + b * 32 * GRAM_STRIDE + s * 16);
        fi[1][b] = load8(ti + b * 32 * GRAM_STRIDE + s * 16);
        fj[1][b] = load8(tj + b * 32 * GRAM_STRIDE + s * 16);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
          for (int ib = 0; ib < 2; ++ib)
            acc[m][jb][ib] = MFMA32(fj[m][jb], fi[m][ib], acc[m][jb][ib]);
    }

    // Buffer buf ^ 1 was last read in chunk kc - 1; every wave has passed the
    // barrier that ended it.
    if (kc + 1 < nkc) write_stage(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue ----
  float lsum = 0.f;
#pragma unroll
  for (int ib = 0; ib < 2; ++ib) {
    const int il = wr * 64 + ib * 32 + l31;  // row inside the tile
    const int i = i0 + il;
    const float ri_s = rs[base + (i < M ? i : M - 1)];
    const float ri_t = rt[base + (i < M ? i : M - 1)];
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      const int jl0 = wc * 64 + jb * 32;  // first column of the MFMA tile inside the tile
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = jl0 + c_row(r, hhalf);
        const float rj_s = rj_lds[0][jl];
        const float A = acc[0][jb][ib][r] * ri_s * rj_s;
        const float B = acc[1][jb][ib][r] * ri_t * rj_lds[1][jl];
        float a = A, b = B;
        bool mask = true;
        if (MODE == 1) {
          a = A < 0.f ? 0.f : A;
          b = B < 0.f ? 0.f : B;
          mask = !(A < 0.f);
        } else if (MODE == 2) {
          mask = !(A < 0.f && B < 0.f);
          a = mask ? A : 0.f;
          b = B < 0.f ? 0.f : B;
        }
        const float e = a - b;
        lsum += e * e;
        p[r] = mask ? e * rj_s : 0.f;
      }
      if constexpr (GRAD) {
        // regs 0..7 are columns 0..15 of the MFMA tile, regs 8..15 columns
        // 16..31; after the exchange this lane holds 8 consecutive ones.
        __hip_bfloat16* dst =
            P + ((long)blockIdx.y * GRAM_TILE + il) * Mpad + j0 + jl0 + hhalf * 8;
        *reinterpret_cast<bf16x8*>(dst) = pack_fragment(p, 0);
        *reinterpret_cast<bf16x8*>(dst + 16) = pack_fragment(p, 8);
      }
    }
  }
  lsum = wave_reduce_sum(lsum);
  if (lane == 0) red_lds[wave] = lsum;
  __syncthreads();
  if (tid == 0)
    partials[tile * nT + blockIdx.x] = ((red_lds[0] + red_lds[1]) + red_lds[2]) + red_lds[3];
}

// One block: thread t sums partials t, t + 256, ... in order, then the block
// reduces. loss = sum / count in fp64 (count = G M^2 can exceed 2^24).
__global__ __launch_bounds__(GRAM_FIN_THREADS) void finish_kernel(
    const float* __restrict__ partials, float* __restrict__ loss, long n, double count) {
  __shared__ float red[16];
  float sum = 0.f;
  for (long i = threadIdx.x; i < n; i += GRAM_FIN_THREADS) sum += partials[i];
  sum = block_reduce_sum(sum, red);
  if (threadIdx.x == 0) *loss = (float)((double)sum / count);
}

// dS_i = c r_i (Draw_i - S_i r_i^2 (S_i . Draw_i)), or c Draw_i without apply_norm.
__global__ __launch_bounds__(GRAM_ROW_THREADS) void norm_bwd_kernel(
    const __hip_bfloat16* __restrict__ draw, const __hip_bfloat16* __restrict__ s,
    const float* __restrict__ rs, __hip_bfloat16* __restrict__ ds, long rows, int D, float c,
    int apply_norm) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const long row = (long)blockIdx.x * (GRAM_ROW_THREADS / WAVE_SIZE) + threadIdx.x / WAVE_SIZE;
  if (row >= rows) return;  // wave-uniform
  const __hip_bfloat16* __restrict__ x = s + row * (long)D;
  const __hip_bfloat16* __restrict__ d = draw + row * (long)D;
  float proj = 0.f, scale = c;
  if (apply_norm) {
    float dot = 0.f;
    for (int k = lane * 8; k < D; k += WAVE_SIZE * 8) {
      const short8_t xv = *reinterpret_cast<const short8_t*>(x + k);
      const short8_t dv = *reinterpret_cast<const short8_t*>(d + k);
#pragma unroll
      for (int e = 0; e < 8; ++e) dot += bf16_to_f32(xv[e]) * bf16_to_f32(dv[e]);
    }
#pragma unroll
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) dot += __shfl_xor(dot, off, WAVE_SIZE);
    const float r = rs[row];
    proj = r * r * dot;
    scale = c * r;
  }
  for (int k = lane * 8; k < D; k += WAVE_SIZE * 8) {
    const short8_t xv = *reinterpret_cast<const short8_t*>(x + k);
    const short8_t dv = *reinterpret_cast<const short8_t*>(d + k);
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      out[e] = scale * (bf16_to_f32(dv[e]) - bf16_to_f32(xv[e]) * proj);
    Pack8<__hip_bfloat16>::store(ds + row * (long)D + k, out);
  }
}

}  // namespace gram

void launch_gram_rnorm(const __hip_bfloat16* s, const __hip_bfloat16* t, float* r, long rows, int D,
                       bool apply_norm, hipStream_t stream) {
  const int per_block = GRAM_ROW_THREADS / WAVE_SIZE;
  const dim3 grid((unsigned)((rows + per_block - 1) / per_block), 2);
  hipLaunchKernelGGL(gram::rnorm_kernel, grid, dim3(GRAM_ROW_THREADS), 0, stream, s, t, r, rows, D,
                     apply_norm ? 1 : 0);
  HIP_CHECK_LAUNCH();
}

void launch_gram_tiles(const __hip_bfloat16* S, const __hip_bfloat16* T, const float* rs,
                       const float* rt, __hip_bfloat16* P, float* partials, int M, int D, int mode,
                       long tile0, int ntiles, hipStream_t stream) {
  const int nT = (M + GRAM_TILE - 1) / GRAM_TILE;
  const long Mpad = (long)nT * GRAM_TILE;
  const dim3 grid((unsigned)nT, (unsigned)ntiles);
  const dim3 block(GRAM_THREADS);
#define GRAM_LAUNCH(MODE, GRAD)                                                              \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(gram::tile_kernel<MODE, GRAD>), grid, block, 0, stream, S, T, \
                     rs, rt, P, partials, M, D, nT, tile0, Mpad)
  if (P != nullptr) {
    if (mode == 0) GRAM_LAUNCH(0, true);
    else if (mode == 1) GRAM_LAUNCH(1, true);
    else GRAM_LAUNCH(2, true);
  } else {
    if (mode == 0) GRAM_LAUNCH(0, false);
    else if (mode == 1) GRAM_LAUNCH(1, false);
    else GRAM_LAUNCH(2, false);
  }
#undef GRAM_LAUNCH
  HIP_CHECK_LAUNCH();
}

void launch_gram_finish(const float* partials, float* loss, long n, double count,
                        hipStream_t stream) {
  hipLaunchKernelGGL(gram::finish_kernel, dim3(1), dim3(GRAM_FIN_THREADS), 0, stream, partials,
                     loss, n, count);
  HIP_CHECK_LAUNCH();
}

void launch_gram_norm_bwd(const __hip_bfloat16* draw, const __hip_bfloat16* s, const float* rs,
                          __hip_bfloat16* ds, long rows, int D, float c, bool apply_norm,
                          hipStream_t stream) {
  const int per_block = GRAM_ROW_THREADS / WAVE_SIZE;
  hipLaunchKernelGGL(gram::norm_bwd_kernel, dim3((unsigned)((rows + per_block - 1) / per_block)),
                     dim3(GRAM_ROW_THREADS), 0, stream, draw, s, rs, ds, rows, D, c,
                     apply_norm ? 1 : 0);
  HIP_CHECK_LAUNCH();
}

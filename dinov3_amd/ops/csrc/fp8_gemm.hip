// FP8 path for the transformer-block linears: e4m3fn forward, and the opt-in
// backward with e5m2 gradients (docs/KERNELS.md "FP8 forward", "FP8 backward").
//
//   fp8_quant_rows : bf16 [M,K] -> fp8 bytes [M,K] + one power-of-two fp32
//                    scale per row (per token for activations, per output
//                    channel for weights). e4m3 or e5m2.
//   fp8_quant_cols_t: bf16 [R,C] -> fp8 bytes [C,Rp] (the transpose, rows
//                    padded with zeros to a multiple of 128) + one scale per
//                    column of the input (+ optional fp32 column sums).
//   fp8_gemm_nt    : y[M,N] = bf16( (q_x[M,K] . q_w[N,K]^T) * s_x[m] * s_w[n]
//                    + bias[n] ) on gfx950's block-scaled MFMA
//                    v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales
//                    (twice the bf16 MFMA rate; the plain fp8 MFMAs only run
//                    at the bf16 rate).
//                    The first operand is e4m3 (forward) or e5m2 (dgrad and
//                    wgrad); the second is always e4m3.
//   probe_mfma_fp8 : one-wave check of the operand lane map assumed below,
//                    for every pairing of the two formats.
//
// Numerics contract (docs/KERNELS.md "FP8 forward"; the torch emulation in
// ops/fp8_linear.py is the bit-exact oracle):
//   amax = max_k |row[k]| = m * 2^e, m in [1,2)
//   s    = 2^(e-8) if m <= 1.75 else 2^(e-7)     (amax == 0 -> s = 1)
//   q    = rne_e4m3(row / s)                     (exact division, no clamp)
// e5m2 uses the same rule with its largest finite value 57344 = 1.75 * 2^15:
//   s    = 2^(e-15) if m <= 1.75 else 2^(e-14)
// The scale exponent is floored at -126 so that s and 1/s stay normal fp32;
// that only touches rows with amax < 2^-118.
//
// Operand lane map of the 16x16x128 f8f6f4 MFMA with fp8 operands (pinned on
// the device by probe_mfma_fp8 with exact integer data):
//   A[i][k]: lane l holds row i = l&15, bytes k = 32*(l>>4) + 0..31 (8 VGPRs)
//   B[k][j]: lane l holds col j = l&15, bytes k = 32*(l>>4) + 0..31
//   D[i][j]: lane l, reg r holds i = 4*(l>>4) + r, j = l&15
// With unit block scales any k-order inside the 128-deep step gives the same
// sum as long as A and B use the same one; both come from the same code here.

#include "fp8_gemm.h"

typedef __attribute__((ext_vector_type(8))) int int8v_t;
typedef __attribute__((ext_vector_type(4))) int int4v_t;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2_t;

#define FP8_UNIT_SCALE 0x7f7f7f7f  // E8M0 1.0 in every byte

// FA / FB: format of the MFMA's A / B operand (FP8_FMT_E4M3 or FP8_FMT_E5M2);
// they are the instruction's cbsz / blgp immediates. op_sel 0, unit scales.
template <int FA, int FB>
DEV_INLINE float4_t mfma_fp8_16x16x128(int8v_t a, int8v_t b, float4_t c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0, FP8_UNIT_SCALE, 0,
                                                          FP8_UNIT_SCALE);
}

// ---------------------------------------------------------------------------
// Row quantiser
// ---------------------------------------------------------------------------

// Power-of-two scale of a row with absolute maximum `amax`; *inv = 1 / scale.
// Largest finite value: 448 = 0.875 * 2^9 (e4m3), 57344 = 0.875 * 2^16 (e5m2).
template <int FMT>
DEV_INLINE float fp8_row_scale(float amax, float* inv) {
  if (!(amax > 0.f)) {
    *inv = 1.f;
    return 1.f;
  }
  int e;
  const float m = frexpf(amax, &e);  // amax = m * 2^e, m in [0.5, 1)
  int se = e - (FMT == FP8_FMT_E5M2 ? 16 : 9) + (m > 0.875f ? 1 : 0);
  se = se < -126 ? -126 : (se > 126 ? 126 : se);
  *inv = __int_as_float((127 - se) << 23);
  return __int_as_float((127 + se) << 23);
}

DEV_INLINE float absmax8(short8_t v, float m) {
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(bf16_to_f32(v[e])));
  return m;
}

// Two fp32 -> two fp8 bytes in the low (HI = false) or high half of `old`.
template <int FMT, bool HI>
DEV_INLINE int cvt_pk_f8(float a, float b, int old) {
  if (FMT == FP8_FMT_E5M2) return __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
  return __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, HI);
}

// 8 bf16 -> 8 fp8 bytes (element 0 in the lowest byte), hardware RNE.
template <int FMT>
DEV_INLINE uint2_t quant8(short8_t v, float inv) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bf16_to_f32(v[e]) * inv;
  int lo = 0, hi = 0;
  lo = cvt_pk_f8<FMT, false>(f[0], f[1], lo);
  lo = cvt_pk_f8<FMT, true>(f[2], f[3], lo);
  hi = cvt_pk_f8<FMT, false>(f[4], f[5], hi);
  hi = cvt_pk_f8<FMT, true>(f[6], f[7], hi);
  uint2_t o;
  o.x = (unsigned int)lo;
  o.y = (unsigned int)hi;
  return o;
}

#define FP8_QUANT_ROWS_PER_BLOCK 4  // one wave per row
#define FP8_QUANT_CACHE 8           // 16-byte chunks a lane keeps in registers

// One wave per row, one pass over global memory while the row fits the
// register cache (K <= 8 * 64 * 8 = 4096); longer rows are read a second time.
template <bool CACHED, int FMT>
__global__ __launch_bounds__(WAVE_SIZE * FP8_QUANT_ROWS_PER_BLOCK) void fp8_quant_rows_kernel(
    const __hip_bfloat16* __restrict__ x, unsigned char* __restrict__ q,
    float* __restrict__ scale, long M, int K) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const long row = (long)blockIdx.x * FP8_QUANT_ROWS_PER_BLOCK + (threadIdx.x / WAVE_SIZE);
  if (row >= M) return;  // wave-uniform
  const short8_t* __restrict__ xr = reinterpret_cast<const short8_t*>(x + row * (long)K);
  uint2_t* __restrict__ qr = reinterpret_cast<uint2_t*>(q + row * (long)K);
  const int nvec = K / FP8_QUANT_VEC;

  short8_t v[FP8_QUANT_CACHE];
  float amax = 0.f;
  if (CACHED) {
#pragma unroll
    for (int c = 0; c < FP8_QUANT_CACHE; ++c) {
      const int idx = c * WAVE_SIZE + lane;
      if (idx < nvec) {
        v[c] = xr[idx];
        amax = absmax8(v[c], amax);
      }
    }
  } else {
    for (int idx = lane; idx < nvec; idx += WAVE_SIZE) amax = absmax8(xr[idx], amax);
  }
#pragma unroll
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, WAVE_SIZE));

  float inv;
  const float s = fp8_row_scale<FMT>(amax, &inv);
  if (lane == 0) scale[row] = s;

  if (CACHED) {
#pragma unroll
    for (int c = 0; c < FP8_QUANT_CACHE; ++c) {
      const int idx = c * WAVE_SIZE + lane;
      if (idx < nvec) qr[idx] = quant8<FMT>(v[c], inv);
    }
  } else {
    for (int idx = lane; idx < nvec; idx += WAVE_SIZE) qr[idx] = quant8<FMT>(xr[idx], inv);
  }
}

template <int FMT>
static void launch_fp8_quant_rows_fmt(const __hip_bfloat16* x, unsigned char* q, float* scale,
                                      long M, int K, hipStream_t stream) {
  const dim3 grid((unsigned)((M + FP8_QUANT_ROWS_PER_BLOCK - 1) / FP8_QUANT_ROWS_PER_BLOCK));
  const dim3 block(WAVE_SIZE * FP8_QUANT_ROWS_PER_BLOCK);
  if (K <= FP8_QUANT_CACHE * WAVE_SIZE * FP8_QUANT_VEC) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_quant_rows_kernel<true, FMT>), grid, block, 0, stream,
                       x, q, scale, M, K);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_quant_rows_kernel<false, FMT>), grid, block, 0, stream,
                       x, q, scale, M, K);
  }
  HIP_CHECK_LAUNCH();
}

void launch_fp8_quant_rows(const __hip_bfloat16* x, unsigned char* q, float* scale, long M,
                           int K, int fmt, hipStream_t stream) {
  if (M <= 0) return;
  if (fmt == FP8_FMT_E5M2) {
    launch_fp8_quant_rows_fmt<FP8_FMT_E5M2>(x, q, scale, M, K, stream);
  } else {
    launch_fp8_quant_rows_fmt<FP8_FMT_E4M3>(x, q, scale, M, K, stream);
  }
}

// ---------------------------------------------------------------------------
// Transposing column quantiser (backward operands)
// ---------------------------------------------------------------------------
// x [R,C] bf16 -> q [C,Rp] fp8, Rp = ceil(R/128)*128, one scale per column of
// x (= per row of q), so that a GEMM contracting over R sees scales that do
// not depend on the contraction index. Two passes over x:
//
// Pass 1 (fp8_col_stats_kernel): a block owns 64 columns; a thread owns 8
// adjacent columns (16-byte loads) and walks the rows slice, slice + S, ...
// of its block's share. The 32 slices of a block are merged through LDS in
// slice order and the block stores one row of a [partials, C] fp32 workspace
// (amax, and the column sums when asked): no atomics. fp8_col_finalize_kernel
// merges the partial rows in row order, so the sums are bit-reproducible (the
// grid depends on R and C only); a max is order-independent anyway.
//
// Pass 2 (fp8_quant_cols_t_kernel): a block owns a tile of 128 rows x 64
// columns. Thread t loads rows 4*(t>>3) .. +3 of column group cg = t&7 (16
// bytes each), scales every column by its own 1/s and converts in registers.
// v_cvt_pk_*_f32 packs two values per call, so pairing rows (r, r+1) and
// (r+2, r+3) of ONE column gives the dword "4 consecutive rows of column c"
// directly: the 4x8 register transpose is free. The dwords go to an LDS image
// [64 columns][128 row bytes], then every lane reads 16 bytes along the rows
// of one column (ds_read_b128) and stores them to q: 8 lanes cover the 128
// contiguous output bytes of a column.
//
// LDS conflicts. The image is swizzled: 16-byte chunk k of column c sits at
// chunk k ^ ((c >> 3) & 7) of the column's 128 bytes.
//  - ds_write_b32: banks are (a/4) % 32, served per 32-lane half. A column is
//    exactly 32 dwords, so the bank is the dword's position inside its
//    column: 4*((rg>>2) ^ cg) + (rg&3) with rg = t>>3. In one half rg>>2 is
//    constant, rg&3 takes 0..3 and cg takes 0..7: 32 distinct banks. (Without
//    the swizzle the 8 column groups of a row group would share a bank.)
//  - ds_read_b128: banks are (a/4) % 64, a 256-byte bank row holds two
//    columns, and the 16-lane groups are {0-3,12-15,20-27}, {4-11,16-19,
//    28-31} (+32). A wave reads 8 columns c0..c0+7 with c0 % 8 == 0, lane l
//    column c0 + (l>>3), chunk l&7, so (c>>3)&7 = g is wave-uniform and the
//    16-byte position in the bank row is (c&1)*8 + ((l&7) ^ g). The first
//    group holds (even c, chunks 0-3), (odd c, 4-7), (even c, 4-7), (odd c,
//    0-3): positions {0-3}^g, 8+{4-7}^g, {4-7}^g, 8+{0-3}^g, all 16 distinct;
//    the second group is the same with the chunk halves swapped.
// tests/test_fp8_backward.py replays both maps.
//
// Rows R..Rp-1 of a tile are loaded as zeros and come out as byte 0x00 (zero in
// both formats): the kernel writes the pad itself.

// 1/s of a power-of-two scale with exponent in [-126, 126].
DEV_INLINE float fp8_pow2_inv(float s) {
  return __int_as_float((254 - (__float_as_int(s) >> 23)) << 23);
}

template <bool WITH_SUM>
__global__ __launch_bounds__(FP8_COLS_THREADS) void fp8_col_stats_kernel(
    const __hip_bfloat16* __restrict__ x, float* __restrict__ part_amax,
    float* __restrict__ part_sum, long R, int C) {
  __shared__ float red_max[FP8_COLS_SLICES][FP8_COLS_TC];
  __shared__ float red_sum[WITH_SUM ? FP8_COLS_SLICES : 1][FP8_COLS_TC];
  const int cg = threadIdx.x & 7;
  const int slice = threadIdx.x >> 3;
  const int col = blockIdx.x * FP8_COLS_TC + cg * FP8_QUANT_VEC;
  float amax[8], sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) amax[e] = sum[e] = 0.f;
  if (col < C) {
    const long step = (long)gridDim.y * FP8_COLS_SLICES;
#pragma unroll 4
    for (long r = (long)blockIdx.y * FP8_COLS_SLICES + slice; r < R; r += step) {
      const short8_t v = *reinterpret_cast<const short8_t*>(x + r * (long)C + col);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf16_to_f32(v[e]);
        amax[e] = fmaxf(amax[e], fabsf(f));
        if (WITH_SUM) sum[e] += f;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red_max[slice][cg * 8 + e] = amax[e];
    if (WITH_SUM) red_sum[slice][cg * 8 + e] = sum[e];
  }
  __syncthreads();
  const int c = threadIdx.x;
  const int ocol = blockIdx.x * FP8_COLS_TC + c;
  if (c < FP8_COLS_TC && ocol < C) {
    float m = red_max[0][c];
    float s = WITH_SUM ? red_sum[0][c] : 0.f;
#pragma unroll
    for (int k = 1; k < FP8_COLS_SLICES; ++k) {
      m = fmaxf(m, red_max[k][c]);
      if (WITH_SUM) s += red_sum[k][c];
    }
    part_amax[(long)blockIdx.y * C + ocol] = m;
    if (WITH_SUM) part_sum[(long)blockIdx.y * C + ocol] = s;
  }
}

// scale (may be null) from the merged amax, colsum (may be null) from the
// merged sums; one thread per column, partial rows in row order.
template <int FMT>
__global__ __launch_bounds__(FP8_COLS_THREADS) void fp8_col_finalize_kernel(
    const float* __restrict__ part_amax, const float* __restrict__ part_sum,
    float* __restrict__ scale, float* __restrict__ colsum, int n_partials, int C) {
  const int col = blockIdx.x * FP8_COLS_THREADS + threadIdx.x;
  if (col >= C) return;
  if (scale != nullptr) {
    float m = 0.f;
    for (int p = 0; p < n_partials; ++p) m = fmaxf(m, part_amax[(long)p * C + col]);
    float inv;
    scale[col] = fp8_row_scale<FMT>(m, &inv);
  }
  if (colsum != nullptr) {
    float s = 0.f;
    for (int p = 0; p < n_partials; ++p) s += part_sum[(long)p * C + col];
    colsum[col] = s;
  }
}

template <int FMT>
__global__ __launch_bounds__(FP8_COLS_THREADS) void fp8_quant_cols_t_kernel(
    const __hip_bfloat16* __restrict__ x, const float* __restrict__ scale,
    unsigned char* __restrict__ q, long R, long Rp, int C) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[FP8_COLS_TC * FP8_COLS_TR];
  const int tid = threadIdx.x;
  const int cg = tid & 7;
  const int rg = tid >> 3;  // 0..31: rows 4*rg .. 4*rg+3 of the tile
  const long row0 = (long)blockIdx.x * FP8_COLS_TR;
  const int col0 = blockIdx.y * FP8_COLS_TC;
  const int col = col0 + cg * FP8_QUANT_VEC;

  if (col < C) {  // a column group past C is neither written to LDS nor read back
    float inv[8];
    {
      const float4_t s0 = *reinterpret_cast<const float4_t*>(scale + col);
      const float4_t s1 = *reinterpret_cast<const float4_t*>(scale + col + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        inv[e] = fp8_pow2_inv(s0[e]);
        inv[4 + e] = fp8_pow2_inv(s1[e]);
      }
    }
    short8_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long r = row0 + rg * 4 + i;
      v[i] = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < R) v[i] = *reinterpret_cast<const short8_t*>(x + r * (long)C + col);
    }
    unsigned char* dst = tile + (cg * 8) * FP8_COLS_TR + (((rg >> 2) ^ cg) * 16) + (rg & 3) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int d = 0;
      d = cvt_pk_f8<FMT, false>(bf16_to_f32(v[0][j]) * inv[j], bf16_to_f32(v[1][j]) * inv[j], d);
      d = cvt_pk_f8<FMT, true>(bf16_to_f32(v[2][j]) * inv[j], bf16_to_f32(v[3][j]) * inv[j], d);
      *reinterpret_cast<int*>(dst + j * FP8_COLS_TR) = d;
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < FP8_COLS_TC / 32; ++p) {
    const int cl = p * 32 + (tid >> 3);
    const int k = tid & 7;
    if (col0 + cl < C) {
      const int4v_t d = *reinterpret_cast<const int4v_t*>(
          tile + cl * FP8_COLS_TR + ((k ^ ((cl >> 3) & 7)) * 16));
      *reinterpret_cast<int4v_t*>(q + (long)(col0 + cl) * Rp + row0 + k * 16) = d;
    }
  }
}

int fp8_cols_partials(long R, int C) {
  const int col_blocks = (C + FP8_COLS_TC - 1) / FP8_COLS_TC;
  long want = (R + FP8_COLS_SLICES - 1) / FP8_COLS_SLICES;  // one row per thread at least
  long cap = 2048 / col_blocks;                              // about 2048 blocks in all
  cap = cap < 1 ? 1 : (cap > FP8_COLS_MAX_PARTIALS ? FP8_COLS_MAX_PARTIALS : cap);
  want = want < 1 ? 1 : want;
  return (int)(want < cap ? want : cap);
}

void launch_fp8_quant_cols_t(const __hip_bfloat16* x, unsigned char* q, float* scale,
                             float* colsum, float* part_amax, float* part_sum, long R, int C,
                             int fmt, hipStream_t stream) {
  if (R <= 0 || C <= 0) return;
  const int np = fp8_cols_partials(R, C);
  const dim3 sgrid((C + FP8_COLS_TC - 1) / FP8_COLS_TC, np);
  const dim3 block(FP8_COLS_THREADS);
  if (colsum != nullptr) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_col_stats_kernel<true>), sgrid, block, 0, stream, x,
                       part_amax, part_sum, R, C);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_col_stats_kernel<false>), sgrid, block, 0, stream, x,
                       part_amax, part_sum, R, C);
  }
  HIP_CHECK_LAUNCH();
  const dim3 fgrid((C + FP8_COLS_THREADS - 1) / FP8_COLS_THREADS);
  const long Rp = (R + FP8_COLS_TR - 1) / FP8_COLS_TR * FP8_COLS_TR;
  const dim3 qgrid((unsigned)(Rp / FP8_COLS_TR), (C + FP8_COLS_TC - 1) / FP8_COLS_TC);
  if (fmt == FP8_FMT_E5M2) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_col_finalize_kernel<FP8_FMT_E5M2>), fgrid, block, 0,
                       stream, part_amax, part_sum, scale, colsum, np, C);
    HIP_CHECK_LAUNCH();
    if (q != nullptr) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_quant_cols_t_kernel<FP8_FMT_E5M2>), qgrid, block, 0,
                         stream, x, scale, q, R, Rp, C);
      HIP_CHECK_LAUNCH();
    }
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_col_finalize_kernel<FP8_FMT_E4M3>), fgrid, block, 0,
                       stream, part_amax, part_sum, scale, colsum, np, C);
    HIP_CHECK_LAUNCH();
    if (q != nullptr) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_quant_cols_t_kernel<FP8_FMT_E4M3>), qgrid, block, 0,
                         stream, x, scale, q, R, Rp, C);
      HIP_CHECK_LAUNCH();
    }
  }
}

// ---------------------------------------------------------------------------
// GEMM: y = epilogue(q_x . q_w^T), both operands K-contiguous
// ---------------------------------------------------------------------------
// Block: 128x128 outputs, 256 threads = 4 waves as 2 (M) x 2 (N); a wave owns
// 64x64 = 4x4 MFMA tiles of 16x16. One K-step is FP8_GEMM_BK = 128 bytes, one
// scaled MFMA deep. LDS: two buffers, each an A image [128 rows][128 B] and a
// B image of the same shape: 2 * 2 * 16 KiB = 64 KiB in one array, so two
// blocks (two waves per SIMD) share a CU.
//
// Staging: global_load_lds, 16 bytes per lane. LDS-DMA writes wave-uniform
// base + lane*16, so the image is linear: thread t, piece i fills row
// i*32 + t/8, 16-byte slot t%8. The conflict fix is a swizzle on the SOURCE
// side, undone on the read: LDS slot c of row r holds k-slot c ^ swz(r),
//   swz(r) = bit1(r) | bit2(r) << 2.
// Fragment reads are ds_read_b128: lane l reads row l&15, k-slots 2*(l>>4)
// and 2*(l>>4)+1. A ds_read_b128 is served in the four 16-lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32 for the upper half), and with
// 128-byte rows the 256-byte bank row holds two rows, so a lane's 16-byte
// position in the bank row is (r&1)*8 + (slot ^ swz(r)). Inside one group the
// rows {0-3,12-15} read slot s and the rows {4-11} read slot s^2; swz maps
// each set's even (and odd) rows onto {0,1,4,5}, so the first set covers
// positions s^{0,1,4,5} and the second s^2^{0,1,4,5} = s^{2,3,6,7}: all 16
// positions distinct, conflict-free. tests/test_fp8_layouts.py replays this.
//
// Edges: rows of A past M and rows of B past N are never loaded. Their LDS
// slots are zeroed once before the K loop (no LDS-DMA ever targets them: the
// lanes that own them stay masked off), so they read as zeros in every K-step
// and the outputs they feed are not stored.

#define FP8_TILE_BYTES (FP8_GEMM_BM * FP8_GEMM_BK)  // one operand image, 16 KiB
#define FP8_BUF_BYTES (2 * FP8_TILE_BYTES)          // A image + B image
#define FP8_STAGE_PIECES (FP8_TILE_BYTES / (FP8_GEMM_THREADS * 16))  // 4 per operand
#define FP8_ROWS_PER_PIECE (FP8_GEMM_THREADS * 16 / FP8_GEMM_BK)      // 32

static_assert(FP8_GEMM_BM == FP8_GEMM_BN, "A and B images share one staging map");
static_assert(FP8_GEMM_BK == 128, "one 16x16x128 MFMA per K-step");

DEV_INLINE int fp8_swz(int r) { return ((r >> 1) & 1) | (((r >> 2) & 1) << 2); }

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

DEV_INLINE void glds16(const unsigned char* src, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)lds_wave_base, 16, 0, 0);
}

DEV_INLINE int8v_t lds_frag(const unsigned char* tile, int off0, int off1) {
  const int4v_t lo = *reinterpret_cast<const int4v_t*>(tile + off0);
  const int4v_t hi = *reinterpret_cast<const int4v_t*>(tile + off1);
  int8v_t f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

// FMT_A: format of the first operand (rows of the output); the second operand
// is always e4m3.
template <bool HAS_BIAS, int FMT_A>
__global__ __launch_bounds__(FP8_GEMM_THREADS, 2) void fp8_gemm_nt_kernel(
    const unsigned char* __restrict__ A, const float* __restrict__ sa,
    const unsigned char* __restrict__ B, const float* __restrict__ sb,
    const __hip_bfloat16* __restrict__ bias, __hip_bfloat16* __restrict__ Y, long M, int N,
    int K) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * FP8_BUF_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int wm = wid >> 1, wn = wid & 1;
  const long brow = (long)blockIdx.y * FP8_GEMM_BM;
  const int bcol = blockIdx.x * FP8_GEMM_BN;

  // ---- staging map ----
  const int srow = tid >> 3;                      // row inside a 32-row piece
  const int sslot = (tid & 7) ^ fp8_swz(srow);    // k-slot this lane fetches
  const unsigned char* a_src = A + (brow + srow) * (long)K + sslot * 16;
  const unsigned char* b_src = B + ((long)bcol + srow) * (long)K + sslot * 16;
  const long piece_stride = (long)FP8_ROWS_PER_PIECE * K;
  bool a_ok[FP8_STAGE_PIECES], b_ok[FP8_STAGE_PIECES];
#pragma unroll
  for (int i = 0; i < FP8_STAGE_PIECES; ++i) {
    a_ok[i] = brow + i * FP8_ROWS_PER_PIECE + srow < M;
    b_ok[i] = bcol + i * FP8_ROWS_PER_PIECE + srow < N;
  }

  // Zero the slots of out-of-range rows in both buffers, once.
  {
    const int4v_t z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < FP8_STAGE_PIECES; ++i) {
      const int off = i * (FP8_GEMM_THREADS * 16) + tid * 16;
      if (!a_ok[i]) {
        *reinterpret_cast<int4v_t*>(lds + off) = z;
        *reinterpret_cast<int4v_t*>(lds + FP8_BUF_BYTES + off) = z;
      }
      if (!b_ok[i]) {
        *reinterpret_cast<int4v_t*>(lds + FP8_TILE_BYTES + off) = z;
        *reinterpret_cast<int4v_t*>(lds + FP8_BUF_BYTES + FP8_TILE_BYTES + off) = z;
      }
    }
  }

  auto stage = [&](int buf, int k0) {
    unsigned char* la = lds + buf * FP8_BUF_BYTES + wid * (WAVE_SIZE * 16);
    unsigned char* lb = la + FP8_TILE_BYTES;
#pragma unroll
    for (int i = 0; i < FP8_STAGE_PIECES; ++i) {
      if (a_ok[i]) glds16(a_src + i * piece_stride + k0, la + i * (FP8_GEMM_THREADS * 16));
    }
#pragma unroll
    for (int i = 0; i < FP8_STAGE_PIECES; ++i) {
      if (b_ok[i]) glds16(b_src + i * piece_stride + k0, lb + i * (FP8_GEMM_THREADS * 16));
    }
  };

  // ---- fragment read map ----
  const int fr = lane & 15, fg = lane >> 4;
  const int foff0 = fr * FP8_GEMM_BK + (((2 * fg) ^ fp8_swz(fr)) * 16);
  const int foff1 = fr * FP8_GEMM_BK + (((2 * fg + 1) ^ fp8_swz(fr)) * 16);

  float4_t acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = float4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = K / FP8_GEMM_BK;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    // Tile kt has landed (every wave drains its own LDS-DMA, then the
    // barrier), and every wave is done reading the other buffer (K-step kt-1).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * FP8_GEMM_BK);

    const unsigned char* ta = lds + buf * FP8_BUF_BYTES + wm * (64 * FP8_GEMM_BK);
    const unsigned char* tb = lds + buf * FP8_BUF_BYTES + FP8_TILE_BYTES + wn * (64 * FP8_GEMM_BK);
    int8v_t af[4], bf[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = lds_frag(ta + m * (16 * FP8_GEMM_BK), foff0, foff1);
#pragma unroll
    for (int n = 0; n < 4; ++n) bf[n] = lds_frag(tb + n * (16 * FP8_GEMM_BK), foff0, foff1);
    // The weight fragment goes in as the MFMA's A operand and the activation
    // fragment as its B operand, so the tile comes out transposed: a lane
    // holds 4 consecutive output columns of one output row (packed stores).
    // So the second operand's format is cbsz and the first operand's is blgp.
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = mfma_fp8_16x16x128<FP8_FMT_E4M3, FMT_A>(bf[n], af[m], acc[m][n]);
  }

  // ---- epilogue: acc * s_x[m] * s_w[n] (+ bias[n]) -> bf16, 8-byte stores ----
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const long row = brow + wm * 64 + m * 16 + fr;
    if (row >= M) continue;
    const float sx = sa[row];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = bcol + wn * 64 + n * 16 + fg * 4;
      if (col >= N) continue;  // N % 16 == 0: a 16-wide tile is all in or all out
      const float4_t sw = *reinterpret_cast<const float4_t*>(sb + col);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[m][n][j] * sx * sw[j];
      if (HAS_BIAS) {
        const uint2_t bb = *reinterpret_cast<const uint2_t*>(bias + col);
        v[0] += bf16_to_f32((short)(bb.x & 0xFFFFu));
        v[1] += bf16_to_f32((short)(bb.x >> 16));
        v[2] += bf16_to_f32((short)(bb.y & 0xFFFFu));
        v[3] += bf16_to_f32((short)(bb.y >> 16));
      }
      uint2_t o;
      o.x = pack2_bf16(v[0], v[1]);
      o.y = pack2_bf16(v[2], v[3]);
      *reinterpret_cast<uint2_t*>(Y + row * (long)N + col) = o;
    }
  }
}

void launch_fp8_gemm_nt(const unsigned char* xq, const float* sx, const unsigned char* wq,
                        const float* sw, const __hip_bfloat16* bias, __hip_bfloat16* y, long M,
                        int N, int K, int fmt_x, hipStream_t stream) {
  if (M <= 0 || N <= 0) return;
  const dim3 grid((N + FP8_GEMM_BN - 1) / FP8_GEMM_BN,
                  (unsigned)((M + FP8_GEMM_BM - 1) / FP8_GEMM_BM));
  const dim3 block(FP8_GEMM_THREADS);
  if (fmt_x == FP8_FMT_E5M2) {  // backward GEMMs; the bindings refuse a bias here
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_gemm_nt_kernel<false, FP8_FMT_E5M2>), grid, block, 0,
                       stream, xq, sx, wq, sw, bias, y, M, N, K);
  } else if (bias != nullptr) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_gemm_nt_kernel<true, FP8_FMT_E4M3>), grid, block, 0,
                       stream, xq, sx, wq, sw, bias, y, M, N, K);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fp8_gemm_nt_kernel<false, FP8_FMT_E4M3>), grid, block, 0,
                       stream, xq, sx, wq, sw, bias, y, M, N, K);
  }
  HIP_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Lane-map probe: C[16,16] = A[16,128] . Bt[16,128]^T, one wave; A is read as
// format FA (the cbsz immediate) and Bt as format FB (blgp).
// ---------------------------------------------------------------------------
template <int FA, int FB>
__global__ void probe_mfma_fp8_kernel(const unsigned char* __restrict__ A,
                                      const unsigned char* __restrict__ Bt,
                                      float* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int8v_t a = lds_frag(A, r * 128 + g * 32, r * 128 + g * 32 + 16);
  const int8v_t b = lds_frag(Bt, r * 128 + g * 32, r * 128 + g * 32 + 16);
  float4_t c = {0.f, 0.f, 0.f, 0.f};
  c = mfma_fp8_16x16x128<FA, FB>(a, b, c);
#pragma unroll
  for (int j = 0; j < 4; ++j) C[(4 * g + j) * 16 + r] = c[j];
}

void launch_probe_mfma_fp8(const unsigned char* A, const unsigned char* Bt, float* C, int fmt_a,
                           int fmt_b, hipStream_t stream) {
  const dim3 grid(1), block(64);
  if (fmt_a == FP8_FMT_E5M2 && fmt_b == FP8_FMT_E5M2) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_mfma_fp8_kernel<FP8_FMT_E5M2, FP8_FMT_E5M2>), grid,
                       block, 0, stream, A, Bt, C);
  } else if (fmt_a == FP8_FMT_E5M2) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_mfma_fp8_kernel<FP8_FMT_E5M2, FP8_FMT_E4M3>), grid,
                       block, 0, stream, A, Bt, C);
  } else if (fmt_b == FP8_FMT_E5M2) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_mfma_fp8_kernel<FP8_FMT_E4M3, FP8_FMT_E5M2>), grid,
                       block, 0, stream, A, Bt, C);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_mfma_fp8_kernel<FP8_FMT_E4M3, FP8_FMT_E4M3>), grid,
                       block, 0, stream, A, Bt, C);
  }
  HIP_CHECK_LAUNCH();
}

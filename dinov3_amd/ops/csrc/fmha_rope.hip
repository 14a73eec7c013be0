// Fused RoPE + multi-head attention, forward and FA2-style backward (K5 + K6).
//
// One kernel of each kind (fwd, dq, dkv, rowsum preprocess), parameterised at
// compile time by a memory-layout policy (fmha_rope.h):
// - PackedLayout reads qkv [B, N, 3, H, hd] bf16 (the qkv GEMM output, no
//   permutes) and writes O token-major [B, N, H, hd] so the out-projection
//   GEMM consumes it directly; backward fills ONE dqkv buffer of qkv's layout.
// - PlainLayout serves the q/k/v [B, H, N, hd] entry points (ops.fmha).
// Rotate-half RoPE (fp32 sin/cos [P, hd] tables, prefix tokens pass through)
// is applied to Q in-register and to K at LDS staging; the inverse rotation of
// dQ/dK runs in the accumulator epilogues. sin_t == nullptr: no RoPE.
//
// Design (MI355X / CDNA4):
// - v_mfma_f32_32x32x16_bf16 tiles (fragment layouts: mfma.h); wave64; each
//   wave owns 32 q rows (fwd, dq) or 32 k rows (dkv) of a (batch, head).
// - Scores are computed SWAPPED — S^T = K @ Q^T — so each lane holds a full q
//   column and the online-softmax row reduction is 16 lane-local values + one
//   shfl_xor(32). P^T (fp32 accum) repacks into the next MFMA's bf16 fragment
//   with v_cvt_pk_bf16_f32 pairs + v_permlane32_swap (pack_fragment).
// - K/V tiles of 2*KVB keys are staged in LDS per barrier pair (V or K also
//   transposed so the second MFMA's A-fragment reads contiguously); the next
//   tile's global loads are issued before the compute phase.
// - backward recomputes P from the saved logsumexp. Three kernels: preprocess
//   D = rowsum(dO*O); dQ (loop over k tiles); dK/dV (loop over q tiles).
//   Where one workgroup holds the whole sequence (hd 64, N <= 256) a single
//   kernel does all three (bwd_fused_kernel): S, P, dP and dS once per tile.

#include "fmha_rope.h"
#include "mfma.h"
#include <cstdlib>
#include <stdexcept>

namespace fmha_rope {

DEV_INLINE float b2f(__bf16 x) {
  union { float f; unsigned i; } v;
  v.i = ((unsigned)*(unsigned short*)&x) << 16;
  return v.f;
}

// rotate a (lo, hi) register pair of 8 bf16 each with fp32 tables at
// sin/cos row + column offset c0 (c0 < hd/2)
DEV_INLINE void rope_rotate8(bf16x8& lo, bf16x8& hi, const float* sinrow,
                             const float* cosrow, int c0) {
  union { unsigned u[4]; bf16x8 v; } lo_out, hi_out;
  float flo[8], fhi[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float c = cosrow[c0 + e];
    const float s = sinrow[c0 + e];
    const float l = b2f(lo[e]);
    const float h = b2f(hi[e]);
    flo[e] = l * c - h * s;
    fhi[e] = h * c + l * s;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo_out.u[e] = cvt_pk_bf16(flo[2 * e], flo[2 * e + 1]);
    hi_out.u[e] = cvt_pk_bf16(fhi[2 * e], fhi[2 * e + 1]);
  }
  lo = lo_out.v;
  hi = hi_out.v;
}

// ---------------------------------------------------------------------------
// pieces shared by the kernels
// ---------------------------------------------------------------------------

// blockIdx.x = b*H + h; a wave's lanes split into two halves of 32
struct BlockCtx {
  int b, h, wave, lane, hhalf, l31;
  int prefix;     // rows [0, prefix) are not rotated
  long stat_off;  // (b*H + h)*N: this head's row 0 of lse / D
  bool use_rope;
};

DEV_INLINE BlockCtx block_ctx(int H, int N, int P, const float* sin_t) {
  BlockCtx c;
  c.b = blockIdx.x / H;
  c.h = blockIdx.x % H;
  c.wave = threadIdx.x / 64;
  c.lane = threadIdx.x & 63;
  c.hhalf = c.lane >> 5;
  c.l31 = c.lane & 31;
  c.prefix = N - P;
  c.stat_off = ((long)c.b * H + c.h) * N;
  c.use_rope = (sin_t != nullptr);
  return c;
}

// rotate the KSLICES A/B fragments of row n (slice s pairs with s + KSLICES/2)
template <int KSLICES>
DEV_INLINE void rope_fragments(bf16x8 (&f)[KSLICES], const float* sin_t, const float* cos_t,
                               int n, const BlockCtx& c) {
  constexpr int HD = KSLICES * 16;
  const int p = n - c.prefix;
  if (c.use_rope && p >= 0) {
    const float* srow = sin_t + (long)p * HD;
    const float* crow = cos_t + (long)p * HD;
#pragma unroll
    for (int s2 = 0; s2 < KSLICES / 2; ++s2)
      rope_rotate8(f[s2], f[s2 + KSLICES / 2], srow, crow, s2 * 16 + c.hhalf * 8);
  }
}

// acc_row += a0 @ b0 + a1 @ b1 (one 32x32 C tile, k = 32)
DEV_INLINE void mfma2_acc(float (&acc_row)[16], bf16x8 a0, bf16x8 b0, bf16x8 a1, bf16x8 b1) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc_row[r];
  acc = MFMA32(a0, b0, acc);
  acc = MFMA32(a1, b1, acc);
#pragma unroll
  for (int r = 0; r < 16; ++r) acc_row[r] = acc[r];
}

// inverse rope on a gradient accumulator of row n (C rows = d): pairs
// (d, d + hd/2) = (tile t, tile t + DTILES/2) reg r
template <int DTILES>
DEV_INLINE void rope_inverse(float (&acc)[DTILES][16], const float* sin_t, const float* cos_t,
                             int n, const BlockCtx& c) {
  const int p = n - c.prefix;
  if (c.use_rope && p >= 0) {
    const float* srow = sin_t + (long)p * DTILES * 32;
    const float* crow = cos_t + (long)p * DTILES * 32;
#pragma unroll
    for (int t = 0; t < DTILES / 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = t * 32 + c_row(r, c.hhalf);
        const float co = crow[d], s = srow[d];
        const float glo = acc[t][r], ghi = acc[t + DTILES / 2][r];
        acc[t][r] = glo * co + ghi * s;
        acc[t + DTILES / 2][r] = ghi * co - glo * s;
      }
  }
}

// accumulators are C[d rows, this lane's row as column]: transposed bf16 store
// of acc * mul (the forward's 1/l; the default folds away)
template <int DTILES>
DEV_INLINE void store_rows_bf16(__hip_bfloat16* row, const float (&acc)[DTILES][16], int hhalf,
                                float mul = 1.0f) {
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = t * 32 + c_row(r, hhalf);
      *reinterpret_cast<short*>(row + d) = f32_to_bf16(acc[t][r] * mul);
    }
}

// 8 bf16 at p, p + stride, ... as one fragment
DEV_INLINE bf16x8 gather8(const __hip_bfloat16* p, int stride) {
  union { unsigned u[4]; bf16x8 v8; } f;
#pragma unroll
  for (int e = 0; e < 8; ++e) reinterpret_cast<__hip_bfloat16*>(&f)[e] = p[e * stride];
  return f.v8;
}

// LDS geometry of the K/V tile of fwd and dq: 2*KVB keys per barrier pair,
// row-major [ROWS][LDS_STRIDE] (k_lds, v_lds) and transposed [HD][T_STRIDE].
template <int HD, int KVB>
struct KvTile {
  static constexpr int ROWS = 2 * KVB;
  static constexpr int LDS_STRIDE = HD + 8;  // +16 B pad vs bank conflicts
  static constexpr int T_STRIDE = ROWS + 8;
  static constexpr int TILE = ROWS * LDS_STRIDE;  // elements of k_lds / v_lds
  static constexpr int T_TILE = HD * T_STRIDE;    // elements of t_lds
};

// Staging of that tile. K rows go (rope applied at the write) to k_lds.
// KT = false (fwd): V goes transposed to t_lds. KT = true (dq): rope'd K also
// goes transposed to t_lds and V goes row-major to v_lds.
// T14 async-STAGE split: each thread owns K_IPT K pair-chunks and V_IPT V
// chunks of the tile in registers; the next tile's global loads are issued
// BEFORE the compute phase so HBM latency hides under the MFMAs instead of
// draining at the pre-compute barrier.
template <class L, int HD, int NT, int KVB, bool KT>
struct KvStage : KvTile<HD, KVB> {
  using KvTile<HD, KVB>::ROWS;
  using KvTile<HD, KVB>::LDS_STRIDE;
  using KvTile<HD, KVB>::T_STRIDE;
  static constexpr int HALF = HD / 2;
  static constexpr int PAIRS_PER_ROW = HALF / 8;  // K pair-items per row
  static constexpr int PER_ROW = HD / 8;          // V items per row
  static constexpr int K_ITEMS = ROWS * PAIRS_PER_ROW;
  static constexpr int V_ITEMS = ROWS * PER_ROW;
  static constexpr int K_IPT = (K_ITEMS + NT - 1) / NT;
  static constexpr int V_IPT = (V_ITEMS + NT - 1) / NT;

  bf16x8 klo[K_IPT], khi[K_IPT], vreg[V_IPT];

  DEV_INLINE void issue_loads(const L& lay, const typename L::Qkv& in, int kbase0, int N) {
#pragma unroll
    for (int j = 0; j < K_IPT; ++j) {
      const int item = threadIdx.x + j * NT;
      const int krow = kbase0 + item / PAIRS_PER_ROW;
      const int c0 = (item % PAIRS_PER_ROW) * 8;
      const bool ok = item < K_ITEMS && krow < N;
      klo[j] = ok ? load8(lay.at(in, krow, 1, c0)) : bf16x8{};
      khi[j] = ok ? load8(lay.at(in, krow, 1, c0 + HALF)) : bf16x8{};
    }
#pragma unroll
    for (int j = 0; j < V_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      const int krow = kbase0 + idx / PER_ROW;
      vreg[j] = (idx < V_ITEMS && krow < N) ? load8(lay.at(in, krow, 2, (idx % PER_ROW) * 8))
                                            : bf16x8{};
    }
  }

  DEV_INLINE void write_tile(int kbase0, int N, const BlockCtx& c, const float* sin_t,
                             const float* cos_t, __hip_bfloat16* k_lds,
                             __hip_bfloat16* v_lds, __hip_bfloat16* t_lds) {
#pragma unroll
    for (int j = 0; j < K_IPT; ++j) {
      const int item = threadIdx.x + j * NT;
      if (item < K_ITEMS) {
        const int lrow = item / PAIRS_PER_ROW;
        const int c0 = (item % PAIRS_PER_ROW) * 8;
        const int krow = kbase0 + lrow;
        const int p = krow - c.prefix;
        if (c.use_rope && krow < N && p >= 0)
          rope_rotate8(klo[j], khi[j], sin_t + (long)p * HD, cos_t + (long)p * HD, c0);
        *reinterpret_cast<bf16x8*>(&k_lds[lrow * LDS_STRIDE + c0]) = klo[j];
        *reinterpret_cast<bf16x8*>(&k_lds[lrow * LDS_STRIDE + HALF + c0]) = khi[j];
        if constexpr (KT) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            t_lds[(c0 + e) * T_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&klo[j])[e];
            t_lds[(c0 + HALF + e) * T_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&khi[j])[e];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      if (idx < V_ITEMS) {
        const int row = idx / PER_ROW;
        const int c8 = (idx % PER_ROW) * 8;
        if constexpr (KT) {
          *reinterpret_cast<bf16x8*>(&v_lds[row * LDS_STRIDE + c8]) = vreg[j];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            t_lds[(c8 + e) * T_STRIDE + row] = reinterpret_cast<__hip_bfloat16*>(&vreg[j])[e];
        }
      }
    }
  }
};

constexpr int SUBK = 32;  // keys per MFMA tile (fixed by the 32x32 MFMA)

// ---------------------------------------------------------------------------
// MFMA layout probe: C[32,32] = A[32,16] @ B[16,32] with the layouts of mfma.h
// ---------------------------------------------------------------------------
__global__ void probe_mfma_kernel(const __hip_bfloat16* __restrict__ A,
                                  const __hip_bfloat16* __restrict__ B,
                                  float* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int i = lane & 31;
  f32x16 c = {};
  c = MFMA32(gather8(A + i * 16 + h * 8, 1), gather8(B + h * 8 * 32 + i, 32), c);
  for (int r = 0; r < 16; ++r) C[c_row(r, h) * 32 + i] = c[r];
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
// QLDS/PREFETCH: the hd-128 long-N configuration holds 304 registers/thread
// with in-register Q fragments + double-buffered K/V staging -> occupancy
// 1 wave/SIMD and fully exposed HBM latency (252 GB/s effective at N=2305).
// QLDS parks the rotated Q fragments in LDS in their REGISTER layout (lane-
// indexed, conflict-free b128), PREFETCH=false drops the register double
// buffer; together they fit 2 waves/SIMD.
template <int HD, int NT, bool QLDS, int KVB>
struct FwdSmem {  // k_lds | vt_lds | per-wave Q fragments (index = slice, lane)
  using Tile = KvTile<HD, KVB>;
  static constexpr int Q_WAVE = (HD / 16) * 64 * 8;
  static constexpr int VT_OFF = Tile::TILE;
  static constexpr int Q_OFF = VT_OFF + Tile::T_TILE;
  static constexpr size_t BYTES =
      (Q_OFF + (QLDS ? (NT / 64) * Q_WAVE : 0)) * sizeof(__hip_bfloat16);
};

template <class L, int HD, int NT = 256, bool QLDS = false, bool PREFETCH = true,
          int MINW = 1, int KVB = 32>
__global__ __launch_bounds__(NT, MINW) void fwd_kernel(
    typename L::Qkv in, const float* __restrict__ sin_t, const float* __restrict__ cos_t,
    __hip_bfloat16* __restrict__ o, float* __restrict__ lse, int B, int H, int N, int P,
    float scale) {
  using Smem = FwdSmem<HD, NT, QLDS, KVB>;
  constexpr int KSLICES = HD / 16;
  constexpr int DTILES = HD / 32;
  constexpr int LDS_STRIDE = Smem::Tile::LDS_STRIDE;
  constexpr int VT_STRIDE = Smem::Tile::T_STRIDE;

  const BlockCtx c = block_ctx(H, N, P, sin_t);
  const L lay(c.b, c.h, H, N, HD);
  const int hhalf = c.hhalf, l31 = c.l31;
  const int q0 = blockIdx.y * (NT / 2) + c.wave * 32;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __hip_bfloat16* k_lds = reinterpret_cast<__hip_bfloat16*>(smem_raw);
  __hip_bfloat16* vt_lds = k_lds + Smem::VT_OFF;
  __hip_bfloat16* q_lds = k_lds + Smem::Q_OFF + (QLDS ? c.wave * Smem::Q_WAVE : 0);

  // Q fragments (+ rope)
  const int qrow = q0 + l31;
  bf16x8 qf[QLDS ? 1 : KSLICES];
  {
    bf16x8 qtmp[KSLICES];
    const int safe = qrow < N ? qrow : (N - 1);
#pragma unroll
    for (int s = 0; s < KSLICES; ++s) qtmp[s] = load8(lay.at(in, safe, 0, s * 16 + hhalf * 8));
    rope_fragments(qtmp, sin_t, cos_t, safe, c);
    if constexpr (QLDS) {
#pragma unroll
      for (int s = 0; s < KSLICES; ++s)
        *reinterpret_cast<bf16x8*>(&q_lds[(s * 64 + c.lane) * 8]) = qtmp[s];
    } else {
#pragma unroll
      for (int s = 0; s < KSLICES; ++s) qf[s] = qtmp[s];
    }
  }

  float o_acc[DTILES][16];
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  KvStage<L, HD, NT, KVB, false> st;
  const int n_super = (N + 2 * KVB - 1) / (2 * KVB);
  if constexpr (PREFETCH) st.issue_loads(lay, in, 0, N);
  for (int kt = 0; kt < n_super; ++kt) {
    const int kbase0 = kt * 2 * KVB;
    __syncthreads();               // compute of tile kt-1 done reading LDS
    if constexpr (!PREFETCH) st.issue_loads(lay, in, kbase0, N);
    st.write_tile(kbase0, N, c, sin_t, cos_t, k_lds, nullptr, vt_lds);
    if constexpr (PREFETCH) {
      if (kt + 1 < n_super) st.issue_loads(lay, in, kbase0 + 2 * KVB, N);  // fly during compute
    }
    __syncthreads();

    for (int sub = 0; sub < (2 * KVB) / SUBK && kbase0 + sub * SUBK < N; ++sub) {
      const int kbase = kbase0 + sub * SUBK;
      const int krow_off = sub * SUBK;

      // S^T tile = K @ Q^T : C[k row, q col]
      f32x16 s_acc = {};
#pragma unroll
      for (int s = 0; s < KSLICES; ++s) {
        bf16x8 af = load8(&k_lds[(krow_off + l31) * LDS_STRIDE + s * 16 + hhalf * 8]);
        bf16x8 qs;
        if constexpr (QLDS) qs = load8(&q_lds[(s * 64 + c.lane) * 8]);
        else qs = qf[s];
        s_acc = MFMA32(af, qs, s_acc);
      }
      float sv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int krow = kbase + c_row(r, hhalf);
        sv[r] = (krow < N) ? s_acc[r] * scale : -INFINITY;
      }
      // online softmax: row (q) stats over this tile's 32 k
      float tmax = sv[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sv[r]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = __expf(sv[r] - m_new);
        psum += sv[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int t = 0; t < DTILES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[t][r] *= alpha;

      // PV: O^T[d, q] += V^T[d, k] @ P^T[k, q]
      bf16x8 p0 = pack_fragment(sv, 0);
      bf16x8 p1 = pack_fragment(sv, 8);
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        const __hip_bfloat16* vt = &vt_lds[(t * 32 + l31) * VT_STRIDE + krow_off + hhalf * 8];
        mfma2_acc(o_acc[t], load8(vt), p0, load8(vt + 16), p1);
      }
    }
  }

  // epilogue: O[q, d] = O^T / l ; lse = m + log(l)
  if (qrow < N) {
    store_rows_bf16(lay.o_row(o, qrow), o_acc, hhalf, 1.0f / l_run);
    if (hhalf == 0) lse[c.stat_off + qrow] = m_run + __logf(l_run);
  }
}

// ---------------------------------------------------------------------------
// Backward dQ: per q block, loop over kv tiles.
//   S^T = K @ Q^T (recompute) ; P^T = exp(S^T*scale - lse[q])
//   dP^T[k,q] = V @ dO^T       ; dS^T = P^T * (dP^T - D[q]) * scale
//   dQ^T[d,q] += K^T[d,k-slice] @ pack(dS^T)
// ---------------------------------------------------------------------------
template <int HD, int KVB>
struct DqSmem {  // k_lds (rope'd K) | v_lds | kt_lds (rope'd K^T)
  using Tile = KvTile<HD, KVB>;
  static constexpr int V_OFF = Tile::TILE;
  static constexpr int KT_OFF = 2 * Tile::TILE;
  static constexpr size_t BYTES = (KT_OFF + Tile::T_TILE) * sizeof(__hip_bfloat16);
};

template <class L, int HD, int NT = 256, int MINW = 1, int KVB = 32>
__global__ __launch_bounds__(NT, MINW) void bwd_dq_kernel(
    typename L::Qkv in, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ sin_t, const float* __restrict__ cos_t,
    const float* __restrict__ lse, const float* __restrict__ D, typename L::DQkv grad, int B,
    int H, int N, int P, float scale) {
  using Smem = DqSmem<HD, KVB>;
  constexpr int KSLICES = HD / 16;
  constexpr int DTILES = HD / 32;
  constexpr int LDS_STRIDE = Smem::Tile::LDS_STRIDE;
  constexpr int KT_STRIDE = Smem::Tile::T_STRIDE;

  const BlockCtx c = block_ctx(H, N, P, sin_t);
  const L lay(c.b, c.h, H, N, HD);
  const int hhalf = c.hhalf, l31 = c.l31;
  const int q0 = blockIdx.y * (NT / 2) + c.wave * 32;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __hip_bfloat16* k_lds = reinterpret_cast<__hip_bfloat16*>(smem_raw);
  __hip_bfloat16* v_lds = k_lds + Smem::V_OFF;
  __hip_bfloat16* kt_lds = k_lds + Smem::KT_OFF;

  const int qrow = q0 + l31;
  const int safe = qrow < N ? qrow : (N - 1);
  bf16x8 qf[KSLICES], dof[KSLICES];
#pragma unroll
  for (int s = 0; s < KSLICES; ++s) {
    qf[s] = load8(lay.at(in, safe, 0, s * 16 + hhalf * 8));
    dof[s] = load8(lay.o_row(dout, safe) + s * 16 + hhalf * 8);
  }
  rope_fragments(qf, sin_t, cos_t, safe, c);
  const float my_lse = lse[c.stat_off + safe];
  const float my_D = D[c.stat_off + safe];

  float dq_acc[DTILES][16];
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[t][r] = 0.f;

  KvStage<L, HD, NT, KVB, true> st;
  const int n_super = (N + 2 * KVB - 1) / (2 * KVB);
  st.issue_loads(lay, in, 0, N);
  for (int kt = 0; kt < n_super; ++kt) {
    const int kbase0 = kt * 2 * KVB;
    __syncthreads();
    st.write_tile(kbase0, N, c, sin_t, cos_t, k_lds, v_lds, kt_lds);
    if (kt + 1 < n_super) st.issue_loads(lay, in, kbase0 + 2 * KVB, N);
    __syncthreads();

    for (int sub = 0; sub < (2 * KVB) / SUBK && kbase0 + sub * SUBK < N; ++sub) {
      const int kbase = kbase0 + sub * SUBK;
      const int krow_off = sub * SUBK;
      f32x16 s_acc = {}, dp_acc = {};
#pragma unroll
      for (int s = 0; s < KSLICES; ++s) {
        bf16x8 kf = load8(&k_lds[(krow_off + l31) * LDS_STRIDE + s * 16 + hhalf * 8]);
        bf16x8 vf = load8(&v_lds[(krow_off + l31) * LDS_STRIDE + s * 16 + hhalf * 8]);
        s_acc = MFMA32(kf, qf[s], s_acc);
        dp_acc = MFMA32(vf, dof[s], dp_acc);
      }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int krow = kbase + c_row(r, hhalf);
        float p = (krow < N && qrow < N) ? __expf(s_acc[r] * scale - my_lse) : 0.f;
        ds[r] = p * (dp_acc[r] - my_D) * scale;
      }
      bf16x8 f0 = pack_fragment(ds, 0);
      bf16x8 f1 = pack_fragment(ds, 8);
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        const __hip_bfloat16* kt_p = &kt_lds[(t * 32 + l31) * KT_STRIDE + krow_off + hhalf * 8];
        mfma2_acc(dq_acc[t], load8(kt_p), f0, load8(kt_p + 16), f1);
      }
    }
  }

  if (qrow < N) {
    rope_inverse(dq_acc, sin_t, cos_t, qrow, c);
    store_rows_bf16(lay.grad_row(grad, 0, qrow), dq_acc, hhalf);
  }
}

// ---------------------------------------------------------------------------
// Backward dK/dV: per kv block of 32 rows per wave, loop over 32-row q tiles,
// SQB (32 or 64) q rows staged per barrier pair.
//   S[q,k] = Q @ K^T (C: rows=q, cols=k; K wave-resident as B)
//   P = exp(S*scale - lse[q]); dP[q,k] = dO @ V^T ; dS = P*(dP - D[q])*scale
// pack_fragment of a C tile (rows=q, cols=k) is the B layout of P / dS, so
//   dV^T[d, k] += dO^T[d, q] @ P[q, k] ; dK^T[d, k] += Q^T[d, q] @ dS[q, k]
// with dO^T / Q^T as A from the transposed LDS tiles.
// ---------------------------------------------------------------------------
template <int HD, int SQB>
struct DkvSmem {  // qt_lds (rope'd Q^T) | dot_lds (dO^T) | lse [SQB] | D [SQB]
  static constexpr int QB = 32;              // q rows per MFMA tile
  static constexpr int QT_STRIDE = SQB + 8;  // column stride, sized for the SQB staged rows
  static constexpr int DOT_OFF = HD * QT_STRIDE;
  static constexpr int STAT_OFF = 2 * HD * QT_STRIDE;  // in bf16 elements
  static constexpr size_t BYTES = STAT_OFF * sizeof(__hip_bfloat16) + 2 * SQB * sizeof(float);
};

template <class L, int HD, int NT = 256, int MINW = 1, int SQB = 32>
__global__ __launch_bounds__(NT, MINW) void bwd_dkv_kernel(
    typename L::Qkv in, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ sin_t, const float* __restrict__ cos_t,
    const float* __restrict__ lse, const float* __restrict__ D, typename L::DQkv grad, int B,
    int H, int N, int P, float scale) {
  using Smem = DkvSmem<HD, SQB>;
  constexpr int KSLICES = HD / 16;
  constexpr int DTILES = HD / 32;
  constexpr int QB = Smem::QB;
  constexpr int QT_STRIDE = Smem::QT_STRIDE;
  constexpr int HALF = HD / 2;

  const BlockCtx c = block_ctx(H, N, P, sin_t);
  const L lay(c.b, c.h, H, N, HD);
  const int hhalf = c.hhalf, l31 = c.l31;
  const int k0 = blockIdx.y * 128 + c.wave * 32;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __hip_bfloat16* qt_lds = reinterpret_cast<__hip_bfloat16*>(smem_raw);
  __hip_bfloat16* dot_lds = qt_lds + Smem::DOT_OFF;
  float* lse_lds = reinterpret_cast<float*>(qt_lds + Smem::STAT_OFF);
  float* d_lds = lse_lds + SQB;

  const int krow = k0 + l31;
  const int safe = krow < N ? krow : (N - 1);
  bf16x8 kf[KSLICES], vf[KSLICES];
#pragma unroll
  for (int s = 0; s < KSLICES; ++s) {
    kf[s] = load8(lay.at(in, safe, 1, s * 16 + hhalf * 8));
    vf[s] = load8(lay.at(in, safe, 2, s * 16 + hhalf * 8));
  }
  rope_fragments(kf, sin_t, cos_t, safe, c);

  float dk_acc[DTILES][16], dv_acc[DTILES][16];
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk_acc[t][r] = 0.f;
      dv_acc[t][r] = 0.f;
    }

  constexpr int PAIRS_PER_ROW = HALF / 8;
  constexpr int PER_ROW = HD / 8;
  constexpr int QK_ITEMS = SQB * PAIRS_PER_ROW;
  constexpr int DO_ITEMS = SQB * PER_ROW;
  // QK_ITEMS can exceed NT (HD=128, NT=128 -> 256 items): loop like the
  // dO staging. (Single-shot staging here silently dropped half the Q tile
  // for hd-128 small-N — caught by tests/test_kernel_layouts.py.)
  constexpr int QK_IPT = (QK_ITEMS + NT - 1) / NT;
  constexpr int DO_IPT = (DO_ITEMS + NT - 1) / NT;
  bf16x8 qlo[QK_IPT], qhi[QK_IPT], doreg[DO_IPT];
  float lse_reg = INFINITY, d_reg = 0.f;
  auto issue_loads = [&](int qbase0) {
#pragma unroll
    for (int j = 0; j < QK_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      const int qrow = qbase0 + idx / PAIRS_PER_ROW;
      const int c0 = (idx % PAIRS_PER_ROW) * 8;
      const bool ok = idx < QK_ITEMS && qrow < N;
      qlo[j] = ok ? load8(lay.at(in, qrow, 0, c0)) : bf16x8{};
      qhi[j] = ok ? load8(lay.at(in, qrow, 0, c0 + HALF)) : bf16x8{};
    }
#pragma unroll
    for (int j = 0; j < DO_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      const int qrow = qbase0 + idx / PER_ROW;
      doreg[j] = (idx < DO_ITEMS && qrow < N) ? load8(lay.o_row(dout, qrow) + (idx % PER_ROW) * 8)
                                              : bf16x8{};
    }
    if (threadIdx.x < SQB) {
      const int qrow = qbase0 + threadIdx.x;
      lse_reg = (qrow < N) ? lse[c.stat_off + qrow] : INFINITY;
      d_reg = (qrow < N) ? D[c.stat_off + qrow] : 0.f;
    }
  };
  auto write_tile = [&](int qbase0) {
#pragma unroll
    for (int j = 0; j < QK_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      if (idx < QK_ITEMS) {
        const int lrow = idx / PAIRS_PER_ROW;
        const int c0 = (idx % PAIRS_PER_ROW) * 8;
        const int qrow = qbase0 + lrow;
        const int p = qrow - c.prefix;
        if (c.use_rope && qrow < N && p >= 0)
          rope_rotate8(qlo[j], qhi[j], sin_t + (long)p * HD, cos_t + (long)p * HD, c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          qt_lds[(c0 + e) * QT_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&qlo[j])[e];
          qt_lds[(c0 + HALF + e) * QT_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&qhi[j])[e];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DO_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      if (idx < DO_ITEMS) {
        const int lrow = idx / PER_ROW;
        const int c8 = (idx % PER_ROW) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          dot_lds[(c8 + e) * QT_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&doreg[j])[e];
      }
    }
    if (threadIdx.x < SQB) {
      lse_lds[threadIdx.x] = lse_reg;
      d_lds[threadIdx.x] = d_reg;
    }
  };

  const int n_q = (N + SQB - 1) / SQB;
  issue_loads(0);
  for (int qt = 0; qt < n_q; ++qt) {
    const int qbase0 = qt * SQB;
    __syncthreads();
    write_tile(qbase0);
    if (qt + 1 < n_q) issue_loads(qbase0 + SQB);
    __syncthreads();

    for (int sub = 0; sub < SQB / QB && (sub == 0 || qbase0 + sub * QB < N); ++sub) {
      const int qbase = qbase0 + sub * QB;
      const int qrow_off = sub * QB;
      // A fragments Q[q = l31][d] and dO[q = l31][d]: strided reads of Q^T / dO^T
      f32x16 s_acc = {}, dp_acc = {};
#pragma unroll
      for (int s = 0; s < KSLICES; ++s) {
        const int d0 = (s * 16 + hhalf * 8) * QT_STRIDE + qrow_off + l31;
        s_acc = MFMA32(gather8(qt_lds + d0, QT_STRIDE), kf[s], s_acc);
        dp_acc = MFMA32(gather8(dot_lds + d0, QT_STRIDE), vf[s], dp_acc);
      }
      float pv[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = qbase + c_row(r, hhalf);
        const bool valid = (qrow < N) && (krow < N);
        const float l = lse_lds[qrow_off + c_row(r, hhalf)];
        float p = valid ? __expf(s_acc[r] * scale - l) : 0.f;
        pv[r] = p;
        ds[r] = p * (dp_acc[r] - d_lds[qrow_off + c_row(r, hhalf)]) * scale;
      }
      bf16x8 p0 = pack_fragment(pv, 0);
      bf16x8 p1 = pack_fragment(pv, 8);
      bf16x8 s0 = pack_fragment(ds, 0);
      bf16x8 s1 = pack_fragment(ds, 8);
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        // A[i = d = t*32 + l31][q = hhalf*8 + e] and the same 16 rows further
        const int a0 = (t * 32 + l31) * QT_STRIDE + qrow_off + hhalf * 8;
        mfma2_acc(dv_acc[t], gather8(dot_lds + a0, 1), p0, gather8(dot_lds + a0 + 16, 1), p1);
        mfma2_acc(dk_acc[t], gather8(qt_lds + a0, 1), s0, gather8(qt_lds + a0 + 16, 1), s1);
      }
    }
  }

  if (krow < N) {
    rope_inverse(dk_acc, sin_t, cos_t, krow, c);
    store_rows_bf16(lay.grad_row(grad, 1, krow), dk_acc, hhalf);
    store_rows_bf16(lay.grad_row(grad, 2, krow), dv_acc, hhalf);
  }
}

// ---------------------------------------------------------------------------
// Backward in one pass, for sequences one workgroup holds (N <= 32 * NT/64):
// one workgroup per (b, h), wave w owns keys 32w .. 32w+31 as in dkv (rope'd K
// and V fragments, dK^T / dV^T accumulators in registers) and the workgroup
// walks the 32-row q slices. Per slice:
//   stage   rope'd Q and dO, each row-major and transposed, lse, and
//           D[q] = sum_d dO*O reduced over the 8 lanes that load the row
//   wave    S = Q @ K^T, dP = dO @ V^T, P, dS once; dV^T += dO^T @ P and
//           dK^T += Q^T @ dS as in dkv. dS (bf16, the bits dK consumes) is
//           transposed through the wave's own LDS slot, then the fp32 partial
//           dQ^T[d, q] = K^T[d, own keys] @ dS^T replaces it there
//   all     add the slots of the waves that hold keys in wave order, inverse
//           rope, store the slice's dQ rows
// Waves whose keys lie wholly past N only stage and reduce. No atomics: the
// result is a function of the inputs alone.
// ---------------------------------------------------------------------------
template <int HD, int NT>
struct FusedBwdSmem {  // q | dO | Q^T | dO^T || lse, D | per-wave dQ slots
  static constexpr int QB = 32;               // q rows per slice
  static constexpr int NW = NT / 64;          // waves = 32-key tiles
  static constexpr int MAX_N = NW * 32;
  static constexpr int ROW_STRIDE = HD + 8;   // row-major q / dO (bf16 elements)
  static constexpr int T_STRIDE = QB + 8;     // Q^T / dO^T / dS^T rows
  static constexpr int SLOT_STRIDE = HD + 4;  // fp32 elements per q row of a slot
  static constexpr int DO_OFF = QB * ROW_STRIDE;
  static constexpr int QT_OFF = 2 * QB * ROW_STRIDE;
  static constexpr int DOT_OFF = QT_OFF + HD * T_STRIDE;
  static constexpr int STAT_OFF = DOT_OFF + HD * T_STRIDE;  // end of the bf16 part
  static constexpr int SLOT_FLOATS = QB * SLOT_STRIDE;
  static constexpr size_t SLOT_BYTE_OFF = STAT_OFF * sizeof(__hip_bfloat16) + 2 * QB * sizeof(float);
  static constexpr size_t BYTES = SLOT_BYTE_OFF + (size_t)NW * SLOT_FLOATS * sizeof(float);
  static_assert(SLOT_BYTE_OFF % 16 == 0 && (ROW_STRIDE * 2) % 16 == 0 && (T_STRIDE * 2) % 16 == 0 &&
                    (SLOT_STRIDE * 4) % 16 == 0,
                "16-byte LDS accesses need 16-byte aligned rows");
  // a slot also serves its own wave as bf16 transposition scratch: [32 keys][ROW_STRIDE]
  // for K before the loop, [QB][T_STRIDE] for dS^T before the slice's partial is written
  static_assert(32 * ROW_STRIDE * sizeof(__hip_bfloat16) <= SLOT_FLOATS * sizeof(float) &&
                QB * T_STRIDE * sizeof(__hip_bfloat16) <= SLOT_FLOATS * sizeof(float));
  static_assert(BYTES <= 160 * 1024, "one workgroup's LDS on gfx950");
};

// MINW = 2: 512 threads are two waves per SIMD already; the 128-thread form
// would otherwise take 350 registers and halve the workgroups per CU
template <class L, int HD, int NT>
__global__ __launch_bounds__(NT, 2) void bwd_fused_kernel(
    typename L::Qkv in, const __hip_bfloat16* __restrict__ dout,
    const __hip_bfloat16* __restrict__ o, const float* __restrict__ sin_t,
    const float* __restrict__ cos_t, const float* __restrict__ lse, typename L::DQkv grad,
    int B, int H, int N, int P, float scale) {
  using Smem = FusedBwdSmem<HD, NT>;
  static_assert(HD == 64, "the reduction's thread map is written for hd 64");
  constexpr int KSLICES = HD / 16;
  constexpr int DTILES = HD / 32;
  constexpr int QB = Smem::QB;
  constexpr int ROW_STRIDE = Smem::ROW_STRIDE;
  constexpr int T_STRIDE = Smem::T_STRIDE;
  constexpr int SLOT_STRIDE = Smem::SLOT_STRIDE;
  constexpr int HALF = HD / 2;

  const BlockCtx c = block_ctx(H, N, P, sin_t);
  const L lay(c.b, c.h, H, N, HD);
  const int hhalf = c.hhalf, l31 = c.l31;
  const int k0 = c.wave * 32;
  const bool wave_active = k0 < N;
  const int n_active = (N + 31) / 32;  // waves that hold keys

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __hip_bfloat16* q_lds = reinterpret_cast<__hip_bfloat16*>(smem_raw);
  __hip_bfloat16* do_lds = q_lds + Smem::DO_OFF;
  __hip_bfloat16* qt_lds = q_lds + Smem::QT_OFF;
  __hip_bfloat16* dot_lds = q_lds + Smem::DOT_OFF;
  float* lse_lds = reinterpret_cast<float*>(q_lds + Smem::STAT_OFF);
  float* d_lds = lse_lds + QB;
  float* slots = reinterpret_cast<float*>(smem_raw + Smem::SLOT_BYTE_OFF);
  float* my_slot = slots + c.wave * Smem::SLOT_FLOATS;
  __hip_bfloat16* ds_lds = reinterpret_cast<__hip_bfloat16*>(my_slot);

  // wave-resident K (rope'd) and V: B fragments [d, key = l31]
  const int krow = k0 + l31;
  const int safe = krow < N ? krow : (N - 1);
  bf16x8 kf[KSLICES], vf[KSLICES];
#pragma unroll
  for (int s = 0; s < KSLICES; ++s) {
    kf[s] = load8(lay.at(in, safe, 1, s * 16 + hhalf * 8));
    vf[s] = load8(lay.at(in, safe, 2, s * 16 + hhalf * 8));
  }
  rope_fragments(kf, sin_t, cos_t, safe, c);
  // the same K as A fragments K^T[d = t*32 + l31][key = u*16 + hhalf*8 + e] of
  // the dQ product: transposed once through the wave's own slot
  bf16x8 ktf[DTILES][2];
  {
    __hip_bfloat16* scr = reinterpret_cast<__hip_bfloat16*>(my_slot);
#pragma unroll
    for (int s = 0; s < KSLICES; ++s)
      *reinterpret_cast<bf16x8*>(&scr[l31 * ROW_STRIDE + s * 16 + hhalf * 8]) = kf[s];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int t = 0; t < DTILES; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
        ktf[t][u] = gather8(scr + (u * 16 + hhalf * 8) * ROW_STRIDE + t * 32 + l31, ROW_STRIDE);
  }

  float dk_acc[DTILES][16], dv_acc[DTILES][16];
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk_acc[t][r] = 0.f;
      dv_acc[t][r] = 0.f;
    }

  // staging of one 32-row slice: Q as (lo, hi) pair chunks for the rope, dO
  // and O as 8-element chunks, 8 consecutive lanes per row
  constexpr int PAIRS_PER_ROW = HALF / 8;
  constexpr int PER_ROW = HD / 8;
  constexpr int QK_ITEMS = QB * PAIRS_PER_ROW;
  constexpr int DO_ITEMS = QB * PER_ROW;
  constexpr int QK_IPT = (QK_ITEMS + NT - 1) / NT;
  constexpr int DO_IPT = (DO_ITEMS + NT - 1) / NT;
  // dO / O chunks start at thread DO_T0: behind the Q chunks where the block has
  // threads for both, so that no wave stages both
  constexpr int DO_T0 = (NT >= QK_ITEMS + DO_ITEMS) ? NT - DO_ITEMS : 0;
  static_assert(PER_ROW == 8 && NT % 8 == 0 && DO_T0 % 8 == 0,
                "D is reduced over 8 consecutive lanes");
  bf16x8 qlo[QK_IPT], qhi[QK_IPT], doreg[DO_IPT], oreg[DO_IPT];
  float lse_reg = INFINITY;
  auto issue_loads = [&](int qbase0) {
#pragma unroll
    for (int j = 0; j < QK_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      const int qrow = qbase0 + idx / PAIRS_PER_ROW;
      const int c0 = (idx % PAIRS_PER_ROW) * 8;
      const bool ok = idx < QK_ITEMS && qrow < N;
      qlo[j] = ok ? load8(lay.at(in, qrow, 0, c0)) : bf16x8{};
      qhi[j] = ok ? load8(lay.at(in, qrow, 0, c0 + HALF)) : bf16x8{};
    }
#pragma unroll
    for (int j = 0; j < DO_IPT; ++j) {
      const int idx = (int)threadIdx.x - DO_T0 + j * NT;
      const int qrow = qbase0 + idx / PER_ROW;
      const bool ok = idx >= 0 && idx < DO_ITEMS && qrow < N;
      doreg[j] = ok ? load8(lay.o_row(dout, qrow) + (idx % PER_ROW) * 8) : bf16x8{};
      oreg[j] = ok ? load8(lay.o_row(o, qrow) + (idx % PER_ROW) * 8) : bf16x8{};
    }
    if (threadIdx.x < QB) {
      const int qrow = qbase0 + threadIdx.x;
      lse_reg = (qrow < N) ? lse[c.stat_off + qrow] : INFINITY;
    }
  };
  auto write_tile = [&](int qbase0) {
#pragma unroll
    for (int j = 0; j < QK_IPT; ++j) {
      const int idx = threadIdx.x + j * NT;
      if (idx < QK_ITEMS) {
        const int lrow = idx / PAIRS_PER_ROW;
        const int c0 = (idx % PAIRS_PER_ROW) * 8;
        const int qrow = qbase0 + lrow;
        const int p = qrow - c.prefix;
        if (c.use_rope && qrow < N && p >= 0)
          rope_rotate8(qlo[j], qhi[j], sin_t + (long)p * HD, cos_t + (long)p * HD, c0);
        *reinterpret_cast<bf16x8*>(&q_lds[lrow * ROW_STRIDE + c0]) = qlo[j];
        *reinterpret_cast<bf16x8*>(&q_lds[lrow * ROW_STRIDE + HALF + c0]) = qhi[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          qt_lds[(c0 + e) * T_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&qlo[j])[e];
          qt_lds[(c0 + HALF + e) * T_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&qhi[j])[e];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DO_IPT; ++j) {
      const int idx = (int)threadIdx.x - DO_T0 + j * NT;
      const int lrow = idx / PER_ROW;
      const int c8 = (idx % PER_ROW) * 8;
      // every lane takes part in the shuffles; chunks outside the slice hold zeros
      float dsum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dsum += b2f(doreg[j][e]) * b2f(oreg[j][e]);
      dsum += __shfl_xor(dsum, 1, 64);
      dsum += __shfl_xor(dsum, 2, 64);
      dsum += __shfl_xor(dsum, 4, 64);
      if (idx >= 0 && idx < DO_ITEMS) {
        *reinterpret_cast<bf16x8*>(&do_lds[lrow * ROW_STRIDE + c8]) = doreg[j];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          dot_lds[(c8 + e) * T_STRIDE + lrow] = reinterpret_cast<__hip_bfloat16*>(&doreg[j])[e];
        if (c8 == 0) d_lds[lrow] = dsum;
      }
    }
    if (threadIdx.x < QB) lse_lds[threadIdx.x] = lse_reg;
  };

  // reduction map: TPR threads per q row, EPT columns of each half per thread
  constexpr int TPR = NT / QB;
  constexpr int EPT = HALF / TPR;
  static_assert(TPR * EPT == HALF && EPT % 2 == 0);
  const int red_q = threadIdx.x / TPR;
  const int red_d = (threadIdx.x % TPR) * EPT;

  const int n_q = (N + QB - 1) / QB;
  issue_loads(0);
  for (int qt = 0; qt < n_q; ++qt) {
    const int qbase = qt * QB;
    // the images' readers (compute of slice qt-1) finished before that
    // slice's second barrier; the slots' readers finish before the next one
    write_tile(qbase);
    if (qt + 1 < n_q) issue_loads(qbase + QB);
    __syncthreads();

    if (wave_active) {
      f32x16 s_acc = {}, dp_acc = {};
#pragma unroll
      for (int s = 0; s < KSLICES; ++s) {
        const int a = l31 * ROW_STRIDE + s * 16 + hhalf * 8;
        s_acc = MFMA32(load8(q_lds + a), kf[s], s_acc);
        dp_acc = MFMA32(load8(do_lds + a), vf[s], dp_acc);
      }
      float pv[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lq = c_row(r, hhalf);
        const bool valid = (qbase + lq < N) && (krow < N);
        float p = valid ? __expf(s_acc[r] * scale - lse_lds[lq]) : 0.f;
        pv[r] = p;
        ds[r] = p * (dp_acc[r] - d_lds[lq]) * scale;
      }
      const bf16x8 p0 = pack_fragment(pv, 0);
      const bf16x8 p1 = pack_fragment(pv, 8);
      const bf16x8 s0 = pack_fragment(ds, 0);
      const bf16x8 s1 = pack_fragment(ds, 8);
      // dS[q = hhalf*8 + e (+16)][key = l31] -> ds_lds[q][key]
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ds_lds[(hhalf * 8 + e) * T_STRIDE + l31] = reinterpret_cast<const __hip_bfloat16*>(&s0)[e];
        ds_lds[(16 + hhalf * 8 + e) * T_STRIDE + l31] = reinterpret_cast<const __hip_bfloat16*>(&s1)[e];
      }
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        // A[i = d = t*32 + l31][q = hhalf*8 + e] and the same 16 rows further
        const int a0 = (t * 32 + l31) * T_STRIDE + hhalf * 8;
        mfma2_acc(dv_acc[t], load8(dot_lds + a0), p0, load8(dot_lds + a0 + 16), p1);
        mfma2_acc(dk_acc[t], load8(qt_lds + a0), s0, load8(qt_lds + a0 + 16), s1);
      }
      // partial dQ^T[d, q = l31] over this wave's keys: B[key = hhalf*8 + e (+16)][q]
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const bf16x8 f0 = load8(ds_lds + l31 * T_STRIDE + hhalf * 8);
      const bf16x8 f1 = load8(ds_lds + l31 * T_STRIDE + 16 + hhalf * 8);
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        f32x16 acc = {};
        acc = MFMA32(ktf[t][0], f0, acc);
        acc = MFMA32(ktf[t][1], f1, acc);
        // regs 4g .. 4g+3 are d = t*32 + 8g + 4*hhalf + 0..3
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4_t v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
          *reinterpret_cast<float4_t*>(&my_slot[l31 * SLOT_STRIDE + t * 32 + 8 * g + 4 * hhalf]) = v;
        }
      }
    }
    __syncthreads();

    // dQ[q, d] = slots added in wave order; columns (d, d + HALF) pair up in the rope
    const int qrow = qbase + red_q;
    if (qrow < N) {
      float glo[EPT], ghi[EPT];
#pragma unroll
      for (int e = 0; e < EPT; ++e) glo[e] = ghi[e] = 0.f;
      for (int w = 0; w < n_active; ++w) {
        const float* sl = slots + w * Smem::SLOT_FLOATS + red_q * SLOT_STRIDE + red_d;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          glo[e] += sl[e];
          ghi[e] += sl[HALF + e];
        }
      }
      const int p = qrow - c.prefix;
      if (c.use_rope && p >= 0) {
        const float* srow = sin_t + (long)p * HD + red_d;
        const float* crow = cos_t + (long)p * HD + red_d;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const float co = crow[e], s = srow[e];
          const float lo = glo[e], hi = ghi[e];
          glo[e] = lo * co + hi * s;
          ghi[e] = hi * co - lo * s;
        }
      }
      __hip_bfloat16* row = lay.grad_row(grad, 0, qrow) + red_d;
#pragma unroll
      for (int e = 0; e < EPT; e += 2) {
        *reinterpret_cast<unsigned*>(row + e) = pack2_bf16(glo[e], glo[e + 1]);
        *reinterpret_cast<unsigned*>(row + HALF + e) = pack2_bf16(ghi[e], ghi[e + 1]);
      }
    }
  }

  // dK and dV rows: an accumulator holds one key per lane and d down the
  // registers, which stored directly is 2 bytes per lane and row. They go
  // through the wave's slot as [key][d] fp32 instead (the dQ partial's layout)
  // and leave as 16-byte pieces, 8 lanes per 128-byte row.
  __syncthreads();  // the last slice's reduction has read the slots
  if (wave_active) {
    if (krow < N) rope_inverse(dk_acc, sin_t, cos_t, krow, c);
    auto store_via_slot = [&](const float (&acc)[DTILES][16], int which) {
#pragma unroll
      for (int t = 0; t < DTILES; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4_t v = {acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
          *reinterpret_cast<float4_t*>(&my_slot[l31 * SLOT_STRIDE + t * 32 + 8 * g + 4 * hhalf]) = v;
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int i = 0; i < 32 / 8; ++i) {
        const int lk = i * 8 + c.lane / 8;
        const int d0 = (c.lane & 7) * 8;
        float v[8];
        *reinterpret_cast<float4_t*>(v) = *reinterpret_cast<const float4_t*>(&my_slot[lk * SLOT_STRIDE + d0]);
        *reinterpret_cast<float4_t*>(v + 4) =
            *reinterpret_cast<const float4_t*>(&my_slot[lk * SLOT_STRIDE + d0 + 4]);
        if (k0 + lk < N) Pack8<__hip_bfloat16>::store(lay.grad_row(grad, which, k0 + lk) + d0, v);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    store_via_slot(dk_acc, 1);
    store_via_slot(dv_acc, 2);
  }
}

// ---------------------------------------------------------------------------
// Backward preprocess: D[b,h,n] = sum_d dO*O (fp32), rows ordered (b, h, n).
// One wave per 8 rows: 8 lanes per row, 8 bf16 per lane per pass. (The name
// dates from the token-major-only version; kept so traces stay comparable.)
// ---------------------------------------------------------------------------
constexpr int PRE_THREADS = 256;
constexpr int PRE_ROWS = PRE_THREADS / 64 * 8;  // rows per block and pass

template <class L>
__global__ void bwd_pre_tm_kernel(const __hip_bfloat16* __restrict__ dout,
                                  const __hip_bfloat16* __restrict__ o,
                                  float* __restrict__ D, int B, int H, int N, int HD) {
  const long rows = (long)B * H * N;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x / 64;
  const int sub = lane / 8;
  const int lane8 = lane & 7;
  const long group0 = ((long)blockIdx.x * (blockDim.x / 64) + wid) * 8;
  for (long g = group0; g < rows; g += (long)gridDim.x * (blockDim.x / 64) * 8) {
    const long row = g + sub;
    float acc = 0.f;
    if (row < rows) {
      const int n = (int)(row % N);
      const int h = (int)((row / N) % H);
      const int b = (int)(row / ((long)N * H));
      const L lay(b, h, H, N, HD);
      const __hip_bfloat16* dop = lay.o_row(dout, n);
      const __hip_bfloat16* op = lay.o_row(o, n);
      for (int i0 = lane8 * 8; i0 < HD; i0 += 64) {
        __hip_bfloat16 a[8], c[8];
        Vec8<__hip_bfloat16>::load(a, dop + i0);
        Vec8<__hip_bfloat16>::load(c, op + i0);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          acc += bf16_to_f32(*(short*)(a + e)) * bf16_to_f32(*(short*)(c + e));
      }
    }
    // reduce across the 8 lanes of this row
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane8 == 0 && row < rows) D[row] = acc;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

constexpr size_t LDS_DEFAULT_MAX = 64 * 1024;  // dynamic LDS a launch gets without opting in

// SMEM comes from the kernel's own *Smem traits. OPT_IN raises the kernel's
// dynamic-LDS limit first (once per kernel).
template <auto KERNEL, size_t SMEM, bool OPT_IN, class... A>
static void launch(dim3 grid, int nt, hipStream_t stream, A... args) {
  static_assert(SMEM <= LDS_DEFAULT_MAX || OPT_IN,
                "more than 64 KiB of dynamic LDS needs the opt-in launch path");
  if constexpr (OPT_IN) {
    static const bool attr_ok =
        hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM) == hipSuccess;
    (void)attr_ok;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(nt), SMEM, stream, args...);
}

template <class L, int HD, int NT, bool QLDS, bool PREFETCH, int MINW, int KVB, class... A>
static void run_fwd(dim3 grid, hipStream_t stream, A... args) {
  launch<fwd_kernel<L, HD, NT, QLDS, PREFETCH, MINW, KVB>, FwdSmem<HD, NT, QLDS, KVB>::BYTES,
         QLDS>(grid, NT, stream, args...);
}
template <class L, int HD, int NT, int MINW, int KVB, class... A>
static void run_dq(dim3 grid, hipStream_t stream, A... args) {
  launch<bwd_dq_kernel<L, HD, NT, MINW, KVB>, DqSmem<HD, KVB>::BYTES, false>(grid, NT, stream,
                                                                             args...);
}
template <class L, int HD, int NT, int SQB, class... A>
static void run_dkv(dim3 grid, hipStream_t stream, A... args) {
  launch<bwd_dkv_kernel<L, HD, NT, 1, SQB>, DkvSmem<HD, SQB>::BYTES, false>(grid, NT, stream,
                                                                            args...);
}

// short sequences (local crops, N <= 64): 128-thread blocks, 64 q rows each
static bool small_n(int N) { return N <= 64; }
static dim3 attn_grid(int B, int H, int N) {
  return dim3(B * H, small_n(N) ? 1 : (N + 127) / 128);
}

template <class L>
void launch_fwd(typename L::Qkv in, const float* sin_t, const float* cos_t,
                __hip_bfloat16* o, float* lse, int B, int H, int N, int P, int HD,
                float scale, hipStream_t stream) {
  const dim3 grid = attn_grid(B, H, N);
  if (HD == 64) {
    if (small_n(N))
      run_fwd<L, 64, 128, false, true, 1, 32>(grid, stream, in, sin_t, cos_t, o, lse, B,
                                              H, N, P, scale);
    else  // KVB=64: 128 keys per barrier pair
      run_fwd<L, 64, 256, false, true, 1, 64>(grid, stream, in, sin_t, cos_t, o, lse, B,
                                              H, N, P, scale);
  } else if (HD == 128) {
    if (small_n(N))
      run_fwd<L, 128, 128, false, true, 1, 32>(grid, stream, in, sin_t, cos_t, o, lse, B,
                                               H, N, P, scale);
    else  // QLDS + no-prefetch: 2 waves/SIMD (the register variant runs at 1)
      run_fwd<L, 128, 256, true, false, 2, 32>(grid, stream, in, sin_t, cos_t, o, lse, B,
                                               H, N, P, scale);
  }
}

template <class L>
void launch_bwd_pre(const __hip_bfloat16* dout, const __hip_bfloat16* o, float* D, int B,
                    int H, int N, int HD, hipStream_t stream) {
  const long rows = (long)B * H * N;
  const int grid = (int)min((rows + PRE_ROWS - 1) / PRE_ROWS, (long)4096);
  hipLaunchKernelGGL(bwd_pre_tm_kernel<L>, dim3(grid), dim3(PRE_THREADS), 0, stream, dout, o,
                     D, B, H, N, HD);
}

template <class L>
void launch_bwd_dq(typename L::Qkv in, const __hip_bfloat16* dout, const float* sin_t,
                   const float* cos_t, const float* lse, const float* D,
                   typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                   hipStream_t stream) {
  const dim3 grid = attn_grid(B, H, N);
  if (HD == 64) {
    if (small_n(N))
      run_dq<L, 64, 128, 1, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H,
                                N, P, scale);
    else  // KVB=64: 128 keys per barrier pair
      run_dq<L, 64, 256, 2, 64>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H,
                                N, P, scale);
  } else if (HD == 128) {
    if (small_n(N))
      run_dq<L, 128, 128, 1, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B,
                                 H, N, P, scale);
    else  // MINW=2 packs to 256 regs (20 B/lane cold scratch) for 2 waves/SIMD
      run_dq<L, 128, 256, 2, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B,
                                 H, N, P, scale);
  }
}

template <class L>
void launch_bwd_dkv(typename L::Qkv in, const __hip_bfloat16* dout, const float* sin_t,
                    const float* cos_t, const float* lse, const float* D,
                    typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                    hipStream_t stream) {
  const dim3 grid = attn_grid(B, H, N);
  // DINOV3_FMHA_DKV64=1 stages 64 q rows per barrier pair where there is more
  // than one 32-row q tile (measured neutral twice, kept for reproduction).
  // getenv per launch is ~ns against the 100 us kernel and keeps the flag
  // flippable from tests.
  // Packed layout only, as before the layouts shared these launchers.
  constexpr int SQB_OPT = L::DKV64_OPTION ? 64 : 32;
  const char* dkv64 = L::DKV64_OPTION ? getenv("DINOV3_FMHA_DKV64") : nullptr;
  const bool use64 = !small_n(N) && dkv64 && dkv64[0] == '1';
  if (HD == 64) {
    if (small_n(N))
      run_dkv<L, 64, 128, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N, P,
                              scale);
    else if (use64)
      run_dkv<L, 64, 256, SQB_OPT>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N, P,
                              scale);
    else
      run_dkv<L, 64, 256, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N, P,
                              scale);
  } else if (HD == 128) {
    if (small_n(N))
      run_dkv<L, 128, 128, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N,
                               P, scale);
    else if (use64)
      run_dkv<L, 128, 256, SQB_OPT>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N,
                               P, scale);
    else
      // occupancy 1 (366 regs with both accumulator sets). A dV-only / dK-only
      // split reached 2 waves/SIMD but measured about 5% slower end to end
      // (it re-streams Q/dO), so it was removed.
      run_dkv<L, 128, 256, 32>(grid, stream, in, dout, sin_t, cos_t, lse, D, grad, B, H, N,
                               P, scale);
  }
}

template <class L, int HD, int NT, class... A>
static void run_fused(dim3 grid, hipStream_t stream, A... args) {
  using Smem = FusedBwdSmem<HD, NT>;
  launch<bwd_fused_kernel<L, HD, NT>, Smem::BYTES, (Smem::BYTES > LDS_DEFAULT_MAX)>(
      grid, NT, stream, args...);
}

// the shapes one workgroup holds: 8 waves of 32 keys each
bool fused_bwd_supported(int N, int HD) {
  return HD == 64 && N >= 1 && N <= FusedBwdSmem<64, 512>::MAX_N;
}

// DINOV3_FMHA_FUSED_BWD=0 forces the three-launch path (A/B runs, tests); read
// per call like DINOV3_FMHA_DKV64
bool fused_bwd_enabled() {
  const char* v = getenv("DINOV3_FMHA_FUSED_BWD");
  return !(v && v[0] == '0');
}

template <class L>
void launch_bwd_fused(typename L::Qkv in, const __hip_bfloat16* dout, const __hip_bfloat16* o,
                      const float* sin_t, const float* cos_t, const float* lse,
                      typename L::DQkv grad, int B, int H, int N, int P, int HD, float scale,
                      hipStream_t stream) {
  // the kernel indexes one LDS slot per 32 keys: a longer sequence would run past them
  if (!fused_bwd_supported(N, HD))
    throw std::invalid_argument("launch_bwd_fused: shape outside fused_bwd_supported(N, HD)");
  const dim3 grid(B * H);
  if (small_n(N))
    run_fused<L, 64, 128>(grid, stream, in, dout, o, sin_t, cos_t, lse, grad, B, H, N, P, scale);
  else
    run_fused<L, 64, 512>(grid, stream, in, dout, o, sin_t, cos_t, lse, grad, B, H, N, P, scale);
}

#define INSTANTIATE_LAUNCHERS(L)                                                            \
  template void launch_bwd_fused<L>(L::Qkv, const __hip_bfloat16*, const __hip_bfloat16*,   \
                                    const float*, const float*, const float*, L::DQkv, int, \
                                    int, int, int, int, float, hipStream_t);                \
  template void launch_fwd<L>(L::Qkv, const float*, const float*, __hip_bfloat16*, float*,  \
                              int, int, int, int, int, float, hipStream_t);                 \
  template void launch_bwd_pre<L>(const __hip_bfloat16*, const __hip_bfloat16*, float*, int, \
                                  int, int, int, hipStream_t);                              \
  template void launch_bwd_dq<L>(L::Qkv, const __hip_bfloat16*, const float*, const float*, \
                                 const float*, const float*, L::DQkv, int, int, int, int,   \
                                 int, float, hipStream_t);                                  \
  template void launch_bwd_dkv<L>(L::Qkv, const __hip_bfloat16*, const float*, const float*, \
                                  const float*, const float*, L::DQkv, int, int, int, int,  \
                                  int, float, hipStream_t);
INSTANTIATE_LAUNCHERS(PackedLayout)
INSTANTIATE_LAUNCHERS(PlainLayout)
#undef INSTANTIATE_LAUNCHERS

}  // namespace fmha_rope

void launch_probe_mfma(const __hip_bfloat16* A, const __hip_bfloat16* B, float* C,
                       hipStream_t stream) {
  hipLaunchKernelGGL(fmha_rope::probe_mfma_kernel, dim3(1), dim3(64), 0, stream, A, B, C);
}

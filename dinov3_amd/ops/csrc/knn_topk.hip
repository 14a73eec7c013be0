// Fused similarity GEMM + top-k selection for k-NN evaluation
// (docs/KERNELS.md "k-NN top-k").
//
//   knn_topk(q [Q,D] bf16, bank [N,D] bf16, k, splits)
//       -> val [Q,k] fp32, idx [Q,k] int32
//
// val[r,:] are the k largest s[r,n] = sum_d q[r,d] * bank[n,d] (bf16 MFMA:
// exact products, fp32 accumulation), idx[r,:] the matching bank rows, ordered
// by (value descending, bank row ascending). That order is total, so the result
// is a function of the computed similarities alone: bit-identical from run to
// run and for every split count. The [Q,N] similarity matrix never exists.
// Non-finite inputs are out of contract.
//
// Candidate key. A similarity and its bank row travel as one 64-bit key,
//   key = ordered(value) << 32 | (0xFFFFFFFF - row),
// ordered() being the usual monotone map of fp32 bits to unsigned (-0 is
// canonicalised to +0 first). A larger key is a better neighbour, keys of
// different rows differ, and key 0 (below every finite value) marks an empty
// slot. Every selection below is a sort by this key.
//
// Main kernel. A block of 4 waves owns KNN_TQ = 32 queries and one slice of
// the bank; the grid is (query tiles, splits). The slice streams through LDS
// in stages of KNN_BN = 128 rows x KNN_BK = 64 columns, double buffered, the
// global loads of the next KNN_PF - 1 stages in flight in registers (issue
// early, write late). Wave w multiplies rows 32w..32w+31 of the tile with the 32 queries,
// swapped (S^T = bank . q^T, as fmha_rope.hip does): a lane's 16 accumulators
// are 16 bank rows of ONE query, lane & 31. The query's current k-th best key
// lives in two registers of its lanes and the filter is a lane-local compare.
// Survivors are appended to the query's list in LDS, the slot taken with an
// LDS integer add; the arrival order this leaves in the list never reaches
// the output, because every read of the list sorts it by key first.
//
// A list has CAP = KCAP + KNN_BN slots: up to k kept keys in front, sorted,
// then the queue. One tile adds at most KNN_BN keys to a list, so a list
// with at most KCAP entries before a tile cannot overflow in it. After a tile
// the block compacts, if any list has grown past KCAP, every list longer
// than k: the owning wave (query i belongs to wave i % 4) ranks each entry by
// counting the entries with a larger key (broadcast LDS reads, entries in
// registers) and writes the entries of rank < k to slot `rank`, which leaves
// the list sorted; then the lanes reload their thresholds. After warm-up a
// tile at bank position n adds about 128 k / n keys to a list, so compaction
// is rare and the MFMA loop is the steady state.
//
// Deviations from a query tile that shrinks with the list capacity: the
// query tile is 32 for both capacities. With the swapped product one wave
// covers exactly 32 queries; a second query group would double the lists
// (96 KiB at CAP = 384), which no longer fit next to the staging buffers.
// The bank tile is re-read by every query tile from L2 / Infinity Cache.
//
// LDS banks of the fragment reads. The staged images have rows of
// KNN_BK + 8 bf16 = 144 bytes = 9 slots of 16 bytes. Lane l reads 16 bytes
// of row l & 31 at a wave-uniform column plus 16 * (l >> 5) bytes
// (ds_read_b128). A ds_read_b128 is served in the lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32): inside a group the column is
// the same and the 16 rows are distinct modulo 16, so their slots
// 9 * row mod 16 are 16 distinct slots of the 256-byte bank row: no
// conflicts. The staging stores are ds_write_b128 of 8 consecutive lanes to
// 128 contiguous bytes of one row: 32 distinct banks.

#include "knn_topk.h"
#include "mfma.h"

typedef bf16x8 knn_bf16x8;
typedef f32x16 knn_f32x16;

#define KNN_TQ 32        // queries per block (one MFMA tile wide)
#define KNN_BN 128       // bank rows per staged tile, 32 per wave
#define KNN_BK 64        // feature columns per staged tile
#define KNN_THREADS 256  // 4 waves
#define KNN_STRIDE (KNN_BK + 8)  // bf16 elements per LDS row
#define KNN_MERGE_THREADS 256
#define KNN_PF 4  // stages whose global loads are in flight or being consumed (even)

namespace knn {

typedef unsigned long long key_t;

DEV_INLINE key_t make_key(float v, unsigned row) {
  unsigned u = __float_as_uint(v);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((key_t)u << 32) | (key_t)(0xFFFFFFFFu - row);
}

DEV_INLINE float key_value(key_t key) {
  unsigned u = (unsigned)(key >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
  return __uint_as_float(u);
}

DEV_INLINE unsigned key_row(key_t key) { return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull); }

// KCAP: largest k of the instantiation. ws != nullptr: write the block's
// sorted keys (0 past the end of a short list) to ws[split, query, k];
// ws == nullptr (one slice): write val / idx directly.
template <int KCAP>
__global__ __launch_bounds__(KNN_THREADS) void topk_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ bank,
    key_t* __restrict__ ws, float* __restrict__ out_val, int* __restrict__ out_idx, long Q,
    long N, int D, int k, long slice_rows) {
  constexpr int CAP = KCAP + KNN_BN;
  constexpr int EPL = CAP / WAVE_SIZE;  // list entries per lane in a compaction
  static_assert(CAP % WAVE_SIZE == 0, "a wave covers a list in whole passes");

  __shared__ __attribute__((aligned(16))) __hip_bfloat16 bank_lds[2][KNN_BN * KNN_STRIDE];
  __shared__ __attribute__((aligned(16))) __hip_bfloat16 q_lds[2][KNN_TQ * KNN_STRIDE];
  __shared__ key_t cand[KNN_TQ * CAP];
  __shared__ int cnt[KNN_TQ];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int l31 = lane & 31;
  const int hhalf = lane >> 5;
  const long q0 = (long)blockIdx.x * KNN_TQ;
  const long n_begin = (long)blockIdx.y * slice_rows;
  const long n_end = n_begin + slice_rows < N ? n_begin + slice_rows : N;
  const long rows = n_end > n_begin ? n_end - n_begin : 0;
  const int ntiles = (int)((rows + KNN_BN - 1) / KNN_BN);
  const int nkc = (D + KNN_BK - 1) / KNN_BK;
  const long nstages = (long)ntiles * nkc;

  if (tid < KNN_TQ) cnt[tid] = 0;

  // ---- staging: thread t owns 16-byte chunk t & 7 of bank rows (t >> 3) + 32 i
  //      and of query row t >> 3 ----
  //      The loads of the next KNN_PF - 1 stages are in flight in registers
  //      (slot = stage % KNN_PF; the stage loop is unrolled by KNN_PF so that
  //      every slot index is a constant): with one wave per SIMD nothing else
  //      hides the load latency. Stages are issued in order, so the position
  //      of the next stage to load is kept as two counters.
  const int srow = tid >> 3;
  const int scol = (tid & 7) * 8;
  knn_bf16x8 breg[KNN_PF][4], qreg[KNN_PF];
  unsigned in_range[KNN_PF];  // bit i: breg[.][i] is inside the slice and D; bit 4: qreg
  long ld_row0 = n_begin;     // first bank row of the tile of the next stage to load
  int ld_kc = 0;              // its column chunk
  // Every load is issued, from a clamped address, and what lies outside the
  // slice, Q or D is replaced by zeros on the way to LDS: loads under a
  // branch would make the compiler drain all of them (vmcnt(0)) before the
  // first use instead of counting the younger stages' loads.
  auto issue_loads = [&](int slot) {
    const int col = ld_kc * KNN_BK + scol;
    const bool col_ok = col < D;
    const int ccol = col_ok ? col : 0;
    unsigned ok = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long grow = ld_row0 + i * 32 + srow;
      const long crow = grow < n_end ? grow : n_end - 1;
      breg[slot][i] = *reinterpret_cast<const knn_bf16x8*>(bank + crow * (long)D + ccol);
      ok |= (col_ok && grow < n_end) ? 1u << i : 0u;
    }
    const long qrow = q0 + srow < Q ? q0 + srow : Q - 1;
    qreg[slot] = *reinterpret_cast<const knn_bf16x8*>(q + qrow * (long)D + ccol);
    ok |= (col_ok && q0 + srow < Q) ? 1u << 4 : 0u;
    in_range[slot] = ok;
    if (++ld_kc == nkc) {
      ld_kc = 0;
      ld_row0 += KNN_BN;
    }
  };
  auto write_tile = [&](int buf, int slot) {
    const unsigned ok = in_range[slot];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<knn_bf16x8*>(&bank_lds[buf][(i * 32 + srow) * KNN_STRIDE + scol]) =
          (ok >> i) & 1 ? breg[slot][i] : knn_bf16x8{};
    *reinterpret_cast<knn_bf16x8*>(&q_lds[buf][srow * KNN_STRIDE + scol]) =
        (ok >> 4) & 1 ? qreg[slot] : knn_bf16x8{};
  };

  // ---- compaction: sort every list longer than k (or, with `all`, every
  //      list) by key and keep its first k entries ----
  auto compact = [&](bool all) {
    for (int qi = wave; qi < KNN_TQ; qi += KNN_THREADS / WAVE_SIZE) {
      key_t* list = cand + qi * CAP;
      const int n = cnt[qi];  // wave-uniform
      const bool go = all ? n > 0 : n > k;
      key_t mine[EPL];
      int rank[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int i = lane + e * WAVE_SIZE;
        mine[e] = (go && i < n) ? list[i] : 0;
        rank[e] = 0;
      }
      if (go) {
        for (int j = 0; j < n; ++j) {
          const key_t kj = list[j];  // same address in every lane: broadcast
#pragma unroll
          for (int e = 0; e < EPL; ++e) rank[e] += kj > mine[e] ? 1 : 0;
        }
      }
      __syncthreads();  // every entry is in registers before any slot is rewritten
      if (go) {
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (mine[e] != 0 && rank[e] < k) list[rank[e]] = mine[e];
        if (lane == 0) cnt[qi] = n < k ? n : k;
      }
    }
    __syncthreads();
  };

  // The query's k-th best key so far, split into value and row: a candidate
  // survives when its key is larger.
  float thr_v = -INFINITY;
  unsigned thr_row = 0xFFFFFFFFu;

  knn_f32x16 acc = {};
#pragma unroll
  for (int p = 0; p < KNN_PF - 1; ++p)
    if (p < nstages) issue_loads(p);
  int kc = 0;                                 // column chunk of the stage computed
  long tile_row0 = n_begin + wave * 32;       // first bank row of this wave's part of the tile
  for (long st0 = 0; st0 < nstages; st0 += KNN_PF) {
#pragma unroll
    for (int p = 0; p < KNN_PF; ++p) {
      const long st = st0 + p;
      if (st >= nstages) break;  // block-uniform
      const int buf = p & 1;  // = st & 1: KNN_PF is even
      // The slot of stage st - 1 went to LDS in that stage and is free.
      if (st + KNN_PF - 1 < nstages) issue_loads((p + KNN_PF - 1) % KNN_PF);
      // Buffer `buf` was last read in stage st - 2; every wave has passed the
      // barrier of stage st - 1 since.
      write_tile(buf, p);
      __syncthreads();

      const __hip_bfloat16* a_base = &bank_lds[buf][(wave * 32 + l31) * KNN_STRIDE + hhalf * 8];
      const __hip_bfloat16* b_base = &q_lds[buf][l31 * KNN_STRIDE + hhalf * 8];
#pragma unroll
      for (int s = 0; s < KNN_BK / 16; ++s) {
        const knn_bf16x8 af = *reinterpret_cast<const knn_bf16x8*>(a_base + s * 16);
        const knn_bf16x8 bf = *reinterpret_cast<const knn_bf16x8*>(b_base + s * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
      }

      if (++kc < nkc) continue;  // block-uniform
      kc = 0;

      // ---- tile finished: filter, queue, maybe compact ----
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        if (v >= thr_v) {
          const long row = tile_row0 + c_row(r, hhalf);
          const float v0 = v + 0.0f;  // -0 -> +0
          if (row < n_end && (v0 > thr_v || (unsigned)row < thr_row)) {
            const int slot = atomicAdd(&cnt[l31], 1);  // < CAP: see the header
            cand[l31 * CAP + slot] = make_key(v0, (unsigned)row);
          }
        }
      }
      acc = knn_f32x16{};
      tile_row0 += KNN_BN;
      __syncthreads();
      const int c_now = cnt[l31];
      if (__syncthreads_or(c_now > KCAP)) {
        compact(false);
        if (c_now > k) {  // this query's list was sorted just now
          const key_t kth = cand[l31 * CAP + k - 1];
          thr_v = key_value(kth);
          thr_row = key_row(kth);
        }
      }
    }
  }

  __syncthreads();
  compact(true);

  for (int e = tid; e < KNN_TQ * k; e += KNN_THREADS) {
    const int qi = e / k;
    const int j = e - qi * k;
    const long qg = q0 + qi;
    if (qg >= Q) break;  // qi grows with e
    const key_t key = j < cnt[qi] ? cand[qi * CAP + j] : 0;
    if (ws != nullptr) {
      ws[((long)blockIdx.y * Q + qg) * k + j] = key;
    } else {
      out_val[qg * k + j] = key_value(key);
      out_idx[qg * k + j] = (int)key_row(key);
    }
  }
}

// Merge of the `splits` sorted lists of one query: the position of a key in
// the merged order is its position in its own list plus, for every other
// list, the number of larger keys there (binary search; keys are distinct).
// Empty slots (key 0) are skipped; at least k real keys exist because k <= N.
__global__ __launch_bounds__(KNN_MERGE_THREADS) void merge_kernel(
    const key_t* __restrict__ ws, float* __restrict__ out_val, int* __restrict__ out_idx, long Q,
    int k, int splits) {
  const long qg = blockIdx.x;
  for (int e = threadIdx.x; e < splits * k; e += KNN_MERGE_THREADS) {
    const int s = e / k;
    const int j = e - s * k;
    const key_t key = ws[((long)s * Q + qg) * k + j];
    if (key == 0) continue;
    int rank = j;
    for (int o = 0; o < splits && rank < k; ++o) {
      if (o == s) continue;
      const key_t* list = ws + ((long)o * Q + qg) * k;
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] > key) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      out_val[qg * k + rank] = key_value(key);
      out_idx[qg * k + rank] = (int)key_row(key);
    }
  }
}

}  // namespace knn

int knn_topk_auto_splits(long Q, long N) {
  const long qtiles = (Q + KNN_TQ - 1) / KNN_TQ;
  if (qtiles >= 256 || qtiles <= 0) return 1;
  long s = (256 + qtiles - 1) / qtiles;
  const long max_s = N / (8 * KNN_BN);
  if (s > max_s) s = max_s;
  if (s > 256) s = 256;
  return s < 1 ? 1 : (int)s;
}

void launch_knn_topk(const __hip_bfloat16* q, const __hip_bfloat16* bank, unsigned long long* ws,
                     float* val, int* idx, long Q, long N, int D, int k, int splits,
                     hipStream_t stream) {
  if (Q <= 0) return;
  const long slice_rows = (N + splits - 1) / splits;
  const dim3 grid((unsigned)((Q + KNN_TQ - 1) / KNN_TQ), (unsigned)splits);
  const dim3 block(KNN_THREADS);
  if (k <= 64) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(knn::topk_kernel<64>), grid, block, 0, stream, q, bank, ws,
                       val, idx, Q, N, D, k, slice_rows);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(knn::topk_kernel<256>), grid, block, 0, stream, q, bank,
                       ws, val, idx, Q, N, D, k, slice_rows);
  }
  HIP_CHECK_LAUNCH();
  if (ws != nullptr) {
    hipLaunchKernelGGL(knn::merge_kernel, dim3((unsigned)Q), dim3(KNN_MERGE_THREADS), 0, stream,
                       ws, val, idx, Q, k, splits);
    HIP_CHECK_LAUNCH();
  }
}

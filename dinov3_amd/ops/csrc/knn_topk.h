// Launcher and host helper of the fused k-NN top-k kernel (knn_topk.hip).
#pragma once

#include "common.h"

// Slices of the bank for `splits == 0`: enough blocks for the 256 CUs (one
// block per CU: the lists and staging buffers take more than half the LDS)
// when there are few query tiles, one slice once the query tiles fill the
// device on their own; a slice keeps at least 8 tiles of rows.
int knn_topk_auto_splits(long Q, long N);

// q [Q, D], bank [N, D] bf16 -> val [Q, k] fp32, idx [Q, k] int32.
// ws: [splits, Q, k] 64-bit keys, or nullptr when splits == 1.
void launch_knn_topk(const __hip_bfloat16* q, const __hip_bfloat16* bank, unsigned long long* ws,
                     float* val, int* idx, long Q, long N, int D, int k, int splits,
                     hipStream_t stream);

// Launchers of the Gram-anchoring loss kernels (gram_loss.hip). s / S (student)
// and t / T (teacher) are bf16 [G M, D]; rs and rt are the fp32 halves of
// r [2, G M].
#pragma once

#include "common.h"

void launch_gram_rnorm(const __hip_bfloat16* s, const __hip_bfloat16* t, float* r, long rows, int D,
                       bool apply_norm, hipStream_t stream);

// Row tiles tile0 .. tile0 + ntiles - 1 of the G * nT row tiles. P (nullptr:
// loss only) is [ntiles * 128, nT * 128] bf16; partials is [G * nT, nT] fp32.
void launch_gram_tiles(const __hip_bfloat16* S, const __hip_bfloat16* T, const float* rs,
                       const float* rt, __hip_bfloat16* P, float* partials, int M, int D, int mode,
                       long tile0, int ntiles, hipStream_t stream);

void launch_gram_finish(const float* partials, float* loss, long n, double count,
                        hipStream_t stream);

void launch_gram_norm_bwd(const __hip_bfloat16* draw, const __hip_bfloat16* s, const float* rs,
                          __hip_bfloat16* ds, long rows, int D, float c, bool apply_norm,
                          hipStream_t stream);

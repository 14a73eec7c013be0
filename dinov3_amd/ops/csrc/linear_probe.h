// Launchers and host helpers of the linear-probe kernels (linear_probe.hip).
#pragma once

#include "common.h"

// Row blocks of a launch: every head gets the same number, all heads together
// stay within PROBE_CE_MAX_BLOCKS (four blocks per CU), and every block runs
// the same number of row rounds. `row_blocks` > 0 overrides the choice.
int probe_ce_row_blocks(long B, int G, int row_blocks);

// Columns of the workspace / of `out`: dbias [G, Cp] when write_grad, then, from
// a 4-float boundary on, G losses and G counts.
void probe_ce_layout(int G, int Cp, bool write_grad, int* ws_cols, int* tail);

// logits [B, G, Cp] (T: float or __hip_bfloat16; overwritten by the gradient
// with write_grad), bias [G, Cp] or nullptr, labels [B].
// out [ws_cols] = column sums of the blocks' partial rows; ws holds nblk rows.
template <typename T>
void launch_probe_ce(T* logits, const float* bias, const long* labels, float* ws, float* out,
                     long B, int G, int Cp, int C, float grad_scale, bool write_grad, int nblk,
                     hipStream_t stream);

// w, mom [G, R] fp32, grad [G, R] (GT: float or __hip_bfloat16), lr [G];
// wd [G] and w_lp [G, R] may be nullptr. R % 8 == 0.
template <typename GT>
void launch_probe_sgd(float* w, float* mom, const GT* grad, const float* lr, const float* wd,
                      __hip_bfloat16* w_lp, int G, long R, float lr_scale, float momentum,
                      hipStream_t stream);

// Launcher and host helpers of the segmentation-probe kernels (seg_probe.hip).
// The SEG_MAX_* limits are in common.h.
#pragma once

#include "common.h"

// Blocks per head of the cross-entropy kernel (nblk) for `quads` cells, and
// rows of the part_db workspace of the gradient finalize.
int seg_ce_quad_blocks(long quads, int G);
int seg_ce_fin_rows(long cells);

// logits [M, h, w, G, Cp] (T: float or __hip_bfloat16), bias [G, Cp] or nullptr,
// labels [M, s h, s w]; loss [G], areas [G, 3, Cp], dbias [G, Cp].
// ws [M h w 4 G Cp] and part_db [seg_ce_fin_rows, G Cp] only with write_grad;
// part_loss [nblk, G], part_area [nblk, G, 3, Cp]; scale (one float on the
// device, or nullptr) multiplies grad_scale.
template <typename T>
void launch_seg_ce(T* logits, const float* bias, const unsigned char* labels, float* ws,
                   float* part_loss, int* part_area, float* part_db, float* loss, long* areas,
                   float* dbias, const float* scale, long M, int h, int w, int s, int G, int Cp,
                   int C, float grad_scale, bool write_grad, int nblk, hipStream_t stream);

// Launcher of the patch-embedding GEMM with fused patchify (patch_embed.hip).
#pragma once

#include "common.h"

// out [Bimg (H/P) (W/P), D] = patches(x [Bimg, C, H, W]) . w [D, C P P]^T + bias [D],
// all bf16; C must be 3 and H, W multiples of P.
void launch_patch_embed_fwd(const __hip_bfloat16* x, const __hip_bfloat16* w,
                            const __hip_bfloat16* bias, __hip_bfloat16* out, int Bimg,
                            int C, int H, int W, int P, int D, hipStream_t stream);

"""Fused multi-head attention, non-causal, short-sequence regime.

DINOv3 sequence lengths are tiny by LLM standards (37 local / 197-201 global /
up to 2309 high-res) at large batch x heads; head_dim 64 (ViT-S..g) or 128
(ViT-7B). The MI355X kernels (csrc/fmha_rope.hip, plain [B, H, N, hd] layout,
no RoPE) therefore tile over (batch*heads, 128-row q blocks) across the 256
CUs, stream K/V through LDS in 64- or 128-key tiles on
v_mfma_f32_32x32x16_bf16, fp32 online softmax, bf16 I/O. They are the same
kernels the model runs on the packed qkv buffer (ops/flat_attention.py).

Forward returns the row log-sum-exp for the backward recompute pass
(flash-attention-2 style backward).

Reference semantics: jax nn.dot_product_attention at
dinov3_jax/layers/attention.py:116 — scale 1/sqrt(hd), no mask, no dropout.
"""

from __future__ import annotations

import math

import torch


class _FmhaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        from . import hip_ops

        o, lse = hip_ops().fmha_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        from . import hip_ops

        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = hip_ops().fmha_bwd(do.contiguous(), q, k, v, o, lse)
        return dq, dk, dv


def fmha_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """fp32 reference: q,k,v [B, H, N, hd] -> o [B, H, N, hd]."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * scale
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhqk,bhkd->bhqd", p, v.float()).to(q.dtype)


def fmha(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q,k,v: [B, H, N, hd] (same shape). Non-causal, unmasked, 1/sqrt(hd) scale."""
    from . import use_hip

    if use_hip(q):
        return _FmhaFn.apply(q.contiguous(), k.contiguous(), v.contiguous())
    return fmha_ref(q, k, v)

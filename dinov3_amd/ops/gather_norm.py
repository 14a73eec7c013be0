"""Drop-path gather fused into LayerNorm, and the LayerNorm backward fused
into the residual-gradient accumulation (csrc/norms.hip).

A drop-path sublayer computes on the kept rows of the flat [R, D] residual
buffer: n = LayerNorm(flat[idx]). Unfused that is `row_gather` + `layernorm_fwd`
forward, and backward a zero-filled [R, D] buffer, a `row_scatter_add_` into it
and autograd's full-buffer add with the gradient that travels down the
residual stream — about 550 MB of traffic per sublayer for `dflat[idx] += dx`.

`gather_layer_norm(flat, idx, ...)` returns `(flat, n)` from ONE autograd node,
so that node's backward receives both gradients and can accumulate the
LayerNorm dx rows straight into the residual gradient:

  forward   gather_layernorm_fwd: reads flat[idx] once, writes n and the
            compact copy `sub` that backward needs. `flat` itself is never
            saved: the fused residual scatter mutates it in place right after.
  backward  layernorm_bwd_scatter_acc_: d_flat[idx] += dx in the last phase of
            the wave-per-row backward; returns d_flat itself.

Accumulating into an incoming gradient is only safe when nothing else can
observe that tensor (it may be an expanded `.sum()` gradient, be shared by the
inputs of an add, or be held by a hook). `own_residual_grad` is an identity
node placed after the last block: its backward hands a private contiguous
clone down the stack and records it in a `GradOwner`; a node that receives any
other tensor (a block called on its own, a gradient autograd re-materialised
on the way) clones first and records its clone. Hooks on the residual stream
*between* the blocks see the shared buffer and must not keep it.

DINOV3_FUSED_GATHER_NORM: on by default on the GPU, `=0` restores the unfused
ops. On CPU a plain-torch emulation of both kernels runs the same graph
(two outputs, in-place accumulation, ownership clone) only when the switch is
set to `1` explicitly.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

__all__ = ["GradOwner", "fused_gather_norm_enabled", "gather_norm_supported",
           "gather_layer_norm", "own_residual_grad"]

# widths of the wave-per-row LayerNorm backward (csrc/norms.hip)
_MAX_WAVE_D = 1536


def fused_gather_norm_enabled(x: torch.Tensor) -> bool:
    from . import use_hip

    v = os.environ.get("DINOV3_FUSED_GATHER_NORM")
    if v is None:
        return use_hip(x)
    return v == "1"


def gather_norm_supported(D: int) -> bool:
    return D % 8 == 0 and D <= _MAX_WAVE_D


class GradOwner:
    """The residual-gradient buffer a block stack owns during one backward."""

    __slots__ = ("buf",)

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def owns(self, g: torch.Tensor) -> bool:
        b = self.buf
        return (b is not None and g.data_ptr() == b.data_ptr() and g.shape == b.shape
                and g.dtype == b.dtype and g.is_contiguous())

    def take(self, g: torch.Tensor) -> torch.Tensor:
        """A private contiguous copy of `g`, recorded as the owned buffer."""
        self.buf = g.clone(memory_format=torch.contiguous_format)
        return self.buf


class _OwnGradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, owner):
        ctx.owner = owner
        return x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ctx.owner.take(g), None


def own_residual_grad(x: torch.Tensor, owner: GradOwner) -> torch.Tensor:
    """Identity; backward passes a clone the nodes below may accumulate into."""
    return _OwnGradFn.apply(x, owner)


class _GatherNormFn(torch.autograd.Function):
    """(flat, idx, w, b) -> (flat itself, LayerNorm(flat[idx]))."""

    @staticmethod
    def forward(ctx, flat, idx, weight, bias, eps, owner):
        from . import hip_ops, use_hip

        if use_hip(flat):
            y, sub, mean, rstd = hip_ops().gather_layernorm_fwd(flat, idx, weight, bias, eps)
        else:  # emulation: the fp32 ops of layer_norm's CPU path
            sub = flat.index_select(0, idx)
            y, mean, rstd = torch.native_layer_norm(
                sub.float(), (sub.shape[-1],), weight.float(), bias.float(), eps)
            y = y.to(flat.dtype)
        ctx.save_for_backward(sub, weight, mean, rstd, idx)
        ctx.owner = owner
        ctx.mark_dirty(flat)  # returned as is, unmodified: the residual stream
        return flat, y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_flat, d_n):
        from . import hip_ops, use_hip

        sub, weight, mean, rstd, idx = ctx.saved_tensors
        owner = ctx.owner
        if owner is None:
            d_flat = d_flat.clone(memory_format=torch.contiguous_format)
        elif not owner.owns(d_flat):
            d_flat = owner.take(d_flat)
        if use_hip(d_flat):
            dw, db = hip_ops().layernorm_bwd_scatter_acc_(
                d_flat, idx, d_n.contiguous(), sub, weight, mean, rstd)
        else:
            wf = weight.float()  # also stands in for bias: only its shape is used
            dx, dw, db = torch.ops.aten.native_layer_norm_backward(
                d_n.float().contiguous(), sub.float(), (sub.shape[-1],), mean, rstd,
                wf, wf, [True, True, True])
            # one rounding, as in the kernel (fp64 buffers add in fp64)
            acc_t = torch.promote_types(d_flat.dtype, torch.float32)
            d_flat[idx] = (d_flat.index_select(0, idx).to(acc_t) + dx.to(acc_t)).to(d_flat.dtype)
            dw, db = dw.to(weight.dtype), db.to(weight.dtype)
        return d_flat, None, dw, db, None, None


def gather_layer_norm(flat: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor,
                      bias: torch.Tensor, eps: float,
                      owner: Optional[GradOwner] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(flat, LayerNorm(flat[idx])). `flat` comes back as the same tensor, now
    an output of the node, and the caller must use that one from here on.

    Widths the kernels do not cover run the unfused pair of ops."""
    from .layernorm import layer_norm
    from .row_ops import gather_rows

    if not gather_norm_supported(flat.shape[-1]):
        return flat, layer_norm(gather_rows(flat, idx), weight, bias, eps)
    return _GatherNormFn.apply(flat, idx, weight.contiguous(), bias.contiguous(), eps, owner)

"""FP8 (OCP e4m3fn) forward for the transformer-block linears.

Numerics contract (docs/KERNELS.md, "FP8 forward"), shared bit for bit by the
HIP kernels (csrc/fp8_gemm.hip) and the torch emulation below:

- one power-of-two fp32 scale per row of a K-contiguous matrix (per token for
  activations ``x[M,K]``, per output channel for weights ``w[N,K]``):
  ``amax = m * 2^e`` with ``m in [1,2)``; ``s = 2^(e-8)`` if ``m <= 1.75`` else
  ``2^(e-7)`` — the smallest power of two with ``amax / s <= 448``;
  ``amax == 0`` gives ``s = 1``. The exponent of ``s`` is floored at -126 so
  that ``s`` and ``1/s`` stay normal fp32 (only rows with amax < 2^-118);
- ``q = rne_e4m3(row / s)``: the division is exact and nothing saturates;
- ``y[m,n] = rne((sum_k q_x[m,k] q_w[n,k]) * s_x[m] * s_w[n] + bias[n])`` with
  the sum and the epilogue in fp32;
- backward is straight-through on the saved full-precision ``x`` and ``w``
  (torch matmuls — the library bf16 path, exactly as for ``F.linear``).

On a HIP device the op needs bf16 inputs and the compiled extension and raises
otherwise; it never falls back silently. On CPU (and under
``DINOV3_DISABLE_HIP=1``) the torch emulation runs for any float dtype.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

__all__ = ["fp8_quantize_rows", "fp8_linear", "fp8_eligible", "FP8_K_ALIGN", "FP8_N_ALIGN"]

FP8_K_ALIGN = 128  # one scaled-MFMA K-step (FP8_GEMM_BK in csrc/common.h)
FP8_N_ALIGN = 16   # one MFMA tile of output columns (FP8_GEMM_N_ALIGN)
_MIN_SCALE_EXP = -126


def fp8_eligible(in_features: int, out_features: int) -> bool:
    """Shapes the fp8 GEMM accepts: K a multiple of 128, N a multiple of 16."""
    return (in_features > 0 and out_features > 0
            and in_features % FP8_K_ALIGN == 0 and out_features % FP8_N_ALIGN == 0)


def _row_scales_ref(x2d: torch.Tensor) -> torch.Tensor:
    amax = x2d.float().abs().amax(dim=-1)
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1)
    exp = e - 9 + (m > 0.875).to(e.dtype)
    exp = exp.clamp(min=_MIN_SCALE_EXP, max=126)
    s = torch.ldexp(torch.ones_like(amax), exp)
    return torch.where(amax > 0, s, torch.ones_like(s))


def _quantize_rows_ref(x2d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    s = _row_scales_ref(x2d)
    q = (x2d.float() / s[:, None]).to(torch.float8_e4m3fn)
    return q, s


def fp8_quantize_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [M,K] -> (q float8_e4m3fn [M,K], scale fp32 [M]) per the contract."""
    from . import hip_ops, use_hip

    assert x.dim() == 2, "fp8_quantize_rows expects [M, K]"
    if use_hip(x):
        if x.dtype != torch.bfloat16:
            raise RuntimeError(f"fp8_quantize_rows on a HIP device needs bf16, got {x.dtype}")
        q, s = hip_ops().fp8_quant_rows(x.contiguous())
        return q.view(torch.float8_e4m3fn), s
    return _quantize_rows_ref(x)


def _gemm_ref(xq, sx, wq, sw, bias, out_dtype):
    acc = xq.float() @ wq.float().t()
    y = acc * sx[:, None] * sw[None, :]
    if bias is not None:
        y = y + bias.float()
    return y.to(out_dtype)


def _forward_2d(x2d: torch.Tensor, weight: torch.Tensor,
                bias: Optional[torch.Tensor]) -> torch.Tensor:
    from . import hip_ops, use_hip

    if x2d.is_cuda and use_hip(x2d):
        if x2d.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16 or (
                bias is not None and bias.dtype != torch.bfloat16):
            raise RuntimeError(
                "fp8_linear on a HIP device needs bf16 x, weight and bias "
                f"(got {x2d.dtype}, {weight.dtype}, {None if bias is None else bias.dtype})")
        ops = hip_ops()
        xq, sx = ops.fp8_quant_rows(x2d.contiguous())
        wq, sw = ops.fp8_quant_rows(weight.contiguous())
        return ops.fp8_gemm_nt(xq, sx, wq, sw, None if bias is None else bias.contiguous())
    xq, sx = _quantize_rows_ref(x2d)
    wq, sw = _quantize_rows_ref(weight)
    return _gemm_ref(xq, sx, wq, sw, bias, x2d.dtype)


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias):
        ctx.save_for_backward(x2d, weight)
        ctx.has_bias = bias is not None
        return _forward_2d(x2d, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy.to(weight.dtype) @ weight
        if ctx.needs_input_grad[1]:
            dw = dy.to(x2d.dtype).t() @ x2d
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(dim=0)
        return dx, dw, db


def fp8_linear(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, weight, bias)`` with the forward GEMM in e4m3 (see module
    docstring). x: [..., K]; weight: [N, K]; bias: [N] or None."""
    K = x.shape[-1]
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K:
        raise RuntimeError(f"fp8_linear: x [..., {K}] does not match weight {tuple(weight.shape)}")
    if not fp8_eligible(K, N):
        raise RuntimeError(
            f"fp8_linear: in_features={K} must be a multiple of {FP8_K_ALIGN} and "
            f"out_features={N} a multiple of {FP8_N_ALIGN}")
    x2d = x.reshape(-1, K)
    y = _Fp8LinearFn.apply(x2d, weight, bias)
    return y.reshape(*x.shape[:-1], N)

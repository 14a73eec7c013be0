"""FP8 forward (OCP e4m3fn) and opt-in FP8 backward (e5m2 gradients) for the
transformer-block linears.

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
- ``backward="bf16"`` (default) is straight-through on the saved
  full-precision ``x`` and ``w`` (torch matmuls — the library bf16 path,
  exactly as for ``F.linear``).

``backward="fp8"`` (docs/KERNELS.md, "FP8 backward") runs dgrad and wgrad on
the same GEMM kernel. Gradients ``dy`` are quantised to e5m2, ``x`` and ``w``
to e4m3, all with the scale rule above and the format's largest finite value
(448, 57344). Scales never depend on the contraction index:

- dgrad ``dx[M,K] = dy[M,N] . w[N,K]`` contracts over N: ``dy`` per row,
  ``w`` per input channel k (the quantised transpose ``wT_q [K,N]``);
- wgrad ``dw[N,K] = dy^T . x`` contracts over the M tokens: ``dy`` per output
  channel n (``dyT_q [N,Mp]``), ``x`` per input channel k (``xT_q [K,Mp]``),
  ``Mp`` = M rounded up to a multiple of 128 with zero pad bytes;
- ``db[n]`` is the fp32 sum over tokens of the unquantised ``dy[:,n]``;
- outputs are ``rne(acc_fp32 * s_row * s_col)`` in the dtype of ``x`` / ``w``.

On a HIP device the op needs bf16 inputs and the compiled extension and raises
otherwise; it never falls back silently. On CPU (and under
``DINOV3_DISABLE_HIP=1``) the torch emulation runs for any float dtype.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

__all__ = ["fp8_quantize_rows", "fp8_quantize_cols_t", "fp8_linear", "fp8_eligible",
           "fp8_bwd_eligible", "FP8_K_ALIGN", "FP8_N_ALIGN", "FP8_ROW_PAD"]

FP8_K_ALIGN = 128  # one scaled-MFMA K-step (FP8_GEMM_BK in csrc/common.h)
FP8_N_ALIGN = 16   # one MFMA tile of output columns (FP8_GEMM_N_ALIGN)
FP8_ROW_PAD = 128  # rows of a transposed operand are padded to this (FP8_COLS_TR)
_MIN_SCALE_EXP = -126

# format -> (torch dtype, frexp offset of the scale rule: MAX = 0.875 * 2^offset,
#            kernel format id = the MFMA's cbsz / blgp immediate)
_FORMATS = {
    "e4m3": (torch.float8_e4m3fn, 9, 0),
    "e5m2": (torch.float8_e5m2, 16, 1),
}


def _fmt(fmt: str):
    try:
        return _FORMATS[fmt]
    except KeyError:
        raise ValueError(f"fp8 format must be 'e4m3' or 'e5m2', got {fmt!r}") from None


def fp8_eligible(in_features: int, out_features: int) -> bool:
    """Shapes the fp8 GEMM accepts: K a multiple of 128, N a multiple of 16."""
    return (in_features > 0 and out_features > 0
            and in_features % FP8_K_ALIGN == 0 and out_features % FP8_N_ALIGN == 0)


def fp8_bwd_eligible(in_features: int, out_features: int) -> bool:
    """Shapes the fp8 backward accepts: both multiples of 128 (dgrad contracts
    over out_features; the transposing quantisers and wgrad tile by 128)."""
    return (in_features > 0 and out_features > 0
            and in_features % FP8_K_ALIGN == 0 and out_features % FP8_K_ALIGN == 0)


def _row_scales_ref(x2d: torch.Tensor, fmt: str = "e4m3") -> torch.Tensor:
    amax = x2d.float().abs().amax(dim=-1)
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1)
    exp = e - _fmt(fmt)[1] + (m > 0.875).to(e.dtype)
    exp = exp.clamp(min=_MIN_SCALE_EXP, max=126)
    s = torch.ldexp(torch.ones_like(amax), exp)
    return torch.where(amax > 0, s, torch.ones_like(s))


def _quantize_rows_ref(x2d: torch.Tensor, fmt: str = "e4m3") -> Tuple[torch.Tensor, torch.Tensor]:
    s = _row_scales_ref(x2d, fmt)
    q = (x2d.float() / s[:, None]).to(_fmt(fmt)[0])
    return q, s


def _quantize_cols_t_ref(x2d: torch.Tensor, fmt: str = "e4m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """x [R,C] -> (q [C,Rp], scale [C]): the row oracle on ``x.t()``, rows
    padded with zero bytes to a multiple of 128."""
    R = x2d.shape[0]
    q, s = _quantize_rows_ref(x2d.t(), fmt)
    pad = -R % FP8_ROW_PAD
    if pad:
        q = torch.nn.functional.pad(q.view(torch.uint8), (0, pad)).view(q.dtype)
    return q.contiguous(), s


def fp8_quantize_rows(x: torch.Tensor, fmt: str = "e4m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """x [M,K] -> (q float8 [M,K] in `fmt`, scale fp32 [M]) per the contract."""
    from . import hip_ops, use_hip

    assert x.dim() == 2, "fp8_quantize_rows expects [M, K]"
    dtype, _, fid = _fmt(fmt)
    if use_hip(x):
        if x.dtype != torch.bfloat16:
            raise RuntimeError(f"fp8_quantize_rows on a HIP device needs bf16, got {x.dtype}")
        q, s = hip_ops().fp8_quant_rows(x.contiguous(), fid)
        return q.view(dtype), s
    return _quantize_rows_ref(x, fmt)


def fp8_quantize_cols_t(x: torch.Tensor, fmt: str = "e4m3", colsum: bool = False):
    """x [R,C] -> (q float8 [C,Rp] in `fmt`, scale fp32 [C]): the transpose,
    quantised with one scale per column of x, rows padded with zeros to
    Rp = ceil(R/128)*128. With ``colsum=True`` a third result holds the fp32
    column sums of x, [C]."""
    from . import hip_ops, use_hip

    assert x.dim() == 2, "fp8_quantize_cols_t expects [R, C]"
    dtype, _, fid = _fmt(fmt)
    if use_hip(x):
        if x.dtype != torch.bfloat16:
            raise RuntimeError(f"fp8_quantize_cols_t on a HIP device needs bf16, got {x.dtype}")
        q, s, sums = hip_ops().fp8_quant_cols_t(x.contiguous(), fid, colsum)
        q = q.view(dtype)
    else:
        q, s = _quantize_cols_t_ref(x, fmt)
        sums = x.float().sum(dim=0) if colsum else None
    return (q, s, sums) if colsum else (q, s)


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


def _backward_fp8(dy, x2d, weight, need_dx, need_dw, need_db):
    """dgrad / wgrad / bias grad per the "FP8 backward" contract; only the
    work that a needed gradient asks for is launched."""
    from . import hip_ops, use_hip

    M, N = dy.shape
    dx = dw = db = None
    if M == 0:  # nothing to contract over: zero grads, no launch
        if need_dx:
            dx = x2d.new_zeros(x2d.shape)
        if need_dw:
            dw = torch.zeros_like(weight)
        if need_db:
            db = dy.new_zeros(N)
        return dx, dw, db

    if dy.is_cuda and use_hip(dy):
        if (dy.dtype != torch.bfloat16 or x2d.dtype != torch.bfloat16
                or weight.dtype != torch.bfloat16):
            raise RuntimeError(
                "fp8_linear backward on a HIP device needs bf16 dy, x and weight "
                f"(got {dy.dtype}, {x2d.dtype}, {weight.dtype})")
        ops = hip_ops()
        e4m3, e5m2 = _FORMATS["e4m3"][2], _FORMATS["e5m2"][2]
        dy = dy.contiguous()
        if need_dx:
            dyq, sdy = ops.fp8_quant_rows(dy, e5m2)
            wtq, swt, _ = ops.fp8_quant_cols_t(weight.contiguous(), e4m3, False)
            dx = ops.fp8_gemm_nt(dyq, sdy, wtq, swt, None, e5m2)
        if need_dw:
            dytq, sdyt, sums = ops.fp8_quant_cols_t(dy, e5m2, need_db)
            xtq, sxt, _ = ops.fp8_quant_cols_t(x2d.contiguous(), e4m3, False)
            dw = ops.fp8_gemm_nt(dytq, sdyt, xtq, sxt, None, e5m2)
            if need_db:
                db = sums.to(dy.dtype)
        elif need_db:
            db = ops.fp8_colsum(dy).to(dy.dtype)
        return dx, dw, db

    if need_dx:
        dyq, sdy = _quantize_rows_ref(dy, "e5m2")
        wtq, swt = _quantize_cols_t_ref(weight, "e4m3")
        dx = _gemm_ref(dyq, sdy, wtq, swt, None, x2d.dtype)
    if need_dw:
        dytq, sdyt = _quantize_cols_t_ref(dy, "e5m2")
        xtq, sxt = _quantize_cols_t_ref(x2d, "e4m3")
        dw = _gemm_ref(dytq, sdyt, xtq, sxt, None, weight.dtype)
    if need_db:
        db = dy.float().sum(dim=0).to(dy.dtype)
    return dx, dw, db


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias, backward):
        ctx.save_for_backward(x2d, weight)
        ctx.has_bias = bias is not None
        ctx.fp8_backward = backward == "fp8"
        return _forward_2d(x2d, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.fp8_backward:
            dx, dw, db = _backward_fp8(dy, x2d, weight, ctx.needs_input_grad[0],
                                       ctx.needs_input_grad[1], need_db)
            return dx, dw, db, None
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy.to(weight.dtype) @ weight
        if ctx.needs_input_grad[1]:
            dw = dy.to(x2d.dtype).t() @ x2d
        if need_db:
            db = dy.sum(dim=0)
        return dx, dw, db, None


def fp8_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
               backward: str = "bf16") -> torch.Tensor:
    """``F.linear(x, weight, bias)`` with the forward GEMM in e4m3 and, with
    ``backward="fp8"``, dgrad and wgrad on e5m2 gradients (see module
    docstring); ``"bf16"`` keeps the straight-through backward.
    x: [..., K]; weight: [N, K]; bias: [N] or None."""
    if backward not in ("bf16", "fp8"):
        raise ValueError(f"fp8_linear: backward must be 'bf16' or 'fp8', got {backward!r}")
    K = x.shape[-1]
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K:
        raise RuntimeError(f"fp8_linear: x [..., {K}] does not match weight {tuple(weight.shape)}")
    if not fp8_eligible(K, N):
        raise RuntimeError(
            f"fp8_linear: in_features={K} must be a multiple of {FP8_K_ALIGN} and "
            f"out_features={N} a multiple of {FP8_N_ALIGN}")
    if backward == "fp8" and not fp8_bwd_eligible(K, N):
        raise RuntimeError(
            f"fp8_linear: backward='fp8' needs in_features={K} and out_features={N} to be "
            f"multiples of {FP8_K_ALIGN}")
    x2d = x.reshape(-1, K)
    y = _Fp8LinearFn.apply(x2d, weight, bias, backward)
    return y.reshape(*x.shape[:-1], N)

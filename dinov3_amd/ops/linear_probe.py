"""The two non-GEMM parts of a linear-probe training step, for a grid of heads
at once (docs/KERNELS.md "Linear probe"): softmax cross-entropy with the
gradient written in place, and SGD with momentum with the bf16 weight copy."""

from __future__ import annotations

from typing import Optional, Tuple

import torch


def probe_ce_ref(logits: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor,
                 C: int, grad_scale: float, write_grad: bool = True
                 ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Plain-torch `probe_ce`, computed in fp64: the oracle of the kernel tests
    and the CPU path; not meant to be fast."""
    if logits.dim() != 3:
        raise ValueError(f"probe_ce: logits must be [B, G, Cp], got {tuple(logits.shape)}")
    B, G, Cp = logits.shape
    if not 1 <= C <= Cp:
        raise ValueError(f"probe_ce: need 1 <= C <= Cp, got C = {C}, Cp = {Cp}")
    z = logits[:, :, :C].double()
    if bias is not None:
        z = z + bias[:, :C].double()
    counted = (labels >= 0)
    target = labels.clamp(min=0)
    top = z.max(dim=2, keepdim=True).values
    shifted = z - top
    lse = shifted.exp().sum(dim=2).log() + top.squeeze(2)  # [B, G]
    picked = z.gather(2, target.view(B, 1, 1).expand(B, G, 1)).squeeze(2)
    loss_sum = ((lse - picked) * counted.view(B, 1)).sum(dim=0).float()
    # the lowest index among the maximal logits
    cols = torch.arange(C, device=z.device).view(1, 1, C).expand(B, G, C)
    pred = torch.where(z == top, cols, torch.full_like(cols, C)).min(dim=2).values
    correct = ((pred == target.view(B, 1)) & counted.view(B, 1)).sum(dim=0).long()
    if not write_grad:
        return loss_sum, correct, None
    grad = (shifted - (lse - top.squeeze(2)).unsqueeze(2)).exp()
    grad.scatter_add_(2, target.view(B, 1, 1).expand(B, G, 1),
                      grad.new_full((B, G, 1), -1.0))
    grad = torch.where(counted.view(B, 1, 1), grad * grad_scale, torch.zeros_like(grad))
    dbias = logits.new_zeros((G, Cp), dtype=torch.float32)
    dbias[:, :C] = grad.sum(dim=0).float()
    logits[:, :, :C] = grad.to(logits.dtype)
    logits[:, :, C:] = 0
    return loss_sum, correct, dbias


def probe_ce(logits: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor, C: int,
             grad_scale: float, write_grad: bool = True, row_blocks: int = 0
             ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Softmax cross-entropy of G heads at once. `logits` [B, G, Cp] (bf16 or
    fp32), `bias` [G, Cp] fp32 or None, `labels` [B] int64. Per row (b, g),
    z = logits + bias over the columns < C; the columns C..Cp-1 do not exist for
    the softmax. Returns (loss_sum [G] fp32: the sum over rows of
    lse(z) - z[label]; correct [G] int64: the rows whose lowest-index argmax is
    the label; dbias [G, Cp] fp32, or None without `write_grad`).

    With `write_grad` every row is overwritten in place with
    (softmax(z) - onehot) * grad_scale in the logits dtype, 0 in the pad
    columns, and dbias is the column sum of those values before they are
    rounded. A row with label -1 is ignored: no loss, no count, zero gradient.
    Other labels outside [0, C) are out of contract.

    On a HIP device: contiguous tensors, Cp % 8 == 0, Cp <= 2048; the result is
    bit-identical from run to run. `row_blocks` (0 = chosen from B and G) is the
    number of blocks that share a head's rows; the sums are bit-identical only
    for equal `row_blocks`.
    """
    from . import hip_ops, use_hip

    if use_hip(logits):
        out = hip_ops().probe_ce(logits, bias, labels, int(C), float(grad_scale), bool(write_grad),
                                 int(row_blocks))
        return out[0], out[1], (out[2] if write_grad else None)
    return probe_ce_ref(logits, bias, labels, C, grad_scale, write_grad)


def probe_sgd_ref_(w: torch.Tensor, mom: torch.Tensor, grad: torch.Tensor, lr: torch.Tensor,
                   wd: Optional[torch.Tensor], lr_scale: float, momentum: float = 0.9,
                   w_lp: Optional[torch.Tensor] = None) -> None:
    """Plain-torch `probe_sgd_`, computed in fp64 and rounded once."""
    if w.dim() != 2 or mom.shape != w.shape or grad.shape != w.shape:
        raise ValueError("probe_sgd_: w, mom and grad must share one [G, R] shape")
    g = grad.double()
    if wd is not None:
        g = g + wd.double().view(-1, 1) * w.double()
    m = momentum * mom.double() + g
    mom.copy_(m.float())
    w.copy_((w.double() - lr.double().view(-1, 1) * lr_scale * m).float())
    if w_lp is not None:
        w_lp.copy_(w.bfloat16())


def probe_sgd_(w: torch.Tensor, mom: torch.Tensor, grad: torch.Tensor, lr: torch.Tensor,
               wd: Optional[torch.Tensor], lr_scale: float, momentum: float = 0.9,
               w_lp: Optional[torch.Tensor] = None) -> None:
    """SGD with momentum (no dampening, no Nesterov) on G heads in place.
    `w`, `mom` [G, R] fp32, `grad` [G, R] bf16 or fp32, `lr` [G] fp32, `wd` [G]
    fp32 or None:

        g' = grad + wd[g] * w
        mom = momentum * mom + g'
        w = w - lr[g] * lr_scale * mom

    With `w_lp` [G, R] bf16 it also writes w_lp = bf16(w), round to nearest
    even: the copy the next forward GEMM reads. On a HIP device R % 8 == 0.
    """
    from . import hip_ops, use_hip

    if use_hip(w):
        hip_ops().probe_sgd_(w, mom, grad, lr, wd, float(lr_scale), float(momentum), w_lp)
        return
    probe_sgd_ref_(w, mom, grad, lr, wd, lr_scale, momentum, w_lp)

"""Gram-anchoring loss with its student gradient out of one pass
(docs/KERNELS.md "Gram loss"): both similarity matrices come from bf16 MFMA
tiles and are consumed in the tile's epilogue, so no fp32 M x M matrix exists;
the gradient's P = dL/dA panel is held one row panel at a time."""

from __future__ import annotations

from typing import Optional

import torch

GRAM_TILE = 128                         # rows and columns of a kernel tile
GRAM_DEFAULT_PANEL_BYTES = 256 << 20    # P row panel held at a time
_MAX_PANEL_TILES = 65535                # row tiles per launch (grid.y)


def _check(student: torch.Tensor, teacher: torch.Tensor) -> None:
    if student.dim() != 3 or student.shape != teacher.shape:
        raise ValueError(f"gram_loss: student and teacher must share one shape [G, M, D], got "
                         f"{tuple(student.shape)} and {tuple(teacher.shape)}")
    if min(student.shape) < 1:
        raise ValueError(f"gram_loss: need G, M, D >= 1, got {tuple(student.shape)}")


def _mode(remove_neg: bool, remove_only_teacher_neg: bool) -> int:
    """0 plain, 1 remove_neg, 2 remove_only_teacher_neg; remove_neg wins, as in GramLoss."""
    return 1 if remove_neg else (2 if remove_only_teacher_neg else 0)


def gram_loss_ref(student: torch.Tensor, teacher: torch.Tensor, *, apply_norm: bool,
                  remove_neg: bool, remove_only_teacher_neg: bool,
                  panel_bytes: Optional[int] = None) -> torch.Tensor:
    """Plain-torch `gram_loss`, differentiated by autograd: in fp64 for fp64
    inputs, else in fp32. The oracle of the kernel tests and the CPU path; it
    holds the G M x M matrices several times over. `panel_bytes` is ignored."""
    _check(student, teacher)
    wide = torch.float64 if student.dtype == torch.float64 else torch.float32
    s = student.to(wide)
    t = teacher.detach().to(wide)  # the gradient flows to the student only
    if apply_norm:
        s = s / s.norm(dim=-1, keepdim=True)
        t = t / t.norm(dim=-1, keepdim=True)
    a = s @ s.transpose(-1, -2)
    b = t @ t.transpose(-1, -2)
    mode = _mode(remove_neg, remove_only_teacher_neg)
    if mode == 1:
        a = torch.where(a < 0, torch.zeros_like(a), a)
        b = torch.where(b < 0, torch.zeros_like(b), b)
    elif mode == 2:
        both_neg = (a < 0) & (b < 0)
        a = torch.where(both_neg, torch.zeros_like(a), a)
        b = torch.where(b < 0, torch.zeros_like(b), b)
    return ((a - b) ** 2).mean()


def _panel_tiles(panel_bytes: int, M: int) -> int:
    """Row tiles of 128 rows whose P rows, padded to whole tiles of columns, fit panel_bytes."""
    n_t = (M + GRAM_TILE - 1) // GRAM_TILE
    return max(1, min(int(panel_bytes) // (GRAM_TILE * n_t * GRAM_TILE * 2), _MAX_PANEL_TILES))


class _GramLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, apply_norm, mode, panel_bytes, need_grad):
        from . import hip_ops

        ops = hip_ops()
        s = student.detach().contiguous()
        t = teacher.detach().contiguous()
        G, M, D = s.shape
        n_t = (M + GRAM_TILE - 1) // GRAM_TILE
        m_pad = n_t * GRAM_TILE
        r = ops.gram_rnorm(s, t, apply_norm)
        partials = torch.empty(G * n_t * n_t, device=s.device, dtype=torch.float32)
        if not need_grad:
            for t0 in range(0, G * n_t, _MAX_PANEL_TILES):
                ops.gram_tiles(s, t, r, mode, t0, min(_MAX_PANEL_TILES, G * n_t - t0), None,
                               partials)
            return ops.gram_finish(partials, float(G * M * M))

        tiles = _panel_tiles(panel_bytes, M)
        draw = torch.empty_like(s)
        if tiles >= n_t:  # a panel holds whole matrices: one batched GEMM per panel
            per = min(tiles // n_t, G)
            panel = torch.empty((per * m_pad, m_pad), device=s.device, dtype=s.dtype)
            for g0 in range(0, G, per):
                k = min(per, G - g0)
                ops.gram_tiles(s, t, r, mode, g0 * n_t, k * n_t, panel, partials)
                p = panel[:k * m_pad].view(k, m_pad, m_pad)[:, :M, :M]
                torch.bmm(p, s[g0:g0 + k], out=draw[g0:g0 + k])
        else:  # panels walk the row tiles of one matrix after the other
            panel = torch.empty((tiles * GRAM_TILE, m_pad), device=s.device, dtype=s.dtype)
            for g in range(G):
                for t0 in range(0, n_t, tiles):
                    k = min(tiles, n_t - t0)
                    row0 = t0 * GRAM_TILE
                    rows = min(k * GRAM_TILE, M - row0)
                    ops.gram_tiles(s, t, r, mode, g * n_t + t0, k, panel, partials)
                    torch.mm(panel[:rows, :M], s[g], out=draw[g, row0:row0 + rows])
        del panel
        loss = ops.gram_finish(partials, float(G * M * M))
        ctx.save_for_backward(ops.gram_norm_bwd(draw, s, r, 4.0 / float(G * M * M), apply_norm))
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (ds,) = ctx.saved_tensors
        return ds * grad_out, None, None, None, None, None


def gram_loss(student: torch.Tensor, teacher: torch.Tensor, *, apply_norm: bool, remove_neg: bool,
              remove_only_teacher_neg: bool, panel_bytes: Optional[int] = None) -> torch.Tensor:
    """Gram-anchoring loss of G independent matrices: `student`, `teacher`
    [G, M, D]; rows L2-normalised with `apply_norm`; A = s s^T, B = t t^T;
    `remove_neg` clamps both at 0, `remove_only_teacher_neg` clamps B at 0 and
    zeroes A where both are negative (exactly the `torch.where` code of
    `loss.GramLoss`); the result is the mean of (a - b)^2 over all G M M
    entries, a 0-dim fp32 tensor. The gradient flows to `student` only.

    On a HIP device both inputs are bf16 and D % 8 == 0 (anything else raises;
    other dtypes take `gram_loss_ref`); rows of zero norm and non-finite inputs
    are out of contract. Products are exact and every sum is fp32 in a fixed
    order: loss and gradient are bit-identical from run to run, and the loss
    for every `panel_bytes`. When `student` requires a gradient it is computed
    in the forward pass and is all that is saved; the backward multiplies it by
    the incoming scalar. Otherwise the gradient part is skipped.

    Workspace: one P row panel of at most `panel_bytes` (default 256 MiB; at
    least one 128-row tile of ceil(M / 128) * 128 columns, bf16), two [G, M, D]
    bf16 tensors, the row norms and one fp32 value per 128 x 128 tile.
    """
    from . import use_hip

    _check(student, teacher)
    if (use_hip(student) and student.dtype == torch.bfloat16
            and teacher.dtype == torch.bfloat16):
        if student.shape[-1] % 8:
            raise ValueError(f"gram_loss: D must be a multiple of 8 on the device, got "
                             f"{student.shape[-1]}")
        if teacher.device != student.device:
            raise ValueError("gram_loss: student and teacher must be on one device")
        pb = GRAM_DEFAULT_PANEL_BYTES if panel_bytes is None else int(panel_bytes)
        if pb < 1:
            raise ValueError(f"gram_loss: panel_bytes must be positive, got {panel_bytes}")
        need_grad = bool(student.requires_grad and torch.is_grad_enabled())
        return _GramLossFn.apply(student, teacher, bool(apply_norm),
                                 _mode(remove_neg, remove_only_teacher_neg), pb, need_grad)
    return gram_loss_ref(student, teacher, apply_norm=apply_norm, remove_neg=remove_neg,
                         remove_only_teacher_neg=remove_only_teacher_neg)

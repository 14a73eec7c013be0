"""The non-GEMM part of a linear segmentation probe's training step
(docs/KERNELS.md "Segmentation probe"): patch-resolution logits upsampled
bilinearly to the label resolution, per-pixel softmax cross-entropy and IoU
counts for a grid of heads at once, the gradient folded back to patch
resolution and written in place. The upsampled logits never exist in memory."""

from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

SEG_MAX_CLASSES = 255  # labels are uint8 and 255 marks an ignored pixel
SEG_IGNORE = 255
_MAX_CP = 256
_MAX_SCALE = 32


def _geometry(logits: torch.Tensor, labels: torch.Tensor, C: int) -> int:
    """Checks the shapes of a `seg_ce` call; returns the scale s."""
    if logits.dim() != 5:
        raise ValueError(f"seg_ce: logits must be [M, h, w, G, Cp], got {tuple(logits.shape)}")
    M, h, w, G, Cp = logits.shape
    if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.shape[0] != M:
        raise ValueError("seg_ce: labels must be uint8 [M, H, W]")
    H, W = labels.shape[1:]
    if h < 1 or w < 1:
        raise ValueError("seg_ce: h and w must be at least 1")
    s = H // h
    if H != s * h or W != s * w:
        raise ValueError(f"seg_ce: need H = s h and W = s w with one integer s, got {H} x {W} "
                         f"labels for {h} x {w} cells")
    if s % 2 or not 2 <= s <= _MAX_SCALE:
        raise ValueError(f"seg_ce: the scale must be even and in [2, {_MAX_SCALE}], got {s}")
    if Cp % 8 or not 0 < Cp <= _MAX_CP:
        raise ValueError(f"seg_ce: Cp must be a positive multiple of 8 and at most {_MAX_CP}, "
                         f"got {Cp}")
    if not 1 <= C <= min(Cp, SEG_MAX_CLASSES):
        raise ValueError(f"seg_ce: need 1 <= C <= min(Cp, {SEG_MAX_CLASSES}), got C = {C}, "
                         f"Cp = {Cp}")
    return s


def _axis_taps(n: int, s: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(y0, y1, wy) of the n*s pixels along an axis of n cells, in fp64."""
    y = torch.arange(n * s, device=device, dtype=torch.float64)
    sy = ((y + 0.5) / s - 0.5).clamp(min=0.0)
    y0 = sy.floor()
    return y0.long(), (y0.long() + 1).clamp(max=n - 1), sy - y0


def seg_ce_ref(logits: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor, C: int,
               grad_scale: Union[float, torch.Tensor], write_grad: bool = True
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Plain-torch `seg_ce`, computed in fp64 from the tap formulas (not through
    `F.interpolate`): the oracle of the kernel tests and the CPU path; not meant
    to be fast. It holds one image's upsampled logits, H W G C doubles, at a time."""
    s = _geometry(logits, labels, C)
    M, h, w, G, Cp = logits.shape
    dev = logits.device
    scale = float(grad_scale)
    y0, y1, wy = _axis_taps(h, s, dev)
    x0, x1, wx = _axis_taps(w, s, dev)
    wy, wx = wy.view(-1, 1, 1, 1), wx.view(1, -1, 1, 1)
    cols = torch.arange(C, device=dev)
    loss_sum = torch.zeros(G, device=dev, dtype=torch.float64)
    areas = torch.zeros((G, 3, Cp), device=dev, dtype=torch.int64)
    dbias = torch.zeros((G, C), device=dev, dtype=torch.float64)
    for m in range(M):
        L = logits[m, :, :, :, :C].double()  # [h, w, G, C]
        top_row = (1.0 - wx) * L[y0][:, x0] + wx * L[y0][:, x1]
        bot_row = (1.0 - wx) * L[y1][:, x0] + wx * L[y1][:, x1]
        z = (1.0 - wy) * top_row + wy * bot_row  # [H, W, G, C]
        if bias is not None:
            z = z + bias[:, :C].double()
        lab = labels[m].long()
        valid = lab != SEG_IGNORE
        target = torch.where(valid, lab, torch.zeros_like(lab))
        if bool(valid.any()) and int(target.max()) >= C:
            raise ValueError(f"seg_ce: labels must lie in [0, {C}) or be {SEG_IGNORE}")
        top = z.max(dim=3, keepdim=True).values
        lse = (z - top).exp().sum(dim=3).log() + top.squeeze(3)  # [H, W, G]
        onehot = (target.view(-1, 1) == cols).view(s * h, s * w, 1, C)
        picked = (z * onehot).sum(dim=3)
        loss_sum += ((lse - picked) * valid.unsqueeze(2)).sum(dim=(0, 1))
        # the lowest index among the maximal logits
        pred = torch.where(z == top, cols.expand_as(z), torch.full_like(cols, C).expand_as(z))
        pred = pred.min(dim=3).values  # [H, W, G]
        for g in range(G):
            pg, tg = pred[:, :, g][valid], target[valid]
            areas[g, 0, :C] += torch.bincount(tg[pg == tg], minlength=C)
            areas[g, 1, :C] += torch.bincount(pg, minlength=C)
            areas[g, 2, :C] += torch.bincount(tg, minlength=C)
        if write_grad:
            d = ((z - lse.unsqueeze(3)).exp() - onehot.double()) * valid.view(s * h, s * w, 1, 1)
            d = d * scale
            rows = torch.zeros((h, s * w, G, C), device=dev, dtype=torch.float64)
            rows.index_add_(0, y0, (1.0 - wy) * d)
            rows.index_add_(0, y1, wy * d)
            cells = torch.zeros((h, w, G, C), device=dev, dtype=torch.float64)
            cells.index_add_(1, x0, (1.0 - wx) * rows)
            cells.index_add_(1, x1, wx * rows)
            dbias += cells.sum(dim=(0, 1))
            logits[m, :, :, :, :C] = cells.to(logits.dtype)
            logits[m, :, :, :, C:] = 0
    if not write_grad:
        return loss_sum.float(), areas, None
    out_db = torch.zeros((G, Cp), device=dev, dtype=torch.float32)
    out_db[:, :C] = dbias.float()
    return loss_sum.float(), areas, out_db


def seg_ce(logits: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor, C: int,
           grad_scale: Union[float, torch.Tensor], write_grad: bool = True
           ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Per-pixel softmax cross-entropy of G linear segmentation heads at once.
    `logits` [M, h, w, G, Cp] (bf16 or fp32) are patch-resolution class scores,
    `bias` [G, Cp] fp32 or None, `labels` [M, H, W] uint8 with H = s h, W = s w
    for one even s in [2, 32]. The logits are upsampled exactly as
    `F.interpolate(mode="bilinear", align_corners=False)` does: along an axis
    pixel y has sy = max((y + 0.5) / s - 0.5, 0), y0 = floor(sy),
    y1 = min(y0 + 1, h - 1), wy = sy - y0, and

        z[c] = (1-wy) ((1-wx) L[y0,x0,c] + wx L[y0,x1,c])
               + wy ((1-wx) L[y1,x0,c] + wx L[y1,x1,c]) + bias[g,c]

    in fp32 over the columns c < C; the columns C..Cp-1 do not exist for the
    softmax. A pixel labelled 255 is ignored: no loss, no counts, no gradient.

    Returns (loss_sum [G] fp32: the sum over pixels of lse(z) - z[label];
    areas [G, 3, Cp] int64: per class the pixels with prediction = label = c,
    with prediction = c, with label = c, the prediction being the lowest index
    among the maximal z; dbias [G, Cp] fp32, or None without `write_grad`).

    With `write_grad` the logits are overwritten in place with the gradient with
    respect to them: for cell (i, j) and class c the sum over every pixel that
    has the cell as a tap of tap weight * (softmax(z)[c] - [c == label]) *
    grad_scale, summed in fp32 and rounded once to the logits dtype, 0 in the
    pad columns; dbias is the sum of those values over all cells before they are
    rounded. `grad_scale` is a float, or a one-element fp32 tensor on the
    logits' device (1 / valid pixels, computed there: no host synchronisation).

    1 <= C <= min(Cp, 255) = SEG_MAX_CLASSES, Cp % 8 == 0, Cp <= 256. Labels in
    [C, 255) are out of contract; no memory access depends on a label. On a HIP
    device the tensors are contiguous and logits and bias 16-byte aligned, the
    result is bit-identical from run to run, and with `write_grad` the call
    allocates a workspace of 16 fp32 values per logit, M h w 4 G Cp in all.
    """
    from . import hip_ops, use_hip

    if use_hip(logits):
        if isinstance(grad_scale, torch.Tensor):
            out = hip_ops().seg_ce(logits, bias, labels, int(C), 1.0, bool(write_grad), grad_scale)
        else:
            out = hip_ops().seg_ce(logits, bias, labels, int(C), float(grad_scale),
                                   bool(write_grad), None)
        return out[0], out[1], (out[2] if write_grad else None)
    return seg_ce_ref(logits, bias, labels, C, grad_scale, write_grad)

"""Gram anchoring loss (parity: dinov3_jax/loss/gram_loss.py:13-51, with the
in-place boolean assignment bug §8 B5 fixed via torch.where)."""

from __future__ import annotations

import os

import torch
import torch.nn as nn


def _fused_eligible(out: torch.Tensor, tgt: torch.Tensor) -> bool:
    """DINOV3_FUSED_GRAM=1 routes device bf16 inputs with D % 8 == 0 to
    ops.gram_loss (docs/KERNELS.md "Gram loss"); off by default until its
    end-to-end effect is measured (profiles/gram_loss.md)."""
    return (os.environ.get("DINOV3_FUSED_GRAM", "0") == "1"
            and out.is_cuda and tgt.is_cuda
            and out.dtype == torch.bfloat16 and tgt.dtype == torch.bfloat16
            and out.shape == tgt.shape and out.shape[-1] % 8 == 0)


class GramLoss(nn.Module):
    def __init__(self, apply_norm: bool = True, img_level: bool = True,
                 remove_neg: bool = True, remove_only_teacher_neg: bool = False):
        super().__init__()
        assert remove_neg != remove_only_teacher_neg
        self.apply_norm = apply_norm
        self.img_level = img_level
        self.remove_neg = remove_neg
        self.remove_only_teacher_neg = remove_only_teacher_neg

    def forward(self, output_feats: torch.Tensor, target_feats: torch.Tensor,
                img_level: bool = True) -> torch.Tensor:
        if _fused_eligible(output_feats, target_feats):
            from ..ops import gram_loss

            if img_level:
                assert output_feats.ndim == 3 and target_feats.ndim == 3
                shape = output_feats.shape
            else:  # one matrix over all tokens
                shape = (1, -1, output_feats.shape[-1])
            return gram_loss(output_feats.reshape(shape), target_feats.reshape(shape),
                             apply_norm=self.apply_norm, remove_neg=self.remove_neg,
                             remove_only_teacher_neg=self.remove_only_teacher_neg)
        out = output_feats.float()
        tgt = target_feats.float()
        if img_level:
            assert out.ndim == 3 and tgt.ndim == 3
        if self.apply_norm:
            tgt = tgt / tgt.norm(dim=-1, keepdim=True)
            out = out / out.norm(dim=-1, keepdim=True)
        if not img_level:
            tgt = tgt.reshape(-1, tgt.shape[-1])
            out = out.reshape(-1, out.shape[-1])
        target_sim = tgt @ tgt.transpose(-1, -2)
        student_sim = out @ out.transpose(-1, -2)
        if self.remove_neg:
            target_sim = torch.where(target_sim < 0, torch.zeros_like(target_sim), target_sim)
            student_sim = torch.where(student_sim < 0, torch.zeros_like(student_sim), student_sim)
        elif self.remove_only_teacher_neg:
            both_neg = (student_sim < 0) & (target_sim < 0)
            student_sim = torch.where(both_neg, torch.zeros_like(student_sim), student_sim)
            target_sim = torch.where(target_sim < 0, torch.zeros_like(target_sim), target_sim)
        return ((student_sim - target_sim) ** 2).mean()

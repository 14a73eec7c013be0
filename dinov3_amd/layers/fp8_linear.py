"""Opt-in FP8 forward for block linears (student.fp8_enabled).

`convert_linears_to_fp8` only sets an attribute ``fp8 = True`` on eligible
``nn.Linear`` modules: no parameter, buffer or class changes, so state_dict
keys and checkpoints are identical with and without it. The blocks route their
GEMMs through `linear_call` / `linear_op`, which run `ops.fp8_linear` on a
flagged module and otherwise make exactly the call they replaced.
"""

from __future__ import annotations

import logging
import re
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.fp8_linear import fp8_eligible, fp8_linear

logger = logging.getLogger("dinov3")

__all__ = ["convert_linears_to_fp8", "linear_call", "linear_op", "fp8_env_enabled"]


def fp8_env_enabled() -> bool:
    """DINOV3_FP8=1 turns the fp8 forward on without touching the config."""
    import os

    return os.environ.get("DINOV3_FP8", "0") == "1"


def linear_op(mod: nn.Module, x: torch.Tensor, weight: torch.Tensor,
              bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, weight, bias)`` for a GEMM owned by `mod`; e4m3 forward
    when `mod` is flagged."""
    if getattr(mod, "fp8", False):
        return fp8_linear(x, weight, bias)
    return F.linear(x, weight, bias)


def linear_call(mod: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """``mod(x)``; a flagged plain ``nn.Linear`` runs the e4m3 forward. A
    Linear subclass with its own forward (LinearKMaskedBias) builds its bias
    itself and goes through `linear_op` there."""
    if getattr(mod, "fp8", False) and type(mod) is nn.Linear:
        return fp8_linear(x, mod.weight, mod.bias)
    return mod(x)


def convert_linears_to_fp8(module: nn.Module, filter: str = "blocks") -> List[str]:
    """Flag every eligible ``nn.Linear`` under `module` whose qualified name
    matches `filter` (regex search). Returns the flagged names."""
    pattern = re.compile(filter)
    converted: List[str] = []
    skipped: List[str] = []
    for name, mod in module.named_modules():
        if not isinstance(mod, nn.Linear) or not pattern.search(name):
            continue
        if fp8_eligible(mod.in_features, mod.out_features):
            mod.fp8 = True
            converted.append(name)
        else:
            skipped.append(f"{name}[{mod.out_features}x{mod.in_features}]")
    logger.info("fp8 forward: %d linear layers converted (filter %r)", len(converted), filter)
    if skipped:
        logger.info("fp8 forward: %d matching layers stay bf16 (need in%%128==0, out%%16==0): %s",
                    len(skipped), ", ".join(skipped))
    return converted

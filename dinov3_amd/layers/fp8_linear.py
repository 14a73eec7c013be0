"""Opt-in FP8 for block linears (student.fp8_enabled, student.fp8_backward).

`convert_linears_to_fp8` only sets attributes on eligible ``nn.Linear``
modules (``fp8 = True``, and ``fp8_bwd = True`` when the fp8 backward is asked
for and the shape allows it): no parameter, buffer or class changes, so
state_dict keys and checkpoints are identical with and without it. The blocks
route their GEMMs through `linear_call` / `linear_op`, which run
`ops.fp8_linear` on a flagged module and otherwise make exactly the call they
replaced.
"""

from __future__ import annotations

import logging
import re
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.fp8_linear import fp8_bwd_eligible, fp8_eligible, fp8_linear

logger = logging.getLogger("dinov3")

__all__ = ["convert_linears_to_fp8", "linear_call", "linear_op", "fp8_env_enabled",
           "fp8_bwd_env_enabled"]


def fp8_env_enabled() -> bool:
    """DINOV3_FP8=1 turns the fp8 forward on without touching the config."""
    import os

    return os.environ.get("DINOV3_FP8", "0") == "1"


def fp8_bwd_env_enabled() -> bool:
    """DINOV3_FP8_BWD=1 turns the fp8 backward on (it needs the fp8 forward)."""
    import os

    return os.environ.get("DINOV3_FP8_BWD", "0") == "1"


def _backward_mode(mod: nn.Module) -> str:
    return "fp8" if getattr(mod, "fp8_bwd", False) else "bf16"


def linear_op(mod: nn.Module, x: torch.Tensor, weight: torch.Tensor,
              bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, weight, bias)`` for a GEMM owned by `mod`; e4m3 forward
    when `mod` is flagged, fp8 backward when it is flagged for that too."""
    if getattr(mod, "fp8", False):
        return fp8_linear(x, weight, bias, backward=_backward_mode(mod))
    return F.linear(x, weight, bias)


def linear_call(mod: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """``mod(x)``; a flagged plain ``nn.Linear`` runs the e4m3 forward. A
    Linear subclass with its own forward (LinearKMaskedBias) builds its bias
    itself and goes through `linear_op` there."""
    if getattr(mod, "fp8", False) and type(mod) is nn.Linear:
        return fp8_linear(x, mod.weight, mod.bias, backward=_backward_mode(mod))
    return mod(x)


def convert_linears_to_fp8(module: nn.Module, filter: str = "blocks",
                           backward: bool = False) -> List[str]:
    """Flag every eligible ``nn.Linear`` under `module` whose qualified name
    matches `filter` (regex search). With `backward`, flagged layers whose
    in and out features are both multiples of 128 also get ``fp8_bwd = True``;
    the others keep the straight-through backward. Returns the flagged names."""
    pattern = re.compile(filter)
    converted: List[str] = []
    skipped: List[str] = []
    bwd_converted: List[str] = []
    bwd_skipped: List[str] = []
    for name, mod in module.named_modules():
        if not isinstance(mod, nn.Linear) or not pattern.search(name):
            continue
        if fp8_eligible(mod.in_features, mod.out_features):
            mod.fp8 = True
            converted.append(name)
            if backward:
                if fp8_bwd_eligible(mod.in_features, mod.out_features):
                    mod.fp8_bwd = True
                    bwd_converted.append(name)
                else:
                    bwd_skipped.append(f"{name}[{mod.out_features}x{mod.in_features}]")
        else:
            skipped.append(f"{name}[{mod.out_features}x{mod.in_features}]")
    logger.info("fp8 forward: %d linear layers converted (filter %r)", len(converted), filter)
    if skipped:
        logger.info("fp8 forward: %d matching layers stay bf16 (need in%%128==0, out%%16==0): %s",
                    len(skipped), ", ".join(skipped))
    if backward:
        logger.info("fp8 backward: %d linear layers converted", len(bwd_converted))
        if bwd_skipped:
            logger.info("fp8 backward: %d fp8 layers keep the bf16 backward "
                        "(need in%%128==0, out%%128==0): %s",
                        len(bwd_skipped), ", ".join(bwd_skipped))
    return converted

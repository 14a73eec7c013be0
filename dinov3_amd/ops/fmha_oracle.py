"""fp64 oracle, elementwise rounding bounds and test-case generators for the
fused RoPE + attention kernels (csrc/fmha_rope.hip).

Pure torch on the CPU; nothing here touches the HIP extension. Everything works
per crop group on ``qkv [B, N, 3, H, hd]`` with ``sin``/``cos`` tables of shape
``[N - prefix, hd]`` (or ``None`` for no RoPE) — the arguments of
``fmha_rope_fwd``. Token-major tensors (``o``, ``dO``, ``dq``/``dk``/``dv`` and
their bounds) are ``[B, N, H, hd]``; ``lse`` is ``[B, H, N]``; ``p`` and the
roped ``q_hat``/``k_hat`` are head-major ``[B, H, N, ...]``.

The oracle follows the kernels only where they *define* the result:

- RoPE has ops/rope.py semantics (rotate-half, rows >= prefix) in fp64 and is
  then rounded to bf16, because the kernels stage the roped q/k as bf16 MFMA
  operands. That rounding is part of the operation, not an error.
- the softmax scale is the fp32 value ``1/sqrt(hd)`` the bindings pass.

Everything else is fp64 and unrounded. Every further rounding step of the
kernels is one term of a bound below, written next to the formula it perturbs.

Bound conventions: one bf16 round-to-nearest-even is ``2^-9`` relative; one
fp32 dot product of length ``hd`` is ``hd * 2^-24`` relative to the dot product
of the absolute values. Every term is doubled because the summation order
inside an MFMA is undocumented (tests/test_fp8_gpu.py
``test_gemm_random_within_rounding_bound`` does the same).

The q/k/v entry points ``fmha_fwd``/``fmha_bwd`` run the same kernels through
their plain ``[B, H, N, hd]`` memory layout, without RoPE: use the same oracle
and bounds with ``sin = cos = None``.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

BF16_RNE = 2.0 ** -9      # one bf16 round-to-nearest-even, relative
FP32_ULP = 2.0 ** -24     # one fp32 rounding, relative
# __expf/__logf intrinsics (exp2/log2 hardware ops of ~1 ulp plus one fp32
# multiply by log2(e) / ln 2 on arguments of magnitude < 2^7) and the fp32
# accumulation of up to 257 probabilities <= 1: argued from how the intrinsics
# are built, not measured. May be raised up to LSE_CONST_MAX only.
LSE_CONST = 2.0 ** -14
# 8x under log(258/257), the smallest shift one lost key causes at N = 257
LSE_CONST_MAX = 2.0 ** -11


def softmax_scale(hd: int) -> float:
    """The fp32 value of 1/sqrt(hd) the bindings compute, as a python float."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())


def _heads(x: torch.Tensor) -> torch.Tensor:
    """token-major [B, N, H, hd] <-> head-major [B, H, N, hd]."""
    return x.permute(0, 2, 1, 3)


def rope_fp64(x: torch.Tensor, sin: Optional[torch.Tensor], cos: Optional[torch.Tensor],
              prefix: int) -> torch.Tensor:
    """ops/rope.py semantics in fp64, unrounded. x: [B, H, N, hd]."""
    x = x.double()
    if sin is None:
        return x
    half = x.shape[-1] // 2
    tail = x[..., prefix:, :]
    rot = torch.cat([-tail[..., half:], tail[..., :half]], dim=-1)
    return torch.cat([x[..., :prefix, :], tail * cos.double() + rot * sin.double()], dim=-2)


def rope_inverse_fp64(g: torch.Tensor, sin: Optional[torch.Tensor], cos: Optional[torch.Tensor],
                      prefix: int) -> torch.Tensor:
    """Gradient of rope_fp64 w.r.t. its input: g*cos + rot^-1(g*sin), rows >= prefix."""
    if sin is None:
        return g
    half = g.shape[-1] // 2
    tail = g[..., prefix:, :]
    gs = tail * sin.double()
    back = torch.cat([gs[..., half:], -gs[..., :half]], dim=-1)
    return torch.cat([g[..., :prefix, :], tail * cos.double() + back], dim=-2)


def _rope_mix_abs(x: torch.Tensor, sin: Optional[torch.Tensor], cos: Optional[torch.Tensor],
                  prefix: int) -> torch.Tensor:
    """R of the bounds: how an elementwise error bound passes through the
    inverse-RoPE epilogue — each half picks up |cos| of itself and |sin| of the
    other half, rows >= prefix only."""
    if sin is None:
        return x
    half = x.shape[-1] // 2
    tail = x[..., prefix:, :]
    xs = tail * sin.double().abs()
    mixed = tail * cos.double().abs() + torch.cat([xs[..., half:], xs[..., :half]], dim=-1)
    return torch.cat([x[..., :prefix, :], mixed], dim=-2)


def _to_bf16_grid(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).double()


@dataclass
class OracleForward:
    o: torch.Tensor       # [B, N, H, hd] fp64, unrounded
    lse: torch.Tensor     # [B, H, N]
    p: torch.Tensor       # [B, H, N, N]
    q_hat: torch.Tensor   # [B, H, N, hd] roped q on the bf16 grid
    k_hat: torch.Tensor   # [B, H, N, hd]
    v: torch.Tensor       # [B, H, N, hd]
    scale: float
    sin: Optional[torch.Tensor]
    cos: Optional[torch.Tensor]
    prefix: int


def oracle_forward(qkv: torch.Tensor, sin: Optional[torch.Tensor], cos: Optional[torch.Tensor],
                   prefix: int) -> OracleForward:
    B, N, three, H, hd = qkv.shape
    assert three == 3
    q, k, v = qkv.detach().cpu().double().permute(2, 0, 3, 1, 4).unbind(0)  # [B, H, N, hd]
    if sin is not None:
        sin, cos = sin.detach().cpu(), cos.detach().cpu()
        assert sin.shape == (N - prefix, hd) and cos.shape == sin.shape
    q_hat = _to_bf16_grid(rope_fp64(q, sin, cos, prefix))
    k_hat = _to_bf16_grid(rope_fp64(k, sin, cos, prefix))
    scale = softmax_scale(hd)
    s = (q_hat @ k_hat.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    return OracleForward(_heads(o).contiguous(), lse, p, q_hat, k_hat, v.contiguous(), scale,
                         sin, cos, prefix)


def oracle_backward(fwd: OracleForward, dO: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dq, dk, dv [B, N, H, hd] fp64 for the upstream gradient dO [B, N, H, hd]."""
    do = _heads(dO.detach().cpu().double())
    o = _heads(fwd.o)
    D = (do * o).sum(-1)                                   # unrounded o
    dP = do @ fwd.v.transpose(-1, -2)
    ds = fwd.p * (dP - D[..., None]) * fwd.scale
    dq = rope_inverse_fp64(ds @ fwd.k_hat, fwd.sin, fwd.cos, fwd.prefix)
    dk = rope_inverse_fp64(ds.transpose(-1, -2) @ fwd.q_hat, fwd.sin, fwd.cos, fwd.prefix)
    dv = fwd.p.transpose(-1, -2) @ do
    return _heads(dq).contiguous(), _heads(dk).contiguous(), _heads(dv).contiguous()


# ---------------------------------------------------------------------------
# elementwise bounds
# ---------------------------------------------------------------------------

def _abs_scores(fwd: OracleForward) -> torch.Tensor:
    """|q_hat| @ |k_hat|^T * scale: what one fp32 score rounding is relative to."""
    return (fwd.q_hat.abs() @ fwd.k_hat.abs().transpose(-1, -2)) * fwd.scale


def forward_bounds(fwd: OracleForward) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bound_o [B, N, H, hd], bound_lse [B, H, N])."""
    hd = fwd.v.shape[-1]
    absv = fwd.v.abs()
    A = _abs_scores(fwd)
    o = _heads(fwd.o)
    # o = (sum_j bf16(p_j) v_j) / l, stored as bf16
    bound_o = (
        2 * 2 * BF16_RNE * o.abs()                     # bf16 store of o, and as much again for the fp32
                                                       # alpha rescales and the 1/l normalisation under it
        + 2 * BF16_RNE * (fwd.p @ absv)                # P rounded to bf16 before the PV MFMA
        + 2 * 2 * hd * FP32_ULP * ((fwd.p * A) @ absv)  # fp32 accumulation of s_ij: moves p_ij and l
    )
    # lse = m + log(sum_j exp(s_j - m))
    bound_lse = (
        2 * hd * FP32_ULP * A.amax(dim=-1)             # fp32 accumulation of the scores
        + LSE_CONST                                    # __expf/__logf and the fp32 sum over keys
        + 2 * 2 * FP32_ULP * fwd.lse.abs()             # fp32 s*scale and m + log(l)
    )
    return _heads(bound_o).contiguous(), bound_lse


def backward_bounds(fwd: OracleForward, dO: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(bound_dq, bound_dk, bound_dv), each [B, N, H, hd]."""
    hd = fwd.v.shape[-1]
    do = _heads(dO.detach().cpu().double())
    o = _heads(fwd.o)
    absdo = do.abs()
    bound_o, _ = forward_bounds(fwd)
    A = _abs_scores(fwd)
    # D_i = sum_d dO_id * bf16(o_id): the pre-pass reads the bf16 o
    dD = (absdo * _heads(bound_o)).sum(-1)
    D = (do * o).sum(-1)
    dP = do @ fwd.v.transpose(-1, -2)
    dPmD = dP - D[..., None]
    ds = fwd.p * dPmD * fwd.scale
    # ds_ij = p_ij (dP_ij - D_i) scale, rounded to bf16 before the dq/dk MFMAs
    E = (
        2 * BF16_RNE * ds.abs()                                    # bf16 ds
        + fwd.scale * fwd.p * dD[..., None]                        # D from the bf16 o
        + 2 * 2 * hd * FP32_ULP * fwd.scale * fwd.p * (
            absdo @ fwd.v.abs().transpose(-1, -2)                  # fp32 accumulation of dP_ij
            + dPmD.abs() * A                                       # fp32 accumulation of s_ij inside p_ij
        )
    )
    dq, dk, dv = (_heads(g) for g in oracle_backward(fwd, dO))
    out_rne = 2 * 2 * BF16_RNE     # bf16 store of each gradient, and as much for its fp32 accumulation
    bound_dq = _rope_mix_abs(E @ fwd.k_hat.abs(), fwd.sin, fwd.cos, fwd.prefix) + out_rne * dq.abs()
    bound_dk = (_rope_mix_abs(E.transpose(-1, -2) @ fwd.q_hat.abs(), fwd.sin, fwd.cos, fwd.prefix)
                + out_rne * dk.abs())
    # dv_j = sum_i bf16(p_ij) dO_i
    bound_dv = 2 * BF16_RNE * (fwd.p.transpose(-1, -2) @ absdo) + out_rne * dv.abs()
    return (_heads(bound_dq).contiguous(), _heads(bound_dk).contiguous(),
            _heads(bound_dv).contiguous())


def worst_ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err/bound; inf if an element errs where the bound is zero or is NaN
    (so an unwritten NaN row never passes)."""
    err, bound = err.double(), bound.double()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, math.inf))
    ratio = torch.where(torch.isnan(ratio), math.inf, ratio)
    return float(ratio.max())


# ---------------------------------------------------------------------------
# case generators
# ---------------------------------------------------------------------------

@dataclass
class Case:
    qkv: torch.Tensor                 # [B, N, 3, H, hd] bf16
    sin: Optional[torch.Tensor]       # [N - prefix, hd] fp32 or None
    cos: Optional[torch.Tensor]
    prefix: int
    dO: torch.Tensor                  # [B, N, H, hd] bf16
    perm: Optional[torch.Tensor] = None   # one-hot cases: [B, H, N], query i attends key perm[i]
    lse_exact: Optional[float] = None     # one-hot cases: the fp32 value every lse equals


def _fewbit(shape, gain: float, g: torch.Generator) -> torch.Tensor:
    return (gain * 8 * torch.randn(shape, generator=g, dtype=torch.float64)).round().clamp(-32, 32) / 8


def _fewbit_tables(P: int, hd: int, g: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """Multiples of 1/4 in [-1, 1]; both halves of a table identical. The
    kernels read only the first half of each table row (columns < hd/2) for
    both halves of the head dim, so a table whose halves differ would be
    applied differently by kernel and ops/rope.py — not a case the model
    produces, and not one these generators make."""
    def one():
        t = torch.randint(-4, 5, (P, hd // 2), generator=g).float() / 4
        return torch.cat([t, t], dim=-1).contiguous()
    return one(), one()


def _assert_rope_exact_in_fp32(case: Case) -> None:
    for which in (0, 1):
        x = case.qkv[:, :, which].double().permute(0, 2, 1, 3)
        y = rope_fp64(x, case.sin, case.cos, case.prefix)
        assert torch.equal(y.float().double(), y), "roped operand is not exact in fp32"


def fewbit_case(B: int, N: int, H: int, hd: int, prefix: int, gain: float, seed: int,
                rope: bool = True) -> Case:
    """q, k, v, dO = round(gain*8*randn).clamp(+-32)/8; tables are multiples
    of 1/4 (not unit rotations — the kernel applies whatever it is given).
    With <= 6-bit operands and 3-bit table entries every RoPE product and sum
    is exact in fp32, so the bf16 rounding of the roped q/k is the same in
    kernel and oracle whatever the FMA contraction; asserted here."""
    g = torch.Generator().manual_seed(seed)
    qkv = _fewbit((B, N, 3, H, hd), gain, g).to(torch.bfloat16)
    dO = _fewbit((B, N, H, hd), gain, g).to(torch.bfloat16)
    sin, cos = _fewbit_tables(N - prefix, hd, g) if rope else (None, None)
    case = Case(qkv, sin, cos, prefix, dO)
    _assert_rope_exact_in_fp32(case)
    return case


def onehot_case(B: int, N: int, H: int, hd: int, prefix: int, seed: int, rope: bool = True) -> Case:
    """Planted one-hot softmax. The roped keys are distinct +-1 codes, the
    roped query i is c * code[perm[i]] (c = 64 for hd 64, 32 for hd 128), the
    tables hold quarter turns (entries in {0, +-1}) and q/k are the exact
    pre-images. Every non-maximal score is >= 110 below the row maximum
    (asserted on the oracle), so its exp is exactly 0 in fp32: o = v[perm],
    lse = (c*hd)*scale, dv = dO scattered by perm and dq = dk = 0, all exactly."""
    g = torch.Generator().manual_seed(seed)
    c = 64.0 if hd == 64 else 32.0
    half = hd // 2
    k_hat = torch.randint(0, 2, (B, H, N, hd), generator=g).double() * 2 - 1
    perm = torch.argsort(torch.rand(B, H, N, generator=g), dim=-1)
    q_hat = c * torch.gather(k_hat, 2, perm[..., None].expand(-1, -1, -1, hd))
    if rope:
        turn = torch.randint(0, 4, (N - prefix, half), generator=g)
        cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
        sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
        sin = torch.cat([sin, sin], dim=-1).contiguous()
        cos = torch.cat([cos, cos], dim=-1).contiguous()
        # a quarter turn is orthogonal: the pre-image is the transposed turn
        q = rope_inverse_fp64(q_hat, sin, cos, prefix)
        k = rope_inverse_fp64(k_hat, sin, cos, prefix)
    else:
        sin = cos = None
        q, k = q_hat, k_hat
    v = torch.randint(-8, 9, (B, H, N, hd), generator=g).double()
    dO = torch.randint(-8, 9, (B, N, H, hd), generator=g).to(torch.bfloat16)
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).contiguous().to(torch.bfloat16)
    scale32 = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt()
    lse_exact = float(torch.tensor(c * hd, dtype=torch.float32) * scale32)
    case = Case(qkv, sin, cos, prefix, dO, perm, lse_exact)

    fwd = oracle_forward(qkv, sin, cos, prefix)
    assert torch.equal(fwd.q_hat, q_hat) and torch.equal(fwd.k_hat, k_hat)
    s = (fwd.q_hat @ fwd.k_hat.transpose(-1, -2)) * fwd.scale
    top2 = s.topk(2, dim=-1)
    assert torch.equal(top2.indices[..., 0], perm)
    assert float((top2.values[..., 0] - top2.values[..., 1]).min()) >= 110.0
    return case


def uniform_case(B: int, N: int, H: int, hd: int, prefix: int, seed: int, rope: bool = True) -> Case:
    """q = 0, few-bit k, integer v in [-8, 8]: every score is 0, so p = 1
    exactly for every key, o = mean_j v_j and lse = log N."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(B, N, 3, H, hd, dtype=torch.float64)
    qkv[:, :, 1] = _fewbit((B, N, H, hd), 1.0, g)
    qkv[:, :, 2] = torch.randint(-8, 9, (B, N, H, hd), generator=g).double()
    dO = _fewbit((B, N, H, hd), 1.0, g).to(torch.bfloat16)
    sin, cos = _fewbit_tables(N - prefix, hd, g) if rope else (None, None)
    return Case(qkv.to(torch.bfloat16), sin, cos, prefix, dO)


# (N, hd, prefix, rope): the smallest sizes that reach every edge of the
# kernels — a partial 32-key MFMA tile (8, 33), the N = 64 -> 65 switch from
# the 128-thread to the 256-thread kernels, a second and third 128-row q block
# holding one row (129, 257), a key super-tile holding one key (129 where the
# super-tile is 128 keys, 257), and the workload's own 197. prefix varies over
# {0, 1, 5}; one shape per head dim runs without RoPE.
EDGE_SHAPES = [
    (8, 64, 5, True), (33, 64, 1, True), (64, 64, 0, True), (65, 64, 1, True),
    (129, 64, 5, True), (197, 64, 5, True), (257, 64, 0, True), (129, 64, 0, False),
    (8, 128, 1, True), (33, 128, 0, True), (64, 128, 5, True), (65, 128, 5, True),
    (129, 128, 0, True), (197, 128, 1, True), (257, 128, 1, True), (33, 128, 0, False),
]
FEWBIT_GAINS = (0.5, 1.0, 2.0)

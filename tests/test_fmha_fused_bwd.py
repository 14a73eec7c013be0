"""CPU check of the single-pass attention backward's rounding order
(fmha_rope::bwd_fused_kernel) against the fp64 oracle's derived bounds.

An fp32 torch emulation of what the fused kernel does differently from the
three-launch path — P and dS rounded to bf16 once and used for dV, dK and dQ,
dQ formed as one fp32 partial per 32-key tile and the partials added in
key-tile order, D from the bf16 o — must stay inside fo.backward_bounds at the
shapes the GPU test (tests/test_fmha_fused_bwd_gpu.py) uses, and the same
emulation with the last key tile's partial lost, or the last query row lost
from dK/dV, must violate a bound at every one of them.
Run with -s to see the worst err/bound of every case.
"""

import functools

import pytest
import torch

from dinov3_amd.ops import fmha_oracle as fo

B, H = 2, 3
# (N, hd, prefix, rope): 37 the workload's local crop (a partly filled second
# tile), 96 three full tiles, 197 the global crop, 224 seven full tiles and an
# idle eighth wave, 225 one row in the eighth tile, 256 the upper limit
FUSED_SHAPES = [
    (37, 64, 1, True), (96, 64, 5, True), (197, 64, 1, True), (224, 64, 1, True),
    (225, 64, 5, True), (256, 64, 0, True), (256, 64, 1, False),
]
SHAPE_IDS = [f"N{n}-hd{hd}-p{p}-{'rope' if r else 'norope'}" for n, hd, p, r in FUSED_SHAPES]
KEY_TILE = 32


def _rope32(x, sin, cos, prefix):
    if sin is None:
        return x
    half = x.shape[-1] // 2
    tail = x[..., prefix:, :]
    rot = torch.cat([-tail[..., half:], tail[..., :half]], dim=-1)
    return torch.cat([x[..., :prefix, :], tail * cos + rot * sin], dim=-2)


def _rope32_inverse(g, sin, cos, prefix):
    if sin is None:
        return g
    half = g.shape[-1] // 2
    tail = g[..., prefix:, :]
    gs = tail * sin
    back = torch.cat([gs[..., half:], -gs[..., :half]], dim=-1)
    return torch.cat([g[..., :prefix, :], tail * cos + back], dim=-2)


def _bf16(x):
    return x.to(torch.bfloat16).float()


def _staged(case):
    q, k, v = case.qkv.float().permute(2, 0, 3, 1, 4).unbind(0)
    q_hat = _bf16(_rope32(q, case.sin, case.cos, case.prefix))
    k_hat = _bf16(_rope32(k, case.sin, case.cos, case.prefix))
    scale = torch.tensor(fo.softmax_scale(q.shape[-1]), dtype=torch.float32)
    return q_hat, k_hat, v, scale


def emu_forward(case):
    """The forward kernel's arithmetic: tiled online softmax in fp32, bf16 P,
    bf16 o. Returns o [B, H, N, hd] bf16 and lse [B, H, N] fp32."""
    q_hat, k_hat, v, scale = _staged(case)
    Bb, Hh, N, hd = v.shape
    m = torch.full((Bb, Hh, N), float("-inf"))
    l = torch.zeros(Bb, Hh, N)
    acc = torch.zeros(Bb, Hh, N, hd)
    for k0 in range(0, N, KEY_TILE):
        s = (q_hat @ k_hat[..., k0:k0 + KEY_TILE, :].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + _bf16(p) @ v[..., k0:k0 + KEY_TILE, :]
        m = m_new
    return (acc * (1.0 / l)[..., None]).to(torch.bfloat16), m + torch.log(l)


def emu_fused_backward(case, o, lse, drop_last_partial=False, drop_last_q_row=False):
    """dq, dk, dv [B, N, H, hd] bf16 in the fused kernel's rounding order."""
    q_hat, k_hat, v, scale = _staged(case)
    N = v.shape[-2]
    do = case.dO.float().permute(0, 2, 1, 3)
    D = (do * o.float()).sum(-1)                                   # from the bf16 o
    p = torch.exp((q_hat @ k_hat.transpose(-1, -2)) * scale - lse[..., None])
    ds = p * (do @ v.transpose(-1, -2) - D[..., None]) * scale
    ds_b, p_b = _bf16(ds), _bf16(p)                                # rounded once, used three times
    tiles = list(range(0, N, KEY_TILE))
    if drop_last_partial:
        tiles = tiles[:-1]
    dq = torch.zeros_like(q_hat)
    for k0 in tiles:                                               # fp32 partials in key-tile order
        dq = dq + ds_b[..., k0:k0 + KEY_TILE] @ k_hat[..., k0:k0 + KEY_TILE, :]
    if drop_last_q_row:
        ds_b, p_b = ds_b.clone(), p_b.clone()
        ds_b[..., N - 1, :] = 0
        p_b[..., N - 1, :] = 0
    dk = ds_b.transpose(-1, -2) @ q_hat
    dv = p_b.transpose(-1, -2) @ do
    dq = _rope32_inverse(dq, case.sin, case.cos, case.prefix)
    dk = _rope32_inverse(dk, case.sin, case.cos, case.prefix)
    return tuple(g.to(torch.bfloat16).permute(0, 2, 1, 3).contiguous() for g in (dq, dk, dv))


@functools.lru_cache(maxsize=None)
def _ref(shape_idx, gain):
    """case, oracle gradients, bounds and the emulated forward: computed once, never modified."""
    N, hd, prefix, rope = FUSED_SHAPES[shape_idx]
    case = fo.fewbit_case(B, N, H, hd, prefix, gain, seed=7000 + 1000 * shape_idx + int(gain * 10),
                          rope=rope)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    return (case, fo.oracle_backward(fwd, case.dO), fo.backward_bounds(fwd, case.dO),
            emu_forward(case))


def _ratios(ref, grads):
    _, ref_grads, bounds, _ = ref
    return {name: fo.worst_ratio((g.double() - r).abs(), b)
            for name, g, r, b in zip(("dq", "dk", "dv"), grads, ref_grads, bounds)}


@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape_idx", range(len(FUSED_SHAPES)), ids=SHAPE_IDS)
def test_fused_order_within_bounds(shape_idx, gain):
    ref = _ref(shape_idx, gain)
    ratios = _ratios(ref, emu_fused_backward(ref[0], *ref[3]))
    print(f"\n  fused emulation err/bound {SHAPE_IDS[shape_idx]} gain {gain}: "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape_idx", range(len(FUSED_SHAPES)), ids=SHAPE_IDS)
def test_lost_partial_or_row_violates_a_bound(shape_idx, gain):
    ref = _ref(shape_idx, gain)
    lost_partial = _ratios(ref, emu_fused_backward(ref[0], *ref[3], drop_last_partial=True))
    lost_row = _ratios(ref, emu_fused_backward(ref[0], *ref[3], drop_last_q_row=True))
    print(f"\n  planted err/bound {SHAPE_IDS[shape_idx]} gain {gain}: "
          f"lost partial dq={lost_partial['dq']:.1f}  "
          f"lost row dk={lost_row['dk']:.1f} dv={lost_row['dv']:.1f}")
    assert lost_partial["dq"] > 1.0, lost_partial
    assert lost_partial["dk"] <= 1.0 and lost_partial["dv"] <= 1.0, "dK/dV do not read the dQ partials"
    assert lost_row["dq"] <= 1.0, "dQ does not read the dK/dV accumulators"
    assert max(lost_row["dk"], lost_row["dv"]) > 1.0, lost_row

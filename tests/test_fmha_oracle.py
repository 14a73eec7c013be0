"""CPU checks of the attention oracle (dinov3_amd/ops/fmha_oracle.py).

A torch emulator of the kernels' arithmetic — tiled online softmax in fp32,
bf16 P, bf16 O; backward with p from lse, D from the bf16 O, bf16 dS and P —
must satisfy every bound at every shape the GPU tests use, and the same
emulator with one planted indexing error must violate at least one. That is
what makes the bounds in tests/test_fmha_exact_gpu.py mean something: loose
enough for a correct kernel, tight enough to catch one lost key or row.
"""

import functools

import pytest
import torch

from dinov3_amd.ops import fmha_oracle as fo

B, H = 2, 3
SHAPE_IDS = [f"N{n}-hd{hd}-p{p}-{'rope' if r else 'norope'}" for n, hd, p, r in fo.EDGE_SHAPES]


# ---------------------------------------------------------------------------
# emulator of the kernels' arithmetic (test helper)
# ---------------------------------------------------------------------------

def _rope32(x, sin, cos, prefix):
    if sin is None:
        return x
    half = x.shape[-1] // 2
    tail = x[..., prefix:, :]
    rot = torch.cat([-tail[..., half:], tail[..., :half]], dim=-1)
    return torch.cat([x[..., :prefix, :], tail * cos + rot * sin], dim=-2)


def _rope32_inverse(g, sin, cos, first_row):
    if sin is None:
        return g
    half = g.shape[-1] // 2
    P = g.shape[-2] - first_row
    sin, cos = sin[sin.shape[0] - P:], cos[cos.shape[0] - P:]
    tail = g[..., first_row:, :]
    gs = tail * sin
    back = torch.cat([gs[..., half:], -gs[..., :half]], dim=-1)
    return torch.cat([g[..., :first_row, :], tail * cos + back], dim=-2)


def _bf16(x):
    return x.to(torch.bfloat16).float()


def _staged(case):
    q, k, v = case.qkv.float().permute(2, 0, 3, 1, 4).unbind(0)
    q_hat = _bf16(_rope32(q, case.sin, case.cos, case.prefix))
    k_hat = _bf16(_rope32(k, case.sin, case.cos, case.prefix))
    scale = torch.tensor(fo.softmax_scale(q.shape[-1]), dtype=torch.float32)
    return q_hat, k_hat, v, scale


def emu_forward(case, drop_key=None, tile=32):
    """o [B, N, H, hd] bf16, lse [B, H, N] fp32. drop_key masks one key out."""
    q_hat, k_hat, v, scale = _staged(case)
    Bb, Hh, N, hd = v.shape
    m = torch.full((Bb, Hh, N), float("-inf"))
    l = torch.zeros(Bb, Hh, N)
    acc = torch.zeros(Bb, Hh, N, hd)
    for k0 in range(0, N, tile):
        s = (q_hat @ k_hat[..., k0:k0 + tile, :].transpose(-1, -2)) * scale
        if drop_key is not None and k0 <= drop_key < k0 + tile:
            s[..., drop_key - k0] = float("-inf")
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + _bf16(p) @ v[..., k0:k0 + tile, :]
        m = m_new
    o = (acc * (1.0 / l)[..., None]).to(torch.bfloat16)
    return o.permute(0, 2, 1, 3).contiguous(), m + torch.log(l)


def emu_backward(case, o, lse, skip_q_row=None, inv_rope_shift=0):
    """dq, dk, dv [B, N, H, hd] bf16 from the emulator's own bf16 o and lse.
    skip_q_row leaves one query row out of dK/dV; inv_rope_shift moves the
    first inverse-rotated row off `prefix`."""
    q_hat, k_hat, v, scale = _staged(case)
    do = case.dO.float().permute(0, 2, 1, 3)
    p = torch.exp((q_hat @ k_hat.transpose(-1, -2)) * scale - lse[..., None])
    D = (do * o.float().permute(0, 2, 1, 3)).sum(-1)
    ds = p * (do @ v.transpose(-1, -2) - D[..., None]) * scale
    ds_b, p_b = _bf16(ds), _bf16(p)
    dq = ds_b @ k_hat
    if skip_q_row is not None:
        ds_b, p_b = ds_b.clone(), p_b.clone()
        ds_b[..., skip_q_row, :] = 0
        p_b[..., skip_q_row, :] = 0
    dk = ds_b.transpose(-1, -2) @ q_hat
    dv = p_b.transpose(-1, -2) @ do
    first = case.prefix + inv_rope_shift
    dq = _rope32_inverse(dq, case.sin, case.cos, first)
    dk = _rope32_inverse(dk, case.sin, case.cos, first)
    return tuple(g.to(torch.bfloat16).permute(0, 2, 1, 3).contiguous() for g in (dq, dk, dv))


# ---------------------------------------------------------------------------
# shared references: computed once, never modified
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fewbit(shape_idx, gain):
    N, hd, prefix, rope = fo.EDGE_SHAPES[shape_idx]
    case = fo.fewbit_case(B, N, H, hd, prefix, gain, seed=1000 * shape_idx + int(gain * 10), rope=rope)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    grads = fo.oracle_backward(fwd, case.dO)
    return case, fwd, grads, fo.forward_bounds(fwd), fo.backward_bounds(fwd, case.dO)


def _fwd_ratios(ref, o, lse):
    _, fwd, _, (bound_o, bound_lse), _ = ref
    return {"o": fo.worst_ratio((o.double() - fwd.o).abs(), bound_o),
            "lse": fo.worst_ratio((lse.double() - fwd.lse).abs(), bound_lse)}


def _bwd_ratios(ref, grads):
    _, _, ref_grads, _, bounds = ref
    return {name: fo.worst_ratio((g.double() - r).abs(), b)
            for name, g, r, b in zip(("dq", "dk", "dv"), grads, ref_grads, bounds)}


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape_idx", range(len(fo.EDGE_SHAPES)), ids=SHAPE_IDS)
def test_emulator_within_bounds(shape_idx, gain):
    ref = _fewbit(shape_idx, gain)
    o, lse = emu_forward(ref[0])
    ratios = _fwd_ratios(ref, o, lse)
    ratios.update(_bwd_ratios(ref, emu_backward(ref[0], o, lse)))
    print(f"\n  emulator err/bound {SHAPE_IDS[shape_idx]} gain {gain}: "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("shape_idx", range(len(fo.EDGE_SHAPES)), ids=SHAPE_IDS)
def test_planted_errors_violate_a_bound(shape_idx):
    """Gain 0.5: the flat softmax, where a lost key or row is hardest to see."""
    N, hd, prefix, rope = fo.EDGE_SHAPES[shape_idx]
    ref = _fewbit(shape_idx, 0.5)
    case = ref[0]
    o, lse = emu_forward(case)
    report = {}
    for key in sorted({0, prefix, N - 1, N // 2}):
        worst = max(_fwd_ratios(ref, *emu_forward(case, drop_key=key)).values())
        report[f"drop_key{key}"] = worst
    dq, dk, dv = emu_backward(case, o, lse, skip_q_row=N // 2)
    r = _bwd_ratios(ref, (dq, dk, dv))
    assert r["dq"] <= 1.0, "skipping a q row in dK/dV must leave dQ alone"
    report["skip_q_row"] = max(r["dk"], r["dv"])
    if rope:
        r = _bwd_ratios(ref, emu_backward(case, o, lse, inv_rope_shift=1))
        assert r["dv"] <= 1.0
        report["inv_rope_prefix+1"] = max(r["dq"], r["dk"])
    print(f"\n  planted err/bound {SHAPE_IDS[shape_idx]}: "
          + " ".join(f"{k}={v:.1f}" for k, v in report.items()))
    assert all(v > 1.0 for v in report.values()), report


@pytest.mark.parametrize("shape_idx", range(len(fo.EDGE_SHAPES)), ids=SHAPE_IDS)
def test_emulator_onehot_bit_exact(shape_idx):
    N, hd, prefix, rope = fo.EDGE_SHAPES[shape_idx]
    case = fo.onehot_case(B, N, H, hd, prefix, seed=77 + shape_idx, rope=rope)
    o, lse = emu_forward(case)
    v = case.qkv[:, :, 2].permute(0, 2, 1, 3)                            # [B, H, N, hd]
    idx = case.perm[..., None].expand(-1, -1, -1, hd)
    want_o = torch.gather(v, 2, idx).permute(0, 2, 1, 3)
    assert torch.equal(o.view(torch.int16), want_o.contiguous().view(torch.int16))
    assert torch.equal(lse, torch.full_like(lse, case.lse_exact))
    # the fp64 oracle agrees with the planted answer (its exp(-110) is ~1e-48, not 0)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    assert (fwd.o - want_o.double()).abs().max() < 1e-40
    assert torch.equal(fwd.lse, torch.full_like(fwd.lse, case.lse_exact))

    dq, dk, dv = emu_backward(case, o, lse)
    do = case.dO.permute(0, 2, 1, 3)
    want_dv = torch.zeros_like(do).scatter_(2, idx, do).permute(0, 2, 1, 3)
    assert torch.equal(dv.view(torch.int16), want_dv.contiguous().view(torch.int16))
    assert not dq.float().any() and not dk.float().any()
    odq, odk, odv = fo.oracle_backward(fwd, case.dO)
    assert max((odv - want_dv.double()).abs().max(), odq.abs().max(), odk.abs().max()) < 1e-40


@pytest.mark.parametrize("shape_idx", range(len(fo.EDGE_SHAPES)), ids=SHAPE_IDS)
def test_uniform_case_is_mean_and_log_n(shape_idx):
    N, hd, prefix, rope = fo.EDGE_SHAPES[shape_idx]
    case = fo.uniform_case(B, N, H, hd, prefix, seed=5 + shape_idx, rope=rope)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    assert (fwd.p - 1.0 / N).abs().max() < 1e-15
    mean_v = case.qkv[:, :, 2].double().mean(dim=1, keepdim=True).expand(-1, N, -1, -1)
    assert (fwd.o - mean_v).abs().max() < 1e-13
    assert (fwd.lse - torch.log(torch.tensor(float(N), dtype=torch.float64))).abs().max() < 1e-13


@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape_idx", range(len(fo.EDGE_SHAPES)), ids=SHAPE_IDS)
def test_cpu_fallback_within_bound_o(shape_idx, gain):
    """_flat_fmha_ref (the path flat_multi_fmha takes off-GPU) in fp32."""
    from dinov3_amd.ops.flat_attention import _flat_fmha_ref

    N, hd, prefix, rope = fo.EDGE_SHAPES[shape_idx]
    ref = _fewbit(shape_idx, gain)
    case, fwd, _, (bound_o, _), _ = ref
    out = _flat_fmha_ref(case.qkv.float().reshape(B * N, 3 * H * hd), H,
                         [(0, B, N, case.sin, case.cos, prefix)])
    ratio = fo.worst_ratio((out.double().view(B, N, H, hd) - fwd.o).abs(), bound_o)
    print(f"\n  _flat_fmha_ref err/bound_o {SHAPE_IDS[shape_idx]} gain {gain}: {ratio:.3f}")
    assert ratio <= 1.0


def test_worst_ratio_rejects_nan_and_zero_bound():
    one, zero = torch.ones(1), torch.zeros(1)
    assert fo.worst_ratio(torch.tensor([float("nan")]), one) == float("inf")
    assert fo.worst_ratio(one, zero) == float("inf")
    assert fo.worst_ratio(zero, zero) == 0.0

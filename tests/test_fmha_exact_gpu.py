"""Fused RoPE + attention kernels against the fp64 oracle, elementwise.

Three input families from dinov3_amd/ops/fmha_oracle.py: few-bit cases held to
bounds derived from the kernels' own rounding steps, planted one-hot cases
compared bit for bit, and uniform (q = 0) cases. tests/test_fmha_oracle.py
shows on the CPU that a correct implementation stays inside these bounds and
that one lost key, one lost query row or an off-by-one RoPE prefix does not.
Run with -s to see the worst err/bound ratio of every case.
"""

import functools
import math

import pytest
import torch

from dinov3_amd.ops import fmha_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 2, 3   # values differ per (b, h) and H is no power of two: stride mix-ups show
SHAPE_IDS = [f"N{n}-hd{hd}-p{p}-{'rope' if r else 'norope'}" for n, hd, p, r in fo.EDGE_SHAPES]
SHAPES = list(range(len(fo.EDGE_SHAPES)))
# (shape, dkv64): the gated 64-row dK/dV staging only exists on the N > 64 path
BWD_CASES = [(i, False) for i in SHAPES] + [(i, True) for i in SHAPES if fo.EDGE_SHAPES[i][0] > 64]
BWD_IDS = [SHAPE_IDS[i] + ("-dkv64" if d else "") for i, d in BWD_CASES]
# the q/k/v [B, H, N, hd] entry points (the kernels' plain layout): (N, hd), no RoPE
QKV_SHAPES = [(33, 64), (129, 64), (197, 128)]


# ---------------------------------------------------------------------------
# shared references: computed once on the CPU, never modified
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fewbit_ref(N, hd, prefix, rope, gain, batch=B):
    seed = 100000 * batch + 100 * N + hd + int(gain * 10) + (7 if rope else 0)
    case = fo.fewbit_case(batch, N, H, hd, prefix, gain, seed=seed, rope=rope)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    return (case, fwd, fo.oracle_backward(fwd, case.dO), fo.forward_bounds(fwd),
            fo.backward_bounds(fwd, case.dO))


@functools.lru_cache(maxsize=None)
def _onehot(N, hd, prefix, rope):
    return fo.onehot_case(B, N, H, hd, prefix, seed=31 * N + hd, rope=rope)


def _tables(case):
    if case.sin is None:
        return None, None
    return case.sin.to(DEV), case.cos.to(DEV)


def _fwd(case):
    from dinov3_amd.ops import hip_ops

    sin, cos = _tables(case)
    e = torch.empty(0, device=DEV)
    o, lse = hip_ops().fmha_rope_fwd(case.qkv.to(DEV), e if sin is None else sin,
                                     e if cos is None else cos, case.prefix)
    return o.cpu(), lse.cpu()


def _flat_fwd_bwd(cases):
    """Run the model's path: every case is one crop group of one flat buffer.
    Returns per group (out [B,N,H,hd], dq, dk, dv) on the CPU."""
    from dinov3_amd.ops.flat_attention import flat_multi_fmha

    metas, off = [], 0
    for c in cases:
        Bc, N = c.qkv.shape[:2]
        metas.append((off, Bc, N, *_tables(c), c.prefix))
        off += Bc * N
    hd = cases[0].qkv.shape[-1]
    qkv_flat = torch.cat([c.qkv.reshape(-1, 3 * H * hd) for c in cases]).to(DEV).requires_grad_(True)
    dout = torch.cat([c.dO.reshape(-1, H * hd) for c in cases]).to(DEV)
    # forward and backward allocate their outputs with torch.empty: leave NaNs
    # in the blocks the caching allocator will hand them, so a row the kernels
    # never write cannot hold a plausible value by luck
    poison = [torch.full_like(qkv_flat, float("nan")), torch.full_like(dout, float("nan"))]
    del poison
    out = flat_multi_fmha(qkv_flat, H, metas)
    out.backward(dout)
    res = []
    for (o0, Bc, N, *_rest) in metas:
        g = qkv_flat.grad[o0:o0 + Bc * N].view(Bc, N, 3, H, hd).cpu()
        res.append((out.detach()[o0:o0 + Bc * N].view(Bc, N, H, hd).cpu(), g[:, :, 0], g[:, :, 1], g[:, :, 2]))
    assert off == qkv_flat.shape[0]
    return res


def _set_dkv64(monkeypatch, on):
    # the launcher reads the variable at every launch
    if on:
        monkeypatch.setenv("DINOV3_FMHA_DKV64", "1")
    else:
        monkeypatch.delenv("DINOV3_FMHA_DKV64", raising=False)


def _check(label, pairs):
    """pairs: name -> (got, ref, bound). Prints the worst err/bound of each
    before asserting that every element is inside its bound."""
    ratios = {k: fo.worst_ratio((got.double() - ref).abs(), bound) for k, (got, ref, bound) in pairs.items()}
    line = " ".join(f"{k}={v:.3f}" for k, v in ratios.items())
    if "lse" in pairs:
        got, ref, _ = pairs["lse"]
        line += f" max|lse err|={float((got.double() - ref).abs().max()):.2e}"
    print(f"\n  err/bound {label}: {line}")
    assert all(v <= 1.0 for v in ratios.values()), (label, ratios)
    return ratios


def _bits(x):
    return x.contiguous().view(torch.int16)


def _onehot_expected(case):
    hd = case.qkv.shape[-1]
    idx = case.perm[..., None].expand(-1, -1, -1, hd)
    v = case.qkv[:, :, 2].permute(0, 2, 1, 3)
    want_o = torch.gather(v, 2, idx).permute(0, 2, 1, 3)
    do = case.dO.permute(0, 2, 1, 3)
    want_dv = torch.zeros_like(do).scatter_(2, idx, do).permute(0, 2, 1, 3)
    return want_o, want_dv


# ---------------------------------------------------------------------------
# forward, through fmha_rope_fwd
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fwd_fewbit_within_bounds(shape, gain):
    case, fwd, _, (bound_o, bound_lse), _ = _fewbit_ref(*fo.EDGE_SHAPES[shape], gain)
    o, lse = _fwd(case)
    _check(f"fwd {SHAPE_IDS[shape]} gain {gain}",
           {"o": (o, fwd.o, bound_o), "lse": (lse, fwd.lse, bound_lse)})


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fwd_onehot_bit_exact(shape):
    case = _onehot(*fo.EDGE_SHAPES[shape])
    o, lse = _fwd(case)
    want_o, _ = _onehot_expected(case)
    assert torch.equal(_bits(o), _bits(want_o))
    assert torch.equal(lse, torch.full_like(lse, case.lse_exact))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fwd_uniform(shape):
    N, hd, prefix, rope = fo.EDGE_SHAPES[shape]
    case = fo.uniform_case(B, N, H, hd, prefix, seed=900 + shape, rope=rope)
    o, lse = _fwd(case)
    v = case.qkv[:, :, 2].double()
    mean_v = v.mean(dim=1, keepdim=True).expand(-1, N, -1, -1)
    mean_abs_v = v.abs().mean(dim=1, keepdim=True).expand(-1, N, -1, -1)
    # sum_j 1.0 * v_j is exact in fp32 (integers): what is left is the bf16
    # store and the fp32 1/N normalisation
    bound_o = 2.0 ** -8 * mean_v.abs() + N * 2.0 ** -24 * mean_abs_v
    _, bound_lse = fo.forward_bounds(fo.oracle_forward(case.qkv, case.sin, case.cos, prefix))
    _check(f"fwd uniform {SHAPE_IDS[shape]}",
           {"o": (o, mean_v, bound_o), "lse": (lse, torch.full_like(bound_lse, math.log(N)), bound_lse)})


# ---------------------------------------------------------------------------
# backward, through flat_multi_fmha(...).backward — the path the model runs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape,dkv64", BWD_CASES, ids=BWD_IDS)
def test_bwd_fewbit_within_bounds(shape, dkv64, gain, monkeypatch):
    _set_dkv64(monkeypatch, dkv64)
    case, fwd, (dq, dk, dv), (bound_o, _), (bdq, bdk, bdv) = _fewbit_ref(*fo.EDGE_SHAPES[shape], gain)
    (out, gq, gk, gv), = _flat_fwd_bwd([case])
    _check(f"bwd {SHAPE_IDS[shape]}{' dkv64' if dkv64 else ''} gain {gain}",
           {"o": (out, fwd.o, bound_o), "dq": (gq, dq, bdq), "dk": (gk, dk, bdk), "dv": (gv, dv, bdv)})


@pytest.mark.parametrize("shape,dkv64", BWD_CASES, ids=BWD_IDS)
def test_bwd_onehot_exact(shape, dkv64, monkeypatch):
    _set_dkv64(monkeypatch, dkv64)
    case = _onehot(*fo.EDGE_SHAPES[shape])
    (out, gq, gk, gv), = _flat_fwd_bwd([case])
    want_o, want_dv = _onehot_expected(case)
    assert torch.equal(_bits(out), _bits(want_o))
    assert torch.equal(_bits(gv), _bits(want_dv))
    # zero as a value: a signed zero is fine, a NaN is not
    assert torch.equal(gq.float(), torch.zeros(gq.shape)) and torch.equal(gk.float(), torch.zeros(gk.shape))


def test_bwd_multi_group_flat_buffer(monkeypatch):
    """A large group then a small one in one flat buffer, each with its own
    tables and prefix: every row of `out` and `dqkv_flat` is inside its group's
    bounds (both buffers are torch.empty — an unwritten row must not pass)."""
    _set_dkv64(monkeypatch, False)
    refs = [_fewbit_ref(197, 64, 5, True, 1.0, 2), _fewbit_ref(33, 64, 1, True, 1.0, 3)]
    results = _flat_fwd_bwd([r[0] for r in refs])
    for i, ((case, fwd, (dq, dk, dv), (bound_o, _), (bdq, bdk, bdv)), (out, gq, gk, gv)) in enumerate(
            zip(refs, results)):
        assert out.shape == fwd.o.shape and gq.shape == dq.shape
        _check(f"multi-group group {i} (B={case.qkv.shape[0]}, N={case.qkv.shape[1]})",
               {"o": (out, fwd.o, bound_o), "dq": (gq, dq, bdq), "dk": (gk, dk, bdk), "dv": (gv, dv, bdv)})


# ---------------------------------------------------------------------------
# the q/k/v entry points: fmha_fwd, fmha_bwd, ops.fmha  (plain-layout kernels)
# ---------------------------------------------------------------------------

def _split_qkv(case):
    """[B, N, 3, H, hd] -> contiguous q, k, v [B, H, N, hd] on the device."""
    return tuple(case.qkv[:, :, w].permute(0, 2, 1, 3).contiguous().to(DEV) for w in range(3))


def _tm(x):
    """head-major device tensor -> token-major CPU tensor, the oracle's layout."""
    return x.detach().permute(0, 2, 1, 3).cpu()


@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("N,hd", QKV_SHAPES)
def test_qkv_entry_points_fewbit(N, hd, gain):
    from dinov3_amd.ops import fmha, hip_ops

    case, fwd, (dq, dk, dv), (bound_o, bound_lse), (bdq, bdk, bdv) = _fewbit_ref(N, hd, 0, False, gain)
    q, k, v = _split_qkv(case)
    do = case.dO.permute(0, 2, 1, 3).contiguous().to(DEV)
    o, lse = hip_ops().fmha_fwd(q, k, v)
    gq, gk, gv = hip_ops().fmha_bwd(do, q, k, v, o, lse)
    _check(f"fmha_fwd/fmha_bwd N{N}-hd{hd} gain {gain}",
           {"o": (_tm(o), fwd.o, bound_o), "lse": (lse.cpu(), fwd.lse, bound_lse),
            "dq": (_tm(gq), dq, bdq), "dk": (_tm(gk), dk, bdk), "dv": (_tm(gv), dv, bdv)})

    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = fmha(q, k, v)
    out.backward(do)
    _check(f"ops.fmha N{N}-hd{hd} gain {gain}",
           {"o": (_tm(out), fwd.o, bound_o), "dq": (_tm(q.grad), dq, bdq),
            "dk": (_tm(k.grad), dk, bdk), "dv": (_tm(v.grad), dv, bdv)})


@pytest.mark.parametrize("N,hd", QKV_SHAPES)
def test_qkv_entry_points_onehot(N, hd):
    from dinov3_amd.ops import fmha, hip_ops

    case = _onehot(N, hd, 0, False)
    want_o, want_dv = _onehot_expected(case)
    q, k, v = _split_qkv(case)
    do = case.dO.permute(0, 2, 1, 3).contiguous().to(DEV)
    o, lse = hip_ops().fmha_fwd(q, k, v)
    gq, gk, gv = hip_ops().fmha_bwd(do, q, k, v, o, lse)
    assert torch.equal(_bits(_tm(o)), _bits(want_o))
    assert torch.equal(lse.cpu(), torch.full(lse.shape, case.lse_exact))
    assert torch.equal(_bits(_tm(gv)), _bits(want_dv))
    assert torch.equal(gq.float().cpu(), torch.zeros(gq.shape)) and torch.equal(gk.float().cpu(), torch.zeros(gk.shape))

    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = fmha(q, k, v)
    out.backward(do)
    assert torch.equal(_bits(_tm(out)), _bits(want_o))
    assert torch.equal(_bits(_tm(v.grad)), _bits(want_dv))
    assert torch.equal(q.grad.float().cpu(), torch.zeros(q.shape)) and torch.equal(k.grad.float().cpu(), torch.zeros(k.shape))


@pytest.mark.parametrize("N,hd", QKV_SHAPES)
def test_plain_and_packed_entry_points_bit_identical(N, hd):
    """There is one kernel per pass: the q/k/v entry points and the packed-qkv
    ones differ in addressing only, so their results agree bit for bit.
    (33, 64): small-N path, partial tile; (129, 64): two q blocks with a
    one-row tail, 128-key staging; (197, 128): Q-in-LDS forward, MINW-2 dq."""
    from dinov3_amd.ops import hip_ops

    case = _fewbit_ref(N, hd, 0, False, 1.0)[0]
    qkv = case.qkv.to(DEV)
    do_tm = case.dO.to(DEV)
    e = torch.empty(0, device=DEV)
    o_p, lse_p = hip_ops().fmha_rope_fwd(qkv, e, e, 0)
    g = hip_ops().fmha_rope_bwd(do_tm, qkv, o_p, lse_p, e, e, 0)

    q, k, v = _split_qkv(case)
    o, lse = hip_ops().fmha_fwd(q, k, v)
    gq, gk, gv = hip_ops().fmha_bwd(do_tm.permute(0, 2, 1, 3).contiguous(), q, k, v, o, lse)

    assert torch.equal(_bits(o.permute(0, 2, 1, 3)), _bits(o_p))
    assert torch.equal(lse.view(torch.int32), lse_p.view(torch.int32))
    for w, (name, got) in enumerate((("dq", gq), ("dk", gk), ("dv", gv))):
        assert torch.equal(_bits(got.permute(0, 2, 1, 3)), _bits(g[:, :, w])), name

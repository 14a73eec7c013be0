"""The single-pass attention backward (fmha_rope::bwd_fused_kernel, hd 64 and
N <= 256) against the fp64 oracle, at the shapes where it takes another path:
a partly filled key tile, exactly full tiles, an idle eighth wave, one row in
the eighth tile, the upper limit, and next to a group that keeps the
three-launch path. tests/test_fmha_fused_bwd.py shows on the CPU that the
kernel's rounding order stays inside these bounds and that a lost dQ partial
or a lost query row does not. Run with -s to see the worst err/bound ratios.
"""

import functools

import pytest
import torch

from dinov3_amd.ops import fmha_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 2, 3
FUSED_SHAPES = [
    (37, 64, 1, True), (96, 64, 5, True), (197, 64, 1, True), (224, 64, 1, True),
    (225, 64, 5, True), (256, 64, 0, True), (256, 64, 1, False),
]
SHAPE_IDS = [f"N{n}-hd{hd}-p{p}-{'rope' if r else 'norope'}" for n, hd, p, r in FUSED_SHAPES]


# ---------------------------------------------------------------------------
# shared references: computed once on the CPU, never modified
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fewbit_ref(N, hd, prefix, rope, gain, batch=B, heads=H):
    seed = 300000 * batch + 100 * N + hd + int(gain * 10) + (7 if rope else 0) + heads
    case = fo.fewbit_case(batch, N, heads, hd, prefix, gain, seed=seed, rope=rope)
    fwd = fo.oracle_forward(case.qkv, case.sin, case.cos, case.prefix)
    return case, fo.oracle_backward(fwd, case.dO), fo.backward_bounds(fwd, case.dO)


@functools.lru_cache(maxsize=None)
def _onehot(N, hd, prefix, rope):
    return fo.onehot_case(B, N, H, hd, prefix, seed=53 * N + hd, rope=rope)


def _tables(case):
    if case.sin is None:
        return None, None
    return case.sin.to(DEV), case.cos.to(DEV)


def _flat_fwd_bwd(cases):
    """Every case is one crop group of one flat buffer, as the model runs it.
    Returns per group (dq, dk, dv) on the CPU and the whole gradient buffer."""
    from dinov3_amd.ops.flat_attention import flat_multi_fmha

    heads, hd = cases[0].qkv.shape[3:]
    metas, off = [], 0
    for c in cases:
        Bc, N = c.qkv.shape[:2]
        metas.append((off, Bc, N, *_tables(c), c.prefix))
        off += Bc * N
    qkv_flat = torch.cat([c.qkv.reshape(-1, 3 * heads * hd) for c in cases]).to(DEV).requires_grad_(True)
    dout = torch.cat([c.dO.reshape(-1, heads * hd) for c in cases]).to(DEV)
    # the outputs are torch.empty: leave NaNs in the blocks the caching allocator
    # will hand out, so a row the kernels never write cannot pass by luck
    poison = [torch.full_like(qkv_flat, float("nan")), torch.full_like(dout, float("nan"))]
    del poison
    out = flat_multi_fmha(qkv_flat, heads, metas)
    out.backward(dout)
    res = []
    for (o0, Bc, N, *_rest) in metas:
        g = qkv_flat.grad[o0:o0 + Bc * N].view(Bc, N, 3, heads, hd).cpu()
        res.append((g[:, :, 0], g[:, :, 1], g[:, :, 2]))
    return res, qkv_flat.grad.cpu()


def _check(label, got, ref, bounds):
    ratios = {k: fo.worst_ratio((g.double() - r).abs(), b)
              for k, g, r, b in zip(("dq", "dk", "dv"), got, ref, bounds)}
    print(f"\n  err/bound {label}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (label, ratios)


def _bits(x):
    return x.contiguous().view(torch.int16)


def _fused_on(monkeypatch, on=True):
    # the bindings read the variable at every call
    if on:
        monkeypatch.delenv("DINOV3_FMHA_FUSED_BWD", raising=False)
    else:
        monkeypatch.setenv("DINOV3_FMHA_FUSED_BWD", "0")
    monkeypatch.delenv("DINOV3_FMHA_DKV64", raising=False)


# ---------------------------------------------------------------------------

def test_predicate():
    from dinov3_amd.ops import hip_ops

    assert hip_ops().fmha_fused_bwd_supported(256, 64) is True
    assert hip_ops().fmha_fused_bwd_supported(257, 64) is False
    assert hip_ops().fmha_fused_bwd_supported(197, 128) is False


@pytest.mark.parametrize("gain", fo.FEWBIT_GAINS)
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=SHAPE_IDS)
def test_fewbit_within_bounds(shape, gain, monkeypatch):
    _fused_on(monkeypatch)
    case, grads, bounds = _fewbit_ref(*shape, gain)
    (got,), _ = _flat_fwd_bwd([case])
    _check(f"fused bwd {shape} gain {gain}", got, grads, bounds)


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=SHAPE_IDS)
def test_onehot_dv_bit_exact(shape, monkeypatch):
    _fused_on(monkeypatch)
    case = _onehot(*shape)
    ((gq, gk, gv),), _ = _flat_fwd_bwd([case])
    hd = case.qkv.shape[-1]
    idx = case.perm[..., None].expand(-1, -1, -1, hd)
    do = case.dO.permute(0, 2, 1, 3)
    want_dv = torch.zeros_like(do).scatter_(2, idx, do).permute(0, 2, 1, 3)
    assert torch.equal(_bits(gv), _bits(want_dv))
    # zero as a value: a signed zero is fine, a NaN is not
    assert torch.equal(gq.float(), torch.zeros(gq.shape)) and torch.equal(gk.float(), torch.zeros(gk.shape))


def test_mixed_buffer(monkeypatch):
    """Two fused groups (512- and 128-thread kernels) and one three-launch
    group (N = 257) in one flat buffer."""
    _fused_on(monkeypatch)
    refs = [_fewbit_ref(197, 64, 1, True, 1.0, 2), _fewbit_ref(37, 64, 1, True, 1.0, 3),
            _fewbit_ref(257, 64, 0, True, 1.0, 1)]
    results, grad = _flat_fwd_bwd([r[0] for r in refs])
    assert not torch.isnan(grad.float()).any()
    for i, ((case, grads, bounds), got) in enumerate(zip(refs, results)):
        _check(f"mixed buffer group {i} (B={case.qkv.shape[0]}, N={case.qkv.shape[1]})", got, grads, bounds)


@pytest.mark.parametrize("N", [37, 197, 256])
def test_plain_and_packed_paths_bit_identical(N, monkeypatch):
    """fmha_bwd (q/k/v [B, H, N, hd]) against fmha_rope_bwd without RoPE:
    one kernel, two layouts."""
    from dinov3_amd.ops import hip_ops

    _fused_on(monkeypatch)
    case = _fewbit_ref(N, 64, 0, False, 1.0)[0]
    qkv = case.qkv.to(DEV)
    do_tm = case.dO.to(DEV)
    e = torch.empty(0, device=DEV)
    o_p, lse_p = hip_ops().fmha_rope_fwd(qkv, e, e, 0)
    g = hip_ops().fmha_rope_bwd(do_tm, qkv, o_p, lse_p, e, e, 0)
    q, k, v = (case.qkv[:, :, w].permute(0, 2, 1, 3).contiguous().to(DEV) for w in range(3))
    o, lse = hip_ops().fmha_fwd(q, k, v)
    got = hip_ops().fmha_bwd(do_tm.permute(0, 2, 1, 3).contiguous(), q, k, v, o, lse)
    for w, (name, x) in enumerate(zip(("dq", "dk", "dv"), got)):
        assert torch.equal(_bits(x.permute(0, 2, 1, 3)), _bits(g[:, :, w])), name


@pytest.mark.parametrize("N", [197, 37])
def test_same_call_twice_bit_identical(N, monkeypatch):
    from dinov3_amd.ops import hip_ops

    _fused_on(monkeypatch)
    case = _fewbit_ref(N, 64, 1, True, 1.0)[0]
    qkv, do = case.qkv.to(DEV), case.dO.to(DEV)
    sin, cos = _tables(case)
    o, lse = hip_ops().fmha_rope_fwd(qkv, sin, cos, case.prefix)
    first = hip_ops().fmha_rope_bwd(do, qkv, o, lse, sin, cos, case.prefix)
    second = hip_ops().fmha_rope_bwd(do, qkv, o, lse, sin, cos, case.prefix)
    assert torch.equal(_bits(first), _bits(second))


def test_more_workgroups_than_cus(monkeypatch):
    """B = 40, H = 16, N = 37: 640 workgroups, so block index and offsets count."""
    _fused_on(monkeypatch)
    case, grads, bounds = _fewbit_ref(37, 64, 1, True, 1.0, 40, 16)
    (got,), _ = _flat_fwd_bwd([case])
    _check("fused bwd B=40 H=16 N=37", got, grads, bounds)


@pytest.mark.parametrize("N", [197, 37])
def test_switch_off_three_launch_path(N, monkeypatch):
    _fused_on(monkeypatch, on=False)
    case, grads, bounds = _fewbit_ref(N, 64, 1, True, 1.0)
    (got,), _ = _flat_fwd_bwd([case])
    _check(f"three-launch bwd N={N}", got, grads, bounds)

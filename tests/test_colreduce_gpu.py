"""Two-stage column reduction and the lean bias+GELU kernels.

Every backward kernel that produces a parameter gradient (dgamma / dbias)
leaves per-block partial column sums in a workspace and a finalize kernel sums
them in a fixed order. These tests drive the bindings directly at the smallest
shapes that reach each code path (a single row, fewer rows than row lanes,
rows that are no multiple of the rows in flight, more than one column tile,
enough rows for the row grid to reach its cap, every LayerNorm chunk count and
the non-wave kernel) against fp32 torch autograd on the same bf16 inputs, with
the tolerances tests/test_ops_gpu.py uses for the same op, and check that two
calls on the same inputs give bit-identical parameter gradients.
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _assert_close(got, want, atol, rtol=1e-2, what=""):
    got = got.float()
    want = want.float()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"{what}: max err {err:.4g} (scale {scale:.4g}, bound {atol + rtol * scale:.4g})")
    assert err <= atol + rtol * scale, f"{what}: max err {err} (scale {scale})"


@pytest.fixture(scope="module")
def ops():
    from dinov3_amd.ops import hip_ops

    return hip_ops()


def _bf16(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).bfloat16()


def _f32_leaf(t):
    return t.detach().float().requires_grad_(True)


# ------------------------------ bias + gelu ------------------------------

# (1, 8): one thread. (3, 1032): rows < row lanes, H/8 odd. (5, 4096): one full
# column tile, rows not a multiple of the 4 in flight. (257, 1024): several row
# lanes, ragged tail. (8203, 384): row grid at its cap. (2, 4104): two column
# tiles, the second almost empty.
BIAS_GELU_SHAPES = [(1, 8), (3, 1032), (5, 4096), (257, 1024), (8203, 384), (2, 4104)]


@pytest.mark.parametrize("rows,H", BIAS_GELU_SHAPES)
def test_bias_gelu_fwd_bwd(ops, rows, H):
    torch.manual_seed(rows * 7919 + H)
    x, b, dy = _bf16(rows, H), _bf16(H), _bf16(rows, H)
    y = ops.bias_gelu_fwd(x, b)
    dx, db = ops.bias_gelu_bwd(dy, x, b)
    dx2, db2 = ops.bias_gelu_bwd(dy, x, b)
    xr, br = _f32_leaf(x), _f32_leaf(b)
    yr = torch.nn.functional.gelu(xr + br, approximate="tanh")
    yr.backward(dy.float())
    _assert_close(y, yr, atol=0.03, what="bias_gelu fwd")
    _assert_close(dx, xr.grad, atol=0.05, what="bias_gelu dx")
    _assert_close(db, br.grad, atol=0.5, rtol=2e-2, what="bias_gelu db")
    assert db.dtype == b.dtype and db.shape == b.shape
    assert torch.equal(db, db2) and torch.equal(dx, dx2)


def test_bias_gelu_extremes(ops):
    """0, +-30, +-100, +-1e4: finite, and equal to the reference to bf16
    rounding. The bound is per element: the op's atol plus one bf16 step
    (2^-8 relative) of the reference value, since max-scaled rtol would be
    meaningless next to 1e4."""
    vals = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4, 0.5], device=DEV)
    x = vals.repeat(3, 2).bfloat16().contiguous()  # [3, 16]
    b = torch.zeros(16, device=DEV).bfloat16()
    dy = torch.ones_like(x)
    y = ops.bias_gelu_fwd(x, b)
    dx, db = ops.bias_gelu_bwd(dy, x, b)
    xr, br = _f32_leaf(x), _f32_leaf(b)
    yr = torch.nn.functional.gelu(xr + br, approximate="tanh")
    yr.backward(dy.float())
    for got, want, atol, what in [(y, yr, 0.03, "fwd"), (dx, xr.grad, 0.05, "dx"),
                                  (db, br.grad, 0.5, "db")]:
        got, want = got.float(), want.detach().float()
        assert torch.isfinite(got).all(), f"bias_gelu extremes {what}: non-finite"
        err = (got - want).abs()
        bound = atol + want.abs() * 2.0 ** -8
        print(f"bias_gelu extremes {what}: max err {err.max().item():.4g}")
        assert (err <= bound).all(), f"bias_gelu extremes {what}: {got} vs {want}"


def test_swiglu_fwd_bwd(ops):
    torch.manual_seed(4)
    rows, H = 5, 344
    x, dy = _bf16(rows, 2 * H), _bf16(rows, H)
    y = ops.swiglu_fwd(x)
    dx = ops.swiglu_bwd(dy, x)
    xr = _f32_leaf(x)
    yr = torch.nn.functional.silu(xr[..., :H]) * xr[..., H:]
    yr.backward(dy.float())
    _assert_close(y, yr, atol=0.05, what="swiglu fwd")
    _assert_close(dx, xr.grad, atol=0.05, what="swiglu dx")


# ------------------------------ LayerScale -------------------------------

# The binding takes gamma and bias as plain tensors, and a Python None does not
# convert to one (TypeError), so "both present" is the only combination it
# accepts; the list keeps the shape of the check should that ever change.
@pytest.mark.parametrize("M,D", list(itertools.product([1, 7, 259], [384, 1024])))
@pytest.mark.parametrize("has_gamma,has_bias", [(True, True)])
def test_ls_scatter_bwd(ops, M, D, has_gamma, has_bias):
    """idx is a random subset of 2*M destination rows; per-row scale present."""
    torch.manual_seed(M * 31 + D)
    R = 2 * M
    idx = torch.randperm(R, device=DEV)[:M]
    src, dy = _bf16(M, D), _bf16(R, D)
    gamma = _bf16(D, scale=0.01) if has_gamma else None
    bias = _bf16(D) if has_bias else None
    scale = torch.rand(M, device=DEV) + 0.5
    dres, dg, db = ops.ls_scatter_bwd(dy, idx, src, gamma, bias, scale)
    _, dg2, db2 = ops.ls_scatter_bwd(dy, idx, src, gamma, bias, scale)

    sr = _f32_leaf(src)
    gr = _f32_leaf(gamma) if has_gamma else None
    br = _f32_leaf(bias) if has_bias else None
    val = sr if br is None else sr + br
    if gr is not None:
        val = gr * val
    ref = torch.zeros(R, D, device=DEV).index_add(0, idx, val * scale.unsqueeze(1))
    ref.backward(dy.float())
    _assert_close(dres, sr.grad, atol=0.03, what="ls_scatter dres")
    for got, got2, leaf, what in [(dg, dg2, gr, "dgamma"), (db, db2, br, "dbias")]:
        if leaf is None:
            assert got is None
            continue
        _assert_close(got, leaf.grad, atol=0.05 + 0.02 * leaf.grad.abs().max().item(),
                      what=f"ls_scatter {what}")
        assert got.dtype == torch.bfloat16 and got.shape == (D,)
        assert torch.equal(got, got2)


@pytest.mark.parametrize("rows,D", list(itertools.product([1, 5, 261], [384, 1024])))
def test_ls_axpy_bwd(ops, rows, D):
    torch.manual_seed(rows * 17 + D)
    res, dout, gamma = _bf16(rows, D), _bf16(rows, D), _bf16(D, scale=0.01)
    dres, dg = ops.ls_axpy_bwd(dout, res, gamma)
    _, dg2 = ops.ls_axpy_bwd(dout, res, gamma)
    rr, gr = _f32_leaf(res), _f32_leaf(gamma)
    (gr * rr).backward(dout.float())
    _assert_close(dres, rr.grad, atol=0.02, what="ls_axpy dres")
    _assert_close(dg, gr.grad, atol=0.3, rtol=2e-2, what="ls_axpy dgamma")
    assert torch.equal(dg, dg2)


@pytest.mark.parametrize("rows,D", list(itertools.product([1, 5, 261], [384, 1024])))
def test_ls_axpy_bias_bwd(ops, rows, D):
    torch.manual_seed(rows * 19 + D)
    res, dout = _bf16(rows, D), _bf16(rows, D)
    gamma, bias = _bf16(D, scale=0.01), _bf16(D)
    dres, dg, db = ops.ls_axpy_bias_bwd(dout, res, gamma, bias)
    _, dg2, db2 = ops.ls_axpy_bias_bwd(dout, res, gamma, bias)
    rr, gr, br = _f32_leaf(res), _f32_leaf(gamma), _f32_leaf(bias)
    (gr * (rr + br)).backward(dout.float())
    _assert_close(dres, rr.grad, atol=0.02, what="ls_axpy_bias dres")
    _assert_close(dg, gr.grad, atol=0.05 + 0.02 * gr.grad.abs().max().item(),
                  what="ls_axpy_bias dgamma")
    _assert_close(db, br.grad, atol=0.05 + 0.02 * br.grad.abs().max().item(),
                  what="ls_axpy_bias dbias")
    assert torch.equal(dg, dg2) and torch.equal(db, db2)


# -------------------------------- norms ----------------------------------

# D = 384 / 1024 / 1536: one / two / three chunks of the wave kernel;
# D = 2056: the block-per-row kernel. rows 1, 3: fewer rows than the waves of a
# block; 6: a ragged second block; 8203: the row grid at its cap.
@pytest.mark.parametrize("rows,D", list(itertools.product([1, 3, 6, 261, 8203],
                                                          [384, 1024, 1536, 2056])))
def test_layernorm_bwd(ops, rows, D):
    torch.manual_seed(rows * 13 + D)
    x, w, b, dy = _bf16(rows, D), _bf16(D), _bf16(D), _bf16(rows, D)
    _, mean, rstd = ops.layernorm_fwd(x, w, b, 1e-6)
    dx, dw, db = ops.layernorm_bwd(dy, x, w, mean, rstd)
    _, dw2, db2 = ops.layernorm_bwd(dy, x, w, mean, rstd)
    xr, wr, br = _f32_leaf(x), _f32_leaf(w), _f32_leaf(b)
    torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-6).backward(dy.float())
    _assert_close(dx, xr.grad, atol=0.08, what="ln dx")
    _assert_close(dw, wr.grad, atol=0.3, rtol=2e-2, what="ln dw")
    _assert_close(db, br.grad, atol=0.3, rtol=2e-2, what="ln db")
    assert dw.dtype == w.dtype and dw.shape == w.shape
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("rows", [3, 261])
def test_rmsnorm_bwd(ops, rows):
    torch.manual_seed(rows)
    D = 384
    x, w, dy = _bf16(rows, D), _bf16(D), _bf16(rows, D)
    _, rstd = ops.rmsnorm_fwd(x, w, 1e-6)
    dx, dw = ops.rmsnorm_bwd(dy, x, w, rstd)
    _, dw2 = ops.rmsnorm_bwd(dy, x, w, rstd)
    xr, wr = _f32_leaf(x), _f32_leaf(w)
    (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * wr).backward(dy.float())
    _assert_close(dx, xr.grad, atol=0.08, what="rms dx")
    _assert_close(dw, wr.grad, atol=0.3, rtol=2e-2, what="rms dw")
    assert torch.equal(dw, dw2)

"""gather_layernorm_fwd / layernorm_bwd_scatter_acc_ (csrc/norms.hip), bf16.

The forward is row_gather + layernorm_fwd with one pass less and must be
bit-equal to that pair. The backward is the wave-per-row LayerNorm backward
whose last phase does dacc[idx[r]] += dx[r]; its dgamma/dbeta must be
bit-equal to layernorm_bwd's, and with a zero accumulator so must the rows it
writes (bf16(0 + dx) is the same rounding as bf16(dx)).

D = 384 / 1024 / 1536: one / two / three chunks of the wave kernel. M = 1, 3:
fewer rows than the waves of a block; 6: a ragged second block; 261: several
blocks; 8203 x 384: the row grid at its cap. The source buffer has R = M + 5
rows and idx is a random non-monotonic subset that holds row 0 and row R - 1
(with M = 1 only row R - 1 fits).
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-6

SHAPES = list(itertools.product([1, 3, 6, 261], [384, 1024, 1536])) + [(8203, 384)]


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


def _bf16(*shape):
    return torch.randn(*shape, device=DEV).bfloat16()


def _make_idx(M, R, seed):
    g = torch.Generator().manual_seed(seed)
    if M == 1:
        return torch.tensor([R - 1], device=DEV)
    mid = (torch.randperm(R - 2, generator=g)[:M - 2] + 1).tolist()
    rows = [0, R - 1] + mid
    rows = [rows[i] for i in torch.randperm(M, generator=g).tolist()]
    if M >= 3 and (rows == sorted(rows) or rows == sorted(rows, reverse=True)):
        rows[0], rows[1] = rows[1], rows[0]
        if rows == sorted(rows) or rows == sorted(rows, reverse=True):
            rows[1], rows[2] = rows[2], rows[1]
    idx = torch.tensor(rows, device=DEV)
    assert idx.unique().numel() == M and 0 in rows and R - 1 in rows
    return idx


def _case(M, D):
    torch.manual_seed(M * 13 + D)
    R = M + 5
    flat, w, b, dy = _bf16(R, D), _bf16(D), _bf16(D), _bf16(M, D)
    return R, flat, w, b, dy, _make_idx(M, R, M * 13 + D)


@pytest.mark.parametrize("M,D", SHAPES)
def test_gather_layernorm_fwd(ops, M, D):
    _, flat, w, b, _, idx = _case(M, D)
    flat0 = flat.clone()
    y, sub, mean, rstd = ops.gather_layernorm_fwd(flat, idx, w, b, EPS)
    sub_ref = ops.row_gather(flat, idx)
    y_ref, mean_ref, rstd_ref = ops.layernorm_fwd(sub_ref, w, b, EPS)
    assert torch.equal(flat, flat0)
    assert torch.equal(sub, sub_ref)
    assert torch.equal(y, y_ref)
    assert torch.equal(mean, mean_ref) and torch.equal(rstd, rstd_ref)


@pytest.mark.parametrize("M,D", SHAPES)
def test_layernorm_bwd_scatter_acc(ops, M, D):
    R, flat, w, b, dy, idx = _case(M, D)
    _, sub, mean, rstd = ops.gather_layernorm_fwd(flat, idx, w, b, EPS)
    dx_ref, dw_ref, db_ref = ops.layernorm_bwd(dy, sub, w, mean, rstd)

    # zero accumulator: the rows written are layernorm_bwd's dx, bit for bit
    dacc = torch.zeros(R, D, device=DEV, dtype=torch.bfloat16)
    dw, db = ops.layernorm_bwd_scatter_acc_(dacc, idx, dy, sub, w, mean, rstd)
    assert torch.equal(dacc[idx], dx_ref)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    other = torch.ones(R, dtype=torch.bool, device=DEV)
    other[idx] = False
    assert not dacc[other].any()

    # random accumulator against the fp32 reference, test_layernorm_bwd's dx bound
    acc0 = _bf16(R, D)
    xr = sub.detach().float().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), w.float(), b.float(), EPS).backward(dy.float())
    want = acc0.float()[idx] + xr.grad
    acc1 = acc0.clone()
    dw1, db1 = ops.layernorm_bwd_scatter_acc_(acc1, idx, dy, sub, w, mean, rstd)
    assert torch.equal(acc1[other], acc0[other])
    _assert_close(acc1[idx], want, atol=0.08, what="scatter-acc rows")
    assert torch.equal(dw1, dw_ref) and torch.equal(db1, db_ref)

    # two calls on equal inputs give equal results
    acc2 = acc0.clone()
    dw2, db2 = ops.layernorm_bwd_scatter_acc_(acc2, idx, dy, sub, w, mean, rstd)
    assert torch.equal(acc2, acc1) and torch.equal(dw2, dw1) and torch.equal(db2, db1)


def test_wrapper_fallback_width():
    """D = 2056 is not a wave-kernel width: the wrapper runs the unfused pair."""
    from dinov3_amd.ops import gather_rows, layer_norm
    from dinov3_amd.ops.gather_norm import gather_layer_norm

    M, D = 6, 2056
    R, flat, w, b, dy, idx = _case(M, D)
    leaves = []
    outs = []
    for fused in (True, False):
        leaf = flat.clone().requires_grad_(True)
        wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        f = leaf * 1.0
        if fused:
            f2, n = gather_layer_norm(f, idx, wl, bl, EPS)
            assert f2 is f
        else:
            n = layer_norm(gather_rows(f, idx), wl, bl, EPS)
        n.backward(dy)
        outs.append(n.detach())
        leaves.append((leaf.grad, wl.grad, bl.grad))
    assert torch.equal(outs[0], outs[1])
    for a, c in zip(*leaves):
        assert torch.equal(a, c)


def test_gather_norm_block_gpu(monkeypatch):
    """Full drop-path block fwd+bwd, fused gather+norm against the switch off
    (shapes and tolerances of test_ops_gpu.py::test_fused_residual_block_gpu)."""
    from dinov3_amd.layers.attention import SelfAttention
    from dinov3_amd.layers.block import DropPathPlan, SelfAttentionBlock
    from dinov3_amd.utils.utils import cat_keep_shapes

    monkeypatch.setenv("DINOV3_DISABLE_HIP", "0")
    monkeypatch.setenv("DINOV3_FUSED_RESIDUAL", "1")
    results = {}
    for fused in (False, True):
        monkeypatch.setenv("DINOV3_FUSED_GATHER_NORM", "1" if fused else "0")
        torch.manual_seed(31)
        # head_dim must be 64 (the FMHA kernel's supported sizes are 64/128)
        blk = SelfAttentionBlock(dim=128, num_heads=2, qkv_bias=True, drop_path=0.5,
                                 init_values=1e-2).to(DEV).bfloat16()
        blk.train()
        torch.manual_seed(32)
        x = torch.randn(6, 32, 128, device=DEV).bfloat16()
        flat, _, _ = cat_keep_shapes([x])
        flat_leaf = flat.clone().requires_grad_(True)
        flat = flat_leaf * 1.0  # non-leaf, as in training
        metas = [SelfAttention._meta_for(x, None, 0)]
        torch.manual_seed(33)
        plan = DropPathPlan(metas, 0.5, 2, flat.device)
        out = blk.forward_flat(flat, metas, plan, 0)
        names = set()
        stack = [out.grad_fn]
        while stack:
            fn = stack.pop()
            if fn is not None and fn not in names:
                names.add(fn)
                stack.extend(f for f, _ in fn.next_functions)
        n_nodes = sum(type(f).__name__ == "_GatherNormFnBackward" for f in names)
        assert n_nodes == (2 if fused else 0)
        out.float().pow(2).sum().backward()
        grads = {n: p.grad.float().clone() for n, p in blk.named_parameters()}
        grads["flat"] = flat_leaf.grad.float().clone()
        results[fused] = (out.detach().float(), grads)
    out_a, grads_a = results[False]
    out_b, grads_b = results[True]
    _assert_close(out_b, out_a, atol=0.05, what="gather-norm block fwd")
    for n in grads_a:
        scale = grads_a[n].abs().max().item()
        _assert_close(grads_b[n], grads_a[n], atol=0.05 + 0.03 * scale, what=f"grad {n}")

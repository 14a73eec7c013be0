"""FP8 backward kernels on the device: the mixed-format MFMA probe, the e5m2
row quantiser and the transposing column quantiser against the CPU oracle, the
e5m2 x e4m3 GEMM, the full autograd of ``fp8_linear(..., backward="fp8")`` and
one end-to-end step with forward and backward in fp8."""

import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, E5M2 = 0, 1  # kernel format ids (the MFMA's cbsz / blgp immediates)

# (M, N, K) of the linear layer. dgrad is an [M,K] GEMM contracting over N,
# wgrad an [N,K] GEMM contracting over M padded to a multiple of 128.
DGRAD_SHAPES = [(33, 128, 128), (130, 384, 256), (257, 384, 1152)]
WGRAD_SHAPES = [(100, 128, 128), (100, 384, 128), (300, 128, 1536), (300, 384, 1536)]


@pytest.fixture(scope="module")
def ops():
    from dinov3_amd.ops import hip_ops

    return hip_ops()


# ------------------------------------------------------------------- probe

def test_probe_mfma_mixed_formats(ops):
    """A holds integers encoded as e5m2, B integers encoded as e4m3, with
    values (3, 5, 6, 7) whose two encodings differ. The product is exact only
    if cbsz describes A and blgp describes B."""
    i = torch.arange(16).view(16, 1)
    j = torch.arange(16).view(1, 16)
    k_row = torch.arange(128).view(1, 128)
    k_col = torch.arange(128).view(128, 1)
    A = ((3 * i + 5 * k_row) % 15 - 7).float()   # [16, 128], -7..7
    B = ((k_col + 3 * j) % 13 - 6).float()       # [128, 16], -6..6, B[k][j] != B[j][k]
    a5 = A.to(torch.float8_e5m2).view(torch.uint8).contiguous().to(DEV)
    bt4 = B.t().contiguous().to(torch.float8_e4m3fn).view(torch.uint8).contiguous().to(DEV)
    assert torch.equal(a5.cpu().view(torch.float8_e5m2).float(), A)
    want = A @ B
    assert torch.equal(ops.probe_mfma_fp8(a5, bt4, E5M2, E4M3).cpu(), want)
    # the same bytes read with the formats swapped, or both as e4m3 (the
    # default), give something else
    assert not torch.equal(ops.probe_mfma_fp8(a5, bt4, E4M3, E5M2).cpu(), want)
    assert not torch.equal(ops.probe_mfma_fp8(a5, bt4).cpu(), want)
    # operands exchanged: now the e5m2 bytes are the B operand
    assert torch.equal(ops.probe_mfma_fp8(bt4, a5, E4M3, E5M2).cpu(), want.t())


# ----------------------------------------------------------- row quantiser

@pytest.mark.parametrize("M,K", [(1, 128), (33, 384), (257, 1536)])
def test_quant_rows_e5m2_bit_equal_to_oracle(M, K):
    from dinov3_amd.ops.fp8_linear import _quantize_rows_ref, fp8_quantize_rows

    g = torch.Generator().manual_seed(2000 + M)
    x = torch.randn(M, K, generator=g)
    x = x * torch.exp2(torch.linspace(-10, 10, M)).view(M, 1)
    if M > 2:
        x[1].zero_()                    # all-zero row: s = 1, q = 0
        x[2] = x[2].clamp(-4.0, 4.0)
        x[2, 5] = -4.0                  # amax an exact power of two
    # elements 2^-30 .. 2^-33 below the row's amax land among the e5m2
    # subnormals (below 2^-14 after scaling) and at the underflow to zero
    amax = x.abs().amax(dim=1)
    for c, f in ((9, 3 * 2.0 ** -31), (10, -5 * 2.0 ** -33), (11, 2.0 ** -32), (12, 2.0 ** -33)):
        x[:, c] = amax * f
    x = x.bfloat16()
    q_ref, s_ref = _quantize_rows_ref(x, "e5m2")
    tiny = q_ref.float().abs()
    assert bool(((tiny > 0) & (tiny < 2.0 ** -14)).any()), "no subnormal in the test data"
    q, s = fp8_quantize_rows(x.to(DEV), fmt="e5m2")
    assert q.dtype == torch.float8_e5m2 and s.dtype == torch.float32
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


# -------------------------------------------------------- column quantiser

@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("C", [128, 384])
@pytest.mark.parametrize("R", [1, 33, 130, 257])
def test_quant_cols_t_bit_equal_to_oracle(R, C, fmt):
    from dinov3_amd.ops.fp8_linear import _quantize_cols_t_ref, fp8_quantize_cols_t

    g = torch.Generator().manual_seed(3000 + R + C)
    x = torch.randn(R, C, generator=g) * torch.exp2(torch.linspace(-10, 10, C)).view(1, C)
    x[:, 7].zero_()                     # all-zero column: s = 1, q = 0
    x = x.bfloat16()
    q_ref, s_ref = _quantize_cols_t_ref(x, fmt)
    Rp = (R + 127) // 128 * 128
    xd = x.to(DEV)
    # leave a freed block of the output's size filled with 0xFF behind, so that
    # a pad the kernel does not write is unlikely to read as zero
    junk = torch.full((C, Rp), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    del junk
    q, s, sums = fp8_quantize_cols_t(xd, fmt=fmt, colsum=True)
    assert q.shape == (C, Rp) and s.shape == (C,) and sums.shape == (C,)
    assert q.dtype == q_ref.dtype and s.dtype == torch.float32 and sums.dtype == torch.float32
    qb = q.cpu().view(torch.uint8)
    assert bool((qb[:, R:] == 0).all()), "pad bytes are not zero"
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(qb, q_ref.view(torch.uint8))
    # column sums: fp32 accumulation of R terms, bf16-rounding headroom
    xd64 = x.double()
    ref = xd64.sum(dim=0)
    bound = (2.0 ** -8) * ref.abs() + R * (2.0 ** -23) * xd64.abs().sum(dim=0)
    err = (sums.cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"colsum {R}x{C}: worst err/bound = {worst:.4f}")
    assert bool((err <= bound).all())
    # without the sums the bytes and scales are the same
    q2, s2 = fp8_quantize_cols_t(xd, fmt=fmt)
    assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(s2, s)


# ----------------------------------------------------------------- the GEMM

def _int_case(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    b = torch.randint(-8, 9, (N,), generator=g).float()
    dy = torch.randint(-8, 9, (M, N), generator=g).float()
    if M > 1:
        dy[M // 2].zero_()
        dy[:, 3].zero_()
    return x.bfloat16(), w.bfloat16(), b.bfloat16(), dy.bfloat16()


@pytest.mark.parametrize("M,N,K", DGRAD_SHAPES + WGRAD_SHAPES)
def test_backward_fp8_integer_exact(M, N, K):
    from dinov3_amd.ops import fp8_linear

    x, w, b, dy = _int_case(M, N, K)
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    fp8_linear(xd, wd, bd, backward="fp8").backward(dy.to(DEV))
    # "+ 0.0": a GEMM accumulates from +0 and never returns -0
    dx_ref = (dy.float() @ w.float() + 0.0).to(torch.bfloat16)
    dw_ref = (dy.float().t() @ x.float() + 0.0).to(torch.bfloat16)
    db_ref = (dy.float().sum(dim=0) + 0.0).to(torch.bfloat16)
    for got, ref in ((xd.grad, dx_ref), (wd.grad, dw_ref), (bd.grad, db_ref)):
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        assert torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))


def _check_product(got, a_q, a_s, b_q, b_s, what):
    """got [Ra,Rb] against the fp64 product of the dequantised operands
    a [Ra,L], b [Rb,L]. Bound: bf16 RNE (2^-8 relative) and fp32 accumulation
    of L terms (L * 2^-24 * sum|a b|), each doubled because the MFMA's internal
    summation order is not documented; L is the padded contraction length."""
    L = a_q.shape[1]
    ah = a_q.cpu().double() * a_s.cpu().double().view(-1, 1)
    bh = b_q.cpu().double() * b_s.cpu().double().view(-1, 1)
    ref = ah @ bh.t()
    bound = (2.0 ** -7) * ref.abs() + L * (2.0 ** -23) * (ah.abs() @ bh.abs().t())
    err = (got.cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst err/bound = {worst:.3f}")
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    assert bool((err <= bound).all()), f"{what}: worst err/bound {worst}"


def _gauss_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (0.05 * torch.randn(N, K, generator=g)).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    dy = (torch.randn(M, N, generator=g) * torch.exp2(torch.linspace(-6, 2, N))).bfloat16()
    return x, w, b, dy


@pytest.mark.parametrize("M,N,K", DGRAD_SHAPES)
def test_mixed_gemm_dgrad_within_rounding_bound(ops, M, N, K):
    from dinov3_amd.ops import fp8_quantize_cols_t, fp8_quantize_rows

    _, w, _, dy = _gauss_case(M, N, K, M + N + K)
    dyq, sdy = fp8_quantize_rows(dy.to(DEV), fmt="e5m2")
    wtq, swt = fp8_quantize_cols_t(w.to(DEV), fmt="e4m3")
    assert wtq.shape == (K, N)
    dx = ops.fp8_gemm_nt(dyq.view(torch.uint8), sdy, wtq.view(torch.uint8), swt, None, E5M2)
    _check_product(dx, dyq, sdy, wtq, swt, f"dgrad {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_mixed_gemm_wgrad_within_rounding_bound(ops, M, N, K):
    from dinov3_amd.ops import fp8_quantize_cols_t

    x, _, _, dy = _gauss_case(M, N, K, M + N + K)
    dytq, sdyt = fp8_quantize_cols_t(dy.to(DEV), fmt="e5m2")
    xtq, sxt = fp8_quantize_cols_t(x.to(DEV), fmt="e4m3")
    Mp = (M + 127) // 128 * 128
    assert dytq.shape == (N, Mp) and xtq.shape == (K, Mp)
    dw = ops.fp8_gemm_nt(dytq.view(torch.uint8), sdyt, xtq.view(torch.uint8), sxt, None, E5M2)
    _check_product(dw, dytq, sdyt, xtq, sxt, f"wgrad {M}x{N}x{K}")


def test_mixed_gemm_refuses_bias(ops):
    q = torch.zeros(128, 128, dtype=torch.uint8, device=DEV)
    s = torch.ones(128, device=DEV)
    b = torch.zeros(128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="bias"):
        ops.fp8_gemm_nt(q, s, q, s, b, E5M2)


# ------------------------------------------------------------ full autograd

@pytest.mark.parametrize("M,N,K", [(130, 256, 384), (300, 384, 1536)])
def test_autograd_fp8_backward_against_cpu_oracle(M, N, K):
    from dinov3_amd.ops import fp8_linear
    from dinov3_amd.ops.fp8_linear import _quantize_cols_t_ref, _quantize_rows_ref

    x, w, b, dy = _gauss_case(M, N, K, 5 + M)
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    fp8_linear(xd, wd, bd, backward="fp8").backward(dy.to(DEV))

    dyq, sdy = _quantize_rows_ref(dy, "e5m2")
    wtq, swt = _quantize_cols_t_ref(w, "e4m3")
    _check_product(xd.grad, dyq, sdy, wtq, swt, f"dx {M}x{N}x{K}")
    dytq, sdyt = _quantize_cols_t_ref(dy, "e5m2")
    xtq, sxt = _quantize_cols_t_ref(x, "e4m3")
    _check_product(wd.grad, dytq, sdyt, xtq, sxt, f"dw {M}x{N}x{K}")

    ref = dy.double().sum(dim=0)
    bound = (2.0 ** -8) * ref.abs() + M * (2.0 ** -23) * dy.double().abs().sum(dim=0)
    err = (bd.grad.cpu().double() - ref).abs()
    print(f"db {M}x{N}: worst err/bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bd.grad.dtype == torch.bfloat16
    assert bool((err <= bound).all())


def test_autograd_fp8_backward_subsets_on_device():
    """Bias grad alone (no quantiser output wanted) and dgrad alone."""
    from dinov3_amd.ops import fp8_linear

    x, w, b, dy = _int_case(130, 256, 384)
    xd, wd = x.to(DEV), w.to(DEV)
    bd = b.to(DEV).requires_grad_(True)
    fp8_linear(xd, wd, bd, backward="fp8").backward(dy.to(DEV))
    assert torch.equal(bd.grad.cpu(), (dy.float().sum(dim=0) + 0.0).to(torch.bfloat16))
    xd = x.to(DEV).requires_grad_(True)
    fp8_linear(xd, wd, None, backward="fp8").backward(dy.to(DEV))
    assert torch.equal(xd.grad.cpu(), (dy.float() @ w.float() + 0.0).to(torch.bfloat16))


def test_fp8_backward_refuses_non_bf16_dy_on_device():
    from dinov3_amd.ops.fp8_linear import _backward_fp8

    x = torch.randn(4, 128, device=DEV).bfloat16()
    w = torch.randn(128, 128, device=DEV).bfloat16()
    dy = torch.randn(4, 128, device=DEV)
    with pytest.raises(RuntimeError, match="bf16"):
        _backward_fp8(dy, x, w, True, True, False)


# --------------------------------------------------------------- end to end

def test_end_to_end_smoke_step_with_fp8_backward():
    """The smoke() recipe with fp8 forward + backward: finite loss, finite grads
    on every student block weight, and block weight grads that differ from the
    forward-only-fp8 run at the same seeds (both losses are printed)."""
    import sys
    import types

    if REPO_ROOT not in sys.path:
        sys.path.insert(0, REPO_ROOT)
    from bench import make_synthetic_batch
    from dinov3_amd.configs import setup_config
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch

    args = types.SimpleNamespace(
        config_file=os.path.join(REPO_ROOT, "dinov3_amd/configs/train/vits_smoke.yaml"),
        opts=["crops.global_crops_size=224", "crops.local_crops_size=96",
              "train.batch_size_per_gpu=2"],
        output_dir="",
    )
    base = setup_config(args, apply_scaling=False)
    base.compute_precision.param_dtype = "bf16"
    dev = torch.device(DEV)

    def step(fp8_backward):
        cfg = copy.deepcopy(base)
        cfg.student.fp8_enabled = True
        cfg.student.fp8_backward = fp8_backward
        torch.manual_seed(0)
        model = SSLMetaArch(cfg).to(device=dev, dtype=torch.bfloat16)
        model.train()
        torch.manual_seed(1)
        batch = make_synthetic_batch(cfg, dev, torch.bfloat16, n_batches=1)[0]
        torch.manual_seed(2)
        loss, _ = model(batch, teacher_temp=0.07, iteration=0)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone()
                 for n, p in model.student_backbone.named_parameters()
                 if "blocks" in n and n.endswith("weight") and p.grad is not None}
        return model, float(loss.detach()), grads

    model, loss_bwd, grads_bwd = step(True)
    assert model.fp8_backward is True
    flagged = [n for n, m in model.student_backbone.named_modules()
               if getattr(m, "fp8_bwd", False)]
    assert flagged, "no student block linear runs the fp8 backward"
    for name, p in model.student_backbone.named_parameters():
        if "blocks" in name and name.endswith("weight"):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    del model
    _, loss_fwd, grads_fwd = step(False)
    print(f"smoke step loss: fp8 fwd+bwd {loss_bwd:.6f}  fp8 fwd only {loss_fwd:.6f}")
    assert loss_bwd == loss_bwd and abs(loss_bwd) != float("inf")
    assert loss_fwd == loss_fwd and abs(loss_fwd) != float("inf")
    assert grads_bwd.keys() == grads_fwd.keys() and grads_bwd
    assert any(not torch.equal(grads_bwd[n], grads_fwd[n]) for n in grads_bwd)

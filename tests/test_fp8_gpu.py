"""FP8 forward kernels on the device: lane-map probe, row quantiser and GEMM
against the CPU oracle, straight-through autograd, and one end-to-end step."""

import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, N, K): one row, ragged M and N below one tile, more than one block in
# both directions, several K-steps (both LDS buffers reused).
GEMM_SHAPES = [(1, 16, 128), (33, 48, 128), (130, 272, 384), (257, 1152, 384), (300, 384, 1536)]


@pytest.fixture(scope="module")
def ops():
    from dinov3_amd.ops import hip_ops

    return hip_ops()


def _to_e4m3_bytes(t):
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def test_probe_mfma_fp8_lane_map(ops):
    """One scaled 16x16x128 MFMA with integer A and asymmetric integer B: pins
    which row/column a lane holds and that A and B use the same k order."""
    i = torch.arange(16).view(16, 1)
    j = torch.arange(16).view(1, 16)
    k_row = torch.arange(128).view(1, 128)
    k_col = torch.arange(128).view(128, 1)
    A = ((3 * i + 5 * k_row) % 9 - 4).float()   # [16, 128]
    B = ((k_col + 3 * j) % 7 - 3).float()       # [128, 16], B[k][j] != B[j][k]
    a = _to_e4m3_bytes(A).contiguous().to(DEV)
    bt = _to_e4m3_bytes(B.t().contiguous()).contiguous().to(DEV)
    c = ops.probe_mfma_fp8(a, bt).cpu()
    assert torch.equal(c, A @ B)


@pytest.mark.parametrize("M,K", [(1, 128), (33, 384), (257, 1536)])
def test_quant_rows_bit_equal_to_oracle(M, K):
    from dinov3_amd.ops.fp8_linear import _quantize_rows_ref, fp8_quantize_rows

    g = torch.Generator().manual_seed(1000 + M)
    x = torch.randn(M, K, generator=g)
    x = x * torch.exp2(torch.linspace(-10, 10, M)).view(M, 1)
    if M > 2:
        x[1].zero_()                    # all-zero row: s = 1, q = 0
        x[2] = x[2].clamp(-4.0, 4.0)
        x[2, 5] = -4.0                  # amax an exact power of two
    x = x.bfloat16()
    q_ref, s_ref = _quantize_rows_ref(x)
    q, s = fp8_quantize_rows(x.to(DEV))
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def test_quant_rows_long_row_path():
    """K > 4096 takes the two-pass (uncached) quantiser."""
    from dinov3_amd.ops.fp8_linear import _quantize_rows_ref, fp8_quantize_rows

    g = torch.Generator().manual_seed(7)
    x = (torch.randn(5, 4096 + 128, generator=g) * 3.0).bfloat16()
    q_ref, s_ref = _quantize_rows_ref(x)
    q, s = fp8_quantize_rows(x.to(DEV))
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def _int_case(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    b = torch.randint(-8, 9, (N,), generator=g).float()
    if M > 1:
        x[M // 2].zero_()
    return x.bfloat16(), w.bfloat16(), b.bfloat16()


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_integer_exact(M, N, K, with_bias):
    from dinov3_amd.ops import fp8_linear

    x, w, b = _int_case(M, N, K)
    ref = x.float() @ w.float().t()
    if with_bias:
        ref = ref + b.float()
    ref = ref.to(torch.bfloat16)
    y = fp8_linear(x.to(DEV), w.to(DEV), b.to(DEV) if with_bias else None)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_random_within_rounding_bound(ops, M, N, K):
    """Against the fp64 product of the kernel's OWN dequantised operands, so
    quantisation error is excluded. Bound: bf16 RNE (2^-8 relative) and fp32
    accumulation of K terms (K * 2^-24 * sum|a b|), each doubled because the
    MFMA's internal summation order is not documented."""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (0.05 * torch.randn(N, K, generator=g)).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    xq, sx = ops.fp8_quant_rows(x.to(DEV))
    wq, sw = ops.fp8_quant_rows(w.to(DEV))
    y = ops.fp8_gemm_nt(xq, sx, wq, sw, b.to(DEV)).cpu().double()
    xh = xq.cpu().view(torch.float8_e4m3fn).double() * sx.cpu().double().view(M, 1)
    wh = wq.cpu().view(torch.float8_e4m3fn).double() * sw.cpu().double().view(N, 1)
    ref = xh @ wh.t() + b.double()
    bound = (2.0 ** -7) * ref.abs() + K * (2.0 ** -23) * (xh.abs() @ wh.abs().t()) \
        + (2.0 ** -23) * b.double().abs()
    err = (y - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"fp8_gemm_nt {M}x{N}x{K}: worst err/bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"worst err/bound {worst}"


def test_autograd_straight_through():
    from dinov3_amd.ops import fp8_linear

    M, N, K = 130, 272, 384
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (0.05 * torch.randn(N, K, generator=g)).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    dy = torch.randn(M, N, generator=g).bfloat16()
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    fp8_linear(xd, wd, bd).backward(dy.to(DEV))

    def check(got, a, bmat, red, what):
        ref = a.double() @ bmat.double()
        bound = (2.0 ** -7) * ref.abs() + red * (2.0 ** -23) * (a.double().abs() @ bmat.double().abs())
        err = (got.cpu().double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{what}: worst err/bound = {worst:.3f}")
        assert got.dtype == torch.bfloat16
        assert bool((err <= bound).all()), f"{what}: worst err/bound {worst}"

    check(xd.grad, dy, w, N, "dx")                       # dx = dy . w
    check(wd.grad, dy.t(), x, M, "dw")                   # dw = dy^T . x
    check(bd.grad.view(1, N), torch.ones(1, M, dtype=torch.bfloat16), dy, M, "db")


def test_fp8_linear_refuses_non_bf16_on_device():
    from dinov3_amd.ops import fp8_linear

    x = torch.randn(4, 128, device=DEV)
    w = torch.randn(16, 128, device=DEV)
    with pytest.raises(RuntimeError, match="bf16"):
        fp8_linear(x, w)


def test_end_to_end_smoke_step_with_fp8():
    """The smoke() recipe with student.fp8_enabled: finite loss, finite grads
    on every student block weight; the same seed with fp8 off gives another
    loss (the gap is printed, not asserted)."""
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

    def step(fp8):
        cfg = copy.deepcopy(base)
        cfg.student.fp8_enabled = fp8
        torch.manual_seed(0)
        model = SSLMetaArch(cfg).to(device=dev, dtype=torch.bfloat16)
        model.train()
        torch.manual_seed(1)
        batch = make_synthetic_batch(cfg, dev, torch.bfloat16, n_batches=1)[0]
        torch.manual_seed(2)
        loss, _ = model(batch, teacher_temp=0.07, iteration=0)
        loss.backward()
        torch.cuda.synchronize()
        return model, float(loss.detach())

    model, loss_fp8 = step(True)
    flagged = [n for n, m in model.student_backbone.named_modules() if getattr(m, "fp8", False)]
    assert flagged, "no student block linear was converted"
    for name, p in model.student_backbone.named_parameters():
        if "blocks" in name and name.endswith("weight"):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    del model
    _, loss_bf16 = step(False)
    print(f"smoke step loss: fp8 {loss_fp8:.6f}  bf16 {loss_bf16:.6f}  "
          f"gap {loss_fp8 - loss_bf16:+.6f}")
    assert loss_fp8 == loss_fp8 and abs(loss_fp8) != float("inf")
    assert loss_bf16 == loss_bf16 and abs(loss_bf16) != float("inf")
    assert loss_fp8 != loss_bf16

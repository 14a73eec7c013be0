"""FP8 forward path on the CPU: the quantiser/linear oracle, the conversion of
block linears and the SSLMetaArch wiring (student.fp8_enabled / DINOV3_FP8)."""

import copy
import logging

import pytest
import torch
import torch.nn as nn

from dinov3_amd.layers.fp8_linear import convert_linears_to_fp8
from dinov3_amd.ops import fp8_eligible, fp8_linear, fp8_quantize_rows


# ---------------------------------------------------------------- quantiser

def _quant_case():
    g = torch.Generator().manual_seed(0)
    M, K = 67, 384
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.linspace(-10, 10, M)).view(M, 1)
    x[3].zero_()
    x[4] = x[4].clamp(-4.0, 4.0)
    x[4, 7] = 4.0  # amax an exact power of two
    x[5] = x[5].clamp(-1.75, 1.75)
    x[5, 0] = 1.75  # the m == 1.75 boundary: amax / s == 448 exactly
    return x.bfloat16()


def test_quantiser_scales_are_minimal_powers_of_two():
    x = _quant_case()
    q, s = fp8_quantize_rows(x)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert q.shape == x.shape and s.shape == (x.shape[0],)
    mant, _ = torch.frexp(s)
    assert bool((mant == 0.5).all()), "scale is not a power of two"
    amax = x.float().abs().amax(dim=1)
    nz = amax > 0
    ratio = amax[nz] / s[nz]
    assert bool((ratio <= 448).all())
    assert bool((2 * ratio > 448).all())
    assert float(amax[5] / s[5]) == 448.0
    assert float(amax[4] / s[4]) == 256.0


def test_quantiser_zero_row_and_finiteness():
    x = _quant_case()
    q, s = fp8_quantize_rows(x)
    assert float(s[3]) == 1.0
    assert bool((q[3].float() == 0).all())
    assert bool(torch.isfinite(q.float()).all())


def test_quantiser_reconstruction_error():
    """Every input within 2^-3 of its row's amax is a normal e4m3 number after
    scaling, so it comes back to <= 2^-4 relative (half an ulp of 3 mantissa bits)."""
    x = _quant_case()
    q, s = fp8_quantize_rows(x)
    xf = x.float()
    rec = q.float() * s[:, None]
    amax = xf.abs().amax(dim=1, keepdim=True)
    big = (xf.abs() >= amax / 8) & (xf != 0)
    rel = ((rec - xf).abs() / xf.abs().clamp_min(1e-30))[big]
    assert big.sum() > 1000
    assert float(rel.max()) <= 2.0 ** -4


def test_quantiser_any_float_dtype_on_cpu():
    x = _quant_case()
    q16, s16 = fp8_quantize_rows(x)
    q32, s32 = fp8_quantize_rows(x.float())
    assert torch.equal(s16, s32)
    assert torch.equal(q16.view(torch.uint8), q32.view(torch.uint8))


# ------------------------------------------------------------ integer exact

def _int_case(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    b = torch.randint(-8, 9, (N,), generator=g).float()
    if M > 1:
        x[M // 2].zero_()
    return x.bfloat16(), w.bfloat16(), b.bfloat16()


@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (33, 48, 128), (130, 272, 384)])
def test_fp8_linear_integer_exact(M, N, K):
    x, w, b = _int_case(M, N, K)
    ref = (x.float() @ w.float().t() + b.float()).to(torch.bfloat16)
    y = fp8_linear(x, w, b)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))
    ref_nb = (x.float() @ w.float().t()).to(torch.bfloat16)
    assert torch.equal(fp8_linear(x, w).view(torch.int16), ref_nb.view(torch.int16))


def test_fp8_linear_shapes_grads_and_eligibility():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 128, generator=g, requires_grad=True)
    w = torch.randn(32, 128, generator=g, requires_grad=True)
    b = torch.randn(32, generator=g, requires_grad=True)
    y = fp8_linear(x, w, b)
    assert y.shape == (2, 5, 32) and y.dtype == torch.float32
    dy = torch.randn(2, 5, 32, generator=g)
    y.backward(dy)
    # straight-through: the gradients of F.linear on the unquantised tensors
    x2, w2, b2 = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    torch.nn.functional.linear(x2, w2, b2).backward(dy)
    torch.testing.assert_close(x.grad, x2.grad)
    torch.testing.assert_close(w.grad, w2.grad)
    torch.testing.assert_close(b.grad, b2.grad)
    with torch.no_grad():
        assert not fp8_linear(x, w, b).requires_grad

    assert fp8_eligible(1024, 3072) and fp8_eligible(128, 16)
    assert not fp8_eligible(1000, 64) and not fp8_eligible(128, 24)
    with pytest.raises(RuntimeError, match="multiple"):
        fp8_linear(torch.randn(3, 100), torch.randn(16, 100))


# --------------------------------------------------------------- conversion

def _vit():
    from dinov3_amd.models.vision_transformer import vit_small

    torch.manual_seed(0)
    return vit_small(img_size=32, drop_path_rate=0.0, layerscale_init=1.0)


def test_convert_flags_exactly_the_block_linears():
    m = _vit()
    keys_before = list(m.state_dict().keys())
    names = convert_linears_to_fp8(m, "blocks")
    want = {f"blocks.{i}.{leaf}" for i in range(12)
            for leaf in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")}
    assert set(names) == want and len(names) == len(want)
    flagged = {n for n, mod in m.named_modules() if getattr(mod, "fp8", False)}
    assert flagged == want
    assert all(isinstance(dict(m.named_modules())[n], nn.Linear) for n in flagged)
    assert list(m.state_dict().keys()) == keys_before
    # converted and unconverted models load each other's weights
    other = _vit()
    other.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(other.state_dict(), strict=True)


def test_convert_with_no_match_keeps_output_bit_equal():
    m = _vit().eval()
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        before = m.forward_features(x)
    assert convert_linears_to_fp8(m, "no_such_module") == []
    with torch.no_grad():
        after = m.forward_features(x)
    for k in ("x_norm_clstoken", "x_norm_patchtokens"):
        assert torch.equal(before[k], after[k])


def test_convert_skips_ineligible_layers(caplog):
    net = nn.ModuleDict({"blocks": nn.Sequential(nn.Linear(128, 16), nn.Linear(100, 16),
                                                 nn.Linear(128, 24))})
    with caplog.at_level(logging.INFO, logger="dinov3"):
        names = convert_linears_to_fp8(net, "blocks")
    assert names == ["blocks.0"]
    assert "stay bf16" in caplog.text and "blocks.1" in caplog.text and "blocks.2" in caplog.text


def test_converted_model_forward_backward():
    m = _vit().train()
    x = torch.randn(2, 3, 32, 32)
    ref = m.forward_features(x)["x_norm_clstoken"]
    ref.float().pow(2).sum().backward()
    had_grad = {n for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)

    convert_linears_to_fp8(m, "blocks")
    out = m.forward_features(x)["x_norm_clstoken"]
    out.float().pow(2).sum().backward()
    assert bool(torch.isfinite(out).all())
    got_grad = {n for n, p in m.named_parameters() if p.grad is not None}
    assert had_grad <= got_grad
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n
    assert not torch.equal(out, ref), "fp8 path not taken"
    rel = float((out - ref).detach().norm() / ref.detach().norm())
    assert rel < 0.5, f"fp8 output is unrelated to the fp32 one (rel {rel})"


# -------------------------------------------------------------- SSLMetaArch

def _flag_names(module):
    return {n for n, mod in module.named_modules() if getattr(mod, "fp8", False)}


def _one_step(model, cfg):
    from bench import make_synthetic_batch

    batch = make_synthetic_batch(cfg, torch.device("cpu"), torch.float32, n_batches=1)[0]
    model.train()
    loss, _ = model(batch, teacher_temp=0.07, iteration=0)
    loss.backward()
    return loss.detach()


@pytest.mark.parametrize("how", ["config", "env"])
def test_meta_arch_fp8_on(smoke_cfg, how, monkeypatch, caplog):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch

    cfg = copy.deepcopy(smoke_cfg)
    if how == "config":
        monkeypatch.delenv("DINOV3_FP8", raising=False)
        cfg.student.fp8_enabled = True
    else:
        monkeypatch.setenv("DINOV3_FP8", "1")
        assert not cfg.student.fp8_enabled
    torch.manual_seed(0)
    with caplog.at_level(logging.INFO, logger="dinov3"):
        model = SSLMetaArch(cfg)
    assert "not implemented" not in caplog.text
    for backbone in (model.student_backbone, model.teacher_backbone):
        names = _flag_names(backbone)
        n_blocks = len(backbone.blocks)
        assert len(names) == 4 * n_blocks
        assert all(n.startswith("blocks.") for n in names)
    for head in (model.student_dino_head, model.teacher_dino_head,
                 model.student_ibot_head, model.teacher_ibot_head):
        assert not _flag_names(head)
    assert not _flag_names(model.student_backbone.patch_embed)
    loss = _one_step(model, cfg)
    assert bool(torch.isfinite(loss))


def test_meta_arch_fp8_off_by_default(smoke_cfg, monkeypatch):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch

    monkeypatch.delenv("DINOV3_FP8", raising=False)
    model = SSLMetaArch(copy.deepcopy(smoke_cfg))
    assert not _flag_names(model)
    assert model.fp8_enabled is False

"""ops.gram_loss on the CPU: the reference against the GramLoss code in fp64,
the gradient's destination, the CPU dispatch, and the DINOV3_FUSED_GRAM switch
on inputs the fused path does not take."""

import pytest
import torch

from dinov3_amd.loss.gram_loss import GramLoss

# (remove_neg, remove_only_teacher_neg)
MODES = [(False, False), (True, False), (False, True)]


def _inputs(G, M, D, dtype=torch.float64):
    """S = randn rounded to bf16, T = S + 0.5 randn drawn in fp64 and rounded to bf16."""
    gen = torch.Generator().manual_seed(1000 * G + M + D)
    s = torch.randn(G, M, D, generator=gen).bfloat16()
    t = (s.double() + 0.5 * torch.randn(G, M, D, generator=gen, dtype=torch.float64)).bfloat16()
    return s.to(dtype), t.to(dtype)


def _gram_loss_code(out, tgt, apply_norm, remove_neg, remove_only_teacher_neg):
    """GramLoss.forward without its cast to fp32 and without the constructor's
    assert (which excludes the unclamped mode), img_level=True."""
    if apply_norm:
        tgt = tgt / tgt.norm(dim=-1, keepdim=True)
        out = out / out.norm(dim=-1, keepdim=True)
    target_sim = tgt @ tgt.transpose(-1, -2)
    student_sim = out @ out.transpose(-1, -2)
    if remove_neg:
        target_sim = torch.where(target_sim < 0, torch.zeros_like(target_sim), target_sim)
        student_sim = torch.where(student_sim < 0, torch.zeros_like(student_sim), student_sim)
    elif remove_only_teacher_neg:
        both_neg = (student_sim < 0) & (target_sim < 0)
        student_sim = torch.where(both_neg, torch.zeros_like(student_sim), student_sim)
        target_sim = torch.where(target_sim < 0, torch.zeros_like(target_sim), target_sim)
    return ((student_sim - target_sim) ** 2).mean()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("apply_norm", [False, True])
@pytest.mark.parametrize("mode", MODES, ids=["plain", "remove_neg", "teacher_neg"])
def test_ref_matches_gramloss_code_fp64(mode, apply_norm, G):
    from dinov3_amd.ops import gram_loss_ref

    s, t = _inputs(G, 37, 24)
    s1, s2 = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
    got = gram_loss_ref(s1, t, apply_norm=apply_norm, remove_neg=mode[0],
                        remove_only_teacher_neg=mode[1])
    want = _gram_loss_code(s2, t, apply_norm, *mode)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert float(want.detach()) > 0
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
    got.backward()
    want.backward()
    torch.testing.assert_close(s1.grad, s2.grad, rtol=1e-10, atol=1e-14 * float(s2.grad.abs().max()))
    if mode != (False, False):  # the module itself, which computes in fp32
        module = GramLoss(apply_norm=apply_norm, remove_neg=mode[0], remove_only_teacher_neg=mode[1])
        torch.testing.assert_close(module(s, t).double(), want.detach(), rtol=1e-4, atol=0)


def test_ref_flattened_is_one_matrix():
    """G = 1 over all tokens is GramLoss with img_level=False."""
    from dinov3_amd.ops import gram_loss_ref

    s, t = _inputs(3, 20, 16, torch.float32)
    module = GramLoss(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False)
    got = gram_loss_ref(s.reshape(1, -1, 16), t.reshape(1, -1, 16), apply_norm=True,
                        remove_neg=True, remove_only_teacher_neg=False)
    torch.testing.assert_close(got, module(s, t, img_level=False), rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", MODES, ids=["plain", "remove_neg", "teacher_neg"])
def test_teacher_receives_no_gradient(mode):
    from dinov3_amd.ops import gram_loss

    s, t = _inputs(2, 19, 16, torch.float32)
    s.requires_grad_(True)
    t.requires_grad_(True)
    gram_loss(s, t, apply_norm=True, remove_neg=mode[0], remove_only_teacher_neg=mode[1]).backward()
    assert t.grad is None
    assert s.grad is not None and bool(s.grad.abs().max() > 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_cpu_op_is_the_reference(dtype):
    from dinov3_amd.ops import gram_loss, gram_loss_ref

    s, t = _inputs(2, 33, 24, dtype)
    kw = dict(apply_norm=True, remove_neg=False, remove_only_teacher_neg=True)
    s1, s2 = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
    got, want = gram_loss(s1, t, panel_bytes=1 << 20, **kw), gram_loss_ref(s2, t, **kw)
    assert got.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert torch.equal(got, want)
    got.backward()
    want.backward()
    assert s1.grad.dtype == dtype and torch.equal(s1.grad, s2.grad)


def test_op_argument_checks_cpu():
    from dinov3_amd.ops import gram_loss

    s, t = _inputs(1, 5, 8, torch.float32)
    kw = dict(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False)
    with pytest.raises(ValueError, match="one shape"):
        gram_loss(s, t[:, :4], **kw)
    with pytest.raises(ValueError, match="one shape"):
        gram_loss(s[0], t[0], **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("img_level", [True, False])
def test_switch_changes_nothing_off_the_fused_path(dtype, img_level, monkeypatch):
    """CPU tensors (of any dtype) never take the fused path: the module returns
    the same bits and the same gradient with DINOV3_FUSED_GRAM=1 as without."""
    s, t = _inputs(2, 21, 16, dtype)
    module = GramLoss(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False)
    results = []
    for value in (None, "1"):
        if value is None:
            monkeypatch.delenv("DINOV3_FUSED_GRAM", raising=False)
        else:
            monkeypatch.setenv("DINOV3_FUSED_GRAM", value)
        x = s.clone().requires_grad_(True)
        loss = module(x, t, img_level=img_level)
        loss.backward()
        results.append((loss.detach(), x.grad))
    assert torch.equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])

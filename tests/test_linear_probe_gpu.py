"""Linear probe on the device: ops.probe_ce and ops.probe_sgd_ against their
fp64 oracles, evaluate_linear_sharded with device tensors against the CPU fp32
run, and do_test behind DINOV3_EVAL_ON_DEVICE."""

import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CE_SHAPES = [(1, 1, 8), (5, 3, 1000), (67, 2, 520), (300, 1, 2048), (33, 2, 1001)]
DTYPES = [torch.bfloat16, torch.float32]


def _ce_inputs(B, G, C, dtype, with_bias, integer, seed=0):
    """(logits [B, G, Cp] in dtype, bias or None, labels with about 10 % of -1), on the CPU."""
    gen = torch.Generator().manual_seed(seed + 7 * B + C)
    Cp = (C + 7) // 8 * 8
    if integer:
        logits = torch.randint(-3, 4, (B, G, Cp), generator=gen).float()
        bias = torch.randint(-3, 4, (G, Cp), generator=gen).float()
    else:
        logits = 4.0 * torch.randn(B, G, Cp, generator=gen)
        bias = 4.0 * torch.randn(G, Cp, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    labels[torch.rand(B, generator=gen) < 0.1] = -1
    if B >= 5:
        labels[B // 2] = -1
    return logits.to(dtype), (bias if with_bias else None), labels


def _run_both(logits, bias, labels, C, scale, **kwargs):
    """(kernel outputs + gradient, oracle outputs + gradient), all on the CPU."""
    from dinov3_amd.ops import probe_ce, probe_ce_ref

    dev_logits = logits.cuda()
    loss, correct, dbias = probe_ce(dev_logits, None if bias is None else bias.cuda(),
                                    labels.cuda(), C, scale, True, **kwargs)
    ref_logits = logits.double()  # the same rounded inputs, the gradient unrounded
    ref = probe_ce_ref(ref_logits, bias, labels, C, scale, True)
    return (loss.cpu(), correct.cpu(), dbias.cpu(), dev_logits.cpu()), ref + (ref_logits,)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,C", CE_SHAPES)
def test_probe_ce_integer_data(B, G, C, dtype, with_bias):
    logits, bias, labels = _ce_inputs(B, G, C, dtype, with_bias, integer=True)
    (loss, correct, dbias, grad), (rloss, rcorrect, rdbias, rgrad) = _run_both(
        logits, bias, labels, C, 1.0)
    assert correct.dtype == torch.int64 and torch.equal(correct, rcorrect)
    ignored = labels < 0
    assert torch.equal(grad[ignored], torch.zeros_like(grad[ignored]))
    assert torch.equal(grad[:, :, C:], torch.zeros_like(grad[:, :, C:]))
    assert torch.equal(dbias[:, C:], torch.zeros_like(dbias[:, C:]))
    assert float((loss.double() - rloss.double()).abs().max()) <= 1e-5 * B * (1.0 + 6.0)  # |z| <= 6


@pytest.mark.parametrize("row_blocks", [0, 3])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,C", CE_SHAPES)
def test_probe_ce_normal_data(B, G, C, dtype, with_bias, row_blocks):
    """Bounds from the arithmetic, not from a run: a probability carries at most
    about 1e-5 relative error (v_exp_f32, the fp32 row sum over <= 2048 terms,
    one reciprocal), and the rounding to bf16 at most 2^-8 of the value (half a
    unit of an 8-bit significand), so the bf16 gradient can come close to
    rtol |ref|; the absolute term takes the probability's error, <= 1e-5 scale."""
    logits, bias, labels = _ce_inputs(B, G, C, dtype, with_bias, integer=False)
    scale = 1.0 / B
    (loss, correct, dbias, grad), (rloss, rcorrect, rdbias, rgrad) = _run_both(
        logits, bias, labels, C, scale, row_blocks=row_blocks)
    rtol = 2.0 ** -8 if dtype == torch.bfloat16 else 2e-5
    err = (grad.double() - rgrad).abs()
    bound = rtol * rgrad.abs() + 2e-5 * scale
    print(f"grad: max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    db_err = float((dbias.double() - rdbias.double()).abs().max())
    print(f"dbias: max err = {db_err:.3e}, bound = {2e-5 * scale * B:.3e}")
    assert db_err <= 2e-5 * scale * B
    z = logits.double() + (0 if bias is None else bias.double())
    loss_bound = 1e-5 * B * (1.0 + float(z[:, :, :C].abs().max()))
    loss_err = float((loss.double() - rloss.double()).abs().max())
    print(f"loss: max err = {loss_err:.3e}, bound = {loss_bound:.3e}")
    assert loss_err <= loss_bound
    # equal bf16 maxima are exact on both sides; fp32 near-ties are too rare to meet here
    assert torch.equal(correct, rcorrect)
    assert torch.equal(grad[:, :, C:], torch.zeros_like(grad[:, :, C:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,C", [(67, 2, 520), (300, 1, 2048), (33, 2, 1001)])
def test_probe_ce_deterministic_and_forward_only(B, G, C, dtype):
    from dinov3_amd.ops import probe_ce

    logits, bias, labels = _ce_inputs(B, G, C, dtype, True, integer=False)
    logits, bias, labels = logits.cuda(), bias.cuda(), labels.cuda()
    a, b = logits.clone(), logits.clone()
    out_a = probe_ce(a, bias, labels, C, 1.0 / B, True)
    out_b = probe_ce(b, bias, labels, C, 1.0 / B, True)
    for x, y in zip(out_a + (a,), out_b + (b,)):
        assert torch.equal(x, y)
    keep = logits.clone()
    loss, correct, none = probe_ce(keep, bias, labels, C, 1.0 / B, False)
    assert none is None and torch.equal(keep, logits)
    assert torch.equal(loss, out_a[0]) and torch.equal(correct, out_a[1])
    # no rows: zeros, no launch
    loss, correct, dbias = probe_ce(logits[:0].contiguous(), bias, labels[:0], C, 1.0, True)
    assert not loss.any() and not correct.any() and not dbias.any()
    assert loss.shape == (G,) and correct.dtype == torch.int64 and dbias.shape == bias.shape


def test_probe_ce_argument_checks():
    from dinov3_amd.ops import probe_ce

    labels = torch.zeros(4, dtype=torch.long, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        probe_ce(torch.zeros(4, 1, 12, device="cuda"), None, labels, 12, 1.0)
    with pytest.raises(RuntimeError, match="2048"):
        probe_ce(torch.zeros(4, 1, 2056, device="cuda"), None, labels, 2056, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        probe_ce(torch.zeros(4, 1, 32, device="cuda")[:, :, ::2], None, labels, 16, 1.0)
    with pytest.raises(RuntimeError, match="contiguous HIP tensor"):  # labels on the host
        probe_ce(torch.zeros(4, 1, 16, device="cuda"), None, labels.cpu(), 16, 1.0)
    with pytest.raises(RuntimeError, match="contiguous HIP tensor"):  # bias on the host
        probe_ce(torch.zeros(4, 1, 16, device="cuda"), torch.zeros(1, 16), labels, 16, 1.0)
    with pytest.raises(RuntimeError, match="bias must be fp32"):
        probe_ce(torch.zeros(4, 1, 16, device="cuda"), torch.zeros(2, 16, device="cuda"), labels,
                 16, 1.0)
    with pytest.raises(RuntimeError, match="C <= Cp"):
        probe_ce(torch.zeros(4, 1, 16, device="cuda"), None, labels, 17, 1.0)


@pytest.mark.parametrize("with_wd", [False, True])
@pytest.mark.parametrize("grad_dtype", DTYPES)
@pytest.mark.parametrize("G,R", [(1, 8), (3, 1000 * 64), (2, 1008)])
def test_probe_sgd_against_oracle(G, R, grad_dtype, with_wd):
    """|w - ref| and |mom - ref| <= 2^-21 (|w| + |mom| + |grad| + wd |w|)
    elementwise: four fp32 roundings with slack. Every step starts from the
    kernel's own state, so the bound is per step."""
    from dinov3_amd.ops import probe_sgd_, probe_sgd_ref_

    gen = torch.Generator().manual_seed(G * 131 + R)
    w = torch.randn(G, R, generator=gen).cuda()
    mom = torch.randn(G, R, generator=gen).cuda()
    lr = torch.tensor([0.1, 0.01, 1.0][:G]).cuda()
    wd = torch.tensor([1e-2, 0.0, 0.5][:G]).cuda() if with_wd else None
    w_lp = torch.zeros(G, R, dtype=torch.bfloat16, device="cuda")
    for scale in (1.0, 0.37):
        grad = torch.randn(G, R, generator=gen).to(grad_dtype).cuda()
        rw, rm = w.double(), mom.double()
        wd_term = (wd.double().view(-1, 1) * rw.abs()) if with_wd else 0.0
        bound = 2.0 ** -21 * (rw.abs() + rm.abs() + grad.double().abs() + wd_term)
        probe_sgd_ref_(rw, rm, grad, lr, wd, scale, 0.9, None)  # fp64 state: no rounding
        probe_sgd_(w, mom, grad, lr, wd, scale, 0.9, w_lp)
        for got, ref, name in ((w, rw, "w"), (mom, rm, "mom")):
            err = (got.double() - ref).abs()
            print(f"{name}: max err/bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), name
        assert torch.equal(w_lp, w.bfloat16())
    # without the bf16 copy nothing else changes
    w2, m2 = w.clone(), mom.clone()
    probe_sgd_(w, mom, grad, lr, wd, 0.5, 0.9, w_lp)
    probe_sgd_(w2, m2, grad, lr, wd, 0.5, 0.9, None)
    assert torch.equal(w, w2) and torch.equal(mom, m2)


def test_probe_sgd_argument_checks():
    from dinov3_amd.ops import probe_sgd_

    w = torch.zeros(2, 12, device="cuda")
    lr = torch.ones(2, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        probe_sgd_(w, w.clone(), w.clone(), lr, None, 1.0, 0.9, None)
    w = torch.zeros(2, 16, device="cuda")
    with pytest.raises(RuntimeError, match="lr"):
        probe_sgd_(w, w.clone(), w.clone(), lr[:1], None, 1.0, 0.9, None)
    with pytest.raises(RuntimeError, match="w_lp"):
        probe_sgd_(w, w.clone(), w.clone(), lr, None, 1.0, 0.9, torch.zeros(2, 16, device="cuda"))


# ------------------------------------------------------------ end to end
def planted_clusters(seed=0, classes=8, dim=64, train_per_class=32, val_per_class=8):
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(classes, dim, generator=g), dim=1)

    def replicas(n):
        x = protos.repeat_interleave(n, dim=0)
        return x + 1e-2 * torch.randn(x.shape, generator=g), torch.arange(classes).repeat_interleave(n)

    return replicas(train_per_class) + replicas(val_per_class)


def overlapping_classes(seed=0, classes=10, dim=32, n_train=1000, n_val=400):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(classes, dim, generator=g)

    def draw(n):
        y = torch.randint(0, classes, (n,), generator=g)
        return centres[y] + 1.5 * torch.randn(n, dim, generator=g) + 3.0, y

    return draw(n_train) + draw(n_val)


GRID = dict(lrs=(1e-3, 1e-2, 1e-1, 1.0), wds=(0.0, 1e-3), epochs=3, batch_size=128)


@functools.lru_cache(maxsize=None)
def _cpu_fp32_reference():
    from dinov3_amd.eval import evaluate_linear_sharded

    return evaluate_linear_sharded(*overlapping_classes(), precision="fp32", **GRID)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_evaluate_linear_sharded_device_planted_clusters(precision):
    from dinov3_amd.eval import evaluate_linear_sharded

    data = [t.cuda() for t in planted_clusters()]
    out = evaluate_linear_sharded(*data, lrs=(1e-3, 1e-2, 1e-1, 1.0), epochs=10, batch_size=48,
                                  precision=precision)
    assert out["top1"] == [1.0] * 4
    assert out["best_head"] == 0


# Largest per-head differences between the device run and the CPU fp32 run of
# this grid, as measured (profiles/linear_probe.md); the test allows three times
# as much, for GEMM algorithm selection differing between machines.
MEASURED = {"bf16": {"val_loss": 2.213e-4, "top1": 0.0}, "fp32": {"val_loss": 3.06e-7, "top1": 0.0}}


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_evaluate_linear_sharded_device_matches_cpu_fp32(precision):
    from dinov3_amd.eval import evaluate_linear_sharded

    ref = _cpu_fp32_reference()
    data = [t.cuda() for t in overlapping_classes()]
    out = evaluate_linear_sharded(*data, precision=precision, **GRID)
    loss_diff = max(abs(a - b) for a, b in zip(out["val_loss"], ref["val_loss"]))
    top1_diff = max(abs(a - b) for a, b in zip(out["top1"], ref["top1"]))
    print(f"{precision}: max |val_loss - cpu fp32| = {loss_diff:.3e}, "
          f"max |top1 - cpu fp32| = {top1_diff:.4f} ({round(top1_diff * 400)} of 400)")
    assert out["heads"] == ref["heads"]
    assert loss_diff <= 3 * MEASURED[precision]["val_loss"]
    assert top1_diff <= 3 * MEASURED[precision]["top1"] + 1e-12


def test_do_test_linear_on_device(smoke_cfg, monkeypatch):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch
    from dinov3_amd.train.train import do_test

    monkeypatch.setenv("DINOV3_EVAL_ON_DEVICE", "1")
    cfg = copy.deepcopy(smoke_cfg)
    cfg.train.dataset_path = "Synthetic:split=TRAIN:length=32"
    model = SSLMetaArch(cfg)
    results = do_test(cfg, model, iteration=0)
    heads = [k for k in results if k.startswith("linear_top1_head")]
    assert len(heads) == 8 and "linear_best_lr" in results
    for key in ["linear_top1", "linear_best_lr"] + heads:
        assert 0.0 <= results[key] <= 1.0, (key, results[key])
    assert results["linear_top1"] == max(results[k] for k in heads)

"""The segmentation-probe kernel against its fp64 oracle on the same rounded
inputs, run-to-run bit-equality, the forward-only form, the argument checks,
the evaluation on the device against its CPU fp32 run, and do_test behind
DINOV3_EVAL_SEG."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (M, h, w, s, G, C): degenerate; plain; the one- and two-class-per-lane boundary on
# single-column and single-row images; non-dyadic weights; ADE20K; Cp = 256, the limit;
# many blocks and interior cells; more quads than the grid has waves, so that a wave walks
# two (1024 blocks over all heads, four waves each)
SHAPES = [(1, 1, 1, 2, 1, 1), (2, 3, 5, 2, 2, 7), (1, 5, 1, 4, 1, 64), (1, 1, 5, 4, 2, 65),
          (2, 4, 4, 14, 3, 21), (1, 2, 3, 16, 1, 150), (1, 1, 4, 8, 2, 255),
          (3, 7, 6, 16, 2, 150), (3, 27, 26, 2, 2, 7)]
DYADIC = [shape for shape in SHAPES if shape[3] in (2, 4, 8, 16)]
DTYPES = [torch.bfloat16, torch.float32]
U = 2.0 ** -24  # unit roundoff of fp32


def _inputs(shape, dtype, with_bias, integer):
    """(logits [M, h, w, G, Cp] in dtype, bias or None, labels with about 10 % of 255; one
    image fully ignored when there are several), on the CPU."""
    M, h, w, s, G, C = shape
    gen = torch.Generator().manual_seed(131 * M + 17 * h + 7 * w + s + C)
    Cp = (C + 7) // 8 * 8
    if integer:
        logits = torch.randint(-3, 4, (M, h, w, G, Cp), generator=gen).float()
        bias = torch.randint(-3, 4, (G, Cp), generator=gen).float()
    else:
        logits = 3.0 * torch.randn(M, h, w, G, Cp, generator=gen)
        bias = torch.randn(G, Cp, generator=gen)
    logits[..., C:] = 50.0  # the pad columns hold the largest values and must not count
    labels = torch.randint(0, C, (M, s * h, s * w), generator=gen).to(torch.uint8)
    labels[torch.rand(labels.shape, generator=gen) < 0.1] = 255
    if M > 1:
        labels[M - 1] = 255
    return logits.to(dtype), (bias if with_bias else None), labels


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, with_bias, integer):
    """One kernel run and one oracle run of a case, shared by the tests that need them."""
    from dinov3_amd.ops import seg_ce, seg_ce_ref

    logits, bias, labels = _inputs(shape, dtype, with_bias, integer)
    C = shape[5]
    valid = int((labels != 255).sum())
    scale = 1.0 / max(valid, 1)
    dev_logits = logits.cuda()
    loss, areas, dbias = seg_ce(dev_logits, None if bias is None else bias.cuda(), labels.cuda(),
                                C, scale, True)
    ref_logits = logits.double()  # the same rounded inputs, the gradient unrounded
    ref = seg_ce_ref(ref_logits, bias, labels, C, scale, True)
    got = (loss.cpu(), areas.cpu(), dbias.cpu(), dev_logits.cpu())
    return (logits, bias, labels, scale), got, ref + (ref_logits,)


def _loss_bound(shape, pixels, Z, rloss):
    """The loss bound of test_seg_ce_normal_data's docstring, per head."""
    M, h, w, s, G, C = shape
    groups, cap = (M * h * w + 3) // 4, max(1024 // G, 1)  # the launch: <= 1024 blocks in all
    rounds = (groups + cap - 1) // cap
    adds = 2.25 * s * s * rounds + 4 + min(groups, cap)
    return pixels * (37 * Z + 23) * U + (adds + 1) * U * rloss.double()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DYADIC, ids=str)
def test_seg_ce_integer_data(shape, dtype, with_bias):
    """Integer logits upsample exactly in fp32 at the dyadic scales: the counts
    are exactly the oracle's, the lowest-index rule among equal maxima included."""
    (logits, bias, labels, _), (loss, areas, dbias, grad), (rloss, rareas, rdbias, rgrad) = _case(
        shape, dtype, with_bias, True)
    M, h, w, s, G, C = shape
    assert areas.dtype == torch.int64 and torch.equal(areas, rareas)
    assert torch.equal(areas[:, 2].sum(dim=1), (labels != 255).sum().expand(G))
    assert torch.equal(grad[..., C:], torch.zeros_like(grad[..., C:]))
    assert torch.equal(dbias[:, C:], torch.zeros_like(dbias[:, C:]))
    if M > 1:  # the last image is ignored as a whole
        assert torch.equal(grad[M - 1], torch.zeros_like(grad[M - 1]))
    pixels = int((labels != 255).sum())
    loss_err = (loss.double() - rloss.double()).abs()
    assert bool((loss_err <= _loss_bound(shape, pixels, 6.0 if with_bias else 3.0, rloss)).all())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_seg_ce_normal_data(shape, dtype, with_bias):
    """Bounds from the kernel's own rounding steps, u = 2^-24, Z = max |logit| +
    max |bias| (|z| <= Z: the taps are a convex combination); none is fitted to a run.

    z. An axis weight is one correctly rounded division, |dw| <= u; 1 - w adds
    one rounding, <= 2u; a tap weight is the product of two such factors a, b,
    |dw_t| <= 2u (a + b) + u a b, which sums to <= 9u over the four taps
    (<= 5u each). Four roundings in the mul/fma chain and one in the bias add:
    |dz| <= 9u Z + 4u Z + u Z <= 16u Z.
    p. Softmax sees differences of z: 2 |dz| = 32u Z relative. z - max rounds
    by <= 2u Z, the scaling by log2(e) inside __expf by as much again, v_exp_f32
    is good to 1 ulp = 2u; the sum over <= 256 terms is <= 4 adds in a lane and
    6 butterfly steps, 10u; one reciprocal, 2u, one product, u:
    eps_p = (36 Z + 15) u relative, and |d(p - onehot)| <= eps_p p + u.
    Gradient of a cell. The tap weights reaching a cell sum to s^2 (s per
    axis), over <= (2s)^2 pixels. Weight errors: 5u (2s)^2 = 20u s^2; softmax
    errors: (eps_p + u) s^2; fp32 accumulation, <= (1.5 s)^2 fmas in a quad, <= 9
    adds in the finalize and the product with grad_scale, each <= u times the
    sum of |terms| <= s^2: (2.25 s^2 + 10) u s^2. Together
    E = grad_scale s^2 u (36 Z + 2.25 s^2 + 46), then one rounding to the logits
    dtype, 2^-8 relative in bf16 and u in fp32.
    dbias. The unrounded cell values, E each, summed over n cells in fp32 in
    some fixed order: <= n E + n u sum |cell values|.
    Loss. Per pixel lse - z[label]: 2 |dz| from the two z, (2 Z + 12) u from
    the exp sum, 11u from v_log_f32 (1 ulp of a log <= ln 256), 3u Z from the
    two additions: (37 Z + 23) u. The terms are >= 0, so every partial sum is
    <= the total; a path has <= 2.25 s^2 adds per quad of the wave, 4 across
    waves, and one per block of the head (<= quads / 4, <= 1024 / G).
    Counts. A prediction can differ only where the two largest z are within
    2 |dz| of each other; each such pixel moves at most three counts."""
    (logits, bias, labels, scale), (loss, areas, dbias, grad), (rloss, rareas, rdbias, rgrad) = \
        _case(shape, dtype, with_bias, False)
    M, h, w, s, G, C = shape
    Z = float(logits[..., :C].double().abs().max()) + (float(bias[:, :C].abs().max())
                                                       if with_bias else 0.0)
    pixels = int((labels != 255).sum())
    E = scale * s * s * U * (36 * Z + 2.25 * s * s + 46)
    rtol = 2.0 ** -8 if dtype == torch.bfloat16 else U
    ref_cells = rgrad[..., :C]
    err = (grad[..., :C].double() - ref_cells).abs()
    bound = rtol * (ref_cells.abs() + E) + E
    print(f"grad: max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(grad[..., C:], torch.zeros_like(grad[..., C:]))
    if M > 1:
        assert torch.equal(grad[M - 1], torch.zeros_like(grad[M - 1]))

    n = M * h * w
    db_err = (dbias[:, :C].double() - rdbias[:, :C].double()).abs()
    db_bound = n * E + n * U * ref_cells.abs().sum(dim=(0, 1, 2)) + U * rdbias[:, :C].abs()
    print(f"dbias: max err/bound = {float((db_err / db_bound).max()):.3f}")
    assert bool((db_err <= db_bound).all())
    assert torch.equal(dbias[:, C:], torch.zeros_like(dbias[:, C:]))

    loss_bound = _loss_bound(shape, pixels, Z, rloss)  # + u rloss: the oracle returns fp32
    loss_err = (loss.double() - rloss.double()).abs()
    print(f"loss: max err/bound = {float((loss_err / loss_bound.clamp(min=1e-30)).max()):.3f}")
    assert bool((loss_err <= loss_bound).all())

    # the pixels whose two largest z are closer than 2 |dz|, from the literal upsampling
    H, W = s * h, s * w
    x = logits[..., :C].double().permute(0, 3, 4, 1, 2).reshape(M, G * C, h, w)
    up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).view(M, G, C, H, W)
    if with_bias:
        up = up + bias[:, :C].double().view(1, G, C, 1, 1)
    assert torch.equal(areas[:, 2], rareas[:, 2])
    if C > 1:
        top2 = up.topk(2, dim=2).values
        near = ((top2[:, :, 0] - top2[:, :, 1]) < 2 * 16 * U * Z) & (labels != 255).unsqueeze(1)
        near = near.sum(dim=(0, 2, 3))  # per head
    else:
        near = torch.zeros(G, dtype=torch.long)
    moved = (areas - rareas).abs().sum(dim=(1, 2))
    print(f"counts: moved {moved.tolist()}, near-ties {near.tolist()}")
    assert bool((moved <= 3 * near).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 5, 2, 2, 7), (1, 1, 5, 4, 2, 65), (3, 7, 6, 16, 2, 150),
                                   (3, 27, 26, 2, 2, 7)], ids=str)
def test_seg_ce_deterministic_and_forward_only(shape, dtype):
    from dinov3_amd.ops import seg_ce

    (logits, bias, labels, scale), got, _ = _case(shape, dtype, True, False)
    C = shape[5]
    logits, bias, labels = logits.cuda(), bias.cuda(), labels.cuda()
    again = logits.clone()
    out = seg_ce(again, bias, labels, C, scale, True)
    for x, y in zip(out + (again,), got):
        assert torch.equal(x.cpu(), y)
    # the scale as a device tensor: the same bits
    third = logits.clone()
    out3 = seg_ce(third, bias, labels, C, torch.tensor([scale], device="cuda"), True)
    for x, y in zip(out3 + (third,), got):
        assert torch.equal(x.cpu(), y)
    keep = logits.clone()
    loss, areas, none = seg_ce(keep, bias, labels, C, scale, False)
    assert none is None and torch.equal(keep, logits)
    assert torch.equal(loss.cpu(), got[0]) and torch.equal(areas.cpu(), got[1])
    # no images: zeros, no launch
    loss, areas, dbias = seg_ce(logits[:0].contiguous(), bias, labels[:0].contiguous(), C, 1.0,
                                True)
    assert not loss.any() and not areas.any() and not dbias.any()
    assert loss.shape == (shape[4],) and areas.dtype == torch.int64
    assert areas.shape == (shape[4], 3, bias.shape[1]) and dbias.shape == bias.shape


def test_seg_ce_argument_checks():
    from dinov3_amd.ops import SEG_MAX_CLASSES, hip_ops, seg_ce

    assert hip_ops().SEG_MAX_CLASSES == SEG_MAX_CLASSES == 255

    def logits(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    labels = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"\[M, h, w, G, Cp\]"):
        seg_ce(logits(2, 2, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        seg_ce(logits(1, 2, 2, 1, 8, dtype=torch.float16), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="uint8"):
        seg_ce(logits(1, 2, 2, 1, 8), None, labels.long(), 3, 1.0)
    with pytest.raises(RuntimeError, match="uint8"):  # another M
        seg_ce(logits(2, 2, 2, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="one integer s"):
        seg_ce(logits(1, 2, 1, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="one integer s"):
        seg_ce(logits(1, 3, 3, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="even"):  # s = 1
        seg_ce(logits(1, 4, 4, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="even"):  # s = 3
        seg_ce(logits(1, 1, 1, 1, 8), None, labels[:, :3, :3].contiguous(), 3, 1.0)
    with pytest.raises(RuntimeError, match="even"):  # s = 34
        seg_ce(logits(1, 1, 1, 1, 8), None,
               torch.zeros(1, 34, 34, dtype=torch.uint8, device="cuda"), 3, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        seg_ce(logits(1, 2, 2, 1, 12), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="256"):
        seg_ce(logits(1, 2, 2, 1, 264), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="C <= min"):
        seg_ce(logits(1, 2, 2, 1, 8), None, labels, 9, 1.0)
    with pytest.raises(RuntimeError, match="C <= min"):
        seg_ce(logits(1, 2, 2, 1, 8), None, labels, 0, 1.0)
    with pytest.raises(RuntimeError, match="C <= min"):  # 256 classes do not fit a uint8 label
        seg_ce(logits(1, 2, 2, 1, 256), None, labels, 256, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        seg_ce(logits(1, 2, 2, 1, 16)[..., ::2], None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="contiguous HIP tensor"):  # labels on the host
        seg_ce(logits(1, 2, 2, 1, 8), None, labels.cpu(), 3, 1.0)
    with pytest.raises(RuntimeError, match="contiguous HIP tensor"):  # bias on the host
        seg_ce(logits(1, 2, 2, 1, 8), torch.zeros(1, 8), labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="bias must be fp32"):
        seg_ce(logits(1, 2, 2, 1, 8), logits(2, 8), labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        seg_ce(logits(1 * 2 * 2 * 8 + 1)[1:].view(1, 2, 2, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(RuntimeError, match="scale must be one fp32"):
        seg_ce(logits(1, 2, 2, 1, 8), None, labels, 3, torch.ones(2, device="cuda"))


# ------------------------------------------------------------ end to end
def planted_segmentation(seed=0, n_train=64, n_val=16, cells=4, s=4, classes=6, dim=32,
                         ignore=0.05, noise=0.5):
    """The planted problem of tests/test_seg_probe.py."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(classes, dim, generator=g)

    def draw(n):
        coarse = torch.randint(0, classes, (n, cells // 2, cells // 2), generator=g)
        cell_cls = coarse.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        feats = protos[cell_cls] + noise * torch.randn(n, cells, cells, dim, generator=g) + 2.0
        labels = cell_cls.repeat_interleave(s, dim=1).repeat_interleave(s, dim=2).to(torch.uint8)
        labels[torch.rand(labels.shape, generator=g) < ignore] = 255
        return feats, labels

    return draw(n_train) + draw(n_val)


PLANTED = dict(num_classes=6, epochs=20, batch_images=16)


@functools.lru_cache(maxsize=None)
def _cpu_fp32_reference():
    from dinov3_amd.eval import evaluate_segmentation_linear

    return evaluate_segmentation_linear(*planted_segmentation(), precision="fp32", **PLANTED)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_evaluate_segmentation_linear_device_against_cpu_fp32(precision):
    """The pass condition is the CPU test's: the best head reaches mIoU 0.95.
    The per-head differences from the CPU fp32 run are printed, not bounded."""
    from dinov3_amd.eval import evaluate_segmentation_linear

    ref = _cpu_fp32_reference()
    data = [t.cuda() for t in planted_segmentation()]
    out = evaluate_segmentation_linear(*data, precision=precision, **PLANTED)
    miou_diff = max(abs(a - b) for a, b in zip(out["miou"], ref["miou"]))
    loss_diff = max(abs(a - b) for a, b in zip(out["val_loss"], ref["val_loss"]))
    print(f"{precision}: best mIoU {out['best_miou']:.4f} (cpu fp32 {ref['best_miou']:.4f}), "
          f"max |mIoU - cpu fp32| = {miou_diff:.3e}, max |val_loss - cpu fp32| = {loss_diff:.3e}")
    assert out["heads"] == ref["heads"] and len(out["miou"]) == 8
    assert ref["best_miou"] >= 0.95
    assert out["best_miou"] >= 0.95
    assert out["best_miou"] == out["miou"][out["best_head"]] == max(out["miou"])


def test_do_test_segmentation_on_device(smoke_cfg, monkeypatch):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch
    from dinov3_amd.train.train import do_test

    monkeypatch.setenv("DINOV3_EVAL_ON_DEVICE", "1")
    monkeypatch.setenv("DINOV3_EVAL_SEG", "SyntheticSeg")
    cfg = copy.deepcopy(smoke_cfg)
    cfg.train.dataset_path = "Synthetic:split=TRAIN:length=32"
    cfg.crops.global_crops_size = 64  # 4 x 4 cells, s = 16
    model = SSLMetaArch(cfg)
    results = do_test(cfg, model, iteration=0)
    heads = [f"seg_miou_head{i}" for i in range(8)]
    for key in ["seg_miou", "seg_pixel_acc", "seg_best_lr"] + heads:
        assert 0.0 <= results[key] <= 1.0, (key, results[key])
    assert results["seg_miou"] == max(results[k] for k in heads)
    assert "knn_top1" in results and "linear_top1" in results

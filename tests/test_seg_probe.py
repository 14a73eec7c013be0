"""Linear segmentation probe on the CPU: the plain-torch oracle of `seg_ce`
against the literal F.interpolate + F.cross_entropy composite and against
literal counting, one head against torch.optim.SGD, the grid against one-head
runs, a gloo world-2 run against the single-process result, a planted problem,
the data side, and do_test behind DINOV3_EVAL_SEG."""

import copy
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

WORLD = 2
ORACLE_SHAPES = [(2, 3, 5, 2, 2, 7), (1, 4, 4, 14, 1, 21), (1, 2, 3, 16, 1, 150),
                 (1, 1, 1, 4, 1, 3), (1, 1, 3, 8, 2, 9)]


def seg_inputs(M, h, w, s, G, C, integer=False, ignore=0.1, seed=0):
    """(logits [M, h, w, G, Cp] fp32 with large pad columns, bias [G, Cp],
    labels [M, s h, s w] uint8 with a share `ignore` of 255)."""
    gen = torch.Generator().manual_seed(seed + 131 * M + 17 * h + 7 * w + s + C)
    Cp = (C + 7) // 8 * 8
    if integer:
        logits = torch.randint(-3, 4, (M, h, w, G, Cp), generator=gen).float()
        bias = torch.randint(-3, 4, (G, Cp), generator=gen).float()
    else:
        logits = 3.0 * torch.randn(M, h, w, G, Cp, generator=gen)
        bias = torch.randn(G, Cp, generator=gen)
    logits[..., C:] = 50.0  # the pad columns hold the largest values and must not count
    labels = torch.randint(0, C, (M, s * h, s * w), generator=gen).to(torch.uint8)
    labels[torch.rand(labels.shape, generator=gen) < ignore] = 255
    return logits, bias, labels


def composite(logits, bias, labels, C, scale):
    """The literal form in fp64: (loss_sum [G], d/dlogits [M, h, w, G, C], dbias [G, C])."""
    M, h, w, G, _ = logits.shape
    H, W = labels.shape[1:]
    x = logits[..., :C].double().clone().requires_grad_(True)
    b = bias[:, :C].double().clone().requires_grad_(True)
    up = F.interpolate(x.permute(0, 3, 4, 1, 2).reshape(M, G * C, h, w), size=(H, W),
                       mode="bilinear", align_corners=False)
    up = up.view(M, G, C, H, W) + b.view(1, G, C, 1, 1)
    losses = torch.stack([F.cross_entropy(up[:, g], labels.long(), ignore_index=255,
                                          reduction="sum") for g in range(G)])
    (losses.sum() * scale).backward()
    return losses.detach(), x.grad, b.grad, up.detach()


@pytest.mark.parametrize("M,h,w,s,G,C", ORACLE_SHAPES)
def test_seg_ce_ref_against_interpolate_and_cross_entropy(M, h, w, s, G, C):
    from dinov3_amd.ops import seg_ce_ref

    logits, bias, labels = seg_inputs(M, h, w, s, G, C)
    scale = 0.37
    want_loss, want_grad, want_db, _ = composite(logits, bias, labels, C, scale)
    work = logits.double()  # the gradient comes back unrounded
    loss, areas, dbias = seg_ce_ref(work, bias, labels, C, scale, True)
    assert loss.dtype == torch.float32 and areas.dtype == torch.int64
    assert dbias.dtype == torch.float32 and dbias.shape == bias.shape
    assert areas.shape == (G, 3, bias.shape[1])
    assert torch.allclose(loss.double(), want_loss, rtol=1e-6, atol=0.0)
    grad_err = float((work[..., :C] - want_grad).abs().max())
    print(f"max |grad - autograd| = {grad_err:.3e}")
    assert grad_err <= 1e-12
    assert torch.allclose(dbias[:, :C].double(), want_db, rtol=1e-6, atol=1e-7)
    assert not work[..., C:].any() and not dbias[:, C:].any()
    assert torch.equal(areas[:, 2].sum(dim=1), (labels != 255).sum().expand(G))
    # without the gradient the logits stay and the sums are the same
    keep = logits.clone()
    loss2, areas2, none = seg_ce_ref(keep, bias, labels, C, scale, False)
    assert none is None and torch.equal(keep, logits)
    assert torch.equal(loss2, loss) and torch.equal(areas2, areas)


@pytest.mark.parametrize("s", [2, 4, 8, 16])
def test_seg_ce_ref_areas_against_literal_counting(s):
    """Integer logits in [-3, 3] (+ an integer bias) upsample exactly at the
    dyadic scales, so equal maxima are equal on every path and the
    lowest-index rule decides the tied pixels."""
    from dinov3_amd.ops import seg_ce_ref

    M, h, w, G, C = 2, 3, 4, 2, 5
    logits, bias, labels = seg_inputs(M, h, w, s, G, C, integer=True)
    _, areas, _ = seg_ce_ref(logits.clone(), bias, labels, C, 1.0, False)
    up = composite(logits, bias, labels, C, 1.0)[3]  # [M, G, C, H, W], exact in fp64
    assert torch.equal(up, (up * 4 * s * s).round() / (4 * s * s))
    ties = 0
    for g in range(G):
        want = torch.zeros(3, C, dtype=torch.long)
        z = up[:, g].permute(0, 2, 3, 1).reshape(-1, C).tolist()
        for row, lab in zip(z, labels.reshape(-1).tolist()):
            if lab == 255:
                continue
            top = max(row)
            ties += row.count(top) > 1
            pred = row.index(top)  # the lowest index among the maxima
            want[1, pred] += 1
            want[2, lab] += 1
            want[0, lab] += pred == lab
        assert torch.equal(areas[g, :, :C], want)
        assert not areas[g, :, C:].any()
    assert ties > 0


def test_seg_ce_ref_ignored_image_and_pad_columns():
    from dinov3_amd.ops import seg_ce_ref

    M, h, w, s, G, C = 3, 2, 3, 4, 2, 5
    logits, bias, labels = seg_inputs(M, h, w, s, G, C)
    labels[1] = 255
    work = logits.clone()
    loss, areas, dbias = seg_ce_ref(work, bias, labels, C, 1.0, True)
    assert not work[1].any()  # a fully ignored image: zero gradient
    assert work[0, ..., :C].any() and work[2, ..., :C].any()
    assert not work[..., C:].any() and not dbias[:, C:].any() and not areas[:, :, C:].any()
    others = [0, 2]
    loss2, areas2, dbias2 = seg_ce_ref(logits[others].clone(), bias, labels[others], C, 1.0, True)
    assert torch.allclose(loss, loss2, rtol=1e-6) and torch.equal(areas, areas2)
    assert torch.allclose(dbias, dbias2, rtol=1e-5, atol=1e-6)
    # nothing at all
    loss0, areas0, dbias0 = seg_ce_ref(logits[:0].clone(), bias, labels[:0], C, 1.0, True)
    assert not loss0.any() and not areas0.any() and not dbias0.any()


def test_seg_ce_argument_checks_cpu():
    from dinov3_amd.ops import SEG_MAX_CLASSES, seg_ce

    assert SEG_MAX_CLASSES == 255
    labels = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="even"):
        seg_ce(torch.zeros(1, 4, 4, 1, 8), None, labels, 3, 1.0)  # s = 1
    with pytest.raises(ValueError, match="one integer s"):
        seg_ce(torch.zeros(1, 2, 1, 1, 8), None, labels, 3, 1.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        seg_ce(torch.zeros(1, 2, 2, 1, 12), None, labels, 3, 1.0)
    with pytest.raises(ValueError, match="C <= min"):
        seg_ce(torch.zeros(1, 2, 2, 1, 8), None, labels, 9, 1.0)
    with pytest.raises(ValueError, match="uint8"):
        seg_ce(torch.zeros(1, 2, 2, 1, 8), None, labels.long(), 3, 1.0)


# ------------------------------------------------------------ evaluation
def planted_segmentation(seed=0, n_train=64, n_val=16, cells=4, s=4, classes=6, dim=32,
                         ignore=0.05, noise=0.5):
    """Classes constant over 2 x 2-cell regions; a cell's feature is its class
    prototype plus noise and a common offset, so that standardising matters."""
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


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_planted_problem_reaches_miou(precision):
    """64 train and 16 val images, 4 x 4 cells, s = 4, 6 classes, D = 32, 5 %
    ignored pixels, 20 epochs of 16 images: a plain-torch run of this setup
    reaches mIoU 0.990 to 0.995 for lr from 1e-3 to 1."""
    from dinov3_amd.eval import evaluate_segmentation_linear

    data = planted_segmentation()
    out = evaluate_segmentation_linear(*data, num_classes=6, epochs=20, batch_images=16,
                                       precision=precision)
    print(f"{precision}: mIoU per head = {[round(v, 4) for v in out['miou']]}")
    assert len(out["miou"]) == 8 and out["heads"][0] == (1e-4, 0.0)
    assert out["best_miou"] >= 0.95
    best = out["best_head"]
    assert out["best_miou"] == out["miou"][best] == max(out["miou"])
    assert best == out["miou"].index(max(out["miou"]))  # the lowest index among equals
    assert out["pixel_acc"][best] >= 0.95 and out["val_loss"][best] < out["val_loss"][0]


def small_problem():
    return planted_segmentation(seed=3, n_train=21, n_val=7, cells=2, s=2, classes=4, dim=12,
                                noise=1.5)


def test_one_head_matches_torch_sgd():
    """The whole protocol for one head in fp32 against autograd through
    F.interpolate and torch.optim.SGD; the two differ by fp32 rounding only."""
    from dinov3_amd.eval.segmentation import _segmentation_linear

    xt, yt, xv, yv = planted_segmentation(seed=1, n_train=40, n_val=8, noise=1.5)
    lr, wd, epochs, batch, C = 0.1, 1e-3, 3, 16, 6
    out, state = _segmentation_linear(xt, yt, xv, yv, C, (lr,), (wd,), epochs, batch, "fp32", True,
                                      0, None, 64)
    rows = xt.double().view(-1, 32)
    mean = rows.mean(dim=0)
    inv_std = (rows.var(dim=0, unbiased=False) + 1e-6).rsqrt()
    st, sv = ((xt.double() - mean) * inv_std).float(), ((xv.double() - mean) * inv_std).float()

    clf = torch.nn.Linear(32, C)
    torch.nn.init.zeros_(clf.weight)
    torch.nn.init.zeros_(clf.bias)
    opt = torch.optim.SGD([{"params": [clf.weight], "weight_decay": wd},
                           {"params": [clf.bias], "weight_decay": 0.0}], lr=lr, momentum=0.9)

    def upsampled(x):
        return F.interpolate(clf(x).permute(0, 3, 1, 2), size=(16, 16), mode="bilinear",
                             align_corners=False)

    total, t = epochs * math.ceil(40 / batch), 0
    for epoch in range(epochs):
        perm = torch.randperm(40, generator=torch.Generator().manual_seed(epoch))
        for i in range(0, 40, batch):
            idx = perm[i: i + batch]
            for group in opt.param_groups:
                group["lr"] = lr * 0.5 * (1.0 + math.cos(math.pi * t / total))
            opt.zero_grad()
            F.cross_entropy(upsampled(st[idx]), yt[idx].long(), ignore_index=255).backward()
            opt.step()
            t += 1
    assert t == 9
    w_diff = float((state["weight"][0] - clf.weight.detach()).abs().max())
    b_diff = float((state["bias"][0] - clf.bias.detach()).abs().max())
    print(f"max |weight difference| = {w_diff:.3e}, max |bias difference| = {b_diff:.3e}")
    assert w_diff <= 1e-5 and b_diff <= 1e-5
    with torch.no_grad():
        want = upsampled(sv)
    valid = yv != 255
    pred = want.argmax(dim=1)
    assert out["pixel_acc"][0] == pytest.approx(
        int((pred == yv)[valid].sum()) / int(valid.sum()), abs=2e-3)  # near-ties may flip
    assert out["val_loss"][0] == pytest.approx(
        float(F.cross_entropy(want, yv.long(), ignore_index=255)), rel=1e-4)
    ious = []
    for c in range(C):
        lab, hit = (yv == c) & valid, (pred == c) & valid
        if int(lab.sum()):
            ious.append(int((lab & hit).sum()) / int((lab | hit).sum()))
    assert out["miou"][0] == pytest.approx(sum(ious) / len(ious), abs=5e-3)


def test_grid_head_equals_one_head_run():
    from dinov3_amd.eval import evaluate_segmentation_linear

    data = small_problem()
    lrs, wds = (1e-3, 1e-1, 1.0), (0.0, 1e-2)
    kwargs = dict(num_classes=4, epochs=3, batch_images=8, precision="fp32")
    grid = evaluate_segmentation_linear(*data, lrs=lrs, wds=wds, **kwargs)
    assert grid["heads"] == [(lr, wd) for lr in lrs for wd in wds]  # lr-major
    assert len(set(grid["miou"])) > 1  # the heads do differ on this data
    for g, (lr, wd) in enumerate(grid["heads"]):
        one = evaluate_segmentation_linear(*data, lrs=(lr,), wds=(wd,), **kwargs)
        for key in ("miou", "pixel_acc"):
            assert grid[key][g] == one[key][0], key
        for key in ("val_loss", "train_loss"):
            assert grid[key][g] == pytest.approx(one[key][0], rel=1e-5), key


def test_evaluate_segmentation_linear_validation():
    from dinov3_amd.eval import evaluate_segmentation_linear

    xt, yt, xv, yv = small_problem()
    bad = yt.clone()
    bad[0, 0, 0] = 4
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        evaluate_segmentation_linear(xt, bad, xv, yv, num_classes=4, epochs=1)
    with pytest.raises(ValueError, match="255"):
        evaluate_segmentation_linear(xt, yt, xv, yv, num_classes=256, epochs=1)
    with pytest.raises(ValueError, match="even multiple"):  # s = 3
        evaluate_segmentation_linear(xt, yt.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, ::2, ::2],
                                     xv, yv, num_classes=4, epochs=1)
    with pytest.raises(ValueError, match="even multiple"):  # 4 x 8 labels for 2 x 2 cells
        evaluate_segmentation_linear(xt, yt.repeat_interleave(2, 2), xv, yv, num_classes=4,
                                     epochs=1)
    with pytest.raises(ValueError, match="uint8"):
        evaluate_segmentation_linear(xt, yt.long(), xv, yv, num_classes=4, epochs=1)


# ------------------------------------------------------------------ gloo
def _sharded_worker(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from dinov3_amd.eval import evaluate_segmentation_linear

    xt, yt, xv, yv = small_problem()  # 21 and 7 images: the rank-strided shards are unequal
    shards = (xt[rank::WORLD], yt[rank::WORLD], xv[rank::WORLD], yv[rank::WORLD])
    grids = [dict(lrs=(1e-2, 1e-1, 1.0)), dict(lrs=(1e-1,))]  # 3 heads; 1 head: rank 1 is idle
    kwargs = dict(num_classes=4, epochs=3, batch_images=8, precision="fp32")
    got = [evaluate_segmentation_linear(*shards, **grid, **kwargs) for grid in grids]
    # explicit ids in another order give the same result
    order = torch.randperm(shards[0].shape[0], generator=torch.Generator().manual_seed(1))
    got.append(evaluate_segmentation_linear(shards[0][order], shards[1][order], shards[2],
                                            shards[3], sample_ids=rank + WORLD * order,
                                            **grids[0], **kwargs))
    dist.destroy_process_group()
    for out, grid in zip(got, grids + grids[:1]):
        ref = evaluate_segmentation_linear(xt, yt, xv, yv, **grid, **kwargs)
        assert out["miou"] == ref["miou"] and out["pixel_acc"] == ref["pixel_acc"], (out, ref)
        assert out["best_head"] == ref["best_head"] and out["heads"] == ref["heads"]
        for key in ("val_loss", "train_loss"):
            assert torch.allclose(torch.tensor(out[key]), torch.tensor(ref[key]), rtol=1e-5,
                                  atol=0.0), (key, out[key], ref[key])
        assert all(v > 0 for v in ref["train_loss"])


def test_evaluate_segmentation_linear_world2_matches_single_process():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_sharded_worker, args=(r, 29551)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    for p in procs:
        assert p.exitcode == 0, f"child exited with {p.exitcode}"


# ------------------------------------------------------------------ data
def test_segmentation_transforms():
    from dinov3_amd.data.transforms import make_segmentation_transforms

    image_t, target_t = make_segmentation_transforms(crop_size=8, mean=(0.5, 0.5, 0.5),
                                                     std=(0.5, 0.5, 0.5))
    img = image_t(torch.rand(3, 20, 12))
    assert img.shape == (3, 8, 8) and img.dtype == torch.float32
    assert float(img.min()) >= -1.0 and float(img.max()) <= 1.0
    label = torch.tensor([[0, 1], [2, 255]])
    out = target_t(label)
    assert out.dtype == torch.uint8 and out.shape == (8, 8)
    assert torch.equal(out, label.repeat_interleave(4, 0).repeat_interleave(4, 1).to(torch.uint8))
    _, reduce_t = make_segmentation_transforms(crop_size=2, reduce_zero_label=True)
    assert reduce_t(torch.tensor([[0, 1], [150, 255]])).tolist() == [[255, 0], [149, 255]]


def test_synthetic_seg_dataset():
    from dinov3_amd.data import make_dataset
    from dinov3_amd.data.datasets import SyntheticSeg

    ds = make_dataset(dataset_str="SyntheticSeg:split=TRAIN:length=6")
    assert isinstance(ds, SyntheticSeg) and len(ds) == 6
    img, lab = ds[3]
    img2, lab2 = ds[3]
    assert torch.equal(img, img2) and torch.equal(lab, lab2)  # seeded by the index
    assert img.shape == (3, 64, 64) and lab.shape == (64, 64)
    valid = lab != 255
    assert 0 < int((~valid).sum()) < 0.1 * lab.numel()
    assert int(lab[valid].max()) < SyntheticSeg.NUM_CLASSES
    assert not torch.equal(lab, ds[4][1])
    val = make_dataset(dataset_str="SyntheticSeg:split=VAL:length=6")
    assert not torch.equal(lab, val[3][1])
    # the image carries the class: the nearest class colour gives the label back
    colours = torch.tensor(SyntheticSeg._COLOURS)
    nearest = (img.permute(1, 2, 0)[:, :, None, :] - colours).square().sum(dim=3).argmin(dim=2)
    assert torch.equal(nearest[valid], lab[valid])


# --------------------------------------------------------------- do_test
def test_do_test_segmentation_keys(smoke_cfg, monkeypatch):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch
    from dinov3_amd.train.train import do_test

    cfg = copy.deepcopy(smoke_cfg)
    cfg.train.dataset_path = "Synthetic:split=TRAIN:length=32"
    cfg.crops.global_crops_size = 32  # 2 x 2 cells: the test is about the plumbing
    model = SSLMetaArch(cfg)
    monkeypatch.delenv("DINOV3_EVAL_SEG", raising=False)
    before = do_test(cfg, model, iteration=0)
    assert set(before) == {"iteration", "knn_top1", "linear_top1"}  # exactly today's keys
    monkeypatch.setenv("DINOV3_EVAL_SEG", "SyntheticSeg")
    results = do_test(cfg, model, iteration=0)
    heads = [f"seg_miou_head{i}" for i in range(8)]
    assert set(results) == set(before) | {"seg_miou", "seg_pixel_acc", "seg_best_lr"} | set(heads)
    for key in ["seg_miou", "seg_pixel_acc", "seg_best_lr"] + heads:
        assert 0.0 <= results[key] <= 1.0, (key, results[key])
    assert results["seg_miou"] == max(results[k] for k in heads)

"""Linear segmentation probe on frozen patch features: the dense counterpart
of the linear classification probe, and the number that shows whether Gram
anchoring keeps the patch features intact while the CLS metrics rise."""

from __future__ import annotations

import logging
import math
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .linear import _check_ids, _gather_by_id, _gather_shards

logger = logging.getLogger("dinov3")

_MOMENTUM = 0.9
_STD_EPS = 1e-6
_IGNORE = 255


@torch.no_grad()
def extract_dense_features(model, data_loader, to_cpu: bool = True
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Run the backbone over a loader of (image, label map); returns
    (`x_norm_patchtokens` reshaped to [M, h, w, D] fp32, label maps [M, H, W]
    uint8), on the host, or on the model's device with `to_cpu=False`."""
    from .. import parallel

    device = parallel.device()
    model.eval()
    feats, labels = [], []
    for images, targets in data_loader:
        images = images.to(device, non_blocking=True)
        if next(model.parameters()).dtype == torch.bfloat16:
            images = images.bfloat16()
        tokens = model.forward_features(images)["x_norm_patchtokens"]
        batch, n, dim = tokens.shape
        patch = getattr(model, "patch_size", None) or round(math.sqrt(
            images.shape[-2] * images.shape[-1] / n))
        h, w = images.shape[-2] // patch, images.shape[-1] // patch
        assert h * w == n, f"{n} patch tokens do not form a {h} x {w} grid"
        tokens = tokens.reshape(batch, h, w, dim).float()
        targets = torch.as_tensor(targets).to(torch.uint8)
        feats.append(tokens.cpu() if to_cpu else tokens)
        labels.append(targets if to_cpu else targets.to(device))
    return torch.cat(feats), torch.cat(labels)


def _segmentation_linear(train_feats, train_labels, val_feats, val_labels, num_classes, lrs, wds,
                         epochs, batch_images, precision, standardize, seed, sample_ids,
                         val_chunk_images):
    """The body of `evaluate_segmentation_linear`; returns (its result, the
    trained heads of this rank as in `eval.linear._linear_sharded`, "weight"
    [G_loc, C, D], or None for a rank without heads)."""
    from .. import parallel
    from ..ops import SEG_MAX_CLASSES, probe_sgd_, seg_ce

    name = "evaluate_segmentation_linear"
    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
    heads = [(float(lr), float(wd)) for lr in lrs for wd in wds]
    if not heads:
        raise ValueError(f"{name}: lrs and wds must not be empty")
    if epochs < 1 or batch_images < 1 or val_chunk_images < 1:
        raise ValueError(f"{name}: epochs, batch_images and val_chunk_images must be >= 1")
    n_cls = int(num_classes)
    if not 1 <= n_cls <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: {n_cls} classes, the limit is {SEG_MAX_CLASSES}")
    # the shapes are the same on every rank, an empty shard's included
    for feats, labels, what in ((train_feats, train_labels, "train"), (val_feats, val_labels, "val")):
        if feats.dim() != 4 or labels.dim() != 3 or labels.dtype != torch.uint8 \
                or labels.shape[0] != feats.shape[0]:
            raise ValueError(f"{name}: {what} features must be [M, h, w, D] and labels uint8 "
                             "[M, H, W]")
        h, w = feats.shape[1:3]
        H, W = labels.shape[1:]
        s = H // max(h, 1)
        if h < 1 or w < 1 or H != s * h or W != s * w or s % 2 or not 2 <= s <= 32:
            raise ValueError(f"{name}: the {what} labels ({H} x {W}) must be an even multiple, "
                             f"2 to 32 and the same along both axes, of the cells ({h} x {w})")
    if val_feats.shape[3] != train_feats.shape[3]:
        raise ValueError(f"{name}: train and val features must share D")

    world, rank, group = 1, 0, None
    if parallel.is_enabled():
        world, rank, group = parallel.subgroup_size(), parallel.subgroup_rank(), parallel.subgroup()
    dev = train_feats.device
    if world > 1 and not dev.type == "cuda" and dist.get_backend(group) == "nccl":
        dev = parallel.device()

    xt, xv = train_feats.to(dev).float().contiguous(), val_feats.to(dev).float().contiguous()
    yt, yv = train_labels.to(dev).contiguous(), val_labels.to(dev).contiguous()
    n_loc, v_loc, dim = xt.shape[0], xv.shape[0], xt.shape[3]
    ht, wt = xt.shape[1:3]
    hv, wv = xv.shape[1:3]

    # 1. global sizes and the label check in one exchange; every rank sees the
    # same numbers, so every rank raises or none does
    def out_of_range(y):
        return int(((y >= n_cls) & (y != _IGNORE)).any()) if y.numel() else 0
    stats = torch.tensor([[n_loc, v_loc, max(out_of_range(yt), out_of_range(yv))]], device=dev,
                         dtype=torch.long)
    if world > 1:
        gathered = torch.empty((world, 3), device=dev, dtype=torch.long)
        dist.all_gather(list(gathered.unbind(0)), stats[0], group=group)
        stats = gathered
    stats = stats.tolist()
    t_lens, v_lens = [r[0] for r in stats], [r[1] for r in stats]
    n_glob, v_glob = sum(t_lens), sum(v_lens)
    if n_glob == 0 or v_glob == 0:
        raise ValueError(f"{name}: empty train or val set")
    if max(r[2] for r in stats):
        raise ValueError(f"{name}: labels must lie in [0, {n_cls}) or be {_IGNORE} (ignored)")

    # 2. standardise with the statistics of all train cells
    mean = inv_std = None
    if standardize:
        rows = xt.view(-1, dim)
        n_rows = n_glob * ht * wt
        mean = rows.sum(dim=0, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(mean, group=group)
        mean /= n_rows
        var = torch.zeros(dim, device=dev, dtype=torch.float64)
        for i in range(0, rows.shape[0], 65536):
            var += (rows[i: i + 65536].double() - mean).square().sum(dim=0)
        if world > 1:
            dist.all_reduce(var, group=group)
        inv_std = (var / n_rows + _STD_EPS).rsqrt()

        def standardized(x):
            out = torch.empty_like(x)
            src, dst = x.view(-1, dim), out.view(-1, dim)
            for i in range(0, src.shape[0], 65536):
                dst[i: i + 65536] = ((src[i: i + 65536].double() - mean) * inv_std).float()
            return out
        xt, xv = standardized(xt), standardized(xv)
    pad = -dim % 8  # the kernels move 8 elements at a time; zero columns add nothing
    if pad:
        xt, xv = torch.nn.functional.pad(xt, (0, pad)), torch.nn.functional.pad(xv, (0, pad))
    lp = precision == "bf16"
    if lp:
        xt, xv = xt.bfloat16(), xv.bfloat16()
    dim_p = dim + pad

    # 3. gather everything once, in global sample-id order
    if sample_ids is None:
        ids_t = rank + world * torch.arange(n_loc, device=dev, dtype=torch.long)
    else:
        ids_t = sample_ids.to(dev).long()
        if ids_t.shape != (n_loc,):
            raise ValueError(f"{name}: sample_ids must hold one id per train image")
    ids_v = rank + world * torch.arange(v_loc, device=dev, dtype=torch.long)
    all_t = all_v = None  # one process, default ids: the images are in id order already
    if world > 1 or sample_ids is not None:
        all_t = _gather_shards(ids_t, t_lens, world, group)
        all_v = _gather_shards(ids_v, v_lens, world, group)
        _check_ids(torch.cat(all_t), n_glob, "train")
        _check_ids(torch.cat(all_v), v_glob, "val")
    xt, yt = (_gather_by_id(t, all_t, t_lens, world, group) for t in (xt, yt))
    xv, yv = (_gather_by_id(t, all_v, v_lens, world, group) for t in (xv, yv))
    valid_t = (yt != _IGNORE).sum(dim=(1, 2)).float()  # per image, once

    # 4. this rank's heads
    mine = list(range(rank, len(heads), world))
    g_loc = len(mine)
    cp = (n_cls + 7) // 8 * 8
    steps_per_epoch = (n_glob + batch_images - 1) // batch_images
    total = epochs * steps_per_epoch
    # per head: val intersection, prediction and label counts, val loss, train loss
    result = torch.zeros((len(heads), 3 * cp + 2), device=dev, dtype=torch.float64)
    if g_loc:
        lr_t = torch.tensor([heads[g][0] for g in mine], device=dev, dtype=torch.float32)
        wd_t = torch.tensor([heads[g][1] for g in mine], device=dev, dtype=torch.float32)
        w = torch.zeros((g_loc, cp * dim_p), device=dev)
        w_mom, b, b_mom = torch.zeros_like(w), torch.zeros((g_loc, cp), device=dev), \
            torch.zeros((g_loc, cp), device=dev)
        w_lp = w.bfloat16() if lp else None
        train_loss = torch.zeros(g_loc, device=dev)
        t = 0
        for epoch in range(epochs):
            perm = torch.randperm(n_glob, generator=torch.Generator().manual_seed(seed + epoch))
            perm = perm.to(dev)
            for i in range(0, n_glob, batch_images):
                idx = perm[i: i + batch_images]
                xb, yb = xt.index_select(0, idx), yt.index_select(0, idx)
                imgs = xb.shape[0]
                cells = xb.view(imgs * ht * wt, dim_p)
                # the mean over the batch's valid pixels, its count taken on the device
                inv_valid = valid_t.index_select(0, idx).sum().clamp(min=1.0).reciprocal().view(1)
                fwd = (w_lp if lp else w).view(g_loc * cp, dim_p)
                logits = (cells @ fwd.T).view(imgs, ht, wt, g_loc, cp)
                loss_sum, _, db = seg_ce(logits, b, yb, n_cls, inv_valid, True)
                dw = logits.view(imgs * ht * wt, g_loc * cp).T @ cells  # the gradient by now
                scale = 0.5 * (1.0 + math.cos(math.pi * t / total))
                probe_sgd_(w, w_mom, dw.view(g_loc, cp * dim_p), lr_t, wd_t, scale, _MOMENTUM, w_lp)
                probe_sgd_(b, b_mom, db, lr_t, None, scale, _MOMENTUM, None)
                if epoch == epochs - 1:
                    train_loss += loss_sum
                t += 1

        # 5. score the heads on val with the forward-only kernel
        val_loss = torch.zeros(g_loc, device=dev)
        areas = torch.zeros((g_loc, 3, cp), device=dev, dtype=torch.long)
        fwd = (w_lp if lp else w).view(g_loc * cp, dim_p)
        for i in range(0, v_glob, val_chunk_images):
            xc = xv[i: i + val_chunk_images]
            imgs = xc.shape[0]
            logits = (xc.view(imgs * hv * wv, dim_p) @ fwd.T).view(imgs, hv, wv, g_loc, cp)
            loss_sum, counts, _ = seg_ce(logits, b, yv[i: i + val_chunk_images], n_cls, 0.0, False)
            val_loss += loss_sum
            areas += counts
        own = torch.tensor(mine, device=dev, dtype=torch.long)
        result[own] = torch.cat([areas.view(g_loc, 3 * cp).double(), val_loss.double().view(-1, 1),
                                 train_loss.double().view(-1, 1)], dim=1)

    # 6. publish
    if world > 1:
        dist.all_reduce(result, group=group)
    result = result.cpu()
    train_valid = max(float(valid_t.double().sum()), 1.0)
    miou, pixel_acc, val_losses, train_losses = [], [], [], []
    for row in result:
        inter, pred, lab = (row[k * cp: k * cp + n_cls] for k in range(3))
        present = lab > 0
        union = pred + lab - inter
        miou.append(float((inter[present] / union[present]).mean()) if bool(present.any()) else 0.0)
        n_valid = max(float(lab.sum()), 1.0)
        pixel_acc.append(float(inter.sum()) / n_valid)
        val_losses.append(float(row[3 * cp]) / n_valid)
        train_losses.append(float(row[3 * cp + 1]) / train_valid)
    best = max(range(len(heads)), key=lambda g: (miou[g], -g))
    out = {"miou": miou, "pixel_acc": pixel_acc, "val_loss": val_losses,
           "train_loss": train_losses, "heads": heads, "best_miou": miou[best],
           "best_head": best}
    logger.info("segmentation probe (%s): best mIoU %.4f at lr=%g wd=%g; per head: %s", precision,
                out["best_miou"], heads[best][0], heads[best][1],
                ", ".join(f"{a:.4f}" for a in miou))
    state = None
    if g_loc:
        state = {"heads": mine, "weight": w.view(g_loc, cp, dim_p)[:, :n_cls, :dim],
                 "bias": b[:, :n_cls], "mean": mean, "inv_std": inv_std}
    return out, state


@torch.no_grad()
def evaluate_segmentation_linear(train_feats: torch.Tensor, train_labels: torch.Tensor,
                                 val_feats: torch.Tensor, val_labels: torch.Tensor,
                                 num_classes: int,
                                 lrs: Sequence[float] = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 1e-1,
                                                         3e-1),
                                 wds: Sequence[float] = (0.0,), epochs: int = 10,
                                 batch_images: int = 16, precision: str = "bf16",
                                 standardize: bool = True, seed: int = 0,
                                 sample_ids: Optional[torch.Tensor] = None,
                                 val_chunk_images: int = 64) -> Dict[str, object]:
    """Linear segmentation probe over a grid of heads on frozen patch features
    `[M, h, w, D]` against dense `uint8` label maps `[M, H, W]` (255 = ignored),
    on the device of the inputs; the result does not depend on the number of
    ranks.

    Protocol. G = len(lrs) * len(wds) independent `Linear(D, C)` heads, ordered
    lr-major, zero at the start, applied per patch; the class logits are
    upsampled bilinearly (align_corners=False) by the even factor H / h = W / w
    (2 to 32) to the label resolution; the loss is the mean softmax
    cross-entropy over the valid pixels of the batch. Standardisation, the
    epoch permutations (`randperm(M, Generator().manual_seed(seed + e))`, in
    batches of `batch_images` images), SGD with momentum 0.9, weight decay on
    the weights only and the per-step cosine schedule are those of
    `evaluate_linear_sharded`; the statistics run over all train cells. Per
    head the val set gives `miou`, the mean of I / (P + L - I) over the classes
    with L > 0 in val (I, P, L: pixels with prediction = label = c, with
    prediction = c, with label = c; a prediction is the lowest class among the
    maximal logits), `pixel_acc` and `val_loss`. The best head has the highest
    mIoU, the lowest index among equals.

    Scope. Fixed square crops only: the image resized bilinearly to the crop
    size, the labels by nearest neighbour (`make_segmentation_transforms`). No
    sliding window, no multi-scale or flip test-time augmentation, and no
    BatchNorm in front of the layer: standardisation takes its place, as in the
    linear probe. The numbers are therefore not those of the published ADE20K
    protocol; they compare checkpoints of one run.

    precision="bf16": features rounded to bf16 once, fp32 master weights with a
    bf16 copy, bf16 logits and gradients; "fp32" is the protocol-exact form.

    Distribution. The inputs are this rank's shards, as in
    `evaluate_linear_sharded` (`sample_ids`, rank-strided default, unequal
    shards). Every rank gathers the whole set once: M h w D 2 bytes of features
    (4 in fp32) plus M H W bytes of labels per rank, about 42 GB + 5 GB for all
    of ADE20K (20 210 images) at ViT-L and 512 px; callers with larger D
    subsample. It then trains the heads g % world == rank with no collective
    and no host synchronisation inside the loop; one all-reduce publishes the
    result. On a HIP device the loss and its gradient are `ops.seg_ce`, which
    never holds the upsampled logits but takes a workspace of 16 fp32 values
    per logit of the batch (319 MB at 16 images, 32 x 32 cells, 8 heads, 150
    classes), the update is `ops.probe_sgd_`, the two GEMMs are the library's.

    Raises for labels in [num_classes, 255), for more than 255 classes, and for
    an odd or mismatched scale. The default lr grid is the linear probe's; it
    has not been tried on real ADE20K features.

    Returns {"miou": [G], "pixel_acc": [G], "val_loss": [G], "train_loss": [G]
    (mean over the last epoch), "heads": [(lr, wd)] * G, "best_miou",
    "best_head"}.
    """
    return _segmentation_linear(train_feats, train_labels, val_feats, val_labels, num_classes, lrs,
                                wds, epochs, batch_images, precision, standardize, seed, sample_ids,
                                val_chunk_images)[0]

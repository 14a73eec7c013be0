"""Linear probe on frozen features (the im1k-linear protocol of the headline
metric, 83.3% for the ViT-L recipe)."""

from __future__ import annotations

import logging
import math
from typing import Dict, Optional, Sequence

import torch
import torch.distributed as dist

logger = logging.getLogger("dinov3")


def evaluate_linear_probe(train_features: torch.Tensor, train_labels: torch.Tensor,
                          test_features: torch.Tensor, test_labels: torch.Tensor,
                          num_classes: int | None = None, epochs: int = 10,
                          lr: float = 0.01, batch_size: int = 1024,
                          device: str = "cpu") -> float:
    """SGD logistic regression on frozen features; returns top-1 accuracy."""
    num_classes = num_classes or int(max(train_labels.max(), test_labels.max()).item()) + 1
    dim = train_features.shape[1]
    clf = torch.nn.Linear(dim, num_classes).to(device)
    opt = torch.optim.SGD(clf.parameters(), lr=lr, momentum=0.9, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(
        opt, T_max=max(1, epochs * (len(train_features) // batch_size + 1)))
    tf = train_features.float().to(device)
    tl = train_labels.long().to(device)
    for epoch in range(epochs):
        perm = torch.randperm(tf.shape[0], device=device)
        for i in range(0, tf.shape[0], batch_size):
            idx = perm[i: i + batch_size]
            loss = torch.nn.functional.cross_entropy(clf(tf[idx]), tl[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
    with torch.no_grad():
        pred = clf(test_features.float().to(device)).argmax(dim=1).cpu()
    acc = (pred == test_labels.long()).float().mean().item()
    logger.info("linear probe top-1: %.4f", acc)
    return acc


PROBE_MAX_CLASSES = 2048  # the class-count limit of ops.probe_ce
_MOMENTUM = 0.9
_STD_EPS = 1e-6


def _gather_shards(t: torch.Tensor, lens, world: int, group):
    """The shards `t` [n_rank, ...] of all ranks, one view per rank."""
    if world == 1:
        return [t]
    pad = max(lens) - t.shape[0]
    if pad:
        t = torch.cat([t, t.new_zeros((pad,) + tuple(t.shape[1:]))])
    out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    dist.all_gather(list(out.unbind(0)), t.contiguous(), group=group)
    return [out[r, :n] for r, n in enumerate(lens)]


def _gather_by_id(t: torch.Tensor, ids, lens, world: int, group) -> torch.Tensor:
    """All-gather the shards `t` and lay the rows out by their global ids; `ids`
    holds the checked id shards of all ranks, or None for the identity."""
    if ids is None:
        return t
    out = torch.empty((sum(lens),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    for shard, shard_ids in zip(_gather_shards(t, lens, world, group), ids):
        out[shard_ids] = shard
    return out


def _check_ids(ids: torch.Tensor, n_glob: int, what: str) -> None:
    seen = torch.zeros(n_glob, dtype=torch.bool, device=ids.device)
    ok = ids.numel() == 0 or (int(ids.min()) >= 0 and int(ids.max()) < n_glob)
    if ok:
        seen[ids] = True
    if not ok or not bool(seen.all()):
        raise ValueError(f"evaluate_linear_sharded: the {what} sample ids of all ranks must be a "
                         f"permutation of 0..{n_glob - 1}; pass sample_ids, or shard with the "
                         "rank-strided sampler")


def _linear_sharded(train_feats, train_labels, val_feats, val_labels, lrs, wds, epochs,
                    batch_size, num_classes, precision, standardize, seed, sample_ids, val_chunk):
    """The body of `evaluate_linear_sharded`; returns (its result, the trained
    heads of this rank: {"heads": global indices, "weight" [G_loc, C, D] and
    "bias" [G_loc, C] fp32, "mean" and "inv_std" [D] fp64 or None}, or None for
    a rank without heads)."""
    from .. import parallel
    from ..ops import probe_ce, probe_sgd_

    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
    heads = [(float(lr), float(wd)) for lr in lrs for wd in wds]
    if not heads:
        raise ValueError("evaluate_linear_sharded: lrs and wds must not be empty")
    if epochs < 1 or batch_size < 1 or val_chunk < 1:
        raise ValueError("evaluate_linear_sharded: epochs, batch_size and val_chunk must be >= 1")

    world, rank, group = 1, 0, None
    if parallel.is_enabled():
        world, rank, group = parallel.subgroup_size(), parallel.subgroup_rank(), parallel.subgroup()
    dev = train_feats.device
    if world > 1 and not dev.type == "cuda" and dist.get_backend(group) == "nccl":
        dev = parallel.device()

    xt, xv = train_feats.to(dev).float(), val_feats.to(dev).float()
    yt, yv = train_labels.to(dev).long(), val_labels.to(dev).long()
    n_loc, v_loc, dim = xt.shape[0], xv.shape[0], xt.shape[1]

    # 1. global sizes and label range in one exchange; every rank sees the same
    # numbers, so every rank raises or none does
    lo = min(int(yt.min()) if n_loc else 0, int(yv.min()) if v_loc else 0)
    hi = max(int(yt.max()) if n_loc else -1, int(yv.max()) if v_loc else -1)
    stats = torch.tensor([[n_loc, v_loc, -lo, hi]], device=dev, dtype=torch.long)
    if world > 1:
        gathered = torch.empty((world, 4), device=dev, dtype=torch.long)
        dist.all_gather(list(gathered.unbind(0)), stats[0], group=group)
        stats = gathered
    stats = stats.tolist()
    t_lens, v_lens = [s[0] for s in stats], [s[1] for s in stats]
    n_glob, v_glob = sum(t_lens), sum(v_lens)
    if n_glob == 0 or v_glob == 0:
        raise ValueError("evaluate_linear_sharded: empty train or val set")
    n_cls = int(num_classes) if num_classes is not None else max(s[3] for s in stats) + 1
    if n_cls > PROBE_MAX_CLASSES:
        raise ValueError(f"evaluate_linear_sharded: {n_cls} classes, the limit is "
                         f"{PROBE_MAX_CLASSES}")
    if max(s[2] for s in stats) > 0 or max(s[3] for s in stats) >= n_cls:
        raise ValueError(f"evaluate_linear_sharded: labels must lie in [0, {n_cls})")

    # 2. standardise with the statistics of the whole train set
    mean = inv_std = None
    if standardize:
        mean = xt.sum(dim=0, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(mean, group=group)
        mean /= n_glob
        var = torch.zeros(dim, device=dev, dtype=torch.float64)
        for i in range(0, n_loc, 65536):
            var += (xt[i: i + 65536].double() - mean).square().sum(dim=0)
        if world > 1:
            dist.all_reduce(var, group=group)
        inv_std = (var / n_glob + _STD_EPS).rsqrt()

        def standardized(x):
            out = torch.empty_like(x)
            for i in range(0, x.shape[0], 65536):
                out[i: i + 65536] = ((x[i: i + 65536].double() - mean) * inv_std).float()
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
            raise ValueError("evaluate_linear_sharded: sample_ids must hold one id per train row")
    ids_v = rank + world * torch.arange(v_loc, device=dev, dtype=torch.long)
    all_t = all_v = None  # one process, default ids: the rows are in id order already
    if world > 1 or sample_ids is not None:
        all_t = _gather_shards(ids_t, t_lens, world, group)
        all_v = _gather_shards(ids_v, v_lens, world, group)
        _check_ids(torch.cat(all_t), n_glob, "train")
        _check_ids(torch.cat(all_v), v_glob, "val")
    xt, yt = (_gather_by_id(t, all_t, t_lens, world, group) for t in (xt, yt))
    xv, yv = (_gather_by_id(t, all_v, v_lens, world, group) for t in (xv, yv))

    # 4. this rank's heads
    mine = list(range(rank, len(heads), world))
    g_loc = len(mine)
    cp = (n_cls + 7) // 8 * 8
    steps_per_epoch = (n_glob + batch_size - 1) // batch_size
    total = epochs * steps_per_epoch
    result = torch.zeros((len(heads), 3), device=dev, dtype=torch.float64)
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
            for i in range(0, n_glob, batch_size):
                idx = perm[i: i + batch_size]
                xb, yb = xt.index_select(0, idx), yt.index_select(0, idx)
                rows = xb.shape[0]
                fwd = (w_lp if lp else w).view(g_loc * cp, dim_p)
                logits = (xb @ fwd.T).view(rows, g_loc, cp)
                loss_sum, _, db = probe_ce(logits, b, yb, n_cls, 1.0 / rows, True)
                dw = logits.view(rows, g_loc * cp).T @ xb  # the logits hold their gradient now
                scale = 0.5 * (1.0 + math.cos(math.pi * t / total))
                probe_sgd_(w, w_mom, dw.view(g_loc, cp * dim_p), lr_t, wd_t, scale, _MOMENTUM, w_lp)
                probe_sgd_(b, b_mom, db, lr_t, None, scale, _MOMENTUM, None)
                if epoch == epochs - 1:
                    train_loss += loss_sum
                t += 1

        # 5. score the heads on val
        val_loss = torch.zeros(g_loc, device=dev)
        hits = torch.zeros(g_loc, device=dev, dtype=torch.long)
        fwd = (w_lp if lp else w).view(g_loc * cp, dim_p)
        for i in range(0, v_glob, val_chunk):
            xc = xv[i: i + val_chunk]
            logits = (xc @ fwd.T).view(xc.shape[0], g_loc, cp)
            loss_sum, correct, _ = probe_ce(logits, b, yv[i: i + val_chunk], n_cls, 0.0, False)
            val_loss += loss_sum
            hits += correct
        own = torch.tensor(mine, device=dev, dtype=torch.long)
        result[own] = torch.stack([hits.double(), val_loss.double(), train_loss.double()], dim=1)

    # 6. publish
    if world > 1:
        dist.all_reduce(result, group=group)
    result = result.tolist()
    top1 = [r[0] / v_glob for r in result]
    best = max(range(len(heads)), key=lambda g: (top1[g], -g))
    out = {"top1": top1, "val_loss": [r[1] / v_glob for r in result],
           "train_loss": [r[2] / n_glob for r in result], "heads": heads,
           "best_top1": top1[best], "best_head": best}
    logger.info("linear probe (sharded, %s): best top-1 %.4f at lr=%g wd=%g; per head: %s",
                precision, out["best_top1"], heads[best][0], heads[best][1],
                ", ".join(f"{a:.4f}" for a in top1))
    state = None
    if g_loc:
        state = {"heads": mine, "weight": w.view(g_loc, cp, dim_p)[:, :n_cls, :dim],
                 "bias": b[:, :n_cls], "mean": mean, "inv_std": inv_std}
    return out, state


@torch.no_grad()
def evaluate_linear_sharded(train_feats: torch.Tensor, train_labels: torch.Tensor,
                            val_feats: torch.Tensor, val_labels: torch.Tensor,
                            lrs: Sequence[float] = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 1e-1, 3e-1),
                            wds: Sequence[float] = (0.0,), epochs: int = 10,
                            batch_size: int = 1024, num_classes: Optional[int] = None,
                            precision: str = "bf16", standardize: bool = True, seed: int = 0,
                            sample_ids: Optional[torch.Tensor] = None,
                            val_chunk: int = 8192) -> Dict[str, object]:
    """Linear probe over a grid of heads on frozen features, on the device of
    the inputs; the result does not depend on the number of ranks.

    Protocol. G = len(lrs) * len(wds) independent `Linear(D, C)` heads, ordered
    lr-major, weight and bias zero at the start. With `standardize` the
    features are shifted and scaled per dimension by the mean and the biased
    variance (+ 1e-6) of the whole train set, accumulated in fp64. Epoch e
    visits `randperm(N, generator=Generator().manual_seed(seed + e))` (a CPU
    generator, N the global train size) in batches of `batch_size`, the last
    one short; the loss is the mean softmax cross-entropy of the batch; SGD with
    momentum 0.9, weight decay on the weights only, and the step size
    lr * 0.5 * (1 + cos(pi * t / T)) at step t of T. A prediction is the lowest
    class among the maximal logits; the best head has the highest val top-1,
    the lowest index among equals.

    precision="bf16": the standardised features are rounded to bf16 once, the
    weights are an fp32 master with a bf16 copy, logits and their gradients are
    bf16; bias, loss, momentum and update stay fp32. "fp32" is the
    protocol-exact form.

    Distribution. The inputs are this rank's shards (the full sets without a
    process group), on any device. `sample_ids` are the global ids of the train
    shard; the default, `rank + world * i`, is the layout of the rank-strided
    sampler, which the val shard is taken to have as well. Shards may differ in
    length. Every rank gathers the whole standardised train and val set once
    (N * D * 2 bytes per rank in bf16, * 4 in fp32: 2.6 GB for ImageNet-1k at
    D = 1024, 10.5 GB at D = 4096, of 288 GB), then trains the heads
    g % world == rank over the same batch sequence with no collective and no
    host synchronisation inside the loop; one all-reduce publishes the
    per-head results. On a HIP device the loss/gradient and the update are
    `ops.probe_ce` and `ops.probe_sgd_`, the two GEMMs are the library's.

    At most 2048 classes. The default lr grid is a spread around the single
    rate of `evaluate_linear_probe`; it has not been tried on real ImageNet
    features.

    Returns {"top1": [G], "val_loss": [G], "train_loss": [G] (mean over the
    last epoch), "heads": [(lr, wd)] * G, "best_top1", "best_head"}.
    """
    return _linear_sharded(train_feats, train_labels, val_feats, val_labels, lrs, wds, epochs,
                           batch_size, num_classes, precision, standardize, seed, sample_ids,
                           val_chunk)[0]

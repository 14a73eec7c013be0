"""Feature extraction + k-NN evaluation.

The reference leaves do_test unimplemented (train.py:315-316) while its
configs name knn/linear benchmarks; this implements the im1k-knn protocol the
headline metric quotes (82.2% for the ViT-L recipe): cosine-similarity k-NN
over L2-normalized cls features with temperature-weighted voting.

`evaluate_knn` is the single-process CPU form. `evaluate_knn_sharded` is the
distributed form that stays on the device: every rank holds the shard of the
bank and of the queries that the rank-strided sampler gave it, searches its
bank shard for every rank's queries with `ops.knn_topk`, and the per-rank
neighbour lists are merged by (similarity descending, sample id ascending), so
the result does not depend on the number of ranks.
"""

from __future__ import annotations

import logging
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .. import parallel

logger = logging.getLogger("dinov3")


@torch.no_grad()
def extract_features(model, data_loader, device=None,
                     to_cpu: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Run the backbone over a loader of (image, label); returns (features, labels),
    on the host, or on `device` with `to_cpu=False`."""
    device = device or parallel.device()
    model.eval()
    feats, labels = [], []
    for images, targets in data_loader:
        images = images.to(device, non_blocking=True)
        if next(model.parameters()).dtype == torch.bfloat16:
            images = images.bfloat16()
        out = model(images)
        if isinstance(out, dict):
            out = out["x_norm_clstoken"]
        if to_cpu:
            feats.append(out.float().cpu())
            labels.append(torch.as_tensor(targets))
        else:
            feats.append(out.float())
            labels.append(torch.as_tensor(targets).to(device))
    return torch.cat(feats), torch.cat(labels)


@torch.no_grad()
def evaluate_knn(train_features: torch.Tensor, train_labels: torch.Tensor,
                 test_features: torch.Tensor, test_labels: torch.Tensor,
                 k: int = 20, temperature: float = 0.07, num_classes: int | None = None,
                 chunk: int = 1024, precision: str = "bf16") -> float:
    """Temperature-weighted cosine k-NN top-1 accuracy (DINO protocol).

    With tensors on a HIP device the inputs are taken to be the full sets and
    the search runs on the device (`evaluate_knn_sharded` without collectives,
    `precision` as there); with CPU tensors `precision` is ignored."""
    if train_features.is_cuda:
        accs = _knn_sharded(train_features, train_labels, test_features, test_labels, (k,),
                            temperature, num_classes, precision, chunk, None, False)[0]
        return accs[k]
    num_classes = num_classes or int(max(train_labels.max(), test_labels.max()).item()) + 1
    train_features = torch.nn.functional.normalize(train_features, dim=1)
    test_features = torch.nn.functional.normalize(test_features, dim=1)
    correct = 0
    total = test_features.shape[0]
    k = min(k, train_features.shape[0])
    for i in range(0, total, chunk):
        tf = test_features[i: i + chunk]
        sim = tf @ train_features.T  # [c, Ntrain]
        topk_sim, topk_idx = sim.topk(k, dim=1)
        topk_labels = train_labels[topk_idx]  # [c, k]
        weights = (topk_sim / temperature).exp()
        votes = torch.zeros(tf.shape[0], num_classes)
        votes.scatter_add_(1, topk_labels, weights)
        pred = votes.argmax(dim=1)
        correct += (pred == test_labels[i: i + chunk]).sum().item()
    acc = correct / max(total, 1)
    logger.info("knn top-1: %.4f (k=%d, T=%.2f)", acc, k, temperature)
    return acc


_ID_PAD = torch.iinfo(torch.int64).max


def _search_fp32(q: torch.Tensor, bank: torch.Tensor, k: int, rows: int = 1024):
    """fp32 matmul + topk in chunks of `rows` queries: the protocol-exact search."""
    vals, idxs = [], []
    for i in range(0, q.shape[0], rows):
        v, ix = (q[i: i + rows] @ bank.T).topk(k, dim=1)
        vals.append(v)
        idxs.append(ix)
    return torch.cat(vals), torch.cat(idxs)


def _knn_sharded(bank_feats, bank_labels, query_feats, query_labels, ks, temperature,
                 num_classes, precision, query_chunk, bank_ids, collectives):
    """The body of `evaluate_knn_sharded`; returns (accuracy per k, merged
    similarities [Q_local, kmax], merged sample ids [Q_local, kmax])."""
    from ..ops import knn_topk

    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1:
        raise ValueError(f"ks must be positive, got {ks}")

    world, rank, group = 1, 0, None
    if collectives and parallel.is_enabled():
        world, rank, group = parallel.subgroup_size(), parallel.subgroup_rank(), parallel.subgroup()
    dev = bank_feats.device
    if world > 1 and not dev.type == "cuda" and dist.get_backend(group) == "nccl":
        dev = parallel.device()

    def gather(t: torch.Tensor) -> torch.Tensor:
        """[world, *t.shape]; every rank passes the same shape."""
        if world == 1:
            return t.unsqueeze(0)
        out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather(list(out.unbind(0)), t.contiguous(), group=group)
        return out

    # 1. L2-normalise in fp32, round once to bf16
    bank = torch.nn.functional.normalize(bank_feats.to(dev).float(), dim=1)
    query = torch.nn.functional.normalize(query_feats.to(dev).float(), dim=1)
    if precision == "bf16":
        bank, query = bank.bfloat16(), query.bfloat16()
        pad = -bank.shape[1] % 32  # the kernel wants D % 32 == 0; zero columns add nothing
        if pad:
            bank = torch.nn.functional.pad(bank, (0, pad))
            query = torch.nn.functional.pad(query, (0, pad))
    bank, query = bank.contiguous(), query.contiguous()
    bank_labels = bank_labels.to(dev).long()
    query_labels = query_labels.to(dev).long()
    n_loc, q_loc, dim = bank.shape[0], query.shape[0], bank.shape[1]

    # 2. absolute sample ids of the bank shard: the rank-strided sampler layout
    if bank_ids is None:
        bank_ids = rank + world * torch.arange(n_loc, device=dev, dtype=torch.long)
    else:
        bank_ids = bank_ids.to(dev).long()

    max_label = max(int(bank_labels.max()) if n_loc else -1,
                    int(query_labels.max()) if q_loc else -1)
    stats = gather(torch.tensor([n_loc, q_loc, max_label], device=dev, dtype=torch.long)).tolist()
    n_glob = sum(s[0] for s in stats)
    q_lens = [s[1] for s in stats]
    if num_classes is None:
        num_classes = max(s[2] for s in stats) + 1
    if n_glob == 0:
        raise ValueError("evaluate_knn_sharded: empty bank")
    k_eff = {k: min(k, n_glob) for k in ks}  # each k clamped to the global bank size
    kmax = max(k_eff.values())
    k_loc = min(kmax, n_loc)

    per_rank = max(1, query_chunk // world)  # the gathered chunk holds about query_chunk rows
    correct = torch.zeros(len(ks), device=dev, dtype=torch.long)
    merged_vals, merged_ids = [], []
    order = sorted(range(len(ks)), key=lambda i: k_eff[ks[i]])
    for lo in range(0, max(q_lens), per_rank):
        # 3. gather the query chunks, padded to the longest shard's piece
        c_pad = min(per_rank, max(q_lens) - lo)
        piece = query[lo: lo + c_pad]
        n_valid = piece.shape[0]
        if n_valid < c_pad:
            piece = torch.cat([piece, piece.new_zeros(c_pad - n_valid, dim)])
        all_q = gather(piece).reshape(world * c_pad, dim)

        # 4. search the local bank shard
        val = torch.full((world * c_pad, kmax), float("-inf"), device=dev)
        lab = torch.zeros((world * c_pad, kmax), device=dev, dtype=torch.long)
        ids = torch.full((world * c_pad, kmax), _ID_PAD, device=dev, dtype=torch.long)
        if k_loc > 0:
            if precision == "bf16":
                v, ix = knn_topk(all_q, bank, k_loc)
            else:
                v, ix = _search_fp32(all_q, bank, k_loc)
            val[:, :k_loc], lab[:, :k_loc], ids[:, :k_loc] = v, bank_labels[ix], bank_ids[ix]

        # 5. gather the per-rank lists, keep this rank's queries: [c_pad, world * kmax]
        def mine(t):
            return gather(t)[:, rank * c_pad: rank * c_pad + n_valid].transpose(0, 1).reshape(
                n_valid, world * kmax)
        val, lab, ids = mine(val), mine(lab), mine(ids)

        # 6. merge by (value descending, id ascending): two stable sorts
        by_id = ids.argsort(dim=1, stable=True)
        val, lab, ids = val.gather(1, by_id), lab.gather(1, by_id), ids.gather(1, by_id)
        by_val = val.argsort(dim=1, descending=True, stable=True)[:, :kmax]
        val, lab, ids = val.gather(1, by_val), lab.gather(1, by_val), ids.gather(1, by_val)
        merged_vals.append(val)
        merged_ids.append(ids)

        # 7. one weighted vote, read off after every k's prefix
        weights = (val / temperature).exp()
        votes = torch.zeros(n_valid, num_classes, device=dev)
        target = query_labels[lo: lo + n_valid]
        done = 0
        for i in order:
            k = k_eff[ks[i]]
            votes.scatter_add_(1, lab[:, done:k], weights[:, done:k])
            done = max(done, k)
            correct[i] += (votes.argmax(dim=1) == target).sum()

    # 8. global counts
    counts = torch.cat([correct, torch.tensor([q_loc], device=dev, dtype=torch.long)])
    if world > 1:
        dist.all_reduce(counts, group=group)
    counts = counts.tolist()
    accs = {k: counts[i] / max(counts[-1], 1) for i, k in enumerate(ks)}
    empty = torch.empty(0, kmax, device=dev)
    return (accs, torch.cat(merged_vals) if merged_vals else empty,
            torch.cat(merged_ids) if merged_ids else empty.long())


@torch.no_grad()
def evaluate_knn_sharded(bank_feats: torch.Tensor, bank_labels: torch.Tensor,
                         query_feats: torch.Tensor, query_labels: torch.Tensor,
                         ks: Sequence[int] = (10, 20, 100, 200), temperature: float = 0.07,
                         num_classes: Optional[int] = None, precision: str = "bf16",
                         query_chunk: int = 8192, bank_ids: Optional[torch.Tensor] = None,
                         return_neighbours: bool = False):
    """Temperature-weighted cosine k-NN top-1 accuracy for every k of `ks`, over
    a bank and a query set sharded across the ranks of `parallel.subgroup()`.

    The inputs are this rank's shards (the full sets when the process group has
    one rank or is not initialised), on any device. `bank_ids` are the absolute
    sample ids of the bank shard; the default, `rank + world * i`, is the layout
    of the rank-strided `EpochSampler`. Ties between equal similarities break
    towards the lower id, so the result is the same for every world size.

    precision="bf16" rounds the normalised features to bf16 once and searches
    with `ops.knn_topk` (the HIP kernel on a device); "fp32" searches with a
    chunked fp32 matmul + topk on the same device, the protocol-exact form.

    Returns {k: accuracy}; with `return_neighbours` also the merged
    (similarities, sample ids), [Q_local, min(max(ks), N_global)] each, of this
    rank's queries.
    """
    accs, vals, ids = _knn_sharded(bank_feats, bank_labels, query_feats, query_labels, ks,
                                   temperature, num_classes, precision, query_chunk, bank_ids,
                                   True)
    logger.info("knn top-1 (sharded, %s): %s", precision,
                ", ".join(f"k={k}: {a:.4f}" for k, a in accs.items()))
    return (accs, vals, ids) if return_neighbours else accs

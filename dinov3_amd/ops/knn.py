"""Top-k neighbour search for k-NN evaluation (docs/KERNELS.md "k-NN top-k")."""

from __future__ import annotations

from typing import Tuple

import torch


def knn_topk_ref(q: torch.Tensor, bank: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-torch `knn_topk`: fp64 matmul, then a stable descending sort, which
    puts the lower bank index first among equal values. The oracle of the kernel
    tests and the CPU path; not meant to be fast."""
    if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1]:
        raise ValueError(f"knn_topk: q [Q, D] and bank [N, D] must share D, got "
                         f"{tuple(q.shape)} and {tuple(bank.shape)}")
    if not 1 <= k <= min(bank.shape[0], 256):
        raise ValueError(f"knn_topk: need 1 <= k <= min(N, 256), got k = {k}, N = {bank.shape[0]}")
    sim = q.double() @ bank.double().T
    val, idx = torch.sort(sim, dim=1, descending=True, stable=True)
    return val[:, :k].float().contiguous(), idx[:, :k].contiguous()


def knn_topk(q: torch.Tensor, bank: torch.Tensor, k: int,
             splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k largest dot products of every row of `q` [Q, D] with the rows of
    `bank` [N, D], and the bank rows they belong to: (val [Q, k] fp32,
    idx [Q, k] int64), ordered by value descending and, among bit-equal values,
    by bank row ascending. Plain dot products: normalising is the caller's job.

    On a HIP device both inputs are contiguous bf16 with D % 32 == 0 and
    1 <= k <= min(N, 256); products are exact, accumulation is fp32, and the
    result is bit-identical from run to run and for every `splits` (the number
    of slices the bank is cut into along N; 0 = chosen from Q and N).
    Non-finite inputs are out of contract: their order is unspecified.
    """
    from . import hip_ops, use_hip

    if use_hip(q):
        val, idx = hip_ops().knn_topk(q, bank, int(k), int(splits))
        return val, idx.long()
    return knn_topk_ref(q, bank, k)

"""Micro-benchmark of ops.knn_topk against the on-device torch route.

GPU-only; opens one process on the device. Usage (wrap it in a time limit):
    timeout 900 python tools/bench_knn_topk.py [--q 8192] [--n 1281167] [--d 1024] [--k 200]

Random unit rows rounded to bf16 (the fp32 arm gets the same rounded values
as fp32). Three arms, alternated inside every round of one process and timed
with device events, one call per arm and round after one warm-up call each:
  knn_topk            the fused kernel, splits chosen by its heuristic
  torch_bf16          per chunk of --chunk queries: q @ bank.T in bf16, then topk
  torch_fp32          the same in fp32
Prints one JSON line per round and a summary line with the median and min/max
per arm, the kernel's FLOP/s (2 Q N D / time), and how far the kernel's values
are from the fp32 arm's and how many neighbour ids the two share.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def unit_rows(n: int, d: int, dev, block: int = 1 << 16) -> torch.Tensor:
    out = torch.empty(n, d, device=dev, dtype=torch.bfloat16)
    for i in range(0, n, block):
        x = torch.randn(min(block, n - i), d, device=dev)
        out[i: i + block] = torch.nn.functional.normalize(x, dim=1).bfloat16()
    return out


def torch_route(q: torch.Tensor, bank: torch.Tensor, k: int, chunk: int):
    vals, idxs = [], []
    for i in range(0, q.shape[0], chunk):
        v, ix = (q[i: i + chunk] @ bank.T).topk(k, dim=1)
        vals.append(v)
        idxs.append(ix)
    return torch.cat(vals), torch.cat(idxs)


def timed_ms(fn):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--q", type=int, default=8192)
    p.add_argument("--n", type=int, default=1281167)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--k", type=int, default=200)
    p.add_argument("--chunk", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--splits", type=int, default=0)
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    from dinov3_amd.ops import knn_topk

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    q = unit_rows(args.q, args.d, dev)
    bank = unit_rows(args.n, args.d, dev)
    q32, bank32 = q.float(), bank.float()
    arms = {
        "knn_topk": lambda: knn_topk(q, bank, args.k, splits=args.splits),
        "torch_bf16": lambda: torch_route(q, bank, args.k, args.chunk),
        "torch_fp32": lambda: torch_route(q32, bank32, args.k, args.chunk),
    }
    outs = {}
    for name, fn in arms.items():  # warm-up, and the outputs for the comparison
        ms, outs[name] = timed_ms(fn)
        print(json.dumps({"warmup": name, "ms": round(ms, 2)}), flush=True)
    kv, ki = outs["knn_topk"]
    fv, fi = outs["torch_fp32"]
    shared = (ki.sort(dim=1).values.unsqueeze(2) == fi.sort(dim=1).values.unsqueeze(1)
              ).any(dim=2).float().mean().item() if args.q * args.k * args.k <= 1 << 31 else None
    agreement = {"max_abs_val_diff_vs_fp32": float((kv - fv).abs().max()),
                 "shared_neighbour_fraction": shared}
    del outs, kv, ki, fv, fi

    samples = {name: [] for name in arms}
    for r in range(args.rounds):
        for name, fn in arms.items():
            samples[name].append(timed_ms(fn)[0])
        print(json.dumps({"round": r, "ms": {n: round(v[-1], 2) for n, v in samples.items()}}),
              flush=True)
    med = {n: statistics.median(v) for n, v in samples.items()}
    flop = 2.0 * args.q * args.n * args.d
    print(json.dumps({
        "Q": args.q, "N": args.n, "D": args.d, "k": args.k, "chunk": args.chunk,
        "rounds": args.rounds, "splits": args.splits,
        "ms_median": {n: round(v, 2) for n, v in med.items()},
        "ms_min_max": {n: [round(min(v), 2), round(max(v), 2)] for n, v in samples.items()},
        "knn_topk_tflops": round(flop / med["knn_topk"] / 1e9, 1),
        "knn_topk_over_torch_bf16": round(med["knn_topk"] / med["torch_bf16"], 3),
        "knn_topk_over_torch_fp32": round(med["knn_topk"] / med["torch_fp32"], 3),
        **agreement,
    }), flush=True)


if __name__ == "__main__":
    main()

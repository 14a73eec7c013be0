"""Micro-benchmark of the fp8 forward linear against the bf16 library GEMM.

GPU-only; opens one process on the device. Usage (wrap it in a time limit):
    timeout 600 python tools/bench_fp8_linear.py [--rounds 5] [--window-ms 300]

For each of the four block GEMMs of the ViT-L/16 step on the flat multi-crop
buffer (M taken from bench.py's default crop configuration) it times, with
device events on random operands and alternating in one process:
  bf16 F.linear | fp8_quant_rows(x) | fp8_quant_rows(w) | fp8_gemm_nt
and prints one JSON line per shape with the median and min/max of each over
the rounds, the fp8 total (both quantisers + GEMM) and achieved FLOP/s.
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
import torch.nn.functional as F

KN_SHAPES = [(1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024)]  # qkv, proj, fc1, fc2


def flat_buffer_rows() -> int:
    """Token rows of the student's flat buffer under bench.py's defaults."""
    import bench

    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        cfg = bench.build_cfg(bench.parse_args())
    finally:
        sys.argv = argv
    B = cfg.train.batch_size_per_gpu
    ps = cfg.student.patch_size
    extra = 1 + int(cfg.student.get("n_storage_tokens", 0) or 0)
    g = (cfg.crops.global_crops_size // ps) ** 2 + extra
    l = (cfg.crops.local_crops_size // ps) ** 2 + extra
    return B * (2 * g + cfg.crops.local_crops_number * l)


def window_ms(fn, iters: int) -> float:
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def calibrate(fn, target_ms: float) -> int:
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    per = max(window_ms(fn, 10) / 10, 1e-4)
    return max(10, int(target_ms / per))


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=300.0)
    p.add_argument("--rows", type=int, default=0, help="override M (default: from bench.py)")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    from dinov3_amd.ops import hip_ops

    ops = hip_ops()
    dev = torch.device("cuda:0")
    M = args.rows or flat_buffer_rows()
    torch.manual_seed(0)

    for K, N in KN_SHAPES:
        x = torch.randn(M, K, device=dev).bfloat16()
        w = (0.05 * torch.randn(N, K, device=dev)).bfloat16()
        xq, sx = ops.fp8_quant_rows(x)
        wq, sw = ops.fp8_quant_rows(w)
        arms = {
            "bf16_linear": lambda: F.linear(x, w),
            "quant_x": lambda: ops.fp8_quant_rows(x),
            "quant_w": lambda: ops.fp8_quant_rows(w),
            "fp8_gemm": lambda: ops.fp8_gemm_nt(xq, sx, wq, sw, None),
        }
        iters = {k: calibrate(fn, args.window_ms) for k, fn in arms.items()}
        samples = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():  # alternate the arms inside every round
                samples[k].append(window_ms(fn, iters[k]) / iters[k] * 1e3)  # us
        med = {k: statistics.median(v) for k, v in samples.items()}
        flop = 2.0 * M * N * K
        total = med["quant_x"] + med["quant_w"] + med["fp8_gemm"]
        out = {
            "M": M, "K": K, "N": N, "rounds": args.rounds, "window_ms": args.window_ms,
            "us_median": {k: round(v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in samples.items()},
            "fp8_total_us": round(total, 2),
            "tflops": {
                "bf16_linear": round(flop / med["bf16_linear"] / 1e6, 1),
                "fp8_gemm": round(flop / med["fp8_gemm"] / 1e6, 1),
                "fp8_total": round(flop / total / 1e6, 1),
            },
            "fp8_total_over_bf16": round(total / med["bf16_linear"], 3),
            "fp8_gemm_over_bf16": round(med["fp8_gemm"] / med["bf16_linear"], 3),
        }
        print(json.dumps(out), flush=True)
        del x, w, xq, wq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

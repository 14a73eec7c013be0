"""Micro-benchmark of the fp8 forward linear against the bf16 library GEMM.

GPU-only; opens one process on the device. Usage (wrap it in a time limit):
    timeout 600 python tools/bench_fp8_linear.py [--rounds 5] [--window-ms 300]

For each of the four block GEMMs of the ViT-L/16 step on the flat multi-crop
buffer (M taken from bench.py's default crop configuration) it times, with
device events on random operands and alternating in one process:
  bf16 F.linear | fp8_quant_rows(x) | fp8_quant_rows(w) | fp8_gemm_nt
and prints one JSON line per shape with the median and min/max of each over
the rounds, the fp8 total (both quantisers + GEMM) and achieved FLOP/s.

With --backward it times the backward of the same layers instead:
  bf16 dy @ w | bf16 dy.t() @ x | fp8_quant_rows(dy, e5m2) | fp8_quant_cols_t(w)
  | fp8_quant_cols_t(dy, e5m2, colsum) | fp8_quant_cols_t(x) | dgrad GEMM | wgrad GEMM
with the same alternating-arms method, one JSON line per shape.
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


def measure(arms, rounds: int, target_ms: float):
    """Median and all samples (us per call) of every arm, the arms alternating
    inside every round."""
    iters = {k: calibrate(fn, target_ms) for k, fn in arms.items()}
    samples = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            samples[k].append(window_ms(fn, iters[k]) / iters[k] * 1e3)
    return {k: statistics.median(v) for k, v in samples.items()}, samples


def bench_backward(ops, dev, M: int, args) -> None:
    E4M3, E5M2 = 0, 1
    for K, N in KN_SHAPES:
        x = torch.randn(M, K, device=dev).bfloat16()
        w = (0.05 * torch.randn(N, K, device=dev)).bfloat16()
        dy = torch.randn(M, N, device=dev).bfloat16()
        dyq, sdy = ops.fp8_quant_rows(dy, E5M2)
        wtq, swt, _ = ops.fp8_quant_cols_t(w, E4M3, False)
        dytq, sdyt, _ = ops.fp8_quant_cols_t(dy, E5M2, True)
        xtq, sxt, _ = ops.fp8_quant_cols_t(x, E4M3, False)
        arms = {
            "bf16_dgrad": lambda: dy @ w,
            "bf16_wgrad": lambda: dy.t() @ x,
            "quant_rows_dy": lambda: ops.fp8_quant_rows(dy, E5M2),
            "quant_cols_w": lambda: ops.fp8_quant_cols_t(w, E4M3, False),
            "quant_cols_dy_colsum": lambda: ops.fp8_quant_cols_t(dy, E5M2, True),
            "quant_cols_x": lambda: ops.fp8_quant_cols_t(x, E4M3, False),
            "fp8_dgrad_gemm": lambda: ops.fp8_gemm_nt(dyq, sdy, wtq, swt, None, E5M2),
            "fp8_wgrad_gemm": lambda: ops.fp8_gemm_nt(dytq, sdyt, xtq, sxt, None, E5M2),
        }
        med, samples = measure(arms, args.rounds, args.window_ms)
        flop = 2.0 * M * N * K
        dgrad_total = med["quant_rows_dy"] + med["quant_cols_w"] + med["fp8_dgrad_gemm"]
        wgrad_total = med["quant_cols_dy_colsum"] + med["quant_cols_x"] + med["fp8_wgrad_gemm"]
        bf16_total = med["bf16_dgrad"] + med["bf16_wgrad"]
        out = {
            "mode": "backward", "M": M, "K": K, "N": N, "rounds": args.rounds,
            "window_ms": args.window_ms,
            "us_median": {k: round(v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in samples.items()},
            "fp8_dgrad_total_us": round(dgrad_total, 2),
            "fp8_wgrad_total_us": round(wgrad_total, 2),
            "tflops": {
                "bf16_dgrad": round(flop / med["bf16_dgrad"] / 1e6, 1),
                "bf16_wgrad": round(flop / med["bf16_wgrad"] / 1e6, 1),
                "fp8_dgrad_gemm": round(flop / med["fp8_dgrad_gemm"] / 1e6, 1),
                "fp8_wgrad_gemm": round(flop / med["fp8_wgrad_gemm"] / 1e6, 1),
            },
            "fp8_dgrad_total_over_bf16": round(dgrad_total / med["bf16_dgrad"], 3),
            "fp8_wgrad_total_over_bf16": round(wgrad_total / med["bf16_wgrad"], 3),
            "fp8_backward_total_over_bf16": round((dgrad_total + wgrad_total) / bf16_total, 3),
        }
        print(json.dumps(out), flush=True)
        del x, w, dy, dyq, wtq, dytq, xtq
        torch.cuda.empty_cache()


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=300.0)
    p.add_argument("--rows", type=int, default=0, help="override M (default: from bench.py)")
    p.add_argument("--backward", action="store_true",
                   help="time dgrad / wgrad and their quantisers instead of the forward")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    from dinov3_amd.ops import hip_ops

    ops = hip_ops()
    dev = torch.device("cuda:0")
    M = args.rows or flat_buffer_rows()
    torch.manual_seed(0)
    if args.backward:
        bench_backward(ops, dev, M, args)
        return

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

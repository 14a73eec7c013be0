"""Micro-benchmark of the Gram-anchoring loss: the eager fp32 module against
ops.gram_loss (docs/KERNELS.md "Gram loss").

GPU-only; opens one process on the device. Usage (wrap it in a time limit):
    timeout 900 python tools/bench_gram_loss.py [--shapes 1x25088x1024,32x256x4096,8x2304x4096]
                                                [--rounds 5] [--inner 3] [--panel-mib 256]

Shapes are G x M x D of one rank: ViT-L/16 at 224 px with batch 64 and the
default gram.img_level=false; dinov3_vit7b16_gram_anchor.yaml; high-resolution
adaptation. Inputs are bf16, teacher = student + 0.5 noise, remove_neg with
apply_norm, as the 7B recipes set them. Arms, alternated inside every round of
one process and timed with device events, --inner back-to-back forward+backward
calls per arm and round (the sample is their mean) after one warm-up call each:
  eager   loss.GramLoss as it runs without DINOV3_FUSED_GRAM: fp32 similarity
          matrices and autograd. Where it cannot be allocated the tool says so
          instead of timing it.
  fused   ops.gram_loss with its gradient (row norms, tile kernel and library
          GEMM per panel, finish, normalisation backward)
  fused_fwd  ops.gram_loss without a gradient
Per arm the tool also reports the torch.cuda.max_memory_allocated delta of one
forward+backward call over what was allocated before it (inputs excluded).
Prints one JSON line per round and one summary line per shape with the median
and min/max per arm and how far the two arms are apart on the first call. No
time or ratio is a pass condition.
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


def timed_ms(fn, inner):
    """Milliseconds per call of `fn()`, `inner` calls between two device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner, out


def peak_delta_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    del out
    return round(delta / 2 ** 20, 1)


def bench_shape(args, shape, dev):
    from dinov3_amd.loss.gram_loss import GramLoss
    from dinov3_amd.ops import gram_loss

    g, m, d = shape
    gen = torch.Generator(device=dev).manual_seed(1000 * g + m + d)
    s = torch.randn(g, m, d, device=dev, generator=gen).bfloat16()
    t = (s.float() + 0.5 * torch.randn(g, m, d, device=dev, generator=gen)).bfloat16()
    module = GramLoss(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False)
    kw = dict(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False,
              panel_bytes=args.panel_mib << 20)
    os.environ.pop("DINOV3_FUSED_GRAM", None)  # the module's eager path

    def eager():
        x = s.detach().requires_grad_(True)
        loss = module(x, t, img_level=True)
        loss.backward()
        return loss.detach(), x.grad

    def fused():
        x = s.detach().requires_grad_(True)
        loss = gram_loss(x, t, **kw)
        loss.backward()
        return loss.detach(), x.grad

    def fused_fwd():
        return gram_loss(s, t, **kw), None

    arms = {"eager": eager, "fused": fused, "fused_fwd": fused_fwd}
    first, skipped, peak = {}, {}, {}
    for name in list(arms):  # warm-up, and the first results for the comparison
        try:
            ms, first[name] = timed_ms(arms[name], 1)
            print(json.dumps({"shape": shape, "warmup": name, "ms": round(ms, 3)}), flush=True)
            peak[name] = peak_delta_mib(arms[name])
        except (torch.OutOfMemoryError, RuntimeError) as e:  # too large to allocate
            if name != "eager":
                raise
            skipped[name] = "not timed: " + str(e).split("\n")[0][:200]
            print(json.dumps({"shape": shape, "warmup": name, "skipped": skipped[name]}), flush=True)
            del arms[name]
            torch.cuda.empty_cache()
    gaps = {}
    if "eager" in first:
        (loss, grad), (e_loss, e_grad) = first["fused"], first["eager"]
        gaps = {"loss_rel": float((loss - e_loss).abs() / e_loss.abs()),
                "grad_abs_over_max": float((grad.float() - e_grad.float()).abs().max()
                                           / e_grad.float().abs().max())}
    first.clear()
    torch.cuda.empty_cache()

    samples = {name: [] for name in arms}
    for r in range(args.rounds):
        for name in arms:
            samples[name].append(timed_ms(arms[name], args.inner)[0])
        print(json.dumps({"shape": shape, "round": r,
                          "ms": {n: round(v[-1], 3) for n, v in samples.items()}}), flush=True)
    med = {n: statistics.median(v) for n, v in samples.items()}
    out = {"G": g, "M": m, "D": d, "rounds": args.rounds, "inner": args.inner,
           "panel_MiB": args.panel_mib,
           "one_fp32_similarity_MiB": round(g * m * m * 4 / 2 ** 20, 1),
           "ms_median": {n: round(v, 3) for n, v in med.items()},
           "ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "peak_delta_MiB": peak, "skipped": skipped, "first_call_gap_to_eager": gaps}
    if "eager" in med:
        out["fused_over_eager"] = round(med["fused"] / med["eager"], 4)
    print(json.dumps(out), flush=True)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", type=str, default="1x25088x1024,32x256x4096,8x2304x4096",
                   help="G x M x D, comma-separated")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--inner", type=int, default=3, help="calls per timed sample")
    p.add_argument("--panel-mib", type=int, default=256, help="panel_bytes of the fused arm, MiB")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    dev = torch.device("cuda:0")
    for spec in args.shapes.split(","):
        bench_shape(args, tuple(int(v) for v in spec.split("x")), dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

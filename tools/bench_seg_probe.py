"""Micro-benchmark of the segmentation probe's training step (ops.seg_ce).

GPU-only; opens one process on the device. Usage (wrap it in a time limit):
    timeout 900 python tools/bench_seg_probe.py [--m 16] [--cells 32] [--s 16] [--c 150]
                                                [--d 1024] [--gs 1,8]

One bf16 training step of G heads, as evaluate_segmentation_linear runs it, at
a shape users run: 16 crops of 512 px at patch size 16, ADE20K's 150 classes.
Arms, per G, alternated inside every round of one process and timed with
device events, --inner back-to-back calls per arm and round (the sample is
their mean) after one warm-up call each:
  seg_ce        the kernel with gradient and its finalize launches, on fresh logits
  seg_ce_fwd    the forward-only kernel (scoring)
  step          index-select of the images, logits GEMM, seg_ce, weight-gradient
                GEMM, probe_sgd_ on the weights and on the bias
  composite     the same loss and gradient with torch ops on the device, from the
                same logits: F.interpolate + F.cross_entropy with autograd. It
                holds the upsampled logits, M G C H W fp32 (2.5 GB per head here),
                several times over; where that cannot be allocated, or exceeds what
                torch's upsampling kernel can index, the tool says so instead of
                timing it.
Prints one JSON line per round and a summary line per G with the median and
min/max per arm, and how far composite and seg_ce are apart on the first call.
No time or ratio is a pass condition.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F


def timed_ms(fn, inner):
    """Milliseconds per call of `fn(i)`, i < inner, `inner` calls between two device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(inner):
        out = fn(i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner, out


def composite(logits, bias, labels, c, scale):
    """(loss_sum [G], d/dlogits [M, h, w, G, c] fp32, dbias [G, c]) through autograd."""
    m, h, w, g, _ = logits.shape
    x = logits[..., :c].float().requires_grad_(True)
    b = bias[:, :c].clone().requires_grad_(True)
    up = F.interpolate(x.permute(0, 3, 4, 1, 2).reshape(m, g * c, h, w), size=labels.shape[1:],
                       mode="bilinear", align_corners=False)
    up = up.view(m, g, c, *labels.shape[1:]) + b.view(1, g, c, 1, 1)
    target = labels.long().unsqueeze(1).expand(m, g, *labels.shape[1:])
    loss = F.cross_entropy(up.transpose(1, 2), target, ignore_index=255, reduction="none")
    loss_sum = loss.sum(dim=(0, 2, 3))
    (loss_sum.sum() * scale).backward()
    return loss_sum.detach(), x.grad, b.grad


def bench_heads(args, g, dev):
    from dinov3_amd.ops import probe_sgd_, seg_ce

    m, hw, s, c, d = args.m, args.cells, args.s, args.c, args.d
    cp = (c + 7) // 8 * 8
    gen = torch.Generator(device=dev).manual_seed(g)
    feats = torch.randn(args.n, hw, hw, d, device=dev, generator=gen).bfloat16()
    # labels constant over 4 x 4-cell regions, 5 % ignored, as a crop of a scene would be
    coarse = torch.randint(0, c, (args.n, (hw + 3) // 4, (hw + 3) // 4), device=dev, generator=gen)
    labels = coarse.repeat_interleave(4 * s, 1).repeat_interleave(4 * s, 2)[:, :hw * s, :hw * s]
    labels = labels.to(torch.uint8).contiguous()
    labels[torch.rand(labels.shape, device=dev, generator=gen) < 0.05] = 255
    valid = (labels != 255).sum(dim=(1, 2)).float()
    w = 0.01 * torch.randn(g, cp * d, device=dev, generator=gen)
    w.view(g, cp, d)[:, c:] = 0
    w_mom, w_lp = torch.zeros_like(w), w.bfloat16()
    b, b_mom = torch.zeros(g, cp, device=dev), torch.zeros(g, cp, device=dev)
    lr, wd = torch.full((g,), 1e-2, device=dev), torch.full((g,), 1e-4, device=dev)
    idx = torch.randperm(args.n, device=dev, generator=gen)[:m]
    lr_scale = 0.5 * (1.0 + math.cos(math.pi * 0.3))
    yb = labels.index_select(0, idx)
    inv_valid = valid.index_select(0, idx).sum().reciprocal().view(1)
    raw = (feats.index_select(0, idx).view(m * hw * hw, d) @ w_lp.view(g * cp, d).T)
    raw = (raw.float() * 10.0).bfloat16().view(m, hw, hw, g, cp)  # logits of a trained head's size

    def step(i):
        xb = feats.index_select(0, idx).view(m * hw * hw, d)
        labs = labels.index_select(0, idx)
        scale = valid.index_select(0, idx).sum().clamp(min=1.0).reciprocal().view(1)
        logits = (xb @ w_lp.view(g * cp, d).T).view(m, hw, hw, g, cp)
        loss, _, db = seg_ce(logits, b, labs, c, scale, True)
        dw = logits.view(m * hw * hw, g * cp).T @ xb
        probe_sgd_(w, w_mom, dw.view(g, -1), lr, wd, lr_scale, 0.9, w_lp)
        probe_sgd_(b, b_mom, db, lr, None, lr_scale, 0.9, None)
        return loss

    def ce_alone(inner):
        work = [raw.clone() for _ in range(inner)]  # ahead of the start event: not timed
        return lambda i: (seg_ce(work[i], b, yb, c, inv_valid, True), work[i])

    arms = {
        "seg_ce": ce_alone,
        "seg_ce_fwd": lambda inner: (lambda i: seg_ce(raw, b, yb, c, 0.0, False)),
        "step": lambda inner: step,
        "composite": lambda inner: (lambda i: composite(raw, b, yb, c, inv_valid)),
    }
    first, skipped = {}, {}
    for name in list(arms):  # warm-up, and the first results for the comparison
        try:
            ms, first[name] = timed_ms(arms[name](1), 1)
            print(json.dumps({"G": g, "warmup": name, "ms": round(ms, 3)}), flush=True)
        except (torch.OutOfMemoryError, RuntimeError) as e:  # too large to allocate or to index
            if name != "composite":
                raise
            skipped[name] = "not timed: " + str(e).split("\n")[0][:200]
            print(json.dumps({"G": g, "warmup": name, "skipped": skipped[name]}), flush=True)
            del arms[name]
            torch.cuda.empty_cache()
    gaps = {}
    if "composite" in first:
        (loss, _, db), grad = first["seg_ce"]
        c_loss, c_grad, c_db = first["composite"]
        gaps = {"loss_rel": float(((loss - c_loss).abs() / c_loss.abs()).max()),
                "grad_abs_over_max": float((grad[..., :c].float() - c_grad).abs().max()
                                           / c_grad.abs().max()),
                "dbias_abs_over_max": float((db[:, :c] - c_db).abs().max() / c_db.abs().max())}
    first.clear()
    torch.cuda.empty_cache()

    samples = {name: [] for name in arms}
    for r in range(args.rounds):
        for name in arms:
            inner = max(1, args.inner // 5) if name == "composite" else args.inner
            samples[name].append(timed_ms(arms[name](inner), inner)[0])
        print(json.dumps({"G": g, "round": r, "ms": {n: round(v[-1], 3) for n, v in samples.items()}}),
              flush=True)
    med = {n: statistics.median(v) for n, v in samples.items()}
    out = {"M": m, "cells": hw, "s": s, "C": c, "Cp": cp, "D": d, "G": g, "rounds": args.rounds,
           "inner": args.inner, "workspace_MB": round(m * hw * hw * 4 * g * cp * 4 / 1e6, 1),
           "upsampled_fp32_GB": round(m * g * c * (hw * s) ** 2 * 4 / 1e9, 2),
           "ms_median": {n: round(v, 3) for n, v in med.items()},
           "ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "skipped": skipped, "first_call_gap_to_composite": gaps}
    if "composite" in med:
        out["seg_ce_over_composite"] = round(med["seg_ce"] / med["composite"], 4)
    print(json.dumps(out), flush=True)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=16, help="images per batch")
    p.add_argument("--cells", type=int, default=32, help="cells per image side")
    p.add_argument("--s", type=int, default=16, help="label pixels per cell side")
    p.add_argument("--c", type=int, default=150)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--gs", type=str, default="1,8", help="head counts, comma-separated")
    p.add_argument("--n", type=int, default=64, help="images of the train set the batch is drawn from")
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    dev = torch.device("cuda:0")
    for g in (int(v) for v in args.gs.split(",")):
        bench_heads(args, g, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

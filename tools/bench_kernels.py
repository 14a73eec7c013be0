"""Per-kernel micro-benchmarks: each HIP op vs its plain-torch counterpart.

GPU-only. Usage (on a GPU box):
    python tools/bench_kernels.py [--iters 50] [--streaming-only]

Prints one line per op: name, HIP us, torch us, speedup, effective GB/s of
the HIP path (bytes moved at the op's minimum traffic).
"""

from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timeit(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def row(name, hip_us, ref_us, bytes_moved):
    gbs = bytes_moved / (hip_us * 1e-6) / 1e9 if hip_us > 0 else 0.0
    print(f"{name:34s} hip {hip_us:9.1f} us   torch {ref_us:9.1f} us   "
          f"x{ref_us / hip_us:5.2f}   {gbs:7.0f} GB/s")


def fmha_bwd_rows(iters, rounds=5):
    """The attention backward alone at the flagship student's two crop groups
    (kept samples after drop-path), on an explicit dO, RoPE on, prefix 1:
    the single-pass kernel against the three launches (pre + dq + dkv) in one
    process, `rounds` alternating rounds each, median and minimum."""
    from dinov3_amd.ops import hip_ops

    ops = hip_ops()
    dev = "cuda"
    for B, N, Hh, hd in ((89, 197, 16, 64), (358, 37, 16, 64)):
        qkv = torch.randn(B, N, 3, Hh, hd, device=dev).bfloat16()
        dout = torch.randn(B, N, Hh, hd, device=dev).bfloat16()
        a = torch.rand(N - 1, hd // 2, device=dev)
        a = torch.cat([a, a], dim=-1)
        sin, cos = a.sin().contiguous(), a.cos().contiguous()
        o, lse = ops.fmha_rope_fwd(qkv, sin, cos, 1)
        dqkv = torch.empty_like(qkv)
        times = {"1": [], "0": []}
        saved = os.environ.get("DINOV3_FMHA_FUSED_BWD")
        for _ in range(rounds):
            for flag in ("1", "0"):  # the bindings read the switch at every call
                os.environ["DINOV3_FMHA_FUSED_BWD"] = flag
                times[flag].append(timeit(
                    lambda: ops.fmha_rope_bwd_out(dout, qkv, o, lse, sin, cos, 1, dqkv), iters))
        if saved is None:
            del os.environ["DINOV3_FMHA_FUSED_BWD"]
        else:
            os.environ["DINOV3_FMHA_FUSED_BWD"] = saved
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(f"{f'fmha_rope_bwd [{B},{N},{Hh},{hd}]':34s} fused {med['1']:7.1f} us (min {min(times['1']):7.1f})   "
              f"three-launch {med['0']:7.1f} us (min {min(times['0']):7.1f})   x{med['0'] / med['1']:5.2f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--fmha-bwd-only", action="store_true",
                   help="only the attention-backward rows (single pass against three launches)")
    p.add_argument("--streaming-only", action="store_true",
                   help="stop after the memory-streaming kernels (norms, bias+GELU, LayerScale)")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU required"
    dev = "cuda"
    it = args.iters
    if args.fmha_bwd_only:
        fmha_bwd_rows(it)
        return

    # ViT-L flat-buffer shapes: R = 2*64*197 + 8*64*37 tokens, D = 1024
    R, D = 2 * 64 * 197 + 8 * 64 * 37, 1024
    H4 = 4 * D

    from dinov3_amd.ops import bias_gelu, hip_ops, l2_normalize, layer_norm
    from dinov3_amd.ops.ls_axpy import ls_axpy

    ops = hip_ops()
    x = torch.randn(R, D, device=dev).bfloat16()
    w = torch.ones(D, device=dev).bfloat16()
    b = torch.zeros(D, device=dev).bfloat16()

    row("layernorm_fwd [R,1024]",
        timeit(lambda: layer_norm(x, w, b), it),
        timeit(lambda: torch.nn.functional.layer_norm(x, (D,), w, b), it),
        R * D * 2 * 2)

    h = torch.randn(R, H4, device=dev).bfloat16()
    hb = torch.randn(H4, device=dev).bfloat16()
    row("bias_gelu_fwd [R,4096]",
        timeit(lambda: bias_gelu(h, hb), it),
        timeit(lambda: torch.nn.functional.gelu(h + hb, approximate="tanh"), it),
        R * H4 * 2 * 2)

    res = torch.randn_like(x)
    gamma = torch.full((D,), 1e-5, device=dev).bfloat16()
    row("ls_axpy_fwd [R,1024]",
        timeit(lambda: ls_axpy(x, res, gamma), it),
        timeit(lambda: x + gamma * res, it),
        R * D * 2 * 3)

    row("l2norm_fwd [8192,256]",
        timeit(lambda: l2_normalize(x[:8192, :256]), it),
        timeit(lambda: torch.nn.functional.normalize(x[:8192, :256].float(), dim=-1), it),
        8192 * 256 * 2 * 2)

    # The streaming kernels at the flagship's real row counts: drop_path 0.3
    # keeps 89 of 128 global and 358 of 512 local crops, so the student MLP /
    # residual / norm kernels see RS rows and the teacher's RT. Bytes are the
    # minimum traffic: each [rows, width] bf16 operand read or written once.
    RS, RT = 89 * 197 + 358 * 37, 64 * (197 * 2)
    for tag, rows in (("student", RS), ("teacher", RT)):
        hs = torch.randn(rows, H4, device=dev).bfloat16()
        row(f"bias_gelu_fwd [{rows},4096] {tag}",
            timeit(lambda: ops.bias_gelu_fwd(hs, hb), it),
            timeit(lambda: torch.nn.functional.gelu(hs + hb, approximate="tanh"), it),
            2 * rows * H4 * 2)
    hs = torch.randn(RS, H4, device=dev).bfloat16()
    dhs = torch.randn_like(hs)

    def gelu_bwd_ref():
        v = (hs + hb).float()
        t = torch.tanh(0.7978845608 * (v + 0.044715 * v ** 3))
        d = 0.5 * (1 + t) + 0.5 * v * (1 - t * t) * 0.7978845608 * (1 + 0.134145 * v * v)
        g = dhs.float() * d
        return g.bfloat16(), g.sum(0).bfloat16()

    row(f"bias_gelu_bwd [{RS},4096]",
        timeit(lambda: ops.bias_gelu_bwd(dhs, hs, hb), it),
        timeit(gelu_bwd_ref, max(it // 4, 3)),
        3 * RS * H4 * 2)

    xs = torch.randn(RS, D, device=dev).bfloat16()
    dflat = torch.randn(R, D, device=dev).bfloat16()
    keep = torch.randperm(R, device=dev)[:RS]
    sc = torch.full((RS,), 1.0 / 0.7, device=dev)
    lb = torch.randn(D, device=dev).bfloat16()

    def ls_scatter_bwd_ref():
        gv = dflat[keep].float() * sc[:, None]
        return ((gv * gamma.float()).bfloat16(), (gv * (xs.float() + lb.float())).sum(0),
                (gv * gamma.float()).sum(0))

    row(f"ls_scatter_bwd [{RS},1024]",
        timeit(lambda: ops.ls_scatter_bwd(dflat, keep, xs, gamma, lb, sc), it),
        timeit(ls_scatter_bwd_ref, it),
        3 * RS * D * 2)

    wl = torch.randn(D, device=dev).bfloat16()
    row(f"layernorm_fwd [{RS},1024]",
        timeit(lambda: ops.layernorm_fwd(xs, wl, b, 1e-6), it),
        timeit(lambda: torch.nn.functional.layer_norm(xs, (D,), wl, b, 1e-6), it),
        2 * RS * D * 2)
    _, ln_mean, ln_rstd = ops.layernorm_fwd(xs, wl, b, 1e-6)
    dys = torch.randn_like(xs)
    xg = xs.detach().requires_grad_(True)
    wg, bg = wl.detach().requires_grad_(True), b.detach().requires_grad_(True)

    def ln_bwd_ref():
        y = torch.nn.functional.layer_norm(xg, (D,), wg, bg, 1e-6)
        return torch.autograd.grad(y, (xg, wg, bg), dys)

    row(f"layernorm_bwd [{RS},1024] (torch: f+b)",
        timeit(lambda: ops.layernorm_bwd(dys, xs, wl, ln_mean, ln_rstd), it),
        timeit(ln_bwd_ref, it),
        3 * RS * D * 2)

    # Drop-path gather fused into LayerNorm, and its backward fused into the
    # residual-gradient accumulation. The second column is the UNFUSED
    # sequence of this project's own ops, not torch: row_gather +
    # layernorm_fwd, and layernorm_bwd + zero fill + row_scatter_add_ + the
    # full-buffer add autograd performs. Bytes: the fused kernels' minimum
    # (fwd: rows read once, y and the compact copy written; bwd: dy, x and the
    # accumulator rows read, the accumulator rows written).
    # RF: rows of the student's flat buffer in the flagship step.
    RF = 44672
    empty_f = torch.empty(0, device=dev)
    xf = torch.randn(RF, D, device=dev).bfloat16()
    dacc = torch.randn(RF, D, device=dev).bfloat16()
    keep_f = torch.randperm(RF, device=dev)[:RS]
    _, sub, g_mean, g_rstd = ops.gather_layernorm_fwd(xf, keep_f, wl, b, 1e-6)

    def gather_ln_unfused():
        return ops.layernorm_fwd(ops.row_gather(xf, keep_f), wl, b, 1e-6)

    row(f"gather_layernorm_fwd [{RS} of {RF},1024]",
        timeit(lambda: ops.gather_layernorm_fwd(xf, keep_f, wl, b, 1e-6), it),
        timeit(gather_ln_unfused, it),
        3 * RS * D * 2)

    def ln_bwd_scatter_unfused():
        dx, dw_, db_ = ops.layernorm_bwd(dys, sub, wl, g_mean, g_rstd)
        buf = torch.zeros(RF, D, dtype=dx.dtype, device=dev)
        ops.row_scatter_add_(buf, keep_f, dx, empty_f)
        return dacc + buf, dw_, db_

    row(f"ln_bwd_scatter_acc [{RS} of {RF},1024]",
        timeit(lambda: ops.layernorm_bwd_scatter_acc_(dacc, keep_f, dys, sub, wl, g_mean,
                                                      g_rstd), it),
        timeit(ln_bwd_scatter_unfused, it),
        4 * RS * D * 2)
    if args.streaming_only:
        return

    # FMHA fwd: global-crop group
    from dinov3_amd.ops.flat_attention import flat_multi_fmha

    B, N, Hh, hd = 128, 197, 16, 64
    qkv = torch.randn(B * N, 3 * Hh * hd, device=dev).bfloat16()
    Pn = N - 1
    a = torch.rand(Pn, hd // 2, device=dev)
    a = torch.cat([a, a], dim=-1)
    sin, cos = a.sin().contiguous(), a.cos().contiguous()
    metas = [(0, B, N, sin, cos, 1)]
    q = qkv.view(B, N, 3, Hh, hd)[:, :, 0].permute(0, 2, 1, 3)

    def sdpa():
        qq = q.contiguous()
        return torch.nn.functional.scaled_dot_product_attention(qq, qq, qq)

    row("fmha_rope_fwd [128,197,16,64]",
        timeit(lambda: flat_multi_fmha(qkv, Hh, metas), it),
        timeit(sdpa, it),
        B * N * 3 * Hh * hd * 2 * 2)

    # FMHA hd-128 at the high-res-adapt shape: ViT-7b/16 @768px -> N=2305
    # (dinov3_vit7b16_high_res_adapt.yaml:162-186), 32 heads x d128
    B2, N2, Hh2, hd2 = 4, 2305, 32, 128
    qkv2 = torch.randn(B2 * N2, 3 * Hh2 * hd2, device=dev).bfloat16()
    Pn2 = N2 - 1
    a2 = torch.rand(Pn2, hd2 // 2, device=dev)
    a2 = torch.cat([a2, a2], dim=-1)
    sin2, cos2 = a2.sin().contiguous(), a2.cos().contiguous()
    metas2 = [(0, B2, N2, sin2, cos2, 1)]
    q2 = qkv2.view(B2, N2, 3, Hh2, hd2)[:, :, 0].permute(0, 2, 1, 3)

    def sdpa2():
        qq = q2.contiguous()
        return torch.nn.functional.scaled_dot_product_attention(qq, qq, qq)

    row("fmha_rope_fwd [4,2305,32,128]",
        timeit(lambda: flat_multi_fmha(qkv2, Hh2, metas2), it),
        timeit(sdpa2, it),
        B2 * N2 * 3 * Hh2 * hd2 * 2 * 2)

    def fmha2_fwd_bwd():
        qkv_g = qkv2.detach().requires_grad_(True)
        out = flat_multi_fmha(qkv_g, Hh2, metas2)
        out.float().sum().backward()

    def sdpa2_fwd_bwd():
        qq = q2.detach().contiguous().requires_grad_(True)
        out = torch.nn.functional.scaled_dot_product_attention(qq, qq, qq)
        out.float().sum().backward()

    row("fmha_rope_f+b [4,2305,32,128]",
        timeit(fmha2_fwd_bwd, max(it // 4, 3)),
        timeit(sdpa2_fwd_bwd, max(it // 4, 3)),
        B2 * N2 * 3 * Hh2 * hd2 * 2 * 6)

    fmha_bwd_rows(it)

    # fused sinkhorn over K=65536 (teacher shapes: M=128 cls rows)
    from dinov3_amd.ops.proto_scores import sinkhorn_knopp_factored

    K = 65536
    logits = torch.randn(128, K, device=dev).bfloat16()

    def dense_sinkhorn():
        Q = (logits.float() / 0.07).T.exp()
        Q = Q / Q.sum()
        for _ in range(3):
            Q = Q / Q.sum(dim=1, keepdim=True) / K
            Q = Q / Q.sum(dim=0, keepdim=True) / 128
        return Q

    row("sinkhorn K=65536 M=128 (3 it)",
        timeit(lambda: sinkhorn_knopp_factored(logits, 0.07, 3), it),
        timeit(dense_sinkhorn, it),
        128 * K * 2 * 6)

    # patch-embed GEMM
    xi = torch.randn(64, 3, 224, 224, device=dev).bfloat16()
    wpe = (torch.randn(1024, 768, device=dev) * 0.02).bfloat16()
    bpe = torch.zeros(1024, device=dev).bfloat16()
    conv_w = wpe.reshape(1024, 3, 16, 16)

    row("patch_embed [64,3,224,224]",
        timeit(lambda: ops.patch_embed_fwd(xi, wpe, bpe, 16), it),
        timeit(lambda: torch.nn.functional.conv2d(xi, conv_w, bpe, stride=16), it),
        64 * 3 * 224 * 224 * 2 + 64 * 196 * 1024 * 2)


if __name__ == "__main__":
    main()

"""GPU kernel numerics: each HIP kernel vs a plain PyTorch fp32 reference."""

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _assert_close(got, want, atol, rtol=1e-2, what=""):
    got = got.float()
    want = want.float()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= atol + rtol * scale, f"{what}: max err {err} (scale {scale})"


@pytest.fixture(scope="module")
def ops():
    from dinov3_amd.ops import hip_ops

    return hip_ops()


def test_mfma_layout_probe(ops):
    """C[32,32] = A[32,16] @ B[16,32]; asymmetric inputs (transpose-detecting)."""
    torch.manual_seed(0)
    A = torch.randn(32, 16, device=DEV).bfloat16()
    B = torch.randn(16, 32, device=DEV).bfloat16()
    C = ops.probe_mfma(A.contiguous(), B.contiguous())
    ref = A.float() @ B.float()
    _assert_close(C, ref, atol=0.05, what="mfma probe")


@pytest.mark.parametrize("rows,D", [(64, 1024), (197, 384), (1000, 4096), (33, 256), (130, 1536)])
def test_layernorm_fwd_bwd(ops, rows, D):
    torch.manual_seed(0)
    x = torch.randn(rows, D, device=DEV).bfloat16().requires_grad_(True)
    w = torch.randn(D, device=DEV).bfloat16().requires_grad_(True)
    b = torch.randn(D, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops import layer_norm

    y = layer_norm(x, w, b, eps=1e-6)
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-6)
    _assert_close(y, yr, atol=0.05, what="ln fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.08, what="ln dx")
    _assert_close(w.grad, wr.grad, atol=0.3, rtol=2e-2, what="ln dw")
    _assert_close(b.grad, br.grad, atol=0.3, rtol=2e-2, what="ln db")


def test_rmsnorm_fwd_bwd(ops):
    torch.manual_seed(1)
    rows, D = 128, 512
    x = torch.randn(rows, D, device=DEV).bfloat16().requires_grad_(True)
    w = torch.randn(D, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops import rms_norm

    y = rms_norm(x, w, eps=1e-6)
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    yr = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * wr
    _assert_close(y, yr, atol=0.05, what="rms fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.08, what="rms dx")
    _assert_close(w.grad, wr.grad, atol=0.3, rtol=2e-2, what="rms dw")


def test_l2norm_fwd_bwd(ops):
    torch.manual_seed(2)
    rows, D = 200, 256
    x = torch.randn(rows, D, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops import l2_normalize

    y = l2_normalize(x, eps=1e-12)
    xr = x.detach().float().requires_grad_(True)
    yr = xr / (xr.norm(dim=-1, keepdim=True) + 1e-12)
    _assert_close(y, yr, atol=0.02, what="l2 fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.02, what="l2 dx")


def test_bias_gelu_fwd_bwd(ops):
    torch.manual_seed(3)
    rows, H = 256, 1024
    x = torch.randn(rows, H, device=DEV).bfloat16().requires_grad_(True)
    b = torch.randn(H, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops import bias_gelu

    y = bias_gelu(x, b)
    xr = x.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    yr = torch.nn.functional.gelu(xr + br, approximate="tanh")
    _assert_close(y, yr, atol=0.03, what="bias_gelu fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.05, what="bias_gelu dx")
    _assert_close(b.grad, br.grad, atol=0.5, rtol=2e-2, what="bias_gelu db")


def test_swiglu_fwd_bwd(ops):
    torch.manual_seed(4)
    rows, H = 128, 344
    x = torch.randn(rows, 2 * H, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops.bias_act import swiglu_gate

    y = swiglu_gate(x)
    xr = x.detach().float().requires_grad_(True)
    yr = torch.nn.functional.silu(xr[..., :H]) * xr[..., H:]
    _assert_close(y, yr, atol=0.05, what="swiglu fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.05, what="swiglu dx")


@pytest.mark.parametrize("prefix", [0, 1, 5])
def test_rope_fwd_bwd(ops, prefix):
    torch.manual_seed(5)
    B, H, N, hd = 2, 4, 37, 64
    P = N - prefix
    x = torch.randn(B, H, N, hd, device=DEV).bfloat16().requires_grad_(True)
    angles = torch.rand(P, hd // 2, device=DEV) * 6.28
    angles = torch.cat([angles, angles], dim=-1)
    sin, cos = angles.sin(), angles.cos()
    from dinov3_amd.ops import rope_apply

    y = rope_apply(x, sin, cos, prefix)
    xr = x.detach().float().requires_grad_(True)
    h = hd // 2
    tail = xr[..., prefix:, :]
    rot = torch.cat([-tail[..., h:], tail[..., :h]], dim=-1)
    yr = torch.cat([xr[..., :prefix, :], tail * cos + rot * sin], dim=-2)
    _assert_close(y, yr, atol=0.03, what="rope fwd")
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.03, what="rope dx")


@pytest.mark.parametrize("N,hd", [(37, 64), (197, 64), (201, 64), (128, 64), (197, 128), (530, 64)])
def test_fmha_fwd_matches_reference(ops, N, hd):
    torch.manual_seed(6)
    B, H = 3, 4
    q = torch.randn(B, H, N, hd, device=DEV).bfloat16()
    k = torch.randn(B, H, N, hd, device=DEV).bfloat16()
    v = torch.randn(B, H, N, hd, device=DEV).bfloat16()
    from dinov3_amd.ops.fmha import fmha_ref

    o, lse = ops.fmha_fwd(q, k, v)
    ref = fmha_ref(q.float(), k.float(), v.float())
    _assert_close(o, ref, atol=0.03, what=f"fmha fwd N={N}")
    # lse sanity: softmax denominators positive/finite
    assert torch.isfinite(lse).all()


@pytest.mark.parametrize("N,hd", [(37, 64), (197, 64), (197, 128)])
def test_fmha_bwd_matches_reference(ops, N, hd):
    torch.manual_seed(7)
    B, H = 2, 3
    q = torch.randn(B, H, N, hd, device=DEV).bfloat16().requires_grad_(True)
    k = torch.randn(B, H, N, hd, device=DEV).bfloat16().requires_grad_(True)
    v = torch.randn(B, H, N, hd, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops import fmha

    o = fmha(q, k, v)
    dy = torch.randn_like(o)
    o.backward(dy)

    qr = q.detach().float().requires_grad_(True)
    kr = k.detach().float().requires_grad_(True)
    vr = v.detach().float().requires_grad_(True)
    s = torch.einsum("bhqd,bhkd->bhqk", qr, kr) / math.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    oref = torch.einsum("bhqk,bhkd->bhqd", p, vr)
    oref.backward(dy.float())
    _assert_close(q.grad, qr.grad, atol=0.05, what=f"fmha dq N={N}")
    _assert_close(k.grad, kr.grad, atol=0.05, what=f"fmha dk N={N}")
    _assert_close(v.grad, vr.grad, atol=0.05, what=f"fmha dv N={N}")


def test_multi_tensor_ema_gpu(ops):
    from dinov3_amd.ops import ema_update_

    torch.manual_seed(8)
    t = [torch.randn(1000, device=DEV).bfloat16(), torch.randn(3, 7, device=DEV).bfloat16()]
    s = [torch.randn_like(x) for x in t]
    t_ref = [x.float().clone() for x in t]
    ema_update_(t, s, 0.9)
    for tr, sv, tv in zip(t_ref, s, t):
        want = 0.9 * tr + 0.1 * sv.float()
        _assert_close(tv, want, atol=0.02, what="ema")


def _adamw_step1_ref(p32, g, lr=0.01, wd=0.05, scale=1.0):
    """fp32 AdamW at step 1 from zero moments: beta = (0.9, 0.999), eps = 1e-8."""
    gm = g.float() * scale
    mh = 0.1 * gm / (1 - 0.9)
    vh = 0.001 * gm * gm / (1 - 0.999)
    return p32 * (1 - lr * wd) - lr * mh / (vh.sqrt() + 1e-8)


def _adamw_state(shapes, grad_dtype=torch.bfloat16):
    p32 = [torch.randn(s, device=DEV) for s in shapes]
    p = [x.bfloat16() for x in p32]
    master = [x.clone() for x in p32]
    g = [torch.randn(s, device=DEV).to(grad_dtype) for s in shapes]
    m = [torch.zeros(s, device=DEV) for s in shapes]
    v = [torch.zeros(s, device=DEV) for s in shapes]
    return p32, p, g, m, v, master


def test_multi_tensor_adamw_gpu(ops):
    from dinov3_amd.ops import multi_tensor_adamw_

    torch.manual_seed(9)
    shapes = [(64, 64), (130,), (1000, 3)]
    p32, p, g, m, v, master = _adamw_state(shapes)
    multi_tensor_adamw_(p, g, m, v, master, 0.01, 0.9, 0.999, 1e-8, 0.05, step=1)
    # torch reference on fp32 copies
    for i, s in enumerate(shapes):
        ref = _adamw_step1_ref(p32[i], g[i])
        _assert_close(master[i], ref, atol=1e-4, what=f"adamw master {i}")
        _assert_close(p[i], ref, atol=0.01, what=f"adamw param {i}")


def test_multi_tensor_l2norm_gpu(ops):
    from dinov3_amd.ops import grad_l2_norm_sq

    g = [torch.randn(100, device=DEV).bfloat16(), torch.randn(55, 3, device=DEV).bfloat16()]
    got = grad_l2_norm_sq(g)
    want = sum(x.float().pow(2).sum() for x in g)
    _assert_close(got, want, atol=0.5, rtol=1e-2, what="l2norm_sq")


def test_multi_tensor_multi_chunk_gpu(ops):
    """One tensor spans two chunks, the second one ragged, between two small tensors."""
    from dinov3_amd.ops import ema_update_, grad_l2_norm_sq, multi_tensor_adamw_
    from dinov3_amd.ops.mt_plan import CHUNK

    assert ops.MT_CHUNK == CHUNK
    torch.manual_seed(20)
    shapes = [(3, 7), (CHUNK + 130,), (130,)]
    t = [torch.randn(s, device=DEV).bfloat16() for s in shapes]
    s_ = [torch.randn_like(x) for x in t]
    t_ref = [x.float().clone() for x in t]
    ema_update_(t, s_, 0.9)
    for i, (tr, sv, tv) in enumerate(zip(t_ref, s_, t)):
        _assert_close(tv, 0.9 * tr + 0.1 * sv.float(), atol=0.02, what=f"ema {i}")

    p32, p, g, m, v, master = _adamw_state(shapes)
    multi_tensor_adamw_(p, g, m, v, master, 0.01, 0.9, 0.999, 1e-8, 0.05, step=1)
    for i in range(len(shapes)):
        ref = _adamw_step1_ref(p32[i], g[i])
        _assert_close(master[i], ref, atol=1e-4, what=f"adamw master {i}")
        _assert_close(p[i], ref, atol=0.01, what=f"adamw param {i}")

    got = grad_l2_norm_sq(g)
    want = sum(x.float().pow(2).sum() for x in g)
    _assert_close(got, want, atol=0.5, rtol=1e-2, what="l2norm_sq")


def test_adamw_planned_fp32_grads_gpu(ops):
    """bf16 params, fp32 grads and fp32 masters: the pairing of the sharded engine."""
    from dinov3_amd.ops.mt_plan import MultiTensorPlan, adamw_planned

    torch.manual_seed(21)
    shapes = [(64, 64), (130,), (1000, 3)]
    p32, p, g, m, v, master = _adamw_state(shapes, grad_dtype=torch.float32)
    n = len(shapes)
    ones = torch.ones(n, device=DEV)
    adamw_planned(MultiTensorPlan([p, g, m, v, master]), ones, ones, torch.zeros(n, device=DEV),
                  torch.zeros(n, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV),
                  0.01, 0.01, 0.05, 0.9, 0.999, 1e-8, 1, True)
    for i in range(n):
        ref = _adamw_step1_ref(p32[i], g[i])
        _assert_close(master[i], ref, atol=1e-4, what=f"adamw master {i}")
        _assert_close(p[i], ref, atol=0.01, what=f"adamw param {i}")


def test_adamw_planned_per_tensor_tables_gpu(ops):
    """Distinct lr multipliers, a frozen last layer, two submodels with their own clip."""
    from dinov3_amd.ops.mt_plan import MultiTensorPlan, adamw_planned

    torch.manual_seed(22)
    shapes = [(64, 64), (130,), (1000, 3)]
    p32, p, g, m, v, master = _adamw_state(shapes)
    lr_mult, sub_id, clip = [1.0, 0.5, 0.25], [0, 1, 0], [1.0, 0.5]
    adamw_planned(MultiTensorPlan([p, g, m, v, master]), torch.tensor(lr_mult, device=DEV),
                  torch.ones(3, device=DEV), torch.tensor([0.0, 0.0, 1.0], device=DEV),
                  torch.tensor(sub_id, dtype=torch.int32, device=DEV),
                  torch.tensor(clip, device=DEV), 0.01, 0.0, 0.05, 0.9, 0.999, 1e-8, 1, True)
    for i in range(2):
        ref = _adamw_step1_ref(p32[i], g[i], lr=0.01 * lr_mult[i], scale=clip[sub_id[i]])
        _assert_close(master[i], ref, atol=1e-4, what=f"adamw master {i}")
        _assert_close(p[i], ref, atol=0.01, what=f"adamw param {i}")
    # is_last with last_lr = 0: no step and a weight-decay factor of 1
    assert torch.equal(master[2], p32[2]), "a frozen last layer must not move"


def test_l2norm_planned_per_submodel_gpu(ops):
    from dinov3_amd.ops.mt_plan import MultiTensorPlan, l2norm_planned

    torch.manual_seed(23)
    g = [torch.randn(s, device=DEV).bfloat16() for s in [(100,), (55, 3), (64, 64)]]
    sub_id = [0, 1, 0]
    got = l2norm_planned(MultiTensorPlan([g]), torch.tensor(sub_id, dtype=torch.int32, device=DEV), 2)
    assert got.shape == (2,)
    for sub in range(2):
        want = sum(x.float().pow(2).sum() for x, i in zip(g, sub_id) if i == sub)
        _assert_close(got[sub], want, atol=0.5, rtol=1e-2, what=f"l2norm submodel {sub}")


def test_bindings_check_every_tensor(ops):
    """A wrong dtype, device or layout raises on the host, before any launch."""
    x = torch.randn(4, 64, device=DEV).bfloat16()
    w = torch.ones(64, device=DEV)
    with pytest.raises(RuntimeError):  # fp32 weight under bf16 activations
        ops.layernorm_fwd(x, w, w.bfloat16(), 1e-6)
    with pytest.raises(RuntimeError):  # int32 row index
        ops.row_gather(x, torch.arange(4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):  # non-contiguous bias
        ops.bias_gelu_fwd(x, torch.zeros(128, device=DEV).bfloat16()[::2])
    with pytest.raises(RuntimeError):  # weight on the host
        ops.layernorm_fwd(x, w.bfloat16().cpu(), w.bfloat16(), 1e-6)


def _proto_binding_calls(ops):
    """name -> (function, good arguments) for every prototype-loss binding;
    tensors by name so that one can be swapped for a malformed one."""
    S, T, B, M, K = 3, 2, 2, 5, 16
    f32 = dict(device=DEV, dtype=torch.float32)
    x3 = torch.zeros(S, B, K, device=DEV).bfloat16()
    xt3 = torch.zeros(T, B, K, device=DEV).bfloat16()
    x2 = torch.zeros(M, K, device=DEV).bfloat16()
    t3, t2 = torch.full((T, B, K), 1.0 / K, **f32), torch.full((M, K), 1.0 / K, **f32)
    rows3, rows2, uT = torch.ones(S * B, **f32), torch.ones(M, **f32), torch.ones(T * B, **f32)
    v, g = torch.full((K,), 1.0 / K, **f32), torch.ones((), **f32)
    return {
        "dino_ce_fwd": (lambda a: ops.dino_ce_fwd(a["x"], a["t"], 0.1, False), dict(x=x3, t=t3)),
        "dino_ce_bwd": (lambda a: ops.dino_ce_bwd(a["g"], a["x"], a["t"], a["lse"], a["st"], 0.1, False),
                        dict(g=g, x=x3, t=t3, lse=rows3, st=rows3)),
        "ibot_ce_fwd": (lambda a: ops.ibot_ce_fwd(a["x"], a["t"], a["w"], 0.1), dict(x=x2, t=t2, w=rows2)),
        "ibot_ce_bwd": (lambda a: ops.ibot_ce_bwd(a["g"], a["x"], a["t"], a["w"], a["lse"], a["st"], 0.1),
                        dict(g=g, x=x2, t=t2, w=rows2, lse=rows2, st=rows2)),
        "sinkhorn_fact_colsum": (lambda a: ops.sinkhorn_fact_colsum(a["x"], a["u"], 0.1), dict(x=x2, u=rows2)),
        "sinkhorn_fact_rowsum": (lambda a: ops.sinkhorn_fact_rowsum(a["x"], a["v"], 0.1), dict(x=x2, v=v)),
        "ibot_ce_fact_fwd": (lambda a: ops.ibot_ce_fact_fwd(a["x"], a["xt"], a["u"], a["v"], a["w"], 0.1, 0.1),
                             dict(x=x2, xt=x2, u=rows2, v=v, w=rows2)),
        "ibot_ce_fact_bwd": (lambda a: ops.ibot_ce_fact_bwd(a["g"], a["x"], a["xt"], a["u"], a["v"], a["w"],
                                                            a["lse"], a["st"], 0.1, 0.1),
                             dict(g=g, x=x2, xt=x2, u=rows2, v=v, w=rows2, lse=rows2, st=rows2)),
        "dino_ce_fact_fwd": (lambda a: ops.dino_ce_fact_fwd(a["x"], a["xt"], a["u"], a["v"], 0.1, 0.1, False),
                             dict(x=x3, xt=xt3, u=uT, v=v)),
        "dino_ce_fact_bwd": (lambda a: ops.dino_ce_fact_bwd(a["g"], a["x"], a["xt"], a["u"], a["v"], a["lse"],
                                                            a["st"], 0.1, 0.1, False),
                             dict(g=g, x=x3, xt=xt3, u=uT, v=v, lse=rows3, st=rows3)),
        "sinkhorn_exp": (lambda a: ops.sinkhorn_exp(a["x"], 0.1), dict(x=x2)),
        "sinkhorn_colsum": (lambda a: ops.sinkhorn_colsum(a["Q"], a["divisor"]), dict(Q=t2.clone(), divisor=g)),
        "sinkhorn_div_row": (lambda a: ops.sinkhorn_div_row(a["Q"], a["col"], float(K), a["B"], True),
                             dict(Q=t2.clone(), col=v, B=g)),
    }


def test_proto_bindings_check_every_tensor(ops):
    """Every tensor of every prototype-loss binding: a wrong dtype, a wrong
    length, a non-contiguous view or a host tensor raises on the host, before
    any launch; so do a K that is no multiple of 8 and misaligned logits in the
    vectorised column sum, and a teacher whose B or K differs."""
    calls = _proto_binding_calls(ops)
    for name, (fn, good) in calls.items():
        fn(good)                                           # the well-formed call goes through
        for key, t in good.items():
            wrong_dtype = t.double() if t.dtype != torch.float64 else t.float()
            # one element more, or one column more (one more student row would be a valid input)
            longer = (torch.cat([t.reshape(-1), t.reshape(-1)[:1]]) if t.dim() <= 1
                      else torch.cat([t, t[..., :1]], dim=-1))
            strided = torch.stack([t, t], dim=-1)[..., 0]
            assert not strided.is_contiguous() or t.numel() <= 1
            bad = {"dtype": wrong_dtype, "host": t.cpu()}
            if (name, key) not in (("sinkhorn_exp", "x"), ("sinkhorn_colsum", "Q")):   # any [M, K] is an input there
                bad["length"] = longer
            if t.numel() > 1:
                bad["non-contiguous"] = strided
            for what, b in bad.items():
                with pytest.raises(RuntimeError):
                    fn({**good, key: b})
                    pytest.fail(f"{name}: {key} with wrong {what} was accepted")
    torch.cuda.synchronize()
    x = torch.zeros(5, 20, device=DEV).bfloat16()
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.sinkhorn_fact_colsum(x, torch.empty(0, device=DEV), 0.1)
    buf = torch.zeros(5 * 16 + 8, device=DEV).bfloat16()
    with pytest.raises(RuntimeError, match="aligned"):
        ops.sinkhorn_fact_colsum(buf[1:81].view(5, 16), torch.empty(0, device=DEV), 0.1)
    fn, good = calls["dino_ce_fact_fwd"]
    with pytest.raises(RuntimeError):                      # teacher with another K
        fn({**good, "xt": torch.zeros(2, 2, 24, device=DEV).bfloat16()})
    with pytest.raises(RuntimeError):                      # teacher with another B
        fn({**good, "xt": torch.zeros(2, 3, 16, device=DEV).bfloat16(), "u": torch.ones(6, device=DEV)})
    torch.cuda.synchronize()


def test_ls_axpy_fwd_bwd(ops):
    torch.manual_seed(10)
    R, D = 300, 1024
    x = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    res = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    gamma = (torch.randn(D, device=DEV) * 0.01).bfloat16().requires_grad_(True)
    from dinov3_amd.ops.ls_axpy import ls_axpy

    out = ls_axpy(x, res, gamma)
    xr = x.detach().float().requires_grad_(True)
    rr = res.detach().float().requires_grad_(True)
    gr = gamma.detach().float().requires_grad_(True)
    ref = xr + gr * rr
    _assert_close(out, ref, atol=0.03, what="ls_axpy fwd")
    dy = torch.randn_like(out)
    out.backward(dy)
    ref.backward(dy.float())
    _assert_close(x.grad, xr.grad, atol=0.02, what="ls_axpy dx")
    _assert_close(res.grad, rr.grad, atol=0.02, what="ls_axpy dres")
    _assert_close(gamma.grad, gr.grad, atol=0.3, rtol=2e-2, what="ls_axpy dgamma")


def test_row_gather_scatter(ops):
    torch.manual_seed(11)
    R, D, M = 64, 256, 24
    flat = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    idx = torch.randperm(R, device=DEV)[:M]
    from dinov3_amd.ops.row_ops import gather_rows, scatter_add_rows

    sub = gather_rows(flat, idx)
    assert torch.equal(sub, flat.detach()[idx])
    res = torch.randn(M, D, device=DEV).bfloat16().requires_grad_(True)
    scale = torch.full((M,), 1.5, device=DEV)
    out = scatter_add_rows(flat, idx, res, scale)
    ref_in = flat.detach().float().requires_grad_(True)
    res_ref = res.detach().float().requires_grad_(True)
    ref = ref_in.index_add(0, idx, res_ref * 1.5)
    _assert_close(out, ref, atol=0.05, what="scatter fwd")
    dy = torch.randn_like(out)
    out.backward(dy)
    ref.backward(dy.float())
    _assert_close(flat.grad, ref_in.grad, atol=0.02, what="scatter dflat")
    _assert_close(res.grad, res_ref.grad, atol=0.03, what="scatter dres")


def test_gather_rows_backward(ops):
    torch.manual_seed(12)
    R, D, M = 32, 64, 10
    flat = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    idx = torch.randperm(R, device=DEV)[:M]
    from dinov3_amd.ops.row_ops import gather_rows

    sub = gather_rows(flat, idx)
    (sub.float() ** 2).sum().backward()
    ref = torch.zeros_like(flat, dtype=torch.float32)
    ref[idx] = 2 * flat.detach()[idx].float()
    _assert_close(flat.grad, ref, atol=0.05, what="gather dflat")


@pytest.mark.parametrize("H,W,P", [(224, 224, 16), (224, 224, 14), (98, 126, 14),
                                   (64, 64, 8)])
def test_patch_embed_gemm_matches_reference(ops, H, W, P):
    torch.manual_seed(13)
    B, C, D = 3, 3, 1024
    x = torch.randn(B, C, H, W, device=DEV).bfloat16()
    w = (torch.randn(D, C * P * P, device=DEV) * 0.02).bfloat16()
    b = torch.randn(D, device=DEV).bfloat16()
    out = ops.patch_embed_fwd(x, w, b, P)
    # fp32 reference with the conv-native (c, dy, dx) flattening
    xr = x.float().reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5)
    rows = xr.reshape(B, (H // P) * (W // P), C * P * P)
    ref = rows @ w.float().T + b.float()
    _assert_close(out, ref, atol=0.15, rtol=2e-2, what=f"patch_embed gemm P={P}")


def test_patch_embed_autograd_wgrad(ops):
    torch.manual_seed(14)
    from dinov3_amd.layers.patch_embed import PatchEmbed

    pe = PatchEmbed(img_size=64, patch_size=16, embed_dim=128).to(DEV).bfloat16()
    x = torch.randn(2, 3, 64, 64, device=DEV).bfloat16()
    out, hp, wp = pe(x)
    out.float().pow(2).sum().backward()
    assert pe.proj.weight.grad is not None and torch.isfinite(pe.proj.weight.grad).all()
    assert pe.proj.bias.grad is not None


needs_fused_residual = pytest.mark.skipif(
    os.environ.get("DINOV3_FUSED_RESIDUAL", "0") != "1",
    reason="gated: set DINOV3_FUSED_RESIDUAL=1 to validate the fused residual kernels")


@needs_fused_residual
def test_ls_axpy_bias_fwd_bwd(ops):
    torch.manual_seed(21)
    R, D = 64, 128
    x = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    res = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    gamma = (torch.randn(D, device=DEV) * 0.01).bfloat16().requires_grad_(True)
    bias = torch.randn(D, device=DEV).bfloat16().requires_grad_(True)
    from dinov3_amd.ops.fused_residual import ls_axpy_bias

    out = ls_axpy_bias(x, res, gamma, bias)
    dy = torch.randn_like(out)
    out.backward(dy)
    xr, rr, gr, br = [t.detach().float().requires_grad_(True) for t in (x, res, gamma, bias)]
    ref = xr + gr * (rr + br)
    ref.backward(dy.float())
    _assert_close(out, ref, atol=0.05, what="ls_axpy_bias fwd")
    _assert_close(x.grad, xr.grad, atol=0.02, what="dx")
    _assert_close(res.grad, rr.grad, atol=0.02, what="dres")
    _assert_close(gamma.grad, gr.grad, atol=0.05 + 0.02 * gr.grad.abs().max().item(), what="dgamma")
    _assert_close(bias.grad, br.grad, atol=0.05 + 0.02 * br.grad.abs().max().item(), what="dbias")


@needs_fused_residual
def test_ls_scatter_add_fwd_bwd(ops):
    torch.manual_seed(22)
    R, D, M = 48, 64, 20
    flat = torch.randn(R, D, device=DEV).bfloat16().requires_grad_(True)
    res = torch.randn(M, D, device=DEV).bfloat16().requires_grad_(True)
    gamma = (torch.randn(D, device=DEV) * 0.01).bfloat16().requires_grad_(True)
    bias = torch.randn(D, device=DEV).bfloat16().requires_grad_(True)
    idx = torch.randperm(R, device=DEV)[:M]
    scale = (torch.rand(M, device=DEV) + 0.5)
    from dinov3_amd.ops.fused_residual import ls_scatter_add_rows

    out = ls_scatter_add_rows(flat.clone(), idx, res, gamma, bias, scale)
    dy = torch.randn_like(out)
    out.backward(dy)
    fr, rr, gr, br = [t.detach().float().requires_grad_(True) for t in (flat, res, gamma, bias)]
    ref = fr.index_add(0, idx, (gr * (rr + br)) * scale.unsqueeze(1))
    ref.backward(dy.float())
    _assert_close(out, ref, atol=0.05, what="ls_scatter fwd")
    _assert_close(flat.grad, fr.grad, atol=0.02, what="dflat")
    _assert_close(res.grad, rr.grad, atol=0.03, what="dres")
    _assert_close(gamma.grad, gr.grad, atol=0.05 + 0.02 * gr.grad.abs().max().item(), what="dgamma")
    _assert_close(bias.grad, br.grad, atol=0.05 + 0.02 * br.grad.abs().max().item(), what="dbias")


@needs_fused_residual
def test_fused_residual_block_gpu():
    """Full block fwd+bwd with the fused residual path vs the default path."""
    from dinov3_amd.layers.attention import SelfAttention
    from dinov3_amd.layers.block import DropPathPlan, SelfAttentionBlock
    from dinov3_amd.utils.utils import cat_keep_shapes

    results = {}
    for fused in (False, True):
        os.environ["DINOV3_DISABLE_HIP"] = "0"
        os.environ["DINOV3_FUSED_RESIDUAL"] = "1" if fused else "0"
        torch.manual_seed(31)
        # head_dim must be 64 (the FMHA kernel's supported sizes are 64/128)
        blk = SelfAttentionBlock(dim=128, num_heads=2, qkv_bias=True, drop_path=0.5,
                                 init_values=1e-2).to(DEV).bfloat16()
        blk.train()
        torch.manual_seed(32)
        x = torch.randn(6, 32, 128, device=DEV).bfloat16()
        flat, _, _ = cat_keep_shapes([x])
        # the fused path mutates the flat buffer in place — feed a NON-leaf
        # (as in training, where it is an op output), keep the leaf for grads
        flat_leaf = flat.clone().requires_grad_(True)
        flat = flat_leaf * 1.0
        metas = [SelfAttention._meta_for(x, None, 0)]
        torch.manual_seed(33)
        plan = DropPathPlan(metas, 0.5, 2, flat.device)
        out = blk.forward_flat(flat, metas, plan, 0)
        out.float().pow(2).sum().backward()
        results[fused] = (out.detach().float(),
                          {n: p.grad.float().clone() for n, p in blk.named_parameters()})
    os.environ["DINOV3_FUSED_RESIDUAL"] = "1"  # restore for other gated tests
    out_a, grads_a = results[False]
    out_b, grads_b = results[True]
    _assert_close(out_b, out_a, atol=0.05, what="fused block fwd")
    for n in grads_a:
        scale = grads_a[n].abs().max().item()
        _assert_close(grads_b[n], grads_a[n], atol=0.05 + 0.03 * scale, what=f"grad {n}")

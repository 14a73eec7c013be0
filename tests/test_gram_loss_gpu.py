"""The fused Gram loss against its fp64 oracle on the same bf16-rounded inputs
with bounds derived from the kernels' rounding steps, panel independence,
run-to-run bit-equality, pad hygiene, the forward-only form, the workspace, the
argument checks, the module switch and one training step behind it."""

import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24     # unit roundoff of fp32
BF16 = 2.0 ** -8   # one round-to-nearest-even to bf16 (8 significant bits), relative
BF16_P = 2.0 ** -9  # the figure the issue sets for the rounding of P: half of BF16
TILE = 128

# (G, M, D): degenerate; less than one tile, one 16-byte chunk; exactly one tile and one
# K-chunk, two matrices; one row past a tile and a D that is no multiple of the K-chunk;
# ragged on both axes; several tiles at ViT-S width
SHAPES = [(1, 1, 8), (1, 33, 8), (2, 128, 64), (3, 129, 72), (1, 257, 200), (1, 300, 384)]
# (remove_neg, remove_only_teacher_neg)
MODES = {"plain": (False, False), "remove_neg": (True, False), "teacher_neg": (False, True)}


def _inputs(G, M, D):
    """S = randn rounded to bf16, T = S + 0.5 randn drawn in fp64 and rounded to bf16 (CPU)."""
    gen = torch.Generator().manual_seed(1000 * G + M + D)
    s = torch.randn(G, M, D, generator=gen).bfloat16()
    t = (s.double() + 0.5 * torch.randn(G, M, D, generator=gen, dtype=torch.float64)).bfloat16()
    return s, t


def _tile_row_bytes(M):
    """panel_bytes at which a panel is exactly one row of tiles."""
    return TILE * ((M + TILE - 1) // TILE) * TILE * 2


def _kw(mode, apply_norm):
    return dict(apply_norm=apply_norm, remove_neg=MODES[mode][0],
                remove_only_teacher_neg=MODES[mode][1])


def _run(s, t, mode, apply_norm, panel_bytes=None, grad=True):
    """(loss, dS or None) of one call on the device, as CPU tensors."""
    from dinov3_amd.ops import gram_loss

    x = s.cuda().requires_grad_(grad)
    loss = gram_loss(x, t.cuda(), panel_bytes=panel_bytes, **_kw(mode, apply_norm))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    if not grad:
        return loss.cpu(), None
    loss.backward()
    assert x.grad.dtype == torch.bfloat16
    return loss.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def _oracle(shape, mode, apply_norm):
    """_oracle_of the inputs of a shape, shared by the tests that need it."""
    return _oracle_of(*_inputs(*shape), mode, apply_norm)


def _oracle_of(s16, t16, mode, apply_norm):
    """The fp64 oracle of a case and the bounds of test_loss_and_gradient_within_bounds'
    docstring: (loss, dS, loss bound, dS bound [G, M], boundary fraction)."""
    from dinov3_amd.ops import gram_loss_ref

    G, M, D = s16.shape
    S, T = s16.double(), t16.double()
    x = S.clone().requires_grad_(True)
    loss = gram_loss_ref(x, T, **_kw(mode, apply_norm))
    loss.backward()
    loss, dS = loss.detach(), x.grad
    N = G * M * M

    ones = torch.ones(G, M, dtype=torch.float64)
    rs = 1.0 / S.norm(dim=-1) if apply_norm else ones
    rt = 1.0 / T.norm(dim=-1) if apply_norm else ones
    outer = lambda r: r.unsqueeze(2) * r.unsqueeze(1)
    A = (S @ S.transpose(1, 2)) * outer(rs)
    B = (T @ T.transpose(1, 2)) * outer(rt)
    eps_a = (3 * D + 16) * U * (S.abs() @ S.abs().transpose(1, 2)) * outer(rs)
    eps_b = (3 * D + 16) * U * (T.abs() @ T.abs().transpose(1, 2)) * outer(rt)
    if apply_norm:  # the size the issue states: the abs-Gram of unit rows is at most 1
        assert float(eps_a.max()) <= (3 * D + 16) * U * (1 + 1e-12)
    boundary = (A.abs() <= eps_a) | (B.abs() <= eps_b)
    zero = torch.zeros_like(A)
    if mode == "plain":
        a, b, mask = A, B, torch.ones_like(A)
        boundary = torch.zeros_like(boundary)  # nothing jumps without a clamp
    elif mode == "remove_neg":
        a, b, mask = A.clamp(min=0), B.clamp(min=0), (A >= 0).double()
    else:
        both = (A < 0) & (B < 0)
        a, b, mask = torch.where(both, zero, A), B.clamp(min=0), (~both).double()
    e = a - b
    frac = float(boundary.double().mean())

    # ---- loss ----
    eta = eps_a + eps_b + U * e.abs()
    if mode == "teacher_neg":
        eta = eta + boundary * A.abs()
    n_part = G * ((M + TILE - 1) // TILE) ** 2
    adds = 64 + 6 + 3 + math.ceil(n_part / 256) + 6 + 6
    loss_bound = float((2 * e.abs() * eta + eta * eta).sum() / N + (adds + 3) * U * loss)

    # ---- gradient ----
    rho = (D / 2 + 2) * U if apply_norm else 0.0
    rj = rs.unsqueeze(1)  # r_j along the columns
    P = e * mask * rj
    dP1 = rj * (eta + e.abs() * (rho + 2 * U))
    dP = dP1 + BF16_P * (P.abs() + dP1) + boundary * e.abs() * rj
    absS = S.abs()
    draw = P @ S
    X = dP @ absS + 2 * M * U * ((P.abs() + dP) @ absS)
    d_draw = X + BF16 * (draw.abs() + X)
    c = 4.0 / N
    if apply_norm:
        ri = rs.unsqueeze(2)
        dot = (S * draw).sum(dim=2, keepdim=True)
        d_dot = (absS * d_draw).sum(dim=2, keepdim=True) + (D + 1) * U * (
            absS * (draw.abs() + d_draw)).sum(dim=2, keepdim=True)
        d_proj = ri ** 2 * (d_dot + dot.abs() * (2 * rho + 3 * U))
        size = draw.abs() + absS * ri ** 2 * dot.abs()
        d_inner = d_draw + absS * d_proj + 2 * U * size
        d_ds = c * ri * (d_inner + (rho + 4 * U) * size)
        formula = c * ri * (draw - S * ri ** 2 * dot)
    else:
        d_ds = c * (d_draw + 2 * U * draw.abs())
        formula = c * draw
    # the closed form of gram_loss.hip's header is the autograd gradient (1e-12 c: at
    # M = 1 with apply_norm e is 0 up to fp64 roundings and so are both gradients)
    assert float((formula - dS).abs().max()) <= 1e-11 * float(dS.abs().max()) + 1e-12 * c
    ds_bound = (d_ds + BF16 * (dS.abs() + d_ds)).amax(dim=2)
    return loss, dS, loss_bound, ds_bound, frac


@pytest.mark.parametrize("panel", ["default", "tile_row"])
@pytest.mark.parametrize("apply_norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_loss_and_gradient_within_bounds(shape, mode, apply_norm, panel):
    """Bounds from the kernels' own rounding steps, u = 2^-24; none is fitted to a run.
    Hats are computed values, plain letters the fp64 oracle on the same bf16 inputs.

    Similarities. Products of bf16 values are exact in fp32. The accumulation over D terms
    inside the MFMAs, in an undocumented order, is bounded as tests/test_fmha_exact_gpu.py
    bounds it: 2 D u times the dot product of the absolute values. r_i = rsqrt(sum of
    squares): D exact-order-free fp32 adds of positive terms and their roundings, D u
    relative, halved by the root, plus 1 ulp = 2u of v_rsq_f32: rho = (D/2 + 2) u. Two
    factors r_i r_j, two multiplications: |A^ - A| <= (2D + D + 4 + 2) u n_ij, and with
    the second-order terms eps_ij = (3D + 16) u n_ij, n = r_i r_j (|S| |S|^T)_ij, which
    is at most 1 for normalised rows: eps <= (3D + 16) u as the issue sizes it. Without
    apply_norm r = 1, rho = 0 and n is the absolute Gram itself.
    Boundary entries. |A| <= eps_A or |B| <= eps_B: the computed value may sit on the
    other side of the clamp. They are capped at 1 % of the entries, asserted here on the
    oracle. max(x, 0) is continuous; in the teacher-only mode a boundary entry's a may be
    A or 0, so its error allowance grows by |A|; in both clamp modes its P may be the
    unmasked value or 0, an allowance of |e| r_j.
    Loss. eta = eps_A + eps_B + u |e| bounds |e^ - e| (1-Lipschitz clamps, one
    subtraction); |e^2 - e^2| <= 2 |e| eta + eta^2. The squares are summed in a fixed
    order whose longest path has 64 adds in a lane, 6 + 3 in the block, ceil(tiles / 256)
    + 12 in the finish kernel; with the square, the fp64 division and the cast:
    (adds + 3) u loss.
    Gradient, per row i in the max norm over k. P^ = bf16(e^ r^_j):
    dP = r_j (eta + |e| (rho + 2u)), then 2^-9 (|P| + dP) for the rounding, plus the
    boundary allowance. 2^-9 per entry of P is the figure the issue sets and is kept as it
    states it; one rounding to bf16 can be off by 2^-8, which is what the two roundings
    whose size the issue leaves open are given here. Draw^ = bf16(P^ @ S) with fp32
    accumulation over M terms in the library's order:
    X = dP @ |S| + 2 M u (|P| + dP) @ |S|, dDraw = X + 2^-8 (|Draw| + X).
    dS_i = c r_i (Draw_i - S_i r_i^2 dot_i), dot_i = S_i . Draw_i: dot carries
    |S_i| . dDraw_i and (D + 1) u |S_i| . |Draw^_i|; r^2 dot carries 2 rho + 3u; the
    product and the subtraction 2u of their operands' sizes; c r_i carries rho + 2u (c is
    4 / (G M^2) rounded to fp32) and the last product u; then one rounding to bf16. Without
    apply_norm only dDraw, c and the store remain."""
    from dinov3_amd.ops import GRAM_DEFAULT_PANEL_BYTES

    s, t = _inputs(*shape)
    rloss, rds, loss_bound, ds_bound, frac = _oracle(shape, mode, apply_norm)
    assert frac <= 0.01, f"boundary entries: {frac:.4%}"
    pb = None if panel == "default" else _tile_row_bytes(shape[1])
    assert _tile_row_bytes(shape[1]) < GRAM_DEFAULT_PANEL_BYTES
    loss, ds = _run(s, t, mode, apply_norm, pb)
    loss_err = abs(float(loss.double() - rloss))
    row_err = (ds.double() - rds).abs().amax(dim=2)
    ratio = float((row_err / ds_bound.clamp(min=1e-300)).max())
    print(f"\n  {shape} {mode} norm={apply_norm} {panel}: loss {float(loss):.6e} err {loss_err:.3e} "
          f"bound {loss_bound:.3e}; grad worst err/bound {ratio:.3f}; boundary {frac:.4%}")
    assert loss_err <= loss_bound
    assert bool((row_err <= ds_bound).all())


PANEL_SHAPES = [(3, 129, 72), (1, 300, 384)]


@pytest.mark.parametrize("shape", PANEL_SHAPES, ids=str)
def test_panel_independence(shape):
    """A panel boundary never splits a reduction: the loss is bit-identical for
    every panel_bytes, and so is the gradient. The gradient goes through the
    library GEMM, one call per panel (a batched one when a panel holds whole
    matrices); of the two forms the issue allows, bit-equality is the one that
    holds: at these shapes the library sums over M in the same order for every
    panel height, so it is asserted. A panel_bytes below one tile row is one
    tile row."""
    s, t = _inputs(*shape)
    row = _tile_row_bytes(shape[1])
    base_loss, base_ds = _run(s, t, "remove_neg", True, None)
    for name, pb in (("one_tile_row", row), ("two_tile_rows", 2 * row), ("tiny", 1)):
        loss, ds = _run(s, t, "remove_neg", True, pb)
        assert torch.equal(loss, base_loss), name
        assert torch.equal(ds, base_ds), name


@pytest.mark.parametrize("mode", list(MODES))
def test_run_to_run_bit_equality(mode):
    s, t = _inputs(1, 300, 384)
    pb = 2 * _tile_row_bytes(300)
    first, second = _run(s, t, mode, True, pb), _run(s, t, mode, True, pb)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@pytest.mark.parametrize("shape", [(3, 129, 72), (1, 33, 8)], ids=str)
def test_pad_hygiene(shape):
    """The inputs are views into larger allocations whose other rows hold large
    values: what lies before the first and past the last row never counts."""
    from dinov3_amd.ops import gram_loss

    G, M, D = shape
    s, t = _inputs(*shape)
    want_loss, want_ds = _run(s, t, "teacher_neg", True, _tile_row_bytes(M))
    guard = 160
    views = []
    for x in (s, t):
        big = torch.full((G * M + 2 * guard, D), 32768.0, dtype=torch.bfloat16, device="cuda")
        big[guard:guard + G * M] = x.cuda().view(G * M, D)
        views.append((big, big[guard:guard + G * M].view(G, M, D)))
    x = views[0][1].detach().requires_grad_(True)
    loss = gram_loss(x, views[1][1], panel_bytes=_tile_row_bytes(M), **_kw("teacher_neg", True))
    loss.backward()
    assert torch.equal(loss.detach().cpu(), want_loss)
    assert torch.equal(x.grad.cpu(), want_ds)
    for big, _ in views:  # and nothing was written around them
        assert bool((big[:guard] == 32768.0).all()) and bool((big[guard + G * M:] == 32768.0).all())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(3, 129, 72), (1, 257, 200)], ids=str)
def test_forward_only(shape, mode):
    """Without a gradient to compute the loss has the same bits."""
    from dinov3_amd.ops import gram_loss

    s, t = _inputs(*shape)
    want, _ = _run(s, t, mode, True)
    no_req, _ = _run(s, t, mode, True, grad=False)
    x = s.cuda().requires_grad_(True)
    with torch.no_grad():
        under_no_grad = gram_loss(x, t.cuda(), **_kw(mode, True))
    assert not under_no_grad.requires_grad
    assert torch.equal(no_req, want) and torch.equal(under_no_grad.cpu(), want)


def test_workspace_is_one_panel():
    """(1, 4096, 64) with a 1 MiB panel: inputs aside, the gradient, Draw and one
    panel are 2 MiB; one fp32 similarity matrix alone would be 64 MiB."""
    from dinov3_amd.ops import gram_loss

    gen = torch.Generator().manual_seed(1000 + 4096 + 64)
    s = torch.randn(1, 4096, 64, generator=gen).bfloat16().cuda()
    t = (s.float() + 0.5 * torch.randn(1, 4096, 64, generator=gen).cuda()).bfloat16()
    kw = _kw("remove_neg", True)

    def step():
        x = s.detach().requires_grad_(True)
        loss = gram_loss(x, t, panel_bytes=1 << 20, **kw)
        loss.backward()
        return loss.detach(), x.grad

    want = step()  # the library's own handles and workspaces exist after this call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = step()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    print(f"\n  workspace delta {delta / 2 ** 20:.2f} MiB")
    assert delta <= 8 << 20
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_argument_checks():
    from dinov3_amd.ops import gram_loss, hip_ops

    ops = hip_ops()
    s = torch.randn(2, 40, 16, device="cuda").bfloat16()
    kw = _kw("remove_neg", True)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.gram_rnorm(s, s[:, :39].contiguous(), True)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.gram_rnorm(s[..., :12].contiguous(), s[..., :12].contiguous(), True)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.gram_rnorm(s.float(), s.float(), True)
    r = ops.gram_rnorm(s, s, True)
    partials = torch.empty(2, device="cuda")
    with pytest.raises(RuntimeError, match="bf16"):
        ops.gram_tiles(s.float(), s.float(), r, 1, 0, 2, None, partials)
    with pytest.raises(RuntimeError, match="row tiles"):
        ops.gram_tiles(s, s, r, 1, 1, 2, None, partials)
    with pytest.raises(RuntimeError, match="panel"):
        ops.gram_tiles(s, s, r, 1, 0, 2, torch.empty(128, 128, device="cuda").bfloat16(), partials)
    with pytest.raises(RuntimeError, match="partials"):
        ops.gram_tiles(s, s, r, 1, 0, 2, None, torch.empty(3, device="cuda"))
    with pytest.raises(ValueError, match="one shape"):
        gram_loss(s, s[:, :39], **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        gram_loss(s[..., :12].contiguous(), s[..., :12].contiguous(), **kw)


@pytest.mark.parametrize("img_level", [True, False])
def test_module_switch(img_level, monkeypatch):
    """GramLoss on device bf16 inputs with the switch set and unset: both within the
    loss bound of the fp64 value, so at most twice the bound apart. The eager path
    computes in fp32 from the same bf16 inputs; its own error is not derived here, the
    assertion is the issue's. fp32 inputs on the device ignore the switch."""
    from dinov3_amd.loss.gram_loss import GramLoss

    shape = (3, 129, 72)
    s, t = _inputs(*shape)
    module = GramLoss(apply_norm=True, remove_neg=True, remove_only_teacher_neg=False)
    if img_level:
        rloss, _, bound, _, frac = _oracle(shape, "remove_neg", True)
    else:
        flat = (1, 3 * 129, 72)
        rloss, _, bound, _, frac = _oracle_of(s.view(flat), t.view(flat), "remove_neg", True)
    assert frac <= 0.01
    out = {}
    for value in ("0", "1"):
        monkeypatch.setenv("DINOV3_FUSED_GRAM", value)
        out[value] = float(module(s.cuda(), t.cuda(), img_level=img_level).double())
        f32 = module(s.cuda().float(), t.cuda().float(), img_level=img_level)
        out["f32_" + value] = f32.cpu()
    print(f"\n  img_level={img_level}: eager {out['0']:.8e} fused {out['1']:.8e} fp64 {float(rloss):.8e} "
          f"bound {bound:.3e}")
    assert abs(out["1"] - float(rloss)) <= bound
    assert abs(out["0"] - float(rloss)) <= bound
    assert abs(out["0"] - out["1"]) <= 2 * bound
    assert torch.equal(out["f32_0"], out["f32_1"])


@pytest.mark.parametrize("variant", ["img_level", "masked"])
def test_smoke_step_with_fused_gram(variant, smoke_cfg, monkeypatch):
    """One training step of the smoke model with the Gram loss on the fused path."""
    import dinov3_amd.ops as ops_pkg
    from bench import make_synthetic_batch
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch

    cfg = copy.deepcopy(smoke_cfg)
    cfg.gram.use_loss = True
    cfg.gram.ckpt = "ignore"
    cfg.gram.remove_neg = True
    cfg.gram.img_level = variant == "img_level"
    if variant == "masked":
        cfg.gram.tokens_used = "masked"
    cfg.compute_precision.param_dtype = "bf16"
    monkeypatch.setenv("DINOV3_FUSED_GRAM", "1")
    calls = []
    fused = ops_pkg.gram_loss

    def counting(student, teacher, **kw):
        calls.append(tuple(student.shape))
        return fused(student, teacher, **kw)

    monkeypatch.setattr(ops_pkg, "gram_loss", counting)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    model = SSLMetaArch(cfg).to(device=dev, dtype=torch.bfloat16)
    model.train()
    batch = make_synthetic_batch(cfg, dev, torch.bfloat16, n_batches=1)[0]
    loss, metrics = model(batch, teacher_temp=0.07, iteration=0)
    loss.backward()
    torch.cuda.synchronize()
    assert len(calls) == 1 and (calls[0][0] > 1) == (variant == "img_level"), calls
    assert torch.isfinite(loss.detach()) and bool(torch.isfinite(torch.as_tensor(metrics["gram_loss"])))
    grads = [p.grad for p in model.student_backbone.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)

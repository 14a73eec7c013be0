"""Prototype-loss kernels (csrc/proto_ce.hip) against the fp64 oracle, elementwise.

Factored and materialized Sinkhorn-Knopp, and the DINO / iBOT cross-entropy
with dense and factored teachers, called through the public functions of
ops/proto_scores.py and the loss modules, with an upstream gradient of 0.37.
Every result is held to the bounds of dinov3_amd/ops/proto_oracle.py;
tests/test_proto_oracle.py shows on the CPU that a correct implementation
stays inside them and that a lost column, row, iteration, teacher term, weight
or gradient factor does not. The atomics make results differ from run to run:
the tests assert bounds, not bits. Run with -s to see the worst err/bound of
every case.
"""

import pytest
import torch

from dinov3_amd.ops import proto_oracle as po

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

SK_CASES = [(M, K, T, kind) for M, K in po.SINKHORN_SHAPES for T in po.SINKHORN_TEMPS
            for kind in po.kinds_for(K)]
MAT_CASES = [(M, K, T, kind) for M, K in po.MATERIALIZED_SHAPES for T in po.SINKHORN_TEMPS
             for kind in po.kinds_for(K)]
DINO_CASES = [(*shape, kind) for shape in po.DINO_SHAPES for kind in po.kinds_for(shape[-1])]
IBOT_CASES = ([(M, K, kind, True) for M, K in po.IBOT_SHAPES for kind in po.kinds_for(K)]
              + [(57, 264, "planted", False)])      # the masks_weight=None default


def _poison(*specs):
    """Fill and free NaN blocks of the sizes the next call allocates with
    torch.empty: an element a kernel never writes then cannot look plausible."""
    blocks = [torch.full(shape, float("nan"), dtype=dtype, device=DEV) for shape, dtype in specs]
    del blocks


def _check(label, pairs):
    """pairs: name -> (got, ref, absolute bound). Prints the worst err/bound of
    each before asserting that every element is inside its bound."""
    ratios = {}
    for name, (got, ref, bound) in pairs.items():
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
        ratios[name] = po.worst_ratio((got - ref).abs(), bound)
    print(f"\n  err/bound {label}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (label, ratios)
    return ratios


def _ce_pairs(ref, loss, dx, lse=None, st=None, scale=1.0):
    pairs = {"loss": (loss.reshape(()) * scale, ref.loss, ref.b_loss), "dx": (dx, ref.dx, ref.b_dx)}
    if lse is not None:
        pairs["lse"] = (lse, ref.lse, ref.b_lse)
        pairs["st"] = (st, ref.st, ref.b_st)
    return pairs


# ---------------------------------------------------------------------------
# Sinkhorn-Knopp
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,temp,kind", SK_CASES)
def test_sinkhorn_factored_within_bounds(M, K, temp, kind):
    from dinov3_amd.ops.proto_scores import sinkhorn_knopp_factored

    case = po.sinkhorn_case(M, K, temp, kind)
    x = case.x.to(DEV)
    _poison(((K,), torch.float32), ((M,), torch.float32))
    fact = sinkhorn_knopp_factored(x, temp)
    assert fact.u.shape == (M,) and fact.v.shape == (K,)
    _check(f"sinkhorn factored {M}x{K} T{temp} {kind}",
           {"u": (fact.u, case.u, case.rel_u * case.u), "v": (fact.v, case.v, case.rel_v * case.v),
            "Q": (fact.materialize(), case.q, po.q_abs_bound(case.q, case.rel_q))})


@pytest.mark.parametrize("with_total", [False, True], ids=["default", "total_columns"])
@pytest.mark.parametrize("M,K,temp,kind", MAT_CASES)
def test_sinkhorn_materialized_within_bounds(M, K, temp, kind, with_total):
    """The materialized HIP path, the loss modules' fallback for logits the
    factored kernels do not take; total_columns cancels in the last
    row-normalise, so the oracle's Q is the same with it."""
    from dinov3_amd.ops.proto_scores import sinkhorn_knopp

    case = po.sinkhorn_case(M, K, temp, kind)
    total = torch.tensor([float(M + 11)], device=DEV) if with_total else None
    _poison(((M, K), torch.float32), ((K,), torch.float32))
    q = sinkhorn_knopp(case.x.to(DEV), temp, total_columns=total)
    _check(f"sinkhorn materialized {M}x{K} T{temp} {kind}",
           {"Q": (q, case.q, po.q_abs_bound(case.q, po.materialized_bounds(case.x, temp)))})


# ---------------------------------------------------------------------------
# cross-entropy, through the public functions and their autograd
# ---------------------------------------------------------------------------

def _upstream(scale=1.0):
    return torch.tensor(po.UPSTREAM * scale, device=DEV)


@pytest.mark.parametrize("factored", [False, True], ids=["dense", "fact"])
@pytest.mark.parametrize("S,T,B,ignore_diag,K,kind", DINO_CASES)
def test_dino_ce_within_bounds(S, T, B, ignore_diag, K, kind, factored):
    from dinov3_amd.ops import hip_ops
    from dinov3_amd.ops.proto_scores import FactoredProbs, dino_softmax_ce

    case = po.dino_case(S, T, B, ignore_diag, K, kind)
    ref = case.fact if factored else case.dense
    x = case.x.to(DEV).requires_grad_(True)
    xt, u, v, t = case.xt.to(DEV), case.u32.to(DEV), case.v32.to(DEV), case.t32.to(DEV)
    teacher = FactoredProbs(xt, u.view(T, B), v, po.TEACHER_TEMP) if factored else t
    _poison(((S, B, K), torch.bfloat16), ((S * B,), torch.float32), ((S * B,), torch.float32))
    loss = dino_softmax_ce(x, teacher, po.STUDENT_TEMP, ignore_diag)
    loss.backward(_upstream())
    # the per-row lse and st the backward reads, from the forward op itself
    _poison(((S * B,), torch.float32), ((S * B,), torch.float32))
    if factored:
        _, lse, st = hip_ops().dino_ce_fact_fwd(x.detach(), xt, u, v, po.STUDENT_TEMP, po.TEACHER_TEMP,
                                                ignore_diag)
    else:
        _, lse, st = hip_ops().dino_ce_fwd(x.detach(), t, po.STUDENT_TEMP, ignore_diag)
    _check(f"dino {'fact' if factored else 'dense'} S{S} T{T} B{B} diag{int(ignore_diag)} K{K} {kind}",
           _ce_pairs(ref, loss, x.grad, lse, st))


@pytest.mark.parametrize("factored", [False, True], ids=["dense", "fact"])
@pytest.mark.parametrize("M,K,kind,weighted", IBOT_CASES)
def test_ibot_ce_within_bounds(M, K, kind, weighted, factored):
    from dinov3_amd.ops import hip_ops
    from dinov3_amd.ops.proto_scores import FactoredProbs, ibot_softmax_ce

    case = po.ibot_case(M, K, kind, weighted)
    ref = case.fact if factored else case.dense
    x = case.x.to(DEV).requires_grad_(True)
    xt, u, v, t, w = (c.to(DEV) for c in (case.xt, case.u32, case.v32, case.t32, case.w))
    teacher = FactoredProbs(xt, u, v, po.TEACHER_TEMP) if factored else t
    _poison(((M, K), torch.bfloat16), ((M,), torch.float32), ((M,), torch.float32))
    loss = ibot_softmax_ce(x, teacher, n_total_rows=M + 3, student_temp=po.STUDENT_TEMP,
                           masks_weight=w if weighted else None)
    loss.backward(_upstream())
    _poison(((M,), torch.float32), ((M,), torch.float32))
    if factored:
        _, lse, st = hip_ops().ibot_ce_fact_fwd(x.detach(), xt, u, v, w, po.STUDENT_TEMP, po.TEACHER_TEMP)
    else:
        _, lse, st = hip_ops().ibot_ce_fwd(x.detach(), t, w, po.STUDENT_TEMP)
    _check(f"ibot {'fact' if factored else 'dense'} {M}x{K} {kind} w{int(weighted)}",
           _ce_pairs(ref, loss, x.grad, lse, st))


# ---------------------------------------------------------------------------
# the training path end to end: loss-module Sinkhorn into loss-module CE
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("S,T,B,ignore_diag,K,kind",
                         [(4, 2, 3, False, 2056, "planted"), (4, 2, 3, True, 2056, "flat"),
                          (2, 2, 3, True, 264, "planted"), (2, 2, 1, False, 65536, "planted")])
def test_dino_loss_chain_within_bounds(S, T, B, ignore_diag, K, kind):
    from dinov3_amd.loss.dino_clstoken_loss import DINOLoss
    from dinov3_amd.ops.proto_scores import FactoredProbs

    case = po.dino_case(S, T, B, ignore_diag, K, kind)
    mod = DINOLoss(K, student_temp=po.STUDENT_TEMP).to(DEV)
    x = case.x.to(DEV).requires_grad_(True)
    _poison(((K,), torch.float32), ((T * B,), torch.float32))
    probs = mod.sinkhorn_knopp_teacher(case.xt.to(DEV).view(T * B, K), po.TEACHER_TEMP)
    assert isinstance(probs, FactoredProbs)
    _poison(((S, B, K), torch.bfloat16), ((S * B,), torch.float32), ((S * B,), torch.float32))
    loss = mod(x, probs.reshape(T, B, -1), ignore_diagonal=ignore_diag)
    loss.backward(_upstream())
    _check(f"DINOLoss chain S{S} T{T} B{B} diag{int(ignore_diag)} K{K} {kind}",
           _ce_pairs(case.chain, loss, x.grad))


@pytest.mark.parametrize("M,K,kind", [(57, 2056, "planted"), (57, 2056, "flat"), (3, 98304, "planted")])
def test_ibot_loss_chain_within_bounds(M, K, kind):
    from dinov3_amd.loss.ibot_patch_loss import iBOTPatchLoss
    from dinov3_amd.ops.proto_scores import FactoredProbs

    case = po.ibot_case(M, K, kind, True)
    mod = iBOTPatchLoss(K, student_temp=po.STUDENT_TEMP).to(DEV)
    x = case.x.to(DEV).requires_grad_(True)
    masks = torch.ones(4, M, dtype=torch.bool, device=DEV)   # forward_masked divides by its 4 rows: exact
    _poison(((K,), torch.float32), ((M,), torch.float32))
    probs = mod.sinkhorn_knopp_teacher(case.xt.to(DEV), po.TEACHER_TEMP,
                                       n_masked_patches_tensor=torch.tensor([M], device=DEV))
    assert isinstance(probs, FactoredProbs)
    _poison(((M, K), torch.bfloat16), ((M,), torch.float32), ((M,), torch.float32))
    loss = mod.forward_masked(x, probs, masks, n_masked_patches=M, masks_weight=case.w.to(DEV))
    loss.backward(_upstream(4.0))
    _check(f"iBOTPatchLoss chain {M}x{K} {kind}", _ce_pairs(case.chain, loss, x.grad, scale=4.0))


# ---------------------------------------------------------------------------
# inputs the factored kernels do not take
# ---------------------------------------------------------------------------

def _misaligned(x):
    """The same values in contiguous storage that starts 2 bytes off a 16-byte boundary."""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=DEV)
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("how", ["K2052", "misaligned"])
@pytest.mark.parametrize("kind", ["planted", "flat"])
def test_unvectorisable_logits_raise_in_binding_and_fall_back_in_modules(how, kind):
    """K % 8 != 0 or storage off a 16-byte boundary: the factored column sum
    loads eight columns at a time, so its binding refuses; the loss modules
    route such logits through the materialized kernels and still return the
    oracle's Q."""
    from dinov3_amd.loss.dino_clstoken_loss import DINOLoss
    from dinov3_amd.loss.ibot_patch_loss import iBOTPatchLoss
    from dinov3_amd.ops import hip_ops

    M, K = (37, 2052) if how == "K2052" else (37, 2056)
    case = po.sinkhorn_case(M, K, po.TEACHER_TEMP, kind)
    x = case.x.to(DEV) if how == "K2052" else _misaligned(case.x.to(DEV))
    with pytest.raises(RuntimeError):
        hip_ops().sinkhorn_fact_colsum(x, torch.empty(0, device=DEV), po.TEACHER_TEMP)
    bound = po.q_abs_bound(case.q, po.materialized_bounds(case.x, po.TEACHER_TEMP))
    q_dino = DINOLoss(K).to(DEV).sinkhorn_knopp_teacher(x, po.TEACHER_TEMP)
    q_ibot = iBOTPatchLoss(K).to(DEV).sinkhorn_knopp_teacher(
        x, po.TEACHER_TEMP, n_masked_patches_tensor=torch.tensor([M], device=DEV))
    assert torch.is_tensor(q_dino) and torch.is_tensor(q_ibot)
    _check(f"module fallback {how} {kind}", {"Q dino": (q_dino, case.q, bound), "Q ibot": (q_ibot, case.q, bound)})


def test_zero_rows():
    """A rank without masked patches: no division by zero on the host, no
    launch with an empty grid; A is zero so the all-reduce of the other ranks
    still has a partner, and the iBOT loss is 0 with a zero gradient."""
    from dinov3_amd.loss.ibot_patch_loss import iBOTPatchLoss
    from dinov3_amd.ops import hip_ops
    from dinov3_amd.ops.proto_scores import sinkhorn_knopp_factored

    K = 264
    empty = torch.empty(0, K, dtype=torch.bfloat16, device=DEV)
    _poison(((K,), torch.float32))
    A = hip_ops().sinkhorn_fact_colsum(empty, torch.empty(0, device=DEV), po.TEACHER_TEMP)
    assert A.shape == (K,) and not A.any()
    assert hip_ops().sinkhorn_fact_rowsum(empty, torch.ones(K, device=DEV), po.TEACHER_TEMP).shape == (0,)
    fact = sinkhorn_knopp_factored(empty, po.TEACHER_TEMP)
    assert fact.u.shape == (0,) and fact.v.shape == (K,)

    mod = iBOTPatchLoss(K, student_temp=po.STUDENT_TEMP).to(DEV)
    probs = mod.sinkhorn_knopp_teacher(empty, po.TEACHER_TEMP,
                                       n_masked_patches_tensor=torch.tensor([0], device=DEV))
    x = po.flat(5, K, seed=3).to(DEV).requires_grad_(True)     # the padded student buffer
    masks = torch.zeros(4, 5, dtype=torch.bool, device=DEV)
    loss = mod.forward_masked(x, probs, masks, n_masked_patches=0,
                              masks_weight=torch.empty(0, device=DEV))
    loss.backward(_upstream())
    torch.cuda.synchronize()
    assert float(loss.detach()) == 0.0
    assert x.grad.shape == x.shape and not x.grad.float().any()

"""The fused similarity + top-k kernel (ops.knn_topk) against the plain-torch
oracle knn_topk_ref: exact on integer data with ties, bounded on random unit
rows, bit-stable across runs and split counts."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (Q, N, D, k): odd query counts around the 32-query tile, bank sizes that are
# no multiple of the 128-row tile nor of 3 or 7, D below / above / not a
# multiple of the 64-column stage, both list capacities, k == N and N == k + 1.
SHAPES = [
    (1, 257, 32, 1),
    (65, 129, 64, 20),
    (70, 1000, 384, 200),
    (5, 256, 64, 256),
    (33, 257, 1152, 256),
    (130, 777, 128, 10),
]
SPLITS = (0, 1, 3, 7)


def _ids(shape):
    return "Q{}-N{}-D{}-k{}".format(*shape)


@functools.lru_cache(maxsize=None)
def _integer_case(shape):
    """Integers in {-2..2} as bf16: every dot product is an exact integer below
    2^24 in any summation order, and ties are everywhere."""
    from dinov3_amd.ops import knn_topk_ref

    Q, N, D, k = shape
    g = torch.Generator().manual_seed(1000 + Q + N)
    q = torch.randint(-2, 3, (Q, D), generator=g).to(torch.bfloat16)
    bank = torch.randint(-2, 3, (N, D), generator=g).to(torch.bfloat16)
    val, idx = knn_topk_ref(q, bank, k)
    return q, bank, val, idx


@functools.lru_cache(maxsize=None)
def _unit_case(shape):
    Q, N, D, k = shape
    g = torch.Generator().manual_seed(2000 + Q + N)
    q = torch.nn.functional.normalize(torch.randn(Q, D, generator=g), dim=1).to(torch.bfloat16)
    bank = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(torch.bfloat16)
    S = q.double() @ bank.double().T
    return q, bank, S


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_knn_topk_exact_on_integers(shape):
    from dinov3_amd.ops import knn_topk

    k = shape[3]
    q, bank, ref_val, ref_idx = _integer_case(shape)
    qd, bd = q.cuda(), bank.cuda()
    outs = []
    for splits in SPLITS:
        val, idx = knn_topk(qd, bd, k, splits=splits)
        assert val.dtype == torch.float32 and idx.dtype == torch.int64
        assert val.shape == (shape[0], k) and idx.shape == (shape[0], k)
        val, idx = val.cpu(), idx.cpu()
        assert torch.equal(idx, ref_idx), f"splits={splits}: idx differs from the oracle"
        assert torch.equal(val, ref_val), f"splits={splits}: val differs from the oracle"
        outs.append((val, idx))
    for val, idx in outs[1:]:
        assert torch.equal(val.view(torch.int32), outs[0][0].view(torch.int32))
        assert torch.equal(idx, outs[0][1])
    # run to run
    val2, idx2 = knn_topk(qd, bd, k, splits=SPLITS[-1])
    assert torch.equal(val2.cpu().view(torch.int32), outs[-1][0].view(torch.int32))
    assert torch.equal(idx2.cpu(), outs[-1][1])


def test_knn_topk_duplicate_rows_lower_index_first():
    from dinov3_amd.ops import knn_topk, knn_topk_ref

    g = torch.Generator().manual_seed(7)
    bank = torch.randint(-2, 3, (300, 64), generator=g).to(torch.bfloat16)
    bank[150] = bank[7]
    bank[299] = bank[7]
    q = bank[7:8].clone()
    ref_val, ref_idx = knn_topk_ref(q, bank, 20)
    assert ref_idx[0, :3].tolist() == [7, 150, 299]  # |b|^2 is 8 sigma above the other rows
    for splits in (1, 3):  # 3 slices of 100 rows: one copy in each
        val, idx = knn_topk(q.cuda(), bank.cuda(), 20, splits=splits)
        assert idx[0, :3].tolist() == [7, 150, 299]
        assert torch.equal(idx.cpu(), ref_idx) and torch.equal(val.cpu(), ref_val)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_knn_topk_random_unit_rows(shape):
    """tol is the fp32 dot-product bound gamma_D * sum|a_i b_i| with
    Cauchy-Schwarz; the factor 2 covers 1 / (1 - D 2^-24) and the output
    rounding. Nothing in it is measured on the kernel."""
    from dinov3_amd.ops import knn_topk

    Q, N, D, k = shape
    q, bank, S = _unit_case(shape)
    tol = 2 * D * 2.0 ** -24 * float(q.double().norm(dim=1).max()) * float(
        bank.double().norm(dim=1).max())
    val, idx = knn_topk(q.cuda(), bank.cuda(), k)
    val, idx = val.cpu().double(), idx.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    assert all(len(set(row)) == k for row in idx.tolist()), "repeated neighbour"
    assert float((val - S.gather(1, idx)).abs().max()) <= tol
    top = S.sort(dim=1, descending=True).values[:, :k]
    assert float((val - top).abs().max()) <= tol
    assert bool((val[:, 1:] <= val[:, :-1]).all())


def test_knn_topk_argument_checks():
    from dinov3_amd.ops import knn_topk

    q = torch.zeros(4, 64, dtype=torch.bfloat16, device="cuda")
    bank = torch.zeros(300, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        knn_topk(q.float(), bank.float(), 5)
    with pytest.raises(RuntimeError):
        knn_topk(q, bank.half(), 5)
    with pytest.raises(RuntimeError):
        knn_topk(q[:, :48].contiguous(), bank[:, :48].contiguous(), 5)  # D % 32 != 0
    with pytest.raises(RuntimeError):
        knn_topk(q, bank[:10], 11)  # k > N
    with pytest.raises(RuntimeError):
        knn_topk(q, bank, 257)
    with pytest.raises(RuntimeError):
        knn_topk(q, bank, 0)
    with pytest.raises(RuntimeError):
        knn_topk(q, bank[::2], 5)  # not contiguous
    with pytest.raises(RuntimeError):
        knn_topk(q[:, ::2], bank[:, :32].contiguous(), 5)
    with pytest.raises(RuntimeError):
        knn_topk(q, bank[:, :32].contiguous(), 5)  # D mismatch


def test_knn_topk_no_queries():
    from dinov3_amd.ops import knn_topk

    q = torch.zeros(0, 64, dtype=torch.bfloat16, device="cuda")
    bank = torch.zeros(300, 64, dtype=torch.bfloat16, device="cuda")
    val, idx = knn_topk(q, bank, 5)
    assert val.shape == (0, 5) and idx.shape == (0, 5)
    assert val.dtype == torch.float32 and idx.dtype == torch.int64

"""CPU checks of the prototype-loss oracle (dinov3_amd/ops/proto_oracle.py).

A torch emulator of the kernels in csrc/proto_ce.hip — the same passes in
fp32, per-thread strided partial sums of 256 lanes, the shuffle tree, the row
tiles and column chunks with their atomics, the final bf16 store — must stay
inside every bound at every shape tests/test_proto_exact_gpu.py uses, and the
same emulator with one planted error must leave at least one bound by 4x,
with the intrinsic constant at its first value and at its ceiling. That is
what makes the GPU bounds mean something.
"""

import pytest
import torch
import torch.nn.functional as F

from dinov3_amd.ops import proto_oracle as po

ULP32 = torch.float32


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ---------------------------------------------------------------------------
# emulator of the kernels' arithmetic (test helper)
# ---------------------------------------------------------------------------

def emu_block_sum(terms):
    """block_reduce_sum of a 256-thread strided walk over the last axis."""
    lead, n = terms.shape[:-1], terms.shape[-1]
    if n == 0:
        return torch.zeros(lead)
    t = F.pad(terms, (0, (-n) % 256)).reshape(*lead, -1, 256)
    acc = torch.zeros(*lead, 256)
    for j in range(t.shape[-2]):                 # thread i: columns i, i + 256, ...
        acc = acc + t[..., j, :]
    acc = acc.reshape(*lead, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):             # wave_reduce_sum, lane 0
        acc = acc[..., :off] + acc[..., off:2 * off]
    w = acc[..., 0]                              # four wave sums in lanes 0..3
    return (w[..., 0] + w[..., 2]) + (w[..., 1] + w[..., 3])


def emu_sinkhorn(x, temp, n_iterations=3, drop_last_col=False, drop_col=None, drop_row=None,
                 ignore_u=False):
    """sinkhorn_knopp_factored in fp32: (u, v)."""
    E = torch.exp(x.float() * _f32(po.inv_temp32(temp)))
    M, K = E.shape
    _, m_tile, mt = po.colsum_tiling(M, K)
    split = po.rowsum_split(M)
    kchunk = -(-K // split)
    u = v = None
    for it in range(n_iterations):
        terms = E if (u is None or ignore_u) else u[:, None] * E
        if drop_row is not None:
            terms = terms.clone()
            terms[drop_row] = 0
        tiles = F.pad(terms, (0, 0, 0, mt * m_tile - M)).reshape(mt, m_tile, K)
        acc = torch.zeros(mt, K)
        for j in range(m_tile):
            acc = acc + tiles[:, j]
        A = acc[0]
        for t in range(1, mt):                   # one atomicAdd per tile
            A = A + acc[t]
        v = torch.reciprocal(A * K)
        terms = E * v
        if drop_last_col:
            terms[:, K - 1] = 0
        if drop_col is not None and drop_col < K:
            terms[:, drop_col] = 0
        sums = emu_block_sum(terms[:, :kchunk])
        for c in range(1, split):                # one atomicAdd per chunk
            sums = sums + emu_block_sum(terms[:, c * kchunk:(c + 1) * kchunk])
        u = 1.0 / sums
    return u, v


def _emu_ce_core(x, ts_fwd, ts_bwd, w, temp, g, denom, drop_last_col=False, drop_col=None):
    """x [R, K] bf16, ts [R, K] fp32 summed teacher rows, w [R] fp32, g the
    fp32 upstream gradient / denom. Returns loss, lse, st, dx (bf16)."""
    it = _f32(po.inv_temp32(temp))
    xi = x.float() * it
    R, K = xi.shape
    m = xi.amax(-1, keepdim=True)
    ex, tsx, tss = torch.exp(xi - m), ts_fwd * xi, ts_fwd.clone()
    for col in ([K - 1] if drop_last_col else []) + ([drop_col] if drop_col is not None and drop_col < K else []):
        ex[:, col] = 0
        tsx[:, col] = 0
        tss[:, col] = 0
    sumexp, dot, st = emu_block_sum(ex), emu_block_sum(tsx), emu_block_sum(tss)
    lse = m[:, 0] + torch.log(sumexp)
    rows = w * (st * lse - dot)
    loss_sum = _f32(0.0)
    for r in range(R):                           # one atomicAdd per row
        loss_sum = loss_sum + rows[r]
    scale = (g * it) * w
    sm = torch.exp(xi - lse[:, None])
    dx = (scale[:, None] * (st[:, None] * sm - ts_bwd)).to(torch.bfloat16)
    return loss_sum / _f32(denom), lse, st, dx


def _emu_teacher(case, S, B, factored, ignore_diag, crop0_twice=False, u_from_b=False, v_shift=False):
    """ts [S * B, K] fp32 as dino_ce(_fact)_{fwd,bwd}_kernel sums it; an iBOT
    case is S = 1 student crop with B = M rows and one teacher crop."""
    K = case.x.shape[-1]
    xt = case.xt.reshape(-1, B, K)
    T = xt.shape[0]
    itt = _f32(po.inv_temp32(po.TEACHER_TEMP))
    v = torch.roll(case.v32, 1) if v_shift else case.v32
    ts = torch.zeros(S, B, K)
    for s in range(S):
        for tt in range(T):
            if ignore_diag and tt == s:
                continue
            src = 0 if crop0_twice else tt
            if factored:
                u = case.u32[0 * B:B] if u_from_b else case.u32[src * B:(src + 1) * B]
                ts[s] = ts[s] + torch.exp(xt[src].float() * itt) * u[:, None] * v
            else:
                ts[s] = ts[s] + case.t32.reshape(T, B, K)[src]
    return ts.reshape(S * B, K)


def emu_dino(case, ignore_diag, factored, kernel_diag=None, no_teacher_dx=False, ignore_g=False,
             drop_last_col=False, drop_col=None, **teacher_plants):
    S, B, K = case.x.shape
    T = case.xt.shape[0]
    ts = _emu_teacher(case, S, B, factored, ignore_diag if kernel_diag is None else kernel_diag,
                      **teacher_plants)
    denom = po.dino_denominator(S, T, B, ignore_diag)
    g = _f32(1.0) if ignore_g else _f32(po.UPSTREAM) / _f32(denom)
    loss, lse, st, dx = _emu_ce_core(case.x.reshape(S * B, K), ts, torch.zeros_like(ts) if no_teacher_dx else ts,
                                     torch.ones(S * B), po.STUDENT_TEMP, g, denom,
                                     drop_last_col, drop_col)
    return loss, lse, st, dx.view(S, B, K)


def emu_ibot(case, factored, shift_w=False, no_teacher_dx=False, ignore_g=False, drop_last_col=False,
             drop_col=None, **teacher_plants):
    M, K = case.x.shape
    ts = _emu_teacher(case, 1, M, factored, False, **teacher_plants)
    w = torch.roll(case.w, 1) if shift_w else case.w
    g = _f32(1.0) if ignore_g else _f32(po.UPSTREAM)
    return _emu_ce_core(case.x, ts, torch.zeros_like(ts) if no_teacher_dx else ts, w,
                        po.STUDENT_TEMP, g, 1.0, drop_last_col, drop_col)


# ---------------------------------------------------------------------------
# ratios
# ---------------------------------------------------------------------------

def _rel_ratio(got, ref, rel):
    return po.worst_ratio((got.double() - ref).abs(), rel * ref.abs())


def sinkhorn_ratios(case, u, v):
    q = torch.exp(case.x.float() / case.temp) * u[:, None] * v      # FactoredProbs.materialize
    return {"u": _rel_ratio(u, case.u, case.rel_u), "v": _rel_ratio(v, case.v, case.rel_v),
            "Q": po.worst_ratio((q.double() - case.q).abs(), po.q_abs_bound(case.q, case.rel_q))}


def ce_ratios(ref, loss, lse, st, dx):
    return {"loss": po.worst_ratio((loss.double() - ref.loss).abs().reshape(1), ref.b_loss.reshape(1)),
            "lse": po.worst_ratio((lse.double() - ref.lse).abs(), ref.b_lse),
            "st": po.worst_ratio((st.double() - ref.st).abs(), ref.b_st),
            "dx": po.worst_ratio((dx.double() - ref.dx).abs(), ref.b_dx)}


def _fmt(r):
    return " ".join(f"{k}={v:.3g}" for k, v in r.items())


SK_CASES = [(M, K, T, kind) for M, K in po.SINKHORN_SHAPES for T in po.SINKHORN_TEMPS
            for kind in po.kinds_for(K)]
DINO_CASES = [(*shape, kind) for shape in po.DINO_SHAPES for kind in po.kinds_for(shape[-1])]
IBOT_CASES = [(M, K, kind, True) for M, K in po.IBOT_SHAPES for kind in po.kinds_for(K)] + [(57, 264, "planted", False)]


# ---------------------------------------------------------------------------
# the emulator is inside every bound; the documented input domain
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,temp,kind", SK_CASES)
def test_sinkhorn_emulator_within_bounds(M, K, temp, kind):
    case = po.sinkhorn_case(M, K, temp, kind)
    assert float(case.x.double().abs().max()) / temp <= 60.0
    assert po.fp32_domain_ok(case.x, temp)
    r = sinkhorn_ratios(case, *emu_sinkhorn(case.x, temp))
    print(f"\n  emulator err/bound sinkhorn {M}x{K} T{temp} {kind}: {_fmt(r)}")
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("S,T,B,ignore_diag,K,kind", DINO_CASES)
@pytest.mark.parametrize("factored", [False, True], ids=["dense", "fact"])
def test_dino_emulator_within_bounds(S, T, B, ignore_diag, K, kind, factored):
    case = po.dino_case(S, T, B, ignore_diag, K, kind)
    assert po.fp32_domain_ok(case.xt.view(T * B, K), po.TEACHER_TEMP)
    out = emu_dino(case, ignore_diag, factored)
    assert all(bool(torch.isfinite(o.float()).all()) for o in out)
    r = ce_ratios(case.fact if factored else case.dense, *out)
    print(f"\n  emulator err/bound dino S{S} T{T} B{B} diag{int(ignore_diag)} K{K} {kind}: {_fmt(r)}")
    assert all(v <= 1.0 for v in r.values()), r
    # the chain bounds only widen the factored ones
    assert bool((case.chain.b_dx >= case.fact.b_dx).all()) and bool(case.chain.b_loss >= case.fact.b_loss)


@pytest.mark.parametrize("M,K,kind,weighted", IBOT_CASES)
@pytest.mark.parametrize("factored", [False, True], ids=["dense", "fact"])
def test_ibot_emulator_within_bounds(M, K, kind, weighted, factored):
    case = po.ibot_case(M, K, kind, weighted)
    assert po.fp32_domain_ok(case.xt, po.TEACHER_TEMP)
    out = emu_ibot(case, factored)
    assert all(bool(torch.isfinite(o.float()).all()) for o in out)
    r = ce_ratios(case.fact if factored else case.dense, *out)
    print(f"\n  emulator err/bound ibot {M}x{K} {kind} w{int(weighted)}: {_fmt(r)}")
    assert all(v <= 1.0 for v in r.values()), r


# ---------------------------------------------------------------------------
# planted errors leave a bound by 4x, at the first constant and at the ceiling
# ---------------------------------------------------------------------------

CONSTANTS = [po.INTRINSIC, po.INTRINSIC_MAX]
SK_PLANT_CASES = [(37, 2056, 0.04, "planted"), (37, 2056, 0.04, "flat"), (37, 4104, 0.04, "planted"),
                  (600, 2048, 0.07, "flat")]
SK_PLANTS = {
    "last column dropped": dict(drop_last_col=True),
    "column 2048 dropped": dict(drop_col=2048),
    "one row dropped from a column sum": dict(drop_row=5),
    "n_iterations - 1": dict(n_iterations=2),
    "u ignored after the first iteration": dict(ignore_u=True),
}


@pytest.mark.parametrize("intrinsic", CONSTANTS, ids=["first", "ceiling"])
@pytest.mark.parametrize("plant", list(SK_PLANTS))
def test_sinkhorn_planted_error_violates_a_bound(plant, intrinsic):
    worst = {}
    for M, K, temp, kind in SK_PLANT_CASES:
        case = po.sinkhorn_case(M, K, temp, kind, intrinsic)
        worst[(M, K, kind)] = max(sinkhorn_ratios(case, *emu_sinkhorn(case.x, temp, **SK_PLANTS[plant])).values())
    print(f"\n  planted '{plant}' err/bound: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > 4.0, worst


DINO_PLANT_CASES = [(4, 2, 3, False, 2056, "planted"), (4, 2, 3, False, 2056, "flat"),
                    (4, 2, 3, True, 264, "planted"), (4, 2, 3, True, 264, "flat")]
DINO_PLANTS = {
    "last column dropped": dict(drop_last_col=True),
    "column 2048 dropped": dict(drop_col=2048),
    "teacher term dropped from dx": dict(no_teacher_dx=True),
    "teacher crop 0 used twice": dict(crop0_twice=True),
    "diagonal flipped": dict(flip_diag=True),
    "u[trow] from row b": dict(u_from_b=True),
    "upstream gradient ignored": dict(ignore_g=True),
    "v shifted by one column": dict(v_shift=True),
}


@pytest.mark.parametrize("intrinsic", CONSTANTS, ids=["first", "ceiling"])
@pytest.mark.parametrize("plant", list(DINO_PLANTS))
def test_dino_planted_error_violates_a_bound(plant, intrinsic):
    kw = dict(DINO_PLANTS[plant])
    flip = kw.pop("flip_diag", False)
    factored_only = "u_from_b" in kw or "v_shift" in kw
    worst = {}
    for S, T, B, ignore_diag, K, kind in DINO_PLANT_CASES:
        case = po.dino_case(S, T, B, ignore_diag, K, kind, intrinsic)
        for factored in ([True] if factored_only else [False, True]):
            # both directions of the diagonal: skipped with ignore_diag off, kept with it on
            out = emu_dino(case, ignore_diag, factored, kernel_diag=(not ignore_diag) if flip else None, **kw)
            worst[(ignore_diag, K, kind, factored)] = max(
                ce_ratios(case.fact if factored else case.dense, *out).values())
    print(f"\n  planted '{plant}' err/bound: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    if flip:   # each direction on its own
        assert max(v for k, v in worst.items() if not k[0]) > 4.0, worst
        assert max(v for k, v in worst.items() if k[0]) > 4.0, worst
    if factored_only or plant == "column 2048 dropped":
        assert max(worst.values()) > 4.0, worst
    else:      # the dense and the factored kernel each show it
        assert max(v for k, v in worst.items() if not k[3]) > 4.0, worst
        assert max(v for k, v in worst.items() if k[3]) > 4.0, worst


IBOT_PLANTS = {
    "last column dropped": dict(drop_last_col=True),
    "column 2048 dropped": dict(drop_col=2048),
    "teacher term dropped from dx": dict(no_teacher_dx=True),
    "row weights shifted by one row": dict(shift_w=True),
    "upstream gradient ignored": dict(ignore_g=True),
    "v shifted by one column": dict(v_shift=True),
}


@pytest.mark.parametrize("intrinsic", CONSTANTS, ids=["first", "ceiling"])
@pytest.mark.parametrize("plant", list(IBOT_PLANTS))
def test_ibot_planted_error_violates_a_bound(plant, intrinsic):
    kw = IBOT_PLANTS[plant]
    worst = {}
    for kind in ("planted", "flat"):
        case = po.ibot_case(57, 2056, kind, True, intrinsic)
        for factored in ([True] if "v_shift" in kw else [False, True]):
            out = emu_ibot(case, factored, **kw)
            worst[(kind, factored)] = max(ce_ratios(case.fact if factored else case.dense, *out).values())
    print(f"\n  planted '{plant}' err/bound: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for factored in ([True] if "v_shift" in kw else [False, True]):
        assert max(v for k, v in worst.items() if k[1] == factored) > 4.0, worst


# ---------------------------------------------------------------------------
# the Python fallbacks of ops/proto_scores.py, in fp32 on the CPU
# ---------------------------------------------------------------------------

FALLBACK_SK_CASES = [c for c in SK_CASES if c[1] <= 4104
                     and po.fallback_domain_ok(po.sinkhorn_case(*c).x, c[2])]


def test_sinkhorn_fallback_domain():
    """The fallback normalises by the global sum first: the planted cases at
    T = 0.04 (e^100 between peak and background) are outside what it can hold
    in fp32, and only those."""
    left_out = [c for c in SK_CASES if c[1] <= 4104 and c not in FALLBACK_SK_CASES]
    assert left_out == [(M, K, 0.04, "planted") for M, K in po.SINKHORN_SHAPES if K <= 4104]


@pytest.mark.parametrize("M,K,temp,kind", FALLBACK_SK_CASES)
def test_sinkhorn_fallback_within_bounds(M, K, temp, kind):
    from dinov3_amd.ops.proto_scores import sinkhorn_knopp

    case = po.sinkhorn_case(M, K, temp, kind)
    for total in (None, torch.tensor(float(M + 11))):
        q = sinkhorn_knopp(case.x.float(), temp, total_columns=total)
        ratio = po.worst_ratio((q.double() - case.q).abs(), po.q_abs_bound(case.q, case.rel_q))
        print(f"\n  sinkhorn_knopp fallback err/bound {M}x{K} T{temp} {kind}: {ratio:.3f}")
        assert ratio <= 1.0


def _backward(loss, x):
    loss.backward(torch.tensor(po.UPSTREAM))
    return x.grad


@pytest.mark.parametrize("S,T,B,ignore_diag,K,kind", [c for c in DINO_CASES if c[4] <= 2056])
def test_dino_fallback_within_bounds(S, T, B, ignore_diag, K, kind):
    from dinov3_amd.ops.proto_scores import FactoredProbs, dino_softmax_ce

    case = po.dino_case(S, T, B, ignore_diag, K, kind)
    for ref, teacher in ((case.dense, case.t32),
                         (case.fact, FactoredProbs(case.xt, case.u32.view(T, B), case.v32, po.TEACHER_TEMP))):
        x = case.x.float().requires_grad_(True)
        loss = dino_softmax_ce(x, teacher, po.STUDENT_TEMP, ignore_diag)
        dx = _backward(loss, x)
        r = {"loss": po.worst_ratio((loss.detach().double() - ref.loss).abs().reshape(1), ref.b_loss.reshape(1)),
             "dx": po.worst_ratio((dx.double() - ref.dx).abs(), ref.b_dx)}
        print(f"\n  dino_softmax_ce fallback err/bound: {_fmt(r)}")
        assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("M,K,kind,weighted", [c for c in IBOT_CASES if c[1] <= 2056])
def test_ibot_fallback_within_bounds(M, K, kind, weighted):
    from dinov3_amd.ops.proto_scores import FactoredProbs, ibot_softmax_ce

    case = po.ibot_case(M, K, kind, weighted)
    for ref, teacher in ((case.dense, case.t32),
                         (case.fact, FactoredProbs(case.xt, case.u32, case.v32, po.TEACHER_TEMP))):
        x = case.x.float().requires_grad_(True)
        loss = ibot_softmax_ce(x, teacher, n_total_rows=M + 3, student_temp=po.STUDENT_TEMP,
                               masks_weight=case.w if weighted else None)
        dx = _backward(loss, x)
        r = {"loss": po.worst_ratio((loss.detach().double() - ref.loss).abs().reshape(1), ref.b_loss.reshape(1)),
             "dx": po.worst_ratio((dx.double() - ref.dx).abs(), ref.b_dx)}
        print(f"\n  ibot_softmax_ce fallback err/bound: {_fmt(r)}")
        assert all(v <= 1.0 for v in r.values()), r


# ---------------------------------------------------------------------------
# the bound check itself, the launchers' tiling, the constants
# ---------------------------------------------------------------------------

def test_bound_check_rejects_nan_and_zero_bound():
    one, zero = torch.ones(1), torch.zeros(1)
    assert po.worst_ratio(torch.tensor([float("nan")]), one) == float("inf")
    assert po.worst_ratio(one, zero) == float("inf")
    assert po.worst_ratio(zero, zero) == 0.0
    # a NaN left in u, Q or dx is outside its bound
    case = po.sinkhorn_case(3, 2040, 0.04, "flat")
    u, v = emu_sinkhorn(case.x, 0.04)
    u[1] = float("nan")
    r = sinkhorn_ratios(case, u, v)
    assert r["u"] == float("inf") and r["Q"] == float("inf")


def test_shape_list_reaches_every_launcher_branch():
    assert po.colsum_tiling(37, 2048) == (1, 1, 37) and po.rowsum_split(37) == 13 and 2048 % 13
    assert po.colsum_tiling(37, 2056)[0] == 2 and po.colsum_tiling(37, 4104)[0] == 3
    assert po.colsum_tiling(600, 2048)[1:] == (2, 300) and po.rowsum_split(600) == 1
    assert po.colsum_tiling(1, 8) == (1, 1, 1)                      # gridDim.y == 1: plain stores
    assert po.colsum_tiling(5, 98304) == (48, 1, 5) and 512 // 48 == 10
    assert po.INTRINSIC <= po.INTRINSIC_MAX

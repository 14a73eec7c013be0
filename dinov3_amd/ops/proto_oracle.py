"""fp64 oracle, elementwise rounding bounds and test-case generators for the
prototype-score kernels (csrc/proto_ce.hip): factored and materialized
Sinkhorn-Knopp, and the DINO / iBOT cross-entropy with a dense or a factored
teacher.

Pure torch on the CPU; nothing here touches the HIP extension.

The oracle follows the kernels only where they *define* the operation:

- the inputs are the bf16 logits;
- ``inv_temp`` is the fp32 value of ``1/temp`` the bindings pass;
- ``dx`` is stored as bf16. The oracle's ``dx`` is unrounded; that rounding is
  one term of its bound.

Everything else is fp64. Every further rounding step of the kernels is one
term of a bound below, written next to the formula it perturbs. Conventions
are those of ops/fmha_oracle.py: one bf16 rounding is ``2^-9`` relative, one
fp32 rounding ``2^-24`` relative. A sum of positive fp32 terms that passes
through at most ``d`` additions on the way from any term to the result has a
relative error of at most ``d * 2^-24``; the depths are the kernels' real ones
(``block_depth``, ``colsum_tiling``, ``rowsum_split``). Relative bounds are
kept as exponents ``r`` (the computed value is within ``exp(+-r)`` of the
exact one), so they add up when factors compound; ``expm1`` turns them into
relative errors at the end.

Input domain: the Sinkhorn kernels compute ``exp(x/T)`` with no max
subtraction, and so does the oracle. The generators keep ``|x|/T <= 60``, and
``fp32_domain_ok`` checks that an fp32 evaluation of every exponential, sum
and scale vector of a case stays finite and normal. Single products
``exp(x/T) * u * v`` may fall below the fp32 normal range (a background column
next to a peak of ``e^100`` times its size); they are positive terms of sums
that are normal, and the bounds carry the absolute ``FP32_TINY`` for them.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .fmha_oracle import BF16_RNE, FP32_ULP, worst_ratio  # noqa: F401  (worst_ratio re-exported)

FP32_TINY = 2.0 ** -126   # smallest normal fp32: the absolute error of a flushed product

# Per-call relative error of __expf / __logf beyond what is proportional to the
# argument. __expf(a) is the hardware exp2 of a * log2(e), __logf(s) the
# hardware log2 times ln 2: the hardware ops are good to about 1 ulp (2^-23) on
# normal results, and the constant multiply adds one fp32 rounding, so 2^-22
# per call is the first value. Argued from how the intrinsics are built, not
# measured; it may be raised up to INTRINSIC_MAX only.
# Measured worst err/bound per case group (MI355X result against this oracle,
# tests/test_proto_exact_gpu.py -s) with the first value, which did not have
# to move:
#   sinkhorn factored       u 0.019  v 0.044  Q 0.029
#   sinkhorn materialized   Q 0.030   (module fallback, K 2052 / misaligned: 0.019)
#   dino dense              loss 0.061  lse 0.211  st 0.076  dx 0.996
#   dino factored           loss 0.045  lse 0.211  st 0.124  dx 0.995
#   ibot dense              loss 0.056  lse 0.260  st 0.139  dx 0.994
#   ibot factored           loss 0.075  lse 0.260  st 0.085  dx 0.994
#   DINOLoss chain          loss 0.006  dx 0.972
#   iBOTPatchLoss chain     loss 0.005  dx 0.973
# dx sits at the bf16 store: round-to-nearest of a value just above a power of
# two is off by 2^-8 / (1 + 2^-8) = 0.996 of that term, whatever the kernel.
INTRINSIC = 2.0 ** -22
# Ceiling: with the constant here, every planted error of
# tests/test_proto_oracle.py still exceeds its bound at least 4x (asserted
# there). The least visible one is a lost column of a flat row (u moves by
# ~1/K = 4.9e-4 against a bound of six compounded sums, each carrying the
# constant once): 35x outside at 37 x 2056 and 16x at 600 x 2048 with 2^-17.
INTRINSIC_MAX = 2.0 ** -17
# Roundings whose effect on exp(a) is |a| * 2^-24 relative: the fp32 product
# x * inv_temp, the intrinsic's multiply by log2(e), and the rounded log2(e).
ARG_ROUNDINGS = 3

CE_BLOCK = 256            # threads per block of every kernel here
COL_WINDOW = CE_BLOCK * 8  # columns per block of the factored column sum


def inv_temp32(temp: float) -> float:
    """The fp32 value (float)(1.0 / temp) the bindings pass, as a python float."""
    return float(torch.tensor(1.0 / temp, dtype=torch.float64).to(torch.float32))


def fp32_scalar(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def block_depth(n_terms: int) -> int:
    """Additions between one term and the result of a 256-thread strided sum
    over n_terms columns: ceil(n/256) per thread, six shuffle levels inside a
    wave, six more over the wave sums (block_reduce_sum)."""
    return -(-n_terms // CE_BLOCK) + 12


def colsum_tiling(M: int, K: int) -> Tuple[int, int, int]:
    """(windows, m_tile, tiles) of launch_sinkhorn_fact_colsum."""
    kw = -(-K // COL_WINDOW)
    tiles = max(1, 512 // max(kw, 1))
    tiles = min(tiles, M)
    m_tile = -(-M // tiles)
    return kw, m_tile, -(-M // m_tile)


def rowsum_split(M: int) -> int:
    """gridDim.y of launch_sinkhorn_fact_rowsum."""
    return min(16, max(1, 512 // M))


def fact_col_depth(M: int, K: int) -> int:
    # u * exp and its add per row of the tile, then one atomic per tile
    _, m_tile, mt = colsum_tiling(M, K)
    return 2 * m_tile + mt


def fact_row_depth(M: int, K: int) -> int:
    # exp * v and its add per column of the chunk, the block tree, one atomic
    # per chunk
    split = rowsum_split(M)
    kchunk = -(-K // split)
    return 2 * (-(-kchunk // CE_BLOCK)) + 12 + split


# ---------------------------------------------------------------------------
# Sinkhorn-Knopp
# ---------------------------------------------------------------------------

def _scaled(x: torch.Tensor, temp: float) -> torch.Tensor:
    return x.detach().cpu().double() * inv_temp32(temp)


def sinkhorn(x: torch.Tensor, temp: float, n_iterations: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u [M], v [K]) fp64 with Q = exp(x/T) * u[:, None] * v: per iteration
    v = 1 / (K * sum_m E u), u = 1 / sum_k E v, starting from u = 1."""
    E = torch.exp(_scaled(x, temp))
    M, K = E.shape
    u = torch.ones(M, dtype=torch.float64)
    v = torch.full((K,), float("inf"), dtype=torch.float64)
    for _ in range(n_iterations):
        v = 1.0 / ((E * u[:, None]).sum(0) * K)
        u = 1.0 / (E * v).sum(1)
    return u, v


def materialize(x: torch.Tensor, temp: float, u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return torch.exp(_scaled(x, temp)) * u.double()[:, None] * v.double()


def exp_rel(a: torch.Tensor, intrinsic: float) -> torch.Tensor:
    """Relative error exponent of __expf(fl(x * inv_temp)) against exp(a)."""
    return ARG_ROUNDINGS * FP32_ULP * a.abs() + intrinsic


def sinkhorn_bounds(x: torch.Tensor, temp: float, n_iterations: int = 3,
                    intrinsic: float = INTRINSIC, col_depth: Optional[int] = None,
                    row_depth: Optional[int] = None, per_iter_elem: int = 0):
    """Relative bounds (rel_u [M], rel_v [K], rel_q [M, K]) of the factored
    kernels; |got - ref| <= rel * ref. col_depth / row_depth default to the
    factored launchers' tiling; the materialized kernels pass their own, and
    per_iter_elem, the fp32 roundings they apply to every stored Q element per
    iteration."""
    a = _scaled(x, temp)
    M, K = a.shape
    col_depth = fact_col_depth(M, K) if col_depth is None else col_depth
    row_depth = fact_row_depth(M, K) if row_depth is None else row_depth
    e = exp_rel(a, intrinsic)                                   # every E[m, k]
    r_u = torch.zeros(M, dtype=torch.float64)
    r_v = torch.zeros(K, dtype=torch.float64)
    for _ in range(n_iterations):
        # A[k] = sum_m E[m, k] u[m]: positive terms, each within its own exponent
        r_a = (e + r_u[:, None]).amax(0) + col_depth * FP32_ULP
        # v = 1 / (A * K): the product and the reciprocal
        r_v = r_a + 3 * FP32_ULP
        # u[m] = 1 / sum_k E[m, k] v[k]; the division is not correctly rounded
        r_u = (e + r_v).amax(1) + row_depth * FP32_ULP + 3 * FP32_ULP
    # Q = exp(x / temp) * u * v: the exponential (x / temp differs from
    # x * inv_temp by the rounding of inv_temp and of the quotient, both inside
    # ARG_ROUNDINGS) and two products
    r_q = e + r_u[:, None] + r_v + (2 + per_iter_elem * n_iterations) * FP32_ULP
    return torch.expm1(r_u), torch.expm1(r_v), torch.expm1(r_q)


def materialized_bounds(x: torch.Tensor, temp: float, n_iterations: int = 3,
                        intrinsic: float = INTRINSIC) -> torch.Tensor:
    """rel_q of the materialized HIP path (_sinkhorn_knopp_hip): the column sum
    walks the M rows in one thread, the row sum is one block per row, and Q is
    stored in fp32 and rescaled twice per iteration (the division by col * K,
    that product, and the row multiplier with its own two roundings)."""
    M, K = x.shape
    return sinkhorn_bounds(x, temp, n_iterations, intrinsic, col_depth=M + 2,
                           row_depth=block_depth(K) + 4, per_iter_elem=5)[2]


def q_abs_bound(q: torch.Tensor, rel_q: torch.Tensor) -> torch.Tensor:
    return rel_q * q + FP32_TINY


def fp32_domain_ok(x: torch.Tensor, temp: float, n_iterations: int = 3) -> bool:
    """An fp32 evaluation of the factored iteration: every exponential, column
    sum, row sum and scale vector is finite and normal."""
    def ok(t):
        return bool(torch.isfinite(t).all() and (t.abs() >= FP32_TINY).all())

    E = torch.exp(x.detach().cpu().float() * torch.tensor(inv_temp32(temp), dtype=torch.float32))
    M, K = E.shape
    good = ok(E)
    u = torch.ones(M)
    for _ in range(n_iterations):
        A = (E * u[:, None]).sum(0)
        v = torch.reciprocal(A * K)
        s = (E * v).sum(1)
        u = 1.0 / s
        good = good and ok(A) and ok(v) and ok(s) and ok(u)
    return good


def fallback_domain_ok(x: torch.Tensor, temp: float) -> bool:
    """The domain of ops.sinkhorn_knopp off the GPU, which is narrower: like
    the reference it divides exp(x/T) by its global sum first, so every
    exp(x/T) / sum has to stay normal in fp32. A planted case at T = 0.04
    spans e^100 and does not: its background columns go through denormals
    there and lose their digits."""
    E = torch.exp(x.detach().cpu().float() / temp)
    q = E / E.sum()
    return bool(torch.isfinite(q).all() and (q >= FP32_TINY).all())


# ---------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------

@dataclass
class CEResult:
    loss: torch.Tensor      # 0-dim fp64
    lse: torch.Tensor       # [rows]
    st: torch.Tensor        # [rows]
    dx: torch.Tensor        # student shape, fp64, unrounded
    b_loss: torch.Tensor
    b_lse: torch.Tensor
    b_st: torch.Tensor
    b_dx: torch.Tensor


@dataclass
class Factored:
    """A factored teacher: t = exp(xt / temp) * u * v with fp32 u, v taken as
    exact inputs. rel_u / rel_v widen the bounds when u, v themselves come out
    of the Sinkhorn kernels (the end-to-end chain)."""
    xt: torch.Tensor                      # [..., K] bf16
    u: torch.Tensor                       # [...] fp32
    v: torch.Tensor                       # [K] fp32
    temp: float
    rel_u: Optional[torch.Tensor] = None
    rel_v: Optional[torch.Tensor] = None


def _teacher_rows(teacher, intrinsic: float):
    """(t, t_err): the teacher probabilities [rows, K] fp64 as the kernel's
    inputs define them, and the absolute error of the kernel's own value."""
    if isinstance(teacher, Factored):
        K = teacher.xt.shape[-1]
        a = _scaled(teacher.xt, teacher.temp).reshape(-1, K)
        t = torch.exp(a) * teacher.u.detach().cpu().double().reshape(-1, 1) * teacher.v.detach().cpu().double()
        # __expf(xt * inv_tt) * u * v: the exponential and two products
        r = exp_rel(a, intrinsic) + 2 * FP32_ULP
        if teacher.rel_u is not None:
            r = r + torch.log1p(teacher.rel_u).reshape(-1, 1) + torch.log1p(teacher.rel_v)
        return t, torch.expm1(r) * t + FP32_TINY
    t = teacher.detach().cpu().double()
    t = t.reshape(-1, t.shape[-1])
    return t, torch.full_like(t, FP32_TINY)  # read as fp32: exact unless a denormal is flushed


def _ce_core(a, ts, ts_err, n_teacher, w, g, inv_temp, denom, intrinsic):
    """a [R, K] = x * inv_temp; ts [R, K] the summed teacher rows and ts_err
    their absolute error; w [R] row weights; g the upstream gradient.
    loss = sum_r w_r (st_r lse_r - dot_r) / denom."""
    R, K = a.shape
    depth = block_depth(K)
    absa = a.abs()
    m = a.amax(-1, keepdim=True)
    lse = torch.logsumexp(a, dim=-1)
    p = torch.exp(a - lse[:, None])
    st = ts.sum(-1)
    dot = (ts * a).sum(-1)
    row = st * lse - dot
    loss = (w * row).sum() / denom
    gs = g / denom
    scale = gs * inv_temp * w[:, None]
    inner = st[:, None] * p - ts
    dx = scale * inner

    # ts = sum over the teacher crops: n_teacher - 1 additions of positive terms
    ts_err = ts_err + max(n_teacher - 1, 0) * FP32_ULP * ts
    # lse = m + __logf(sum_i __expf(xi - m)), xi = fl(x * inv_temp), m = max xi
    e = (FP32_ULP * (absa                                  # xi: shifts every term and m alike
                     + ARG_ROUNDINGS * (a - m).abs())      # xi - m, and the intrinsic's argument
         + intrinsic)                                      # __expf
    b_lse = ((p * e).sum(-1)                               # each term's share of the sum
             + depth * FP32_ULP                            # fp32 accumulation of the sum
             + intrinsic * (1 + (lse - m[:, 0]))           # __logf of a sum in [1, K]
             + FP32_ULP * lse.abs())                       # m + log, stored as fp32
    # st = sum_i ts_i
    b_st = ts_err.sum(-1) + depth * FP32_ULP * st
    # dot = sum_i ts_i * xi
    tsa = ts * absa
    b_dot = (ts_err * absa).sum(-1) + (2 + depth) * FP32_ULP * tsa.sum(-1)
    # row = st * lse - dot, then w * row into one atomic sum over the rows
    b_row = (st * b_lse + lse.abs() * b_st + b_st * b_lse + b_dot
             + 2 * FP32_ULP * ((st * lse).abs() + dot.abs()))
    b_loss = ((w.abs() * b_row).sum() + (R + 1) * FP32_ULP * (w * row).abs().sum()) / denom \
        + 2 * FP32_ULP * loss.abs()                        # loss_sum / denom in fp32
    # dx = bf16(scale * (st * sm - ts)), sm = __expf(xi - lse) with the stored lse
    r_sm = (b_lse[:, None]                                  # the stored lse
            + FP32_ULP * (absa + ARG_ROUNDINGS * (a - lse[:, None]).abs())
            + intrinsic)
    rel_sm = torch.expm1(r_sm)
    inner_err = (st[:, None] * p * (rel_sm + FP32_ULP)      # sm, and the product st * sm
                 + p * (1 + rel_sm) * b_st[:, None]         # the stored st
                 + ts_err                                   # the teacher term
                 + FP32_ULP * inner.abs()                   # the subtraction
                 + FP32_TINY)
    # the bf16 store: half an ulp of an 8-bit significand is up to 2^-8 of the
    # value just above a power of two, twice BF16_RNE (fmha_oracle.py doubles too)
    b_dx = (2 * BF16_RNE * dx.abs()
            + (1 + 2 * BF16_RNE) * (scale.abs() * inner_err
                                + 4 * FP32_ULP * dx.abs()))  # g / denom, * inv_temp, * w, * inner
    return CEResult(loss, lse, st, dx, b_loss, b_lse, b_st, b_dx)


def dino_denominator(S: int, T: int, B: int, ignore_diag: bool) -> float:
    return float(B * S * T - B * min(S, T)) if ignore_diag else float(B * S * T)


def dino_ce(x: torch.Tensor, teacher, temp: float, ignore_diag: bool, g: float,
            intrinsic: float = INTRINSIC) -> CEResult:
    """x [S, B, K] bf16; teacher a dense fp32 [T, B, K] or a Factored with xt
    [T, B, K] and u [T * B]. Same denominators as ops.dino_softmax_ce."""
    S, B, K = x.shape
    t, t_err = _teacher_rows(teacher, intrinsic)
    T = t.shape[0] // B
    t, t_err = t.view(T, B, K), t_err.view(T, B, K)
    keep = torch.ones(S, T, dtype=torch.float64)
    if ignore_diag:
        for s in range(min(S, T)):
            keep[s, s] = 0.0
    ts = torch.einsum("st,tbk->sbk", keep, t).reshape(S * B, K)
    ts_err = torch.einsum("st,tbk->sbk", keep, t_err).reshape(S * B, K)
    a = _scaled(x, temp).reshape(S * B, K)
    w = torch.ones(S * B, dtype=torch.float64)
    res = _ce_core(a, ts, ts_err, T, w, g, inv_temp32(temp), dino_denominator(S, T, B, ignore_diag),
                   intrinsic)
    res.dx, res.b_dx = res.dx.view(S, B, K), res.b_dx.view(S, B, K)
    return res


def ibot_ce(x: torch.Tensor, teacher, w: torch.Tensor, temp: float, g: float,
            intrinsic: float = INTRINSIC) -> CEResult:
    """x [M, K] bf16; teacher a dense fp32 [M, K] or a Factored; w [M] fp32 row
    weights. loss = sum_r w_r (st_r lse_r - dot_r), as ops.ibot_softmax_ce."""
    t, t_err = _teacher_rows(teacher, intrinsic)
    a = _scaled(x, temp)
    return _ce_core(a, t, t_err, 1, w.detach().cpu().double(), g, inv_temp32(temp), 1.0, intrinsic)


# ---------------------------------------------------------------------------
# case generators: seeded, few-bit (exact in bf16), different in every row
# ---------------------------------------------------------------------------

UPSTREAM = fp32_scalar(0.37)     # the upstream gradient of every backward here
PEAK_COLUMNS = (0, 7, 8, 255, 256, 2047, 2048, -8, -1)


def planted(M: int, K: int, seed: int, first: int = 0) -> torch.Tensor:
    """Multiples of 1/16 in [-2, 0], and in row m a +2 peak at column
    PEAK_COLUMNS[(m + first) % 9] mod K: the edges of the eight-column loads,
    of the 256-thread stride and of the 2048-column window. At T = 0.04 the
    peak is e^50 above the background and carries the whole row sum."""
    g = torch.Generator().manual_seed(seed)
    x = -torch.randint(0, 33, (M, K), generator=g).double() / 16
    for m in range(M):
        x[m, PEAK_COLUMNS[(m + first) % len(PEAK_COLUMNS)] % K] = 2.0
    return x.to(torch.bfloat16)


def flat(M: int, K: int, seed: int) -> torch.Tensor:
    """Values in {0, -1/64, ..., -4/64}: every column carries a comparable
    share, so one lost row moves v[k] by ~1/M and one lost column u[m] by ~1/K."""
    g = torch.Generator().manual_seed(seed)
    return (-torch.randint(0, 5, (M, K), generator=g).double() / 64).to(torch.bfloat16)


def logits(kind: str, M: int, K: int, seed: int, first: int = 0) -> torch.Tensor:
    return planted(M, K, seed, first) if kind == "planted" else flat(M, K, seed)


def row_weights(M: int, seed: int) -> torch.Tensor:
    """fp32 multiples of 1/64 in (0, 1/4], exact zeros in rows 1, 8, 15, ... and
    one large value in the last row."""
    g = torch.Generator().manual_seed(seed)
    w = (1 + torch.randint(0, 16, (M,), generator=g)).float() / 64
    w[1::7] = 0.0
    if M > 2:
        w[M - 1] = 16.0
    return w


# (M, K) of the factored Sinkhorn tests: the smallest sizes at which each branch
# of the two launchers exists. (1, 8): one thread, one row; (3, 2040): a window
# eight columns short; (37, 2048): one full window, row split 13 with an uneven
# chunk; (37, 2056): one thread in a second window; (37, 4104): the same in a
# third; (600, 2048): m_tile 2 and row split 1; (8, 65536) and (5, 98304): the
# configured widths, the second with 48 windows, so 10 tiles, no power of two.
SINKHORN_SHAPES = [(1, 8), (3, 2040), (37, 2048), (37, 2056), (37, 4104), (600, 2048),
                   (8, 65536), (5, 98304)]
SINKHORN_TEMPS = (0.04, 0.07)
FLAT_MAX_K = 2056                # flat cases only up to here: the 4x condition of INTRINSIC_MAX
MATERIALIZED_SHAPES = [(37, 2056), (33, 1000)]

# (S, T, B, ignore_diag, K)
DINO_SHAPES = ([(4, 2, 3, False, K) for K in (8, 264, 2056)]
               + [(2, 2, 3, True, K) for K in (8, 264, 2056)]
               + [(4, 2, 3, True, K) for K in (8, 264, 2056)]
               + [(2, 2, 1, False, 65536)])
# (M, K)
IBOT_SHAPES = [(1, 264), (1, 2056), (57, 264), (57, 2056), (3, 98304)]
STUDENT_TEMP = 0.1
TEACHER_TEMP = 0.04


def kinds_for(K: int):
    return ("planted", "flat") if K <= FLAT_MAX_K else ("planted",)


# ---------------------------------------------------------------------------
# reference cases: built once per (shape, kind, constant), never modified
# ---------------------------------------------------------------------------

@dataclass
class SinkhornCase:
    x: torch.Tensor        # [M, K] bf16
    temp: float
    u: torch.Tensor        # fp64
    v: torch.Tensor
    q: torch.Tensor
    rel_u: torch.Tensor
    rel_v: torch.Tensor
    rel_q: torch.Tensor


_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def sinkhorn_case(M: int, K: int, temp: float, kind: str,
                  intrinsic: float = INTRINSIC) -> SinkhornCase:
    def make():
        x = logits(kind, M, K, seed=1000 * M + K + (17 if kind == "flat" else 0))
        u, v = sinkhorn(x, temp)
        return SinkhornCase(x, temp, u, v, materialize(x, temp, u, v),
                            *sinkhorn_bounds(x, temp, intrinsic=intrinsic))
    return _cached(("sk", M, K, temp, kind, intrinsic), make)


@dataclass
class CECase:
    x: torch.Tensor        # student logits bf16, [S, B, K] or [M, K]
    xt: torch.Tensor       # teacher logits bf16, [T, B, K] or [M, K]
    t32: torch.Tensor      # dense teacher: the oracle's Q of xt, rounded to fp32
    u32: torch.Tensor      # factored teacher: the oracle's u, v rounded to fp32
    v32: torch.Tensor
    w: Optional[torch.Tensor]
    dense: CEResult
    fact: CEResult
    chain: CEResult        # fact, widened by the Sinkhorn kernels' own u / v bounds


def _teacher(xt_rows: torch.Tensor):
    u, v = sinkhorn(xt_rows, TEACHER_TEMP)
    rel_u, rel_v, _ = sinkhorn_bounds(xt_rows, TEACHER_TEMP)
    return (materialize(xt_rows, TEACHER_TEMP, u, v).float(), u.float(), v.float(),
            # the chain starts from the fp64 u, v; u32 / v32 are one rounding off
            rel_u + FP32_ULP, rel_v + FP32_ULP)


def dino_case(S: int, T: int, B: int, ignore_diag: bool, K: int, kind: str,
              intrinsic: float = INTRINSIC) -> CECase:
    def make():
        seed = 7 * S + 100 * B + K + (17 if kind == "flat" else 0) + (3 if ignore_diag else 0)
        x = logits(kind, S * B, K, seed, first=3).view(S, B, K)
        xt = logits(kind, T * B, K, seed + 1).view(T, B, K)
        t32, u32, v32, rel_u, rel_v = _teacher(xt.view(T * B, K))
        fact = Factored(xt, u32, v32, TEACHER_TEMP)
        chain = Factored(xt, u32, v32, TEACHER_TEMP, rel_u, rel_v)
        run = lambda teacher: dino_ce(x, teacher, STUDENT_TEMP, ignore_diag, UPSTREAM, intrinsic)
        return CECase(x, xt, t32.view(T, B, K), u32, v32, None, run(t32.view(T, B, K)), run(fact),
                      run(chain))
    return _cached(("dino", S, T, B, ignore_diag, K, kind, intrinsic), make)


def ibot_case(M: int, K: int, kind: str, weighted: bool = True,
              intrinsic: float = INTRINSIC) -> CECase:
    """weighted: row_weights; otherwise the masks_weight=None default of
    ops.ibot_softmax_ce, 1 / n_total_rows in fp32 with n_total_rows = M + 3."""
    def make():
        seed = 31 * M + K + (17 if kind == "flat" else 0)
        x = logits(kind, M, K, seed, first=3)
        xt = logits(kind, M, K, seed + 1)
        t32, u32, v32, rel_u, rel_v = _teacher(xt)
        w = row_weights(M, seed + 2) if weighted else torch.full((M,), 1.0 / (M + 3))
        fact = Factored(xt, u32, v32, TEACHER_TEMP)
        chain = Factored(xt, u32, v32, TEACHER_TEMP, rel_u, rel_v)
        run = lambda teacher: ibot_ce(x, teacher, w, STUDENT_TEMP, UPSTREAM, intrinsic)
        return CECase(x, xt, t32, u32, v32, w, run(t32), run(fact), run(chain))
    return _cached(("ibot", M, K, kind, weighted, intrinsic), make)

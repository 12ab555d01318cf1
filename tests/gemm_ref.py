"""Plain fp64 numpy references, per-element bounds and case generators for the dense GEMMs cr_gemm_rows / cr_gemm_wgrad
(csrc/cr_gemm.hip, csrc/cr_gemm_bf.hip), as include/castrec.h states them.  tests/test_gemm_gpu.py holds every kernel form to
these; tests/test_gemm_host.py checks the references against torch autograd, shows that a CPU emulation of each arithmetic stays
inside the bound stated for it, restates the dispatch and proves the premises the GPU cases rest on.

Every input is drawn as a float32 value (row_ops_ref.draw) and widened, so no input rounding enters a bound.  u = 2^-24 and
bound(S, n, r) = 2 (r + n) u S are row_ops_ref's: an output element is a sum of n addends, each through r fp32 roundings before it
is added, S the fp64 sum of the addends' absolute values.

rows_ref.  value = (((A op(B) + bias) relu) * keep / (1 - rate) + residual) * (mask_ids != 0) + C0, castrec.h's epilogue order.
S follows the value: sum_k |a b| + |bias|, UNCHANGED by the relu (a kernel off by e in front of the relu is off by at most e
behind it, also when the two sit on different sides of zero), times the dropout factor, + |residual|, zero in a masked row, + |C0|.
n = K plus one each for bias, residual and the accumulated value.  Sp is the product part of S alone (through the dropout factor and
the row mask): what an operand rounding scales with.

Bounds (rows_bound / wgrad_bound), by the kernel the dispatch picks:
  fp32 form    v_mfma_f32_16x16x4_f32 is a k-ordered fp32 fmaf chain, one rounding per product, no wider accumulator.  So
               bound(S, n, r) with r = 1 (the product's step of the chain) + 1 with dropout (* 1/(1 - rate)); the adds of the epilogue
               are among the n - 1 roundings of the sum.  The weight gradient: n = M (the per-slab chains and the fp64 sum of the slabs
               are one sum of M addends), r = 1; db is a sum of exact addends, r = 0, n = M.
  split form   x = hi + lo + e (hi = bf16(x), lo = bf16(x - hi), both to nearest even).  bf16 keeps 8 significant bits, so its unit
               roundoff is 2^-8: |x - hi| <= 2^-8 |x|, |lo| <= 2^-8 (1 + 2^-8) |x|, |e| <= 2^-16 |x| (test_gemm_host asserts the first
               and the last on drawn data).  a b - (ah bh + ah bl + al bh) = al bl + ea b + a eb - ea eb, at most
               E_SPLIT = 3 * 2^-16 * (1 + 2^-7) times |a b|: E_SPLIT * Sp per element.  (Half these operand figures, 2^-9 and 2^-18,
               i.e. 3 * 2^-18 * (1 + 2^-8) * Sp, is NOT a bound: the emulation of the stated arithmetic itself leaves it, by up to
               1.97 x at a weight gradient over one row and 1.42 x at K = 9 in plain bf16 -- the operand images are a deterministic
               function of the input, the same bits in kernel and emulation, so no correct kernel could meet it.)  To that the
               accumulation term, over 3 K addends whose absolute sum is at most (1 + 2^-7) Sp:
               BF_ACC * bound((1 + 2^-7) S, n + 2 K, r).
  plain bf16   against the matched model (operands through bf16_ref.bf16_rne, fp64 products; S from the rounded operands):
               BF_ACC * bound(S, n, r), the accumulation term alone.  Against the exact product: two operands off by 2^-8 each,
               E_BF16 = 2^-7 + 2^-16 times Sp more.
  db, bf16     k_gemm_wgrad_bf sums the images it staged: hi + lo in the split form (2 M addends, each exact, plus the fold of the
               four waves: n = 2 M + 4, r = 0, and 2^-16 * S for the e the images do not hold), the ROUNDED G in plain bf16 (matched
               model colsum(bf16(G)), n = M + 4; against the exact sum 2^-8 * S more).
BF_ACC is the one constant that cannot be derived here: how v_mfma_f32_16x16x32_bf16 rounds its internal 32-term sum.  It is 1 (the
same bound() as the fp32 chain): on the MI355X every bf16 form stayed inside it -- plain bf16 against the matched model, where the
accumulation term stands alone, included -- so nothing was measured into it ("GEMM forms against fp64", has the largest
error / bound of each test).

Shapes go by the kernels' units, not by the workload: 64 x 64 output tiles, 64-deep K chunks, 32-wide (bf16) or 4-wide (fp32)
k-steps, 8-float items; the weight gradient takes 32-row (fp32) or 64-row (bf16) chunks."""
import functools
import itertools
import types

import numpy as np
import torch

import bf16_ref as br
import dropout_ref as dr
from row_ops_ref import F64, U, _mask, bound, draw, pick_seed, wide

BF_ACC = 1.0
E_SPLIT = 3 * 2.0 ** -16 * (1 + 2.0 ** -7)          # the dropped lo lo term and the two e terms
E_BF16 = 2.0 ** -7 + 2.0 ** -16                     # two operands rounded to 8 bits
PREC_F32, PREC_X3, PREC_BF16 = 0, 1, 2
MAX_BATCH = 4                                       # CR_MAX_BATCH

DIMS = [8, 9, 15, 16, 31, 32, 33, 63, 64, 65, 67, 71, 72, 127, 128, 129, 136, 200]
SMALL = [1, 3, 7]
M_ROWS = [1, 17, 65, 130]
OTHER = [9, 64, 67]


def _unique(seq):
    return list(dict.fromkeys(seq))


# (M, N, K): every n as N against K in OTHER and as K against N in OTHER
SHAPES = _unique([(M, n, k) for n in DIMS + SMALL for k in OTHER for M in M_ROWS]
                 + [(M, n, k) for k in DIMS + SMALL for n in OTHER for M in M_ROWS])
EPILOGUES = list(itertools.product([False, True], repeat=6))        # bias, relu, dropout, residual, mask, accumulate
EPI_SHAPE = (130, 67, 72)
WGRAD_KN = [(K, N) for K in (9, 64, 67, 136) for N in (8, 65, 71, 128)]
WGRAD_M = [1, 31, 64, 97, 300]
WGRAD_SLABS = ["1", "5", "M+3"]


def n_slabs_of(name, M):
    return {"1": 1, "5": 5, "M+3": M + 3}[name]


def pitch(n, extra=0):
    """an odd pitch above n"""
    return ((n + 3) | 1) + 2 * extra


def bf16(a):
    """float32 array -> fp64 of its bf16 image (to nearest even)"""
    return br.bf16_rne(torch.from_numpy(np.ascontiguousarray(a, np.float32).astype(F64))).numpy()


def split(a):
    hi = bf16(a)
    return hi, bf16((wide(a) - hi).astype(np.float32))          # x - hi is exact in fp32


# ------------------------------------------------------------------------------------------------ dispatch (cr_gemm.hip)
def kernel_of(problems, entry="rows"):
    """problems: [(precision, K, N)] of one launch.  The bf16 kernels run if and only if all precisions are equal and nonzero and
    every K, N >= 8 (cr_gemm_rows_bf_supported / cr_gemm_wgrad_bf_supported); everything else is the exact fp32 kernel."""
    p0 = problems[0][0]
    bf = all(p == p0 and p != PREC_F32 and K >= 8 and N >= 8 for p, K, N in problems)
    name = "k_gemm_rows" if entry == "rows" else "k_gemm_wgrad"
    return name + ("_bf<%s>" % ("true" if p0 == PREC_X3 else "false") if bf else "")


def form_of(prec, K, N):
    """the arithmetic a single problem gets: "f32", "x3" or "bf16" """
    k = kernel_of([(prec, K, N)])
    return "f32" if k == "k_gemm_rows" else "x3" if "true" in k else "bf16"


# ------------------------------------------------------------------------------------------------ cr_gemm_rows
@functools.lru_cache(maxsize=None)
def rows_case(M, N, K, bias=True, relu=True, drop=False, residual=True, mask=True, accumulate=False, row_offset=0):
    """One problem (the same numbers for both orientations of B: c.B is [K, N], the trans_b launch gets its transpose).  Pitches
    are odd, differ from the widths and from each other."""
    rs = np.random.RandomState((1000003 * M + 1009 * N + K) % (2 ** 31) + 7 * (bias + 2 * relu + 4 * drop + 8 * residual + 16 * mask + 32 * accumulate))
    c = types.SimpleNamespace(M=M, N=N, K=K, A=draw(rs, M, K), B=draw(rs, K, N), bias=draw(rs, N) if bias else None, relu=relu,
                              residual=draw(rs, M, N, scale=2.0) if residual else None, mask_ids=_mask(rs, M) if mask else None,
                              accumulate=accumulate, C0=draw(rs, M, N, scale=2.0) if accumulate else None,
                              rate=0.25 if drop else 0.0, step=5, site=6, seed=0, row_offset=row_offset,
                              lda=pitch(K), ldb=pitch(N), ldbt=pitch(K, 1), ldc=pitch(N, 1), ldr=pitch(N, 2))
    if drop:
        c.seed = pick_seed(c.rate, M, N, c.step, c.site, row_offset, 23)
    return c


def factor(c):
    """[M, N] fp64 keep / (1 - rate) (the fp32 factor, widened); ones without dropout"""
    if c.rate == 0:
        return np.ones((c.M, c.N), F64)
    return dr.rows_mask(c.seed, c.step, c.site, c.rate, c.M, c.N, c.row_offset).astype(F64) * float(dr.thresh_scale(c.rate)[1])


def rows_ref(c, matched=False):
    """(value, S, n, Sp), the first, second and fourth [M, N] fp64 (module docstring).  matched: the operands A, B through bf16 first."""
    A, B = (bf16(c.A), bf16(c.B)) if matched else (wide(c.A), wide(c.B))
    v, S, n = A @ B, np.abs(A) @ np.abs(B), c.K
    Sp = S.copy()
    if c.bias is not None:
        v, S, n = v + wide(c.bias), S + np.abs(wide(c.bias)), n + 1
    if c.relu:
        v = np.maximum(v, 0.0)
    f = factor(c)
    v, S, Sp = v * f, S * f, Sp * f
    if c.residual is not None:
        v, S, n = v + wide(c.residual), S + np.abs(wide(c.residual)), n + 1
    if c.mask_ids is not None:
        live = (c.mask_ids != 0)[:, None]
        v, S, Sp = np.where(live, v, 0.0), np.where(live, S, 0.0), np.where(live, Sp, 0.0)
    if c.accumulate:
        v, S, n = v + wide(c.C0), S + np.abs(wide(c.C0)), n + 1
    return v, S, n, Sp


@functools.lru_cache(maxsize=None)
def rows_refs(*key):
    """(case, exact reference, matched reference) of rows_case(*key): computed once, shared by every test, never written"""
    c = rows_case(*key)
    return c, rows_ref(c), rows_ref(c, matched=True)


def rows_bound(c, ref, form, matched=False):
    """per-element allowance of the kernel form against rows_ref(c, matched) (matched only with form "bf16")"""
    v, S, n, Sp = ref
    r = 1 + (c.rate > 0)
    if form == "f32":
        return bound(S, n, r)
    if form == "x3":
        return E_SPLIT * Sp + BF_ACC * bound((1 + 2.0 ** -7) * S, n + 2 * c.K, r)
    acc = BF_ACC * bound(S, n, r)
    return acc if matched else (1 + 2.0 ** -8) * acc + E_BF16 * Sp


# ------------------------------------------------------------------------------------------------ cr_gemm_wgrad
@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K):
    rs = np.random.RandomState(7919 * M + 131 * N + K)
    return types.SimpleNamespace(M=M, N=N, K=K, A=draw(rs, M, K), G=draw(rs, M, N), lda=pitch(K), ldg=pitch(N, 1))


def wgrad_ref(c, matched=False):
    """dW = A^T G [K, N] and db = colsum(G) [N] with their absolute sums: (dW, S_W, db, S_b).  matched: A and G through bf16 first
    (db is then what plain bf16 sums: the rounded G)."""
    A, G = (bf16(c.A), bf16(c.G)) if matched else (wide(c.A), wide(c.G))
    return A.T @ G, np.abs(A).T @ np.abs(G), G.sum(0), np.abs(G).sum(0)


@functools.lru_cache(maxsize=None)
def wgrad_refs(M, N, K):
    c = wgrad_case(M, N, K)
    return c, wgrad_ref(c), wgrad_ref(c, matched=True)


def wgrad_bound(c, ref, form, matched=False):
    """(allowance for the fp64 sum of the dW slabs, for that of the db slabs)"""
    dW, SW, db, Sb = ref
    if form == "f32":
        return bound(SW, c.M, 1), bound(Sb, c.M, 0)
    if form == "x3":
        return (E_SPLIT * SW + BF_ACC * bound((1 + 2.0 ** -7) * SW, 3 * c.M, 1),
                2.0 ** -16 * Sb + bound((1 + 2.0 ** -8) * Sb, 2 * c.M + 4, 0))
    accW, accb = BF_ACC * bound(SW, c.M, 1), bound(Sb, c.M + 4, 0)
    return (accW, accb) if matched else ((1 + 2.0 ** -8) * accW + E_BF16 * SW, (1 + 2.0 ** -8) * accb + 2.0 ** -8 * Sb)


def slab_rows(M, n_slabs):
    """[(first row, end row)] per slab: rps = ceil(M / n_slabs), slab s takes [s rps, min(M, (s + 1) rps))"""
    rps = -(-M // n_slabs)
    return [(min(M, s * rps), min(M, (s + 1) * rps)) for s in range(n_slabs)]


# ------------------------------------------------------------------------------------------------ the arithmetic, emulated
def _chain(acc, a, b):
    """acc [I, J] float32 += a [I, k] b [k, J], one fp32 fmaf per k in order: float32(float64 a b + acc)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    for k in range(a.shape[1]):
        acc = (a[:, k, None] * b[None, k, :] + acc.astype(F64)).astype(np.float32)
    return acc


def emu_product(a, b, form):
    """float32 [I, J] = a [I, k] @ b [k, J] as the kernel form accumulates it: the fp32 chain in k order; the bf16 forms per 32-wide
    k-step lo hi, hi lo, hi hi (cr_bf16.hpp mma: small terms first), every product exact and every add rounded to fp32"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    if form == "f32":
        return _chain(acc, a, b)
    (ah, al), (bh, bl) = (split(a), split(b)) if form == "x3" else ((bf16(a), None), (bf16(b), None))
    for k0 in range(0, a.shape[1], 32):
        s = slice(k0, k0 + 32)
        if form == "x3":
            acc = _chain(_chain(acc, al[:, s], bh[s]), ah[:, s], bl[s])
        acc = _chain(acc, ah[:, s], bh[s])
    return acc


def emu_rows(c, form):
    """cr_gemm_rows on the CPU: emu_product, then the epilogue of k_gemm_rows in np.float32, statement by statement"""
    f32 = np.float32
    v = emu_product(c.A, c.B, form)
    if c.bias is not None:
        v = v + c.bias
    if c.relu:
        v = np.maximum(v, f32(0))
    if c.rate > 0:
        v = v * factor(c).astype(f32)
    if c.residual is not None:
        v = v + c.residual
    if c.mask_ids is not None:
        v = np.where((c.mask_ids != 0)[:, None], v, f32(0))
    if c.accumulate:
        v = c.C0 + v
    assert v.dtype == f32
    return v


def emu_wgrad(c, form, n_slabs):
    """cr_gemm_wgrad on the CPU: (dW slabs [n_slabs, K, N], db slabs [n_slabs, N]) float32"""
    dW, db = np.zeros((n_slabs, c.K, c.N), np.float32), np.zeros((n_slabs, c.N), np.float32)
    for s, (m0, m1) in enumerate(slab_rows(c.M, n_slabs)):
        if m0 == m1:
            continue
        A, G = c.A[m0:m1], c.G[m0:m1]
        dW[s] = emu_product(np.ascontiguousarray(A.T), G, form)
        if form == "f32":
            terms = [wide(G)]
        elif form == "x3":
            terms = list(split(G))
        else:
            terms = [bf16(G)]
        acc = np.zeros(c.N, np.float32)
        for m in range(m1 - m0):
            for t in terms:
                acc = (acc.astype(F64) + t[m]).astype(np.float32)
        db[s] = acc
    return dW, db


# ------------------------------------------------------------------------------------------------ the batched and dispatch cases
# test_rows_batched: CR_MAX_BATCH problems of 1, 2, 6 and 9 output tiles, mixed orientation, distinct epilogues
#            (M, N, K, trans_b, bias, relu, drop, residual, mask, accumulate)
BATCHED = [(50, 40, 67, False, True, False, False, False, False, False),
           (65, 64, 9, True, False, True, True, False, True, False),
           (130, 67, 72, False, True, True, False, True, False, True),
           (129, 135, 130, True, True, False, True, True, True, True)]
# test_wgrad_batched: three (M, N, K) in one launch over one grid of slabs (2, 3 and 2 tiles; at M = 3 two slabs have no rows)
WGRAD_BATCHED = [(97, 71, 67), (3, 8, 136), (300, 128, 9)]
WGRAD_BATCHED_SLABS = 5


def tiles(M, N):
    return -(-M // 64) * -(-N // 64)

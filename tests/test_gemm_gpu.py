"""cr_gemm_rows / cr_gemm_wgrad (csrc/cr_gemm.hip, csrc/cr_gemm_bf.hip) against the fp64 numpy references of tests/gemm_ref.py, element
by element under the bounds derived there (tests/test_gemm_host.py checks the references, shows a CPU emulation of each arithmetic
inside its bound on these very cases, and proves that each case reaches the kernel and the path it is named for).  Every operand is a
view one float past a 16-byte boundary with an odd pitch.  Every buffer a kernel writes is wider than what it may write, starts as a
NaN with a payload and must come back bit for bit outside the written region: the pad columns of ldc / ldw, the words in front of the
matrix and behind its last row, the slab words outside the [K, N] and [N] regions.  The pads of the inputs hold the same NaN, so a
kernel that masks by multiplying instead of selecting fails.  A test walks its shapes itself and reports every failing one.

What reaches what (prec 0 / 1 / 2 = CR_PREC_F32 / BF16X3 / BF16; a bf16 precision with K or N below 8 is the fp32 kernel):
  k_gemm_rows                          test_rows_shapes[0-*], [1-*] and [2-*] at K or N in 1, 3, 7; test_rows_epilogues[0]
      !trans_b | trans_b               [*-nn] | [*-nt]
      load guards gm < M, gk < K, bn < N   M = 1, 17, 65, 130; every K and N that is no multiple of 64
      prefetch k0 + 64 < K             K = 65 .. 200 (2 .. 4 chunks); ksteps < 64: K % 64 != 0; K % 4 != 0: zero-filled k
      col >= N, row >= M in the epilogue   as the load guards
      bias, relu, dropout, residual, mask_ids, accumulate   test_rows_epilogues[0]: all 64 combinations, row_offset 900, ldc != N, ldr != ldc
      blockIdx.x >= tiles (early return), blockIdx.y   test_rows_batched[0]; test_rows_dispatch (mixed precisions -> this kernel)
  k_gemm_rows_bf<true> | <false>       test_rows_shapes[1-*] | [2-*] at K, N >= 8; test_rows_epilogues[1] | [2]
      !trans_b (row_frag_perm + tr_frag) | trans_b (row_frag)   [*-nn] | [*-nt]
      stage_issue / stage_put: rok false (rows past M, K or N)   M, N, K no multiple of 64
      item_issue c >= d (whole chunk past the tile's width)      widths 8 .. 56 of the last tile
      chunk crossing d, read into the next row and masked        widths that are no multiple of 8, rows but the last
      item_fix -> d - 8 and item_refill (last row's partial chunk)   the same widths, last row of A (M - 1), of B (K - 1 | N - 1)
      d < 8 behind a full tile (d - 8 reaches into the tile before)   N or K = 65, 67, 71, 129: as N [*-nn] B's columns; as K A's chunk
                                       and, [*-nt], B's; both at N = K = 67
      ksteps 1 | 2                     K % 64 in 1 .. 32 | else;  k0 + 64 < K prefetch: K >= 65;  `if (k0) __syncthreads`: the same
      epilogue flags                   test_rows_epilogues[1] | [2]
      blockIdx.x >= tiles, blockIdx.y  test_rows_batched[1] | [2]: 1, 2, 6 and 9 tiles in one launch
  k_gemm_wgrad                         test_wgrad_forms[0]; test_wgrad_batched[0] (the walk over the tile counts)
      mb >= me (slab without rows)     n_slabs = M + 3, and 5 at M = 1; prefetch mc + 32 < me: M = 64, 97, 300 in one slab
      k0 == 0 column sums, db == NULL  K = 67, 136 have tiles with k0 != 0; [*]: db present and NULL
      krow < K, col < N, ldw           every (K, N); ldw = N and N + 11
      pi >= batch.n                    never true: the grid is exactly the batch's tile count (read in cr_gemm_wgrad); the same in the bf16 form
  k_gemm_wgrad_bf<true> | <false>      test_wgrad_forms[1] | [2]; test_wgrad_batched[1] | [2]
      as k_gemm_wgrad; msteps 1 | 2: slab rows % 64 in 1 .. 32 | else; rows past `me` zero-filled (the next slab's): n_slabs = 5
      `mc != mb` barrier and the mc + 64 < me prefetch: M = 97, 300 in one slab (2 and 5 chunks)
      K and N tiles narrower than 8 behind a full one: K = 67, N = 65, 71; the fold of the four waves' column sums: db present
  stage_tile (cr_gemm_bf.hip)          not instantiated by any kernel of the file (stage_issue + stage_put are its two halves)
  host checks of both entry points     test_rejects; n_problems = 5: test_rows_batched
  cr_gemm_rows_bf_supported / cr_gemm_wgrad_bf_supported   test_rows_dispatch; the K, N < 8 cases of test_rows_shapes[1-*], [2-*]"""
import numpy as np
import pytest
import torch

import gemm_ref as G
from ops_harness import SENTINEL, Pad, dev, new_state

pytestmark = pytest.mark.gpu

F64 = np.float64
PRECS = pytest.mark.parametrize("prec", [0, 1, 2])
ORIENT = pytest.mark.parametrize("trans_b", [False, True], ids=["nn", "nt"])


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


class Fails(list):
    """the failing cases of one test, and the largest error / bound it saw (printed in front of the assertion)"""
    top = 0.0

    def report(self, what):
        print("%s: largest error / bound %.3f" % (what, self.top))
        assert not self, "%d failed:\n%s" % (len(self), "\n".join(self[:40]))


def outside(got, ref, allow, what, fails):
    """appends "what: count, worst element, error / bound" when an element is outside its bound (a NaN -- never written -- is)"""
    err = np.abs(np.asarray(got, F64) - ref)
    bad = ~(err <= allow)
    fails.top = max(fails.top, float(np.nan_to_num(np.where(err == 0, 0.0, err / (allow + 1e-300)), nan=np.inf).max()))
    if bad.any():
        ratio = np.where(bad, np.nan_to_num(err / (allow + 1e-300), nan=np.inf), 0)
        i = np.unravel_index(np.argmax(ratio), err.shape)
        fails.append("%s: %d of %d outside; worst at %s got %r, reference %r, error / bound %.3g" % (
            what, int(bad.sum()), bad.size, i, float(np.asarray(got)[i]), float(ref[i]), float(ratio[i])))


def bits(t):
    return t.view(torch.int32)


class Rows:
    """the device side of one gemm_ref.rows_case: operands and output in Pads one float past the boundary, and the descriptor"""

    def __init__(self, ops, c, prec, trans_b):
        self.c, M, N, K = c, c.M, c.N, c.K
        self.A = Pad(M, c.lda, [(0, K)], c.A, lead=1)
        self.B = Pad(N, c.ldbt, [(0, K)], np.ascontiguousarray(c.B.T), lead=1) if trans_b else Pad(K, c.ldb, [(0, N)], c.B, lead=1)
        self.C = Pad(M, c.ldc, [(0, N)], c.C0 if c.accumulate else None, lead=1)
        self.bias = Pad(1, N, [(0, N)], c.bias, lead=1) if c.bias is not None else None
        self.R = Pad(M, c.ldr, [(0, N)], c.residual, lead=1) if c.residual is not None else None
        self.mask = dev(c.mask_ids, torch.int32) if c.mask_ids is not None else None
        self.state = new_state(step=c.step)
        rng = ops.Drop(c.rate, c.seed, self.state, c.row_offset).rng(c.site) if c.rate > 0 else ops.NO_DROP
        self.desc = ops.gemm_desc(self.A.t, c.lda, self.B.t, c.ldbt if trans_b else c.ldb, self.C.t, c.ldc, M, N, K,
                                  bias=self.bias.t if self.bias else None, trans_b=trans_b, relu=c.relu, rng=rng,
                                  residual=self.R.t if self.R else None, ldr=c.ldr, mask_ids=self.mask, accumulate=c.accumulate, precision=prec)

    def check(self, prec, exact, matched, what, fails, inputs=False):
        c, got = self.c, self.C.read()
        form = G.form_of(prec, c.K, c.N)
        outside(got, exact[0], G.rows_bound(c, exact, form), what + " against the exact product", fails)
        if form == "bf16":
            outside(got, matched[0], G.rows_bound(c, matched, form, matched=True), what + " against the matched model", fails)
        if not self.C.untouched():
            fails.append(what + ": words outside C[M, N] were written")
        if inputs and not all(p.untouched() for p in (self.A, self.B, self.bias, self.R) if p is not None):
            fails.append(what + ": an input's pad was written")


# ------------------------------------------------------------------------------------------------ cr_gemm_rows
@ORIENT
@PRECS
def test_rows_shapes(ops, prec, trans_b):
    """the shape sweep with bias, relu, residual and row mask on"""
    fails = Fails()
    for M, N, K in G.SHAPES:
        c, exact, matched = G.rows_refs(M, N, K)
        r = Rows(ops, c, prec, trans_b)
        ops.gemm_rows([r.desc])
        r.check(prec, exact, matched, "M %d N %d K %d" % (M, N, K), fails)
    fails.report("rows, precision %d, %s" % (prec, "A B^T" if trans_b else "A B"))


@PRECS
def test_rows_epilogues(ops, prec):
    """all 64 combinations of bias / relu / dropout / residual / mask / accumulate at M = 130, N = 67, K = 72, both orientations;
    dropout with row_offset 900 and ldc != N: a mask indexed by the pitch is another mask"""
    fails = Fails()
    for flags in G.EPILOGUES:
        c, exact, matched = G.rows_refs(*G.EPI_SHAPE, *flags, 900)
        for trans_b in (False, True):
            r = Rows(ops, c, prec, trans_b)
            ops.gemm_rows([r.desc])
            r.check(prec, exact, matched, "bias %d relu %d drop %d res %d mask %d acc %d %s" % (flags + ("nt" if trans_b else "nn",)), fails, inputs=True)
    fails.report("epilogues, precision %d" % prec)


def batched_rows(ops, precs):
    return [Rows(ops, G.rows_refs(M, N, K, *flags, 900)[0], p, t) for p, (M, N, K, t, *flags) in zip(precs, G.BATCHED)]


@PRECS
def test_rows_batched(ops, prec):
    """CR_MAX_BATCH problems of 1, 2, 6 and 9 tiles in one launch (a grid of 9 x 4: the smaller problems' surplus workgroups return)"""
    fails = Fails()
    together, alone = batched_rows(ops, [prec] * 4), batched_rows(ops, [prec] * 4)
    ops.gemm_rows([r.desc for r in together])
    for i, (r, s) in enumerate(zip(together, alone)):
        ops.gemm_rows([s.desc])
        M, N, K, t, *flags = G.BATCHED[i]
        _, exact, matched = G.rows_refs(M, N, K, *flags, 900)
        r.check(prec, exact, matched, "problem %d" % i, fails, inputs=True)
        if not torch.equal(bits(r.C.whole), bits(s.C.whole)):
            fails.append("problem %d: the batched launch and the launch alone differ" % i)
    fails.report("batched rows, precision %d" % prec)
    five = batched_rows(ops, [prec] * 4)
    with pytest.raises(RuntimeError, match=r"n_problems=5 out of \[1,4\]"):
        ops.gemm_rows([r.desc for r in five] + [five[0].desc])
    torch.cuda.synchronize()
    assert all(bool((bits(r.C.whole) == bits(a.C.whole)).all()) for r, a in zip(five, batched_rows(ops, [prec] * 4)))      # nothing ran


def test_rows_dispatch(ops):
    """what cr_gemm_rows_bf_supported declines is computed by the exact fp32 kernel: the bits of precision 0"""
    mixed, plain = batched_rows(ops, [0, 1, 2, 1]), batched_rows(ops, [0] * 4)
    ops.gemm_rows([r.desc for r in mixed])
    ops.gemm_rows([r.desc for r in plain])
    for i, (r, s) in enumerate(zip(mixed, plain)):
        assert torch.equal(bits(r.C.whole), bits(s.C.whole)), "mixed precisions, problem %d" % i
    mixed, split = batched_rows(ops, [1, 2, 1, 1]), batched_rows(ops, [1] * 4)           # no precision 0 in it, still fp32
    ops.gemm_rows([r.desc for r in mixed])
    ops.gemm_rows([r.desc for r in split])
    for i, (r, s) in enumerate(zip(mixed, plain)):
        assert torch.equal(bits(r.C.whole), bits(s.C.whole)), "precisions 1 2 1 1, problem %d" % i
    assert not torch.equal(bits(split[3].C.whole), bits(plain[3].C.whole))              # (the split form's bits are others)
    for n in G.SMALL:
        for M, N, K in ((17, n, 64), (17, 64, n), (65, n, n)):
            for trans_b in (False, True):
                c = G.rows_refs(M, N, K)[0]
                got = [Rows(ops, c, p, trans_b) for p in (0, 1, 2)]
                for r in got:
                    ops.gemm_rows([r.desc])
                assert torch.equal(bits(got[1].C.whole), bits(got[0].C.whole)) and torch.equal(bits(got[2].C.whole), bits(got[0].C.whole)), (M, N, K)


# ------------------------------------------------------------------------------------------------ cr_gemm_wgrad
GAP = 3                        # sentinel words between a slab's [K, ldw] and [N] regions


class Slabs:
    """n_slabs slabs of `stride` floats one float past the boundary, all SENTINEL, kept and checked on the device.  layout: per
    problem (K, N, ldw) a [K, ldw] region, GAP words, an [N] region, GAP words."""

    def __init__(self, n_slabs, problems):
        self.ns, self.problems, self.off = n_slabs, problems, []
        o = 0
        for K, N, ldw in problems:
            self.off.append((o, o + K * ldw + GAP))
            o += K * ldw + GAP + N + GAP
        self.stride = (o + 5) | 1
        self.whole = torch.full((1 + n_slabs * self.stride + 9,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.whole[1:]
        self.body = self.t[:n_slabs * self.stride].view(n_slabs, self.stride)

    def dW(self, i):
        K, N, ldw = self.problems[i]
        return self.body[:, self.off[i][0]:self.off[i][0] + K * ldw].view(self.ns, K, ldw)[:, :, :N]

    def db(self, i):
        return self.body[:, self.off[i][1]:self.off[i][1] + self.problems[i][1]]

    def ptr(self, i):
        return self.t[self.off[i][0]:], self.t[self.off[i][1]:]

    def outside_untouched(self, written_db):
        """every word outside the [K, N] regions (and the [N] regions of the problems in written_db) still holds SENTINEL"""
        keep = torch.ones_like(self.whole, dtype=torch.bool)
        inner = keep[1:1 + self.ns * self.stride].view(self.ns, self.stride)
        for i, (K, N, ldw) in enumerate(self.problems):
            inner[:, self.off[i][0]:self.off[i][0] + K * ldw].view(self.ns, K, ldw)[:, :, :N] = False
            if i in written_db:
                inner[:, self.off[i][1]:self.off[i][1] + N] = False
        return bool((bits(self.whole)[keep] == SENTINEL).all())


def check_wgrad(sl, i, c, prec, refs, n_slabs, has_db, what, fails):
    exact, matched = refs
    form = G.form_of(prec, c.K, c.N)
    W, b = sl.dW(i), sl.db(i)
    if bool((bits(W) == SENTINEL).any()) or (has_db and bool((bits(b) == SENTINEL).any())):
        fails.append(what + ": a slab word inside [K, N] / [N] was not written")
        return
    empty = [s for s, (m0, m1) in enumerate(G.slab_rows(c.M, n_slabs)) if m0 == m1]
    if empty and (bool((W[empty] != 0).any()) or (has_db and bool((b[empty] != 0).any()))):
        fails.append(what + ": a slab without rows is not zero")
    dW = W.double().sum(0).cpu().numpy()
    db = b.double().sum(0).cpu().numpy() if has_db else None
    for ref, m in ((exact, False), (matched, True)) if form == "bf16" else ((exact, False),):
        bW, bb = G.wgrad_bound(c, ref, form, matched=m)
        tag = what + (" against the matched model" if m else " against the exact product")
        outside(dW, ref[0], bW, tag + ", dW", fails)
        if has_db:
            outside(db, ref[2], bb, tag + ", db", fails)


@PRECS
def test_wgrad_forms(ops, prec):
    """(K, N) x M x n_slabs x ldw x db: the fp64 sum of the slabs per element, no sentinel left inside, none lost outside, slabs
    without rows exact zeros, a second launch into fresh buffers bit-identical"""
    fails = Fails()
    for K, N in G.WGRAD_KN:
        for M in G.WGRAD_M:
            c, exact, matched = G.wgrad_refs(M, N, K)
            A, Gm = Pad(M, c.lda, [(0, K)], c.A, lead=1), Pad(M, c.ldg, [(0, N)], c.G, lead=1)
            for name in G.WGRAD_SLABS:
                ns = G.n_slabs_of(name, M)
                for ldw in (N, N + 11):
                    for has_db in (True, False):
                        what = "K %d N %d M %d slabs %s ldw %d db %d" % (K, N, M, name, ldw, has_db)
                        runs = []
                        for _ in range(2):
                            sl = Slabs(ns, [(K, N, ldw)])
                            dW, db = sl.ptr(0)
                            ops.gemm_wgrad([ops.wgrad_desc(A.t, c.lda, Gm.t, c.ldg, dW, db if has_db else None, M, N, K, ldw=ldw, precision=prec)], sl.stride, ns)
                            runs.append(sl)
                        check_wgrad(runs[0], 0, c, prec, (exact, matched), ns, has_db, what, fails)
                        if not runs[0].outside_untouched([0] if has_db else []):
                            fails.append(what + ": words outside the slab regions were written")
                        if not torch.equal(bits(runs[0].whole), bits(runs[1].whole)):
                            fails.append(what + ": two launches differ")
            if not (A.untouched() and Gm.untouched()):
                fails.append("K %d N %d M %d: an input's pad was written" % (K, N, M))
    fails.report("weight gradient, precision %d" % prec)


@PRECS
def test_wgrad_batched(ops, prec):
    """three problems of different (M, K, N) in one launch over one grid of slabs: each the bits of its launch alone"""
    fails = Fails()
    ns = G.WGRAD_BATCHED_SLABS
    problems = [(K, N, N + 11 * (i % 2)) for i, (M, N, K) in enumerate(G.WGRAD_BATCHED)]
    cases = [G.wgrad_refs(M, N, K) for M, N, K in G.WGRAD_BATCHED]
    pads = [(Pad(c.M, c.lda, [(0, c.K)], c.A, lead=1), Pad(c.M, c.ldg, [(0, c.N)], c.G, lead=1)) for c, _, _ in cases]

    def descs(sl, which):
        return [ops.wgrad_desc(pads[i][0].t, cases[i][0].lda, pads[i][1].t, cases[i][0].ldg, *sl.ptr(i), cases[i][0].M, cases[i][0].N,
                               cases[i][0].K, ldw=problems[i][2], precision=prec) for i in which]
    together = Slabs(ns, problems)
    ops.gemm_wgrad(descs(together, range(3)), together.stride, ns)
    if not together.outside_untouched([0, 1, 2]):
        fails.append("words outside the slab regions were written")
    for i, (c, exact, matched) in enumerate(cases):
        check_wgrad(together, i, c, prec, (exact, matched), ns, True, "problem %d" % i, fails)
        alone = Slabs(ns, problems)
        ops.gemm_wgrad(descs(alone, [i]), alone.stride, ns)
        if not (torch.equal(bits(alone.dW(i)), bits(together.dW(i))) and torch.equal(bits(alone.db(i)), bits(together.db(i)))):
            fails.append("problem %d: the batched launch and the launch alone differ" % i)
        if not alone.outside_untouched([i]):
            fails.append("problem %d alone: words outside its regions were written" % i)
    fails.report("batched weight gradient, precision %d" % prec)


# ------------------------------------------------------------------------------------------------ what the host refuses
def test_rejects(ops):
    """every refusal comes from the host checks in front of the launch (cr_gemm.hip: CR_REQUIRE returns before hipLaunchKernelGGL); the
    outputs still hold their sentinels afterwards"""
    M, N, K = 17, 33, 9
    c = G.rows_refs(M, N, K)[0]
    w = G.wgrad_refs(M, N, K)[0]
    outs = []

    def rows(trans_b=False, **over):
        r = Rows(ops, c, 0, trans_b)
        outs.append(r.C)
        for k, v in over.items():
            setattr(r.desc, k, v)
        ops.gemm_rows([r.desc])

    def wgrad(n_slabs=2, **over):
        A, Gm, sl = Pad(M, w.lda, [(0, K)], w.A, lead=1), Pad(M, w.ldg, [(0, N)], w.G, lead=1), Slabs(2, [(K, N, N)])
        outs.append(sl)
        d = ops.wgrad_desc(A.t, w.lda, Gm.t, w.ldg, *sl.ptr(0), M, N, K)
        for k, v in over.items():
            setattr(d, k, v)
        ops.gemm_wgrad([d], sl.stride, n_slabs)

    for call, kw, msg in [(rows, dict(lda=K - 1), r"cr_gemm_rows\[0\]: leading dimension too small"),
                          (rows, dict(ldc=N - 1), r"cr_gemm_rows\[0\]: leading dimension too small"),
                          (rows, dict(ldb=N - 1), r"cr_gemm_rows\[0\]: ldb too small"),
                          (rows, dict(trans_b=True, ldb=K - 1), r"cr_gemm_rows\[0\]: ldb too small"),
                          (rows, dict(A=None), r"cr_gemm_rows\[0\]: NULL pointer"),
                          (rows, dict(B=None), r"cr_gemm_rows\[0\]: NULL pointer"),
                          (rows, dict(C=None), r"cr_gemm_rows\[0\]: NULL pointer"),
                          (rows, dict(M=0), r"cr_gemm_rows\[0\]: bad shape 0x33x9"),
                          (rows, dict(K=0), r"cr_gemm_rows\[0\]: bad shape 17x33x0"),
                          (rows, dict(precision=3), r"cr_gemm_rows\[0\]: unknown precision 3"),
                          (rows, dict(precision=-1), r"cr_gemm_rows\[0\]: unknown precision -1"),
                          (wgrad, dict(lda=K - 1), r"cr_gemm_wgrad\[0\]: leading dimension too small"),
                          (wgrad, dict(ldg=N - 1), r"cr_gemm_wgrad\[0\]: leading dimension too small"),
                          (wgrad, dict(ldw=N - 1), r"cr_gemm_wgrad\[0\]: leading dimension too small"),
                          (wgrad, dict(G=None), r"cr_gemm_wgrad\[0\]: NULL pointer"),
                          (wgrad, dict(dW=None), r"cr_gemm_wgrad\[0\]: NULL pointer"),
                          (wgrad, dict(N=0), r"cr_gemm_wgrad\[0\]: bad shape"),
                          (wgrad, dict(n_slabs=0), r"cr_gemm_wgrad: bad slab geometry"),
                          (wgrad, dict(precision=3), r"cr_gemm_wgrad\[0\]: unknown precision 3"),
                          (wgrad, dict(precision=7), r"cr_gemm_wgrad\[0\]: unknown precision 7")]:
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert all(o.untouched() if isinstance(o, Pad) else o.outside_untouched([]) and bool((bits(o.dW(0)) == SENTINEL).all()) for o in outs)

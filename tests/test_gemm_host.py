"""tests/gemm_ref.py on the CPU: the fp64 references of cr_gemm_rows / cr_gemm_wgrad agree with torch autograd in fp64, a CPU
emulation of each arithmetic (the fp32 fmaf chain in k order, the split and plain bf16 products through bf16_rne) stays inside the
bound stated for it on every generated case -- the proof that a kernel computing exactly what castrec.h says passes -- the dispatch
of cr_gemm.hip restated in Python sends each named case to the kernel it is named for, and every premise the cases of
tests/test_gemm_gpu.py rest on holds on the generated inputs themselves."""
import numpy as np
import pytest
import torch

import gemm_ref as G
from row_ops_ref import wide

F64 = np.float64
FORMS = ["f32", "x3", "bf16"]


def close(got, want, tol=1e-12):
    want = np.asarray(want, F64)
    assert np.abs(np.asarray(got, F64) - want).max() <= tol * max(np.abs(want).max(), 1e-300)


def worst(got, ref, allow):
    """largest error / bound (0 / 0 counts as 0: an element that must be exact and is)"""
    err = np.abs(np.asarray(got, F64) - ref)
    return float(np.where(err == 0, 0.0, err / np.maximum(allow, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("flags", [(True,) * 6, (True, True, True, True, True, False), (False,) * 6])
def test_rows_ref_against_autograd(flags):
    """forward, and the two gradients of its product: cr_gemm_wgrad's reference is d/dB, the trans_b form's d/dA"""
    M, N, K = G.EPI_SHAPE
    c = G.rows_case(M, N, K, *flags, row_offset=900)
    t = lambda a: torch.tensor(wide(a), requires_grad=True)
    A, B = t(c.A), t(c.B)
    P = A @ B
    v = P + torch.tensor(wide(c.bias)) if c.bias is not None else P
    v = torch.relu(v) if c.relu else v
    v = v * torch.tensor(G.factor(c))
    v = v + torch.tensor(wide(c.residual)) if c.residual is not None else v
    v = v * torch.tensor((c.mask_ids != 0).astype(F64))[:, None] if c.mask_ids is not None else v
    v = v + torch.tensor(wide(c.C0)) if c.accumulate else v
    ref, S, n, Sp = G.rows_ref(c)
    close(ref, v.detach().numpy())
    assert n == K + sum(flags[i] for i in (0, 3, 5))
    assert (S >= np.abs(ref) - 1e-12).all() and (Sp <= S + 1e-12).all()
    w = G.wgrad_case(M, N, K)
    P.backward(torch.tensor(wide(w.G)))
    # d/dB of sum(G * (A B)) = A^T G: the weight gradient of the forward on case c's A
    w2 = G.types.SimpleNamespace(**{**w.__dict__, "A": c.A})
    dW, SW, db, Sb = G.wgrad_ref(w2)
    close(dW, B.grad.numpy())
    close(db, wide(w.G).sum(0))
    assert (SW >= np.abs(dW) - 1e-12).all() and (Sb >= np.abs(db) - 1e-12).all()
    # d/dA = G B^T: a trans_b problem with A := G [M, N] and B := this B [K, N], no epilogue
    d = G.types.SimpleNamespace(**{**G.rows_case(M, K, N, False, False, False, False, False, False).__dict__, "A": w.G, "B": np.ascontiguousarray(c.B.T)})
    close(G.rows_ref(d)[0], A.grad.numpy())


def test_matched_model_is_the_rounded_product():
    c = G.rows_case(17, 33, 67, False, False, False, False, False, False)
    r = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    close(G.rows_ref(c, matched=True)[0], r(c.A) @ r(c.B))
    hi, lo = G.split(c.A)
    x = wide(c.A)
    assert (np.abs(x - hi) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(x - hi - lo) <= 2.0 ** -16 * np.abs(x)).all()      # 8 significant bits, twice


# ------------------------------------------------------------------------------------------------ the emulation inside the bounds
def rows_ratio(c, exact, matched, form):
    got = G.emu_rows(c, form)
    w = worst(got, exact[0], G.rows_bound(c, exact, form))
    if form == "bf16":
        w = max(w, worst(got, matched[0], G.rows_bound(c, matched, form, matched=True)))
    return w


@pytest.mark.parametrize("form", FORMS)
def test_emulation_inside_bound_shapes(form):
    """every shape of the sweep, epilogue as test_rows_shapes runs it; a shape with K or N below 8 is emulated in the form the
    dispatch gives it (fp32)"""
    prec = FORMS.index(form)
    top = 0.0
    for M, N, K in G.SHAPES:
        c, exact, matched = G.rows_refs(M, N, K)
        top = max(top, rows_ratio(c, exact, matched, G.form_of(prec, K, N)))
    print("largest emulated error / bound, %s: %.3f" % (form, top))
    assert top <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_emulation_inside_bound_epilogues(form):
    top = 0.0
    for flags in G.EPILOGUES:
        c, exact, matched = G.rows_refs(*G.EPI_SHAPE, *flags, 900)
        top = max(top, rows_ratio(c, exact, matched, form))
    assert top <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_emulation_inside_bound_wgrad(form):
    prec = FORMS.index(form)
    top = 0.0
    for K, N in G.WGRAD_KN:
        for M in G.WGRAD_M:
            c, exact, matched = G.wgrad_refs(M, N, K)
            for name in G.WGRAD_SLABS:
                dW, db = G.emu_wgrad(c, G.form_of(prec, K, N), G.n_slabs_of(name, M))
                dW, db = dW.astype(F64).sum(0), db.astype(F64).sum(0)
                for ref, m in ((exact, False), (matched, True)) if form == "bf16" else ((exact, False),):
                    bW, bb = G.wgrad_bound(c, ref, form, matched=m)
                    top = max(top, worst(dW, ref[0], bW), worst(db, ref[2], bb))
    assert top <= 1.0


def test_bounds_have_no_room_for_the_named_defects():
    """what the GPU tests must notice, on the CPU: a dropped al * bh product of the split form, a column of a narrow last tile
    lost, and a dropout mask indexed by the pitch instead of N each leave the bound by a wide margin"""
    M, N, K = G.EPI_SHAPE
    c, exact, _ = G.rows_refs(M, N, K, False, False, False, False, False, False, 900)
    (ah, al), (bh, bl) = G.split(c.A), G.split(c.B)
    no_lo_hi = ah @ bh + ah @ bl
    allow = G.rows_bound(c, exact, "x3")
    assert worst(no_lo_hi, exact[0], allow) > 10 and (np.abs(no_lo_hi - exact[0]) > allow).mean() > 0.5      # most elements, not one
    lost = exact[0].copy()
    lost[:, N - 1] -= wide(c.A)[:, K - 1] * wide(c.B)[K - 1, N - 1]       # one k of the last column
    assert worst(lost, exact[0], G.rows_bound(c, exact, "x3")) > 20
    d, dexact, _ = G.rows_refs(M, N, K, True, True, True, True, True, False, 900)
    wrong = G.types.SimpleNamespace(**{**d.__dict__, "N": d.ldc})          # the mask of an [M, ldc] matrix, its first N columns
    f_wrong = G.factor(wrong)[:, :N]
    assert (f_wrong != G.factor(d)).mean() > 0.2


# ------------------------------------------------------------------------------------------------ dispatch
def test_dispatch_restated():
    assert G.kernel_of([(0, 64, 64)]) == "k_gemm_rows"
    assert G.kernel_of([(1, 64, 64)]) == "k_gemm_rows_bf<true>" and G.kernel_of([(2, 8, 8)]) == "k_gemm_rows_bf<false>"
    assert G.kernel_of([(1, 64, 64), (2, 64, 64)]) == "k_gemm_rows"                     # mixed precision: exact fp32
    assert G.kernel_of([(1, 64, 64), (0, 64, 64), (2, 64, 64)]) == "k_gemm_rows"
    assert G.kernel_of([(2, 64, 64), (2, 7, 64)]) == "k_gemm_rows" and G.kernel_of([(1, 64, 7)]) == "k_gemm_rows"
    assert G.kernel_of([(2, 9, 8)] * 3, "wgrad") == "k_gemm_wgrad_bf<false>" and G.kernel_of([(1, 9, 7)], "wgrad") == "k_gemm_wgrad"
    for prec in (1, 2):
        for M, N, K in G.SHAPES:                                                       # the sweep: fp32 exactly where a dimension is in SMALL
            assert (G.form_of(prec, K, N) == "f32") == (K in G.SMALL or N in G.SMALL)
        assert G.form_of(prec, G.EPI_SHAPE[2], G.EPI_SHAPE[1]) != "f32"
        assert "_bf" in G.kernel_of([(prec, b[2], b[1]) for b in G.BATCHED])
        assert "_bf" in G.kernel_of([(prec, K, N) for M, N, K in G.WGRAD_BATCHED], "wgrad")
        for K, N in G.WGRAD_KN:
            assert "_bf" in G.kernel_of([(prec, K, N)], "wgrad")
    assert G.kernel_of([(p, b[2], b[1]) for p, b in zip((0, 1, 2, 1), G.BATCHED)]) == "k_gemm_rows"


# ------------------------------------------------------------------------------------------------ premises
def narrow_behind_full(n):
    """a last tile (chunk) of fewer than 8 columns behind a full one: item_issue's d - 8 is negative"""
    return n > 64 and 0 < n % 64 < 8


def test_premises_shapes():
    assert [n for n in G.DIMS if narrow_behind_full(n)] == [65, 67, 71, 129]
    Ns, Ks, Ms = {s[1] for s in G.SHAPES}, {s[2] for s in G.SHAPES}, {s[0] for s in G.SHAPES}
    assert Ns == Ks == set(G.DIMS + G.SMALL) and Ms == set(G.M_ROWS)
    for n in G.DIMS + G.SMALL:                                  # every n as N and as K, against a narrow, a full and a tile + 3 partner
        for o in G.OTHER:
            for M in G.M_ROWS:
                assert (M, n, o) in G.SHAPES and (M, o, n) in G.SHAPES
    assert any(narrow_behind_full(N) and narrow_behind_full(K) for M, N, K in G.SHAPES)            # (67, 67): both at once
    assert max(Ks) > 192 and max(Ns) > 192                      # four K chunks, four column tiles
    assert any(M > 128 and N > 64 and K > 64 for M, N, K in G.SHAPES)       # more than one tile each way and more than one K chunk
    assert any(K % 32 not in (0,) and K > 32 for K in Ks) and any(K % 4 for K in Ks)
    M, N, K = G.EPI_SHAPE
    assert M > 128 and narrow_behind_full(N) and K > 64 and K % 32 == 8
    c = G.rows_case(M, N, K, row_offset=900)
    assert N < c.ldc < c.ldr and c.ldb > N and K < c.lda < c.ldbt and all(p % 2 for p in (c.lda, c.ldb, c.ldbt, c.ldc, c.ldr))
    assert [G.tiles(b[0], b[1]) for b in G.BATCHED] == [1, 2, 6, 9] and len(G.BATCHED) == G.MAX_BATCH
    assert {b[3] for b in G.BATCHED} == {False, True} and len({b[4:] for b in G.BATCHED}) == 4


def test_premises_epilogues():
    assert len(G.EPILOGUES) == 64 and len(set(G.EPILOGUES)) == 64
    for flags in G.EPILOGUES:
        c, exact, _ = G.rows_refs(*G.EPI_SHAPE, *flags, 900)
        if flags[2]:
            keep = (G.factor(c) != 0).mean()
            assert 0.6 < keep < 0.9 and c.row_offset == 900
        if flags[4]:
            assert 0 < (c.mask_ids != 0).sum() < c.M
        if flags[1]:
            pre = wide(c.A) @ wide(c.B) + (wide(c.bias) if flags[0] else 0.0)
            assert 0.2 < (pre < 0).mean() < 0.8
    c = G.rows_refs(*G.SHAPES[-1])[0]                                 # the shape sweep's epilogue: bias, relu, residual, mask
    assert c.bias is not None and c.relu and c.residual is not None and c.mask_ids is not None and c.rate == 0 and not c.accumulate
    for M, N, K in G.SHAPES:
        if M * N >= 64:
            c = G.rows_refs(M, N, K)[0]
            pre = wide(c.A) @ wide(c.B) + wide(c.bias)
            assert 0.2 < (pre < 0).mean() < 0.8, (M, N, K)


def test_premises_wgrad():
    assert any(narrow_behind_full(N) for K, N in G.WGRAD_KN) and any(narrow_behind_full(K) for K, N in G.WGRAD_KN)
    assert any(K > 128 for K, N in G.WGRAD_KN) and any(N > 64 for K, N in G.WGRAD_KN)
    assert all(K >= 8 and N >= 8 for K, N in G.WGRAD_KN)
    for M in G.WGRAD_M:
        rows = G.slab_rows(M, G.n_slabs_of("M+3", M))
        assert sum(b - a for a, b in rows) == M and sum(a == b for a, b in rows) >= 3          # at least one slab without rows
        assert all(b - a <= 1 for a, b in rows)
    rows = G.slab_rows(300, 1)
    assert rows == [(0, 300)]                                         # five 64-row chunks (bf16), ten 32-row chunks (fp32), a 44-row tail
    assert max(b - a for a, b in G.slab_rows(300, 5)) == 60 and max(b - a for a, b in G.slab_rows(97, 1)) == 97
    assert sum(a == b for a, b in G.slab_rows(1, 5)) == 4 and sum(a == b for a, b in G.slab_rows(31, 5)) == 0
    assert sum(a == b for a, b in G.slab_rows(G.WGRAD_BATCHED[1][0], G.WGRAD_BATCHED_SLABS)) == 2
    assert len({(N, K) for M, N, K in G.WGRAD_BATCHED}) == 3

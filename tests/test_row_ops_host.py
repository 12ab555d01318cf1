"""tests/row_ops_ref.py on the CPU: the fp64 references agree with torch autograd in fp64 (1e-12 relative, every option on), the
fp32 restatement of the LayerNorm stays about 1e-6 from fp64 on ordinary rows, and every premise the cases of
tests/test_row_ops_gpu.py rest on holds on the generated inputs themselves -- so a GPU case cannot pass because its input
missed the path it is named for."""
import numpy as np
import pytest
import torch

import row_ops_ref as R

F64 = np.float64


def close(got, want, tol=1e-12):
    want = np.asarray(want, F64)
    assert np.abs(np.asarray(got, F64) - want).max() <= tol * max(np.abs(want).max(), 1e-300)


# ------------------------------------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("D,M", [(5, 35), (13, 35), (66, 35)])
def test_embed_ref_against_autograd(D, M):
    c = R.embed_fwd_case(D, M, True)
    t = lambda a: torch.tensor(R.wide(a), requires_grad=True)
    table, pos, add = t(c.table), t(c.pos), t(c.addend)
    f = torch.tensor(R.row_factor(c, M, D))
    tz = torch.cat([torch.zeros(1, D, dtype=torch.float64), table[1:]], 0)
    out = (tz[torch.tensor(c.ids, dtype=torch.int64)] * c.scale + pos.repeat(M // c.T, 1) + add) * f
    ref, S, n = R.embed_ref(c)
    close(ref, out.detach().numpy())
    assert n == 3 and (S >= np.abs(ref) - 1e-12).all()
    # backward of the same graph, the gradient arriving as two partials
    b = R.embed_bwd_case(D, M, c.T, c.V, True, True)
    b.__dict__.update(ids=c.ids, mask_ids=c.mask_ids, seed=c.seed, step=c.step, site=c.site, row_offset=c.row_offset, scale=c.scale,
                      tg_start=None)
    out.backward(torch.tensor(R.wide(b.dout) + R.wide(b.out2)))
    r = R.embed_bwd_ref(b)
    close(r["table_grad"][0], table.grad.numpy())
    close(r["pos_grad"][0], pos.grad.numpy())
    close(r["d_addend"][0], add.grad.numpy())
    assert r["d_addend"][2] == 2 and r["pos_grad"][2] == 2 * (M // c.T)
    live = c.ids != 0
    assert np.array_equal(r["table_grad"][2][:, 0], 2 * np.bincount(c.ids[live], minlength=c.V))
    assert (r["table_grad"][0][0] == 0).all()                          # zero_pad: row 0 gets nothing


@pytest.mark.parametrize("D,M", [(1, 7), (6, 7), (17, 67), (65, 7)])
def test_layernorm_ref_against_autograd(D, M):
    c = R.ln_case(D, M)
    x, g, b = (torch.tensor(R.wide(a), requires_grad=True) for a in (c.x, c.gamma, c.beta))
    mean = x.mean(-1, keepdim=True); var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = g * ((x - mean) / (var + R.LN_EPS) ** 0.5) + b
    y.backward(torch.tensor(R.wide(c.dy)))
    r = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy)
    close(r.y, y.detach().numpy())
    for m in range(M):                                                  # per row: the zero row's 1e4 must not hide the others
        close(r.dx[m], x.grad.numpy()[m])
    close(r.dgamma, g.grad.numpy()); close(r.dbeta, b.grad.numpy())
    acc = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, c.dx0)
    close(acc.dx, R.wide(c.dx0) + x.grad.numpy())


@pytest.mark.parametrize("form", [f[0] for f in R.ELT_FORMS])
def test_eltwise_ref_against_torch(form):
    c = R.elt_case(form, 37, 50, True, True, False)
    x, y0 = torch.tensor(R.wide(c.x)), torch.tensor(R.wide(c.y0))
    aux = torch.tensor(R.wide(c.aux)) if c.aux is not None else None
    keep = torch.tensor(R.dr.rows_mask(c.seed, c.step, c.site, 0.25, 37, 50, c.row_offset))
    s = float(np.float32(1) / (np.float32(1) - np.float32(0.25)))
    v = {"copy": lambda: x, "rowmask": lambda: x, "add": lambda: x + aux, "relu_bwd": lambda: x * (aux > 0),
         "dropout": lambda: x * keep * s, "gradprep_regen": lambda: x * keep * s, "gradprep_aux": lambda: x * (aux > 0) * s}[form]()
    want = y0 + v * torch.tensor(c.mask_ids != 0)[:, None]
    got, S, n = R.eltwise_ref(c)
    close(got, want.numpy())
    assert n == (3 if form == "add" else 2)


def test_layernorm_fp32_restatement_on_ordinary_rows():
    for D in (6, 50, 200, 512):
        c = R.ln_case(D, 1)
        r32, r64 = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, fp32=True), R.layernorm_ref(c.x, c.gamma, c.beta, c.dy)
        for k in ("y", "dx"):
            e = np.abs(getattr(r32, k).astype(F64) - getattr(r64, k)).max() / np.abs(getattr(r64, k)).max()
            print("D=%d %s: fp32 restatement %.2e from fp64" % (D, k, e))
            assert e < 3e-6 and getattr(r32, k).dtype == np.float32


def test_layernorm_envelope_tells_formulas_apart():
    """what the bound is for: on the mean-1e3 row a one-pass variance E[x^2] - mean^2 in fp32 is orders of magnitude outside
    4 * E + 16 * u * max|y|, while the fp32 restatement summed in the other direction stays inside it"""
    c = R.ln_case(50, 7)
    r32, r64 = R.layernorm_ref(c.x, c.gamma, c.beta, fp32=True), R.layernorm_ref(c.x, c.gamma, c.beta)
    allow = R.ln_bound(r32.y, r64.y)
    x = c.x.astype(np.float32)
    mean = x.mean(1, keepdims=True, dtype=np.float32)
    var = np.maximum((x * x).mean(1, keepdims=True, dtype=np.float32) - mean * mean, 0)
    one_pass = c.gamma * ((x - mean) / np.sqrt(var + np.float32(1e-8))) + c.beta
    k = c.kinds.index("mean1e3")
    assert np.abs(one_pass.astype(F64) - r64.y)[k].max() > 10 * allow[k, 0]
    rev = R.layernorm_ref(c.x[:, ::-1], c.gamma[::-1], c.beta[::-1], fp32=True).y[:, ::-1]
    assert (np.abs(rev.astype(F64) - r64.y) <= allow).all()
    # dgamma: the rows' envelopes carried through the column sum hold the other summation order and reject the one-pass xhat
    b32, b64 = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, fp32=True), R.layernorm_ref(c.x, c.gamma, c.beta, c.dy)
    allow = R.ln_dgamma_bound(b32, b64, c.dy)
    rev = R.layernorm_ref(c.x[::-1, ::-1], c.gamma[::-1], c.beta[::-1], c.dy[::-1, ::-1], fp32=True).dgamma[::-1]
    assert (np.abs(rev.astype(F64) - b64.dgamma) <= allow).all()
    wrong = (c.dy * ((x - mean) / np.sqrt(var + np.float32(1e-8)))).sum(0, dtype=np.float32)
    assert (np.abs(wrong.astype(F64) - b64.dgamma) > 10 * allow).any()
    assert (allow < 1e-2 * np.abs(b64.dgamma_terms).max(0)).all()              # and a missing row is far outside it


def test_layernorm_special_row_errors():
    """E per kind of row at D = 50 (printed; recorded in the docstring of test_row_ops_gpu.test_layernorm_fwd)"""
    c = R.ln_case(50, 7)
    r32, r64 = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, fp32=True), R.layernorm_ref(c.x, c.gamma, c.beta, c.dy)
    for m, kind in enumerate(c.kinds):
        print("%-11s E(y) = %.2e  E(dx) = %.2e   max|y| = %.2e  max|dx| = %.2e" % (
            kind, np.abs(r32.y[m] - r64.y[m]).max(), np.abs(r32.dx[m] - r64.dx[m]).max(), np.abs(r64.y[m]).max(), np.abs(r64.dx[m]).max()))
    assert (r32.y[1] == r64.y[1]).all() and (r32.y[2] == r64.y[2]).all()          # zero and constant rows: y = beta exactly


# ------------------------------------------------------------------------------------------------ premises of the GPU cases
def dropout_and_mask_premises(c, M, N):
    if c.rate > 0:
        k = R.keep_fraction(c, M, N)
        assert (0.6 < k < 0.9) if M * N > 1 else k == 1.0, k
    if c.mask_ids is not None and M > 1:
        assert (c.mask_ids == 0).any() and (c.mask_ids != 0).any()


def covers_everything(*outputs):
    for v, S, n in outputs:
        assert np.isfinite(v).all() and np.isfinite(S).all() and (np.asarray(n) >= 0).all() and np.shape(S) == np.shape(v)


@pytest.mark.parametrize("D", R.EMBED_FWD_D)
def test_premises_embed_fwd(D):
    for M in R.EMBED_FWD_M:
        for full in (True, False):
            c = R.embed_fwd_case(D, M, full)
            assert c.ids.min() == 0 and c.ids.max() == c.V - 1 and M % c.T == 0
            assert len({D, c.ld_out, c.ld_add}) == 3 and c.ld_out >= c.col_off + D + 3
            dropout_and_mask_premises(c, M, D)
            out = R.embed_ref(c)
            covers_everything(out)
            assert out[0].shape == (M, D)
            if full:                                             # zeroed by the options and not: both present
                assert (out[0] == 0).any() and (out[0] != 0).any()


def test_premises_embed_bwd_large():
    cases = [R.bwd_pos_case(D, B, h) for (D, B) in R.BWD_POS for h in (False, True)]
    cases += [R.bwd_pos_case(50, 17, True, False)]
    cases += [R.bwd_rows16_case(D, M, T, h) for (D, M, T) in R.BWD_ROWS16 for h in (False, True)] + [R.bwd_rows16_case(*R.BWD_ROWS16_LOOP, True)]
    for c in cases:
        dropout_and_mask_premises(c, c.M, c.D)
        r = R.embed_bwd_ref(c)
        covers_everything(*r.values())
        assert c.ids.min() == 0 and c.ids.max() == c.V - 1 and len({c.D, c.ld_out, c.ld_add}) == 3
        assert ("pos_grad" in r) == c.want_pos and ("table_grad" in r) == c.want_table
        if c.want_table:
            assert c.tg_start is not None and (c.tg_start != 0).all()       # accumulates onto a non-zero start
            assert (r["table_grad"][0][0] == R.wide(c.tg_start)[0]).all()   # zero_pad
    # k_embed_bwd: B = 3 (u = 0 only), 17 (u = 1 for one wave), 70 (every u, and a second pass of the b0 loop: B > 64)
    assert {B for _, B in R.BWD_POS} == {3, 17, 70}
    # k_embed_bwd_rows16: 2048 workgroups x 16 rows per trip
    assert R.BWD_ROWS16_LOOP[1] > 2048 * 16


@pytest.mark.parametrize("D,V,M,T,ns,kind", R.SMALL)
def test_premises_embed_bwd_small(D, V, M, T, ns, kind):
    for has2 in (False, True):
        c = R.small_case(D, V, M, T, ns, has2)
        dropout_and_mask_premises(c, M, D)
        r = R.embed_bwd_ref(c)
        covers_everything(*r.values())
        assert c.tg_start is None and c.slab_stride > V * D and M % T == 0
        in_lds = V * D <= R.EMB_SMALL_MAX
        assert in_lds == (kind != "fallback")
        if kind == "owner":
            rps, windows, most = R.small_table_windows(c)
            assert D <= 64 and rps > 64 and windows >= 2 and most > 16, (rps, windows, most)
            assert np.isin(c.ids, (1, 5)).mean() > 0.55
        elif kind == "atomic":
            assert D > 64
        elif kind == "tiny":
            assert M < ns                                        # slabs without rows
    assert (5 * 9) % 4 != 0                                      # the slab tail
    assert 64 * 192 == 128 * 96 == R.EMB_SMALL_MAX               # on the boundary; one more row is past it


@pytest.mark.parametrize("D", R.LN_D)
def test_premises_layernorm(D):
    for M in R.LN_M:
        c = R.ln_case(D, M)
        r = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, c.dx0)
        r32 = R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, c.dx0, fp32=True)
        x = R.wide(c.x)
        for rows in (x, r.y):                                    # a flag is decidable: the sum is exactly 0 or far from it
            s, a = rows.sum(1), np.abs(rows).sum(1)
            assert ((s == 0) | (np.abs(s) > 1e-3 * a)).all(), (D, M)
        assert np.array_equal(r.x_nonzero, r32.x_nonzero) and np.array_equal(r.y_nonzero, r32.y_nonzero)
        assert [k == "zero" for k in c.kinds] == (r.x_nonzero == 0).tolist()
        if M == 7:
            assert set(c.kinds) == set(R.LN_KINDS)
            k = c.kinds.index("mean1e3")
            assert D == 1 or abs(x[k].mean()) > 300 * x[k].std()
        for t in (r.y, r.dx, r.dgamma, r.dbeta):
            assert np.isfinite(t).all()


@pytest.mark.parametrize("form", [f[0] for f in R.ELT_FORMS])
def test_premises_eltwise(form):
    for (M, N) in R.ELT_SHAPES:
        for masked in (False, True):
            c = R.elt_case(form, M, N, masked, True, False)
            dropout_and_mask_premises(c, M, N)
            covers_everything(R.eltwise_ref(c))
            assert (c.row_offset != 0) == (c.rate > 0)
            if c.aux is not None and M > 1:
                assert (c.aux > 0).any() and (c.aux <= 0).any()
    assert 2100 * 251 > 2048 * 256                               # a second trip of the grid-stride loop

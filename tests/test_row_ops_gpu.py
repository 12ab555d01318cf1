"""cr_embed_fwd / cr_embed_bwd (csrc/cr_embed.hip), cr_layernorm_fwd / cr_layernorm_bwd (csrc/cr_layernorm.hip) and cr_eltwise
(csrc/cr_eltwise.hip) against the fp64 numpy references of tests/row_ops_ref.py, element by element under the bounds derived there
(tests/test_row_ops_host.py checks the references and proves, on these very inputs, that each case reaches the path it is named for).
Every buffer a kernel writes is wider than what it may write, starts as a NaN with a payload, and must come back bit for bit outside
the written region: the columns left of col_off and right of col_off + D, the pad columns of every pitch, the slab words beyond V * D,
the words behind the last row.  Regions a call must write start as that NaN too.  All pitches of a call differ from each other and from D.

What reaches what:
  k_embed_fwd (scalar)                test_embed_fwd[1-*], [3-*] (D < 4); [260-*] (ceil(D/4) > 64)
  k_embed_fwd_vec<1|2|4|8>            [4-*] | [5-*], [8-*] | [13-*] | [20-*], [31-*]
  k_embed_fwd_vec<16|32|64>           [50-*], [64-*] | [66-*], [128-*] | [130-*], [256-*]
      rotated last chunk (D % 4 != 0): 5, 13, 31, 50, 66, 130; exact: 4, 8, 20, 64, 128, 256; `act` tails: M = 35, 1029 (no multiple
      of any rows-per-iteration); [*-full]: every option on; [*-bare]: zero_pad 0, no option
  k_embed_bwd<false|true>             test_embed_bwd_pos[D-B-one|two]: D 5 .. 512 (1 .. 8 columns per lane), B = 3 (u = 0 only), 17 (u = 1
                                      in one wave), 70 (every u and a second pass of the b0 loop); table_grad == NULL: test_embed_bwd_pos_no_table;
                                      D = 513 refused: test_embed_bwd_refuses_513; through the fallback: test_embed_bwd_small[128-97-*]
  k_embed_bwd_rows16<false|true>      test_embed_bwd_rows16[D-M-T-one|two]; its grid-stride loop: test_embed_bwd_rows16_grid_stride; through the fallback:
                                      test_embed_bwd_small[64-193-*]
  k_embed_bwd_small<false|true>       test_embed_bwd_small[D-V-M-T-ns-kind-one|two]
      owner waves (D <= 64), `while (todo)` more than once, two and more 64-row windows: kind "owner"; slab tail n % 4: [5-9-*];
      LDS atomics (D > 64): kind "atomic"; on the LDS boundary: [64-192-*], [128-96-*]; slabs without rows: [50-9-5-5-8-tiny-*]
  k_embed_zero_slabs + fallback       kind "fallback": [64-193-*], [128-97-*] (V * D = 12 288 + D)
  k_ln_fwd<16, 4> / <64, 8>           test_layernorm_fwd[D-M], D <= 64 / D = 65, 128, 200, 257, 512; D = 513: test_layernorm_refuses_513
  k_ln_bwd<16, 4> / <64, 8>           test_layernorm_bwd[D-M-slabs-acc]: n_slabs 1, 5, M + 3 (slabs without rows), accumulate off / on
  k_eltwise                           test_eltwise[form-M-N-mask-acc-place]: the six ops (CR_ELT_GRADPREP with the stored gate and with
                                      the regenerated mask), row mask, accumulate, y == x; [*-2100-251-*]: its grid-stride loop;
                                      dropout with row_offset 900
Dropout runs with row_offset != 0 in every case that has it (700 embedding, 900 element-wise)."""
import numpy as np
import pytest
import torch

import row_ops_ref as R
from ops_harness import SENTINEL, Pad, dev, new_state, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = np.float64


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


def within(got, ref, allow, what):
    err = np.abs(np.asarray(got, F64) - ref)
    bad = ~(err <= allow)                                   # a NaN (never written) is bad
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(err / (allow + 1e-300), nan=np.inf), 0)), err.shape)
        raise AssertionError("%s: %d of %d elements outside their bound; at %s got %r, reference %r, allowed %.3g" % (
            what, int(bad.sum()), bad.size, i, float(np.asarray(got)[i]), float(ref[i]), float(np.broadcast_to(allow, err.shape)[i])))


def rng_of(ops, c):
    state = new_state(step=c.step)
    return state, (ops.Drop(c.rate, c.seed, state, c.row_offset).rng(c.site) if c.rate > 0 else ops.NO_DROP)


# ------------------------------------------------------------------------------------------------ embedding forward
@pytest.mark.parametrize("full", [True, False], ids=["full", "bare"])
@pytest.mark.parametrize("M", R.EMBED_FWD_M)
@pytest.mark.parametrize("D", R.EMBED_FWD_D)
def test_embed_fwd(ops, D, M, full):
    c = R.embed_fwd_case(D, M, full)
    out = Pad(M, c.ld_out, [(c.col_off, D)])
    ids, table = dev(c.ids, torch.int32), dev(c.table)
    pos = dev(c.pos) if full else None
    add = Pad(M, c.ld_add, [(0, D)], c.addend) if full else None
    mask = dev(c.mask_ids, torch.int32) if full else None
    state, rng = rng_of(ops, c)
    ops.embed_fwd(ids, table, c.T, out.t, c.ld_out, col_off=c.col_off, zero_pad=bool(c.zero_pad), scale=c.scale, pos_table=pos,
                  addend=add.t if full else None, ld_add=c.ld_add, rng=rng, mask_ids=mask)
    torch.cuda.synchronize()
    ref, S, n = R.embed_ref(c)
    within(out.read(), ref, R.bound(S, n, R.R_EMBED_FWD), "out")
    assert out.untouched()
    if not full:
        assert np.array_equal(out.read(), c.table[c.ids])            # a bare gather copies


# ------------------------------------------------------------------------------------------------ embedding backward
def run_embed_bwd(ops, c):
    from castrec_amd import lib as L
    M, D, V = c.M, c.D, c.V
    dout = Pad(M, c.ld_out, [(c.col_off, D)], c.dout)
    out2 = Pad(M, c.ld_out, [(c.col_off, D)], c.out2) if c.out2 is not None else None
    ids, mask = dev(c.ids, torch.int32), dev(c.mask_ids, torch.int32)
    state, rng = rng_of(ops, c)
    f = L.EmbedDesc(ids.data_ptr(), None, M, c.T, D, V, c.zero_pad, c.scale, None, None, c.ld_add, rng, mask.data_ptr(), None,
                    c.ld_out, c.col_off)
    da = Pad(M, c.ld_add, [(0, D)])
    pg = Pad(c.T, D, [(0, D)]) if c.want_pos else None
    tg = None
    if c.n_slabs:
        tg = Pad(c.n_slabs, c.slab_stride, [(0, V * D)])
    elif c.want_table:
        tg = Pad(V, D, [(0, D)], c.tg_start)
    ops.embed_bwd(f, dout.t, table_grad=tg.t if tg else None, pos_grad=pg.t if pg else None, d_addend=da.t,
                  slab_stride=c.slab_stride, n_slabs=c.n_slabs, out2=out2.t if out2 else None)
    torch.cuda.synchronize()
    ref = R.embed_bwd_ref(c)
    v, S, n = ref["d_addend"]
    within(da.read(), v, R.bound(S, n, R.R_EMBED_G), "d_addend")
    assert da.untouched()
    if pg:
        v, S, n = ref["pos_grad"]
        within(pg.read(), v, R.bound(S, n, R.R_EMBED_G), "pos_grad")
        assert pg.untouched()
    if tg:
        v, S, n = ref["table_grad"]
        got = tg.read().astype(F64)
        if c.n_slabs:
            assert np.isfinite(got).all(), "a slab word below V * D was not written"
            got = got.sum(0)
        within(got.reshape(V, D), v, R.bound(S, n, R.R_EMBED_TABLE), "table_grad")
        assert tg.untouched()
    assert dout.untouched() and (out2 is None or out2.untouched())


TWO = pytest.mark.parametrize("has2", [False, True], ids=["one", "two"])


@TWO
@pytest.mark.parametrize("D,B", R.BWD_POS)
def test_embed_bwd_pos(ops, D, B, has2):
    run_embed_bwd(ops, R.bwd_pos_case(D, B, has2))


def test_embed_bwd_pos_no_table(ops):
    run_embed_bwd(ops, R.bwd_pos_case(50, 17, True, False))


def test_embed_bwd_refuses_513(ops):
    with pytest.raises(RuntimeError, match="D=513 > 512"):
        run_embed_bwd(ops, R.embed_bwd_case(513, 9, 3, 11, False, True))


@TWO
@pytest.mark.parametrize("D,M,T", R.BWD_ROWS16)
def test_embed_bwd_rows16(ops, D, M, T, has2):
    run_embed_bwd(ops, R.bwd_rows16_case(D, M, T, has2))


def test_embed_bwd_rows16_grid_stride(ops):
    run_embed_bwd(ops, R.bwd_rows16_case(*R.BWD_ROWS16_LOOP, True))


@TWO
@pytest.mark.parametrize("D,V,M,T,ns,kind", R.SMALL)
def test_embed_bwd_small(ops, D, V, M, T, ns, kind, has2):
    run_embed_bwd(ops, R.small_case(D, V, M, T, ns, has2))


# ------------------------------------------------------------------------------------------------ layer normalisation
def ln_refs(c, accumulate=False):
    dx0 = c.dx0 if accumulate else None
    return (R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, dx0, fp32=True), R.layernorm_ref(c.x, c.gamma, c.beta, c.dy, dx0))


@pytest.mark.parametrize("M", R.LN_M)
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_fwd(ops, D, M):
    """A row's bound is 4 * E + 16 * u * max|y|, E the deviation of the fp32 restatement from fp64 on that row.  E per kind of row at
    D = 50 (test_row_ops_host.test_layernorm_special_row_errors prints them):
        ordinary     E(y) 2.2e-07  E(dx) 7.2e-08 (max|dx| 1.0)      zero        E(y) 0        E(dx) 1.3e-03 (max|dx| 2.1e+04)
        constant     E(y) 0        E(dx) 2.1e-03 (max|dx| 5.2e+04)  mean1e3     E(y) 4.7e-04  E(dx) 3.7e-05 (max|dx| 3.0)
        spread1e-3   E(y) 4.0e-04  E(dx) 8.3e-02 (max|dx| 2.6e+03)  spike1e4    E(y) 3.1e-07  E(dx) 1.8e-10 (max|dx| 1.7e-03)
    A one-pass variance E[x^2] - mean^2 is off by ~0.1 on the mean1e3 row."""
    c = R.ln_case(D, M)
    x, y = Pad(M, D + 1, [(0, D)], c.x), Pad(M, D + 2, [(0, D)])
    xnz, ynz = Pad(M, 1, [(0, 1)]), Pad(M, 1, [(0, 1)])
    g, b = dev(c.gamma), dev(c.beta)
    ops.layernorm_fwd(x.t, D + 1, g, b, y.t, D + 2, M, D, x_nonzero=xnz.t, y_nonzero=ynz.t)
    torch.cuda.synchronize()
    r32, r64 = ln_refs(c)
    within(y.read(), r64.y, R.ln_bound(r32.y, r64.y), "y")
    assert np.array_equal(xnz.read()[:, 0], r64.x_nonzero) and np.array_equal(ynz.read()[:, 0], r64.y_nonzero)
    assert y.untouched() and xnz.untouched() and ynz.untouched() and x.untouched()
    if M != 7:                                                   # ordinary rows: the tensor-level bound of test_ops_gpu holds as well
        assert relerr(y.read(), r64.y) < 3e-6


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "acc"])
@pytest.mark.parametrize("slabs", ["1", "5", "M+3"])
@pytest.mark.parametrize("M", R.LN_M)
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_bwd(ops, D, M, slabs, accumulate):
    c = R.ln_case(D, M)
    ns = {"1": 1, "5": 5, "M+3": M + 3}[slabs]
    stride = 2 * D + 5
    x, dy = Pad(M, D + 1, [(0, D)], c.x), Pad(M, D + 3, [(0, D)], c.dy)
    dx = Pad(M, D + 4, [(0, D)], c.dx0 if accumulate else None)
    sl = Pad(ns, stride, [(0, D), (D + 2, D)])
    g = dev(c.gamma)
    ops.layernorm_bwd(x.t, D + 1, g, dy.t, D + 3, dx.t, D + 4, sl.t, sl.t[D + 2:], stride, ns, M, D, accumulate=accumulate)
    torch.cuda.synchronize()
    r32, r64 = ln_refs(c, accumulate)
    within(dx.read(), r64.dx, R.ln_bound(r32.dx, r64.dx), "dx")
    dg, db = sl.read(0).astype(F64), sl.read(1).astype(F64)
    assert np.isfinite(dg).all() and np.isfinite(db).all(), "a slab was not written"
    within(dg.sum(0), r64.dgamma, R.ln_dgamma_bound(r32, r64, c.dy), "dgamma")
    within(db.sum(0), r64.dbeta, R.ln_bound(r32.dbeta, r64.dbeta, np.abs(r64.dbeta_terms).max(0)), "dbeta")
    assert dx.untouched() and sl.untouched() and x.untouched() and dy.untouched()
    if M != 7:
        assert relerr(dx.read(), r64.dx) < 2e-5
        assert relerr(dg.sum(0), r64.dgamma) < 5e-6 and relerr(db.sum(0), r64.dbeta) < 5e-6


def test_layernorm_refuses_513(ops):
    M, D = 3, 513
    x, y, g = torch.zeros(M, D, device="cuda"), torch.zeros(M, D, device="cuda"), torch.ones(D, device="cuda")
    with pytest.raises(RuntimeError, match="D=513 > 512"):
        ops.layernorm_fwd(x, D, g, g, y, D, M, D)
    sl = torch.zeros(2 * D, device="cuda")
    with pytest.raises(RuntimeError, match="D=513 > 512"):
        ops.layernorm_bwd(x, D, g, x, D, y, D, sl, sl[D:], 2 * D, 1, M, D)


# ------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "acc"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
@pytest.mark.parametrize("M,N", R.ELT_SHAPES)
@pytest.mark.parametrize("form", [f[0] for f in R.ELT_FORMS])
def test_eltwise(ops, form, M, N, masked, accumulate, inplace):
    c = R.elt_case(form, M, N, masked, accumulate, inplace)
    x = Pad(M, N + 1, [(0, N)], c.x)
    aux = Pad(M, N + 2, [(0, N)], c.aux) if c.aux is not None else None
    y = x if inplace else Pad(M, N + 3, [(0, N)], c.y0 if accumulate else None)
    mask = dev(c.mask_ids, torch.int32) if masked else None
    state, rng = rng_of(ops, c)
    ops.eltwise(c.op, x.t, x.ld, y.t, y.ld, M, N, aux=aux.t if aux else None, ldaux=N + 2, rng=rng, mask_ids=mask, accumulate=accumulate)
    torch.cuda.synchronize()
    ref, S, n = R.eltwise_ref(c)
    got = y.read()
    if c.op in R.ELT_EXACT:
        assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32)), "not bit for bit"
    else:
        within(got, ref, R.bound(S, n, R.R_ELT[c.op]), "y")
    assert y.untouched() and x.untouched() and (aux is None or aux.untouched())

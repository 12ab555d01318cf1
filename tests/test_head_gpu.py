"""cr_head_fwd_bwd and cr_head_fwd_bwd_ln (csrc/cr_head.hip) against the fp64 autograd reference of tests/head_ref.py: every instantiation
of the three kernels at the smallest shapes that reach it, every output under the bound the suite already holds that quantity to
(logits, loss sum 2e-6; d_seq_emb, table gradient, coef_out 3e-6: test_head_fwd_bwd_and_test_logits; dx 2e-5, dgamma / dbeta summed over
the slabs 5e-6: test_layernorm_fwd_bwd -- all relative to the tensor's scale; a plain fp32 evaluation of the graph stays below 3e-7).

What reaches what (the dispatch of cr_head_fwd_bwd / cr_head_fwd_bwd_ln; "pitch" is ld, ldx, lddx and ldd together):
  k_head<16,4>  D 50          k_head<32,4>  D 72            k_head<64,8>  D 136, 260 (column slots 4..7), pitch D + 4
  k_head_ln<16,4>    D 50 pitch 52 with table_grad (the contiguous scatter); D 25 (odd)
  k_head_ln<32,4>    D 72 with table_grad (the strided scatter)
  k_head_ln<64,8>    D 260 with table_grad; D 130 (even, no multiple of 4, > 128: no vector form takes it)
  k_head_ln_v<16,4>  D 48 pitch 52      k_head_ln_v<32,4>  D 72 pitch 76      k_head_ln_v<64,4>  D 132, 256
  k_head_ln_v<16,2>  D 24 pitch 26      k_head_ln_v<32,2>  D 48 pitch 50      k_head_ln_v<64,2>  D 70
Rows: two workgroups of 2 * STEP + 3 rows, the last one row short (STEP = 16 * 64 / LPR rows per iteration of a workgroup: three iterations
and a ragged end use every stage of the vector form's pipeline) -- M = 261 / 133 / 69 at 16 / 32 / 64 lanes per row; and M = 5 on four
workgroups: two rows, two, one, none (its slab must be exact zeros, the state snapshot must still be taken).  k_head: M = 261 and 5.

Every output buffer starts as NaN: written elements must be finite, the pitch gap and the rows behind the last must still be NaN (a 16- or
8-byte store must not run over the row's end).  Inputs carry spare rows behind the last as well.  Each case launches twice: with every
optional output, and with d_seq_emb, the logits and coef_out NULL."""
import types

import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

SPARE = 4           # rows behind the last one of every row array


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


def relerr(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (np.abs(want).max() + 1e-30))


def rows_in(a, pitch):
    """a [M, D] as a device array of M + SPARE rows of `pitch` floats (gap and spare rows: finite junk the kernel has no business reading)"""
    M, D = a.shape
    h = np.full((M + SPARE, pitch), 3.0, np.float32)
    h[:M, :D] = a
    return torch.from_numpy(h).cuda()


def nan_rows(M, pitch):
    return torch.full((M + SPARE, pitch), float("nan"), device="cuda")


def written(buf, M, D):
    """the [M, D] block the kernel owns: all finite, everything else of the buffer still NaN"""
    g = buf.cpu().numpy()
    assert np.isfinite(g[:M, :D]).all(), "an owned element was not written"
    assert np.isnan(g[:M, D:]).all() and np.isnan(g[M:]).all(), "a store ran over the row's end or behind the last row"
    return g[:M, :D]


def case(ln, D, pitch, M, n_slabs=0, tg=False):
    return types.SimpleNamespace(ln=ln, D=D, pitch=pitch, M=M, n_slabs=n_slabs, tg=tg)


def run(ops, c):
    """Two launches of case c; every output as a numpy array, keyed `full.*` (all optional outputs given) and `bare.*` (d_seq_emb, logits,
    coef_out NULL).  The structural checks (NaN gaps, state block, rows of the table gradient that must not move) are made here."""
    P = R.problem(c.M, c.D)
    M, D, V = c.M, c.D, R.V
    dev = lambda a, t=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(t).cuda()
    sd, xd = rows_in(P.s, c.pitch), rows_in(P.x, c.pitch)
    tabd, gd = dev(P.table), dev(P.gamma)
    posd, negd = dev(np.concatenate([P.pos, np.zeros(SPARE, np.int32)]), torch.int32), dev(np.concatenate([P.neg, np.zeros(SPARE, np.int32)]), torch.int32)
    tg0 = (0.25 * np.random.RandomState(5).standard_normal((V, D))).astype(np.float32)
    stride = 2 * D + 3
    got = {}
    for tag in ("full", "bare"):
        full = tag == "full"
        state = torch.zeros(16, device="cuda"); state[4:5].view(torch.int32)[0] = 7
        ds = nan_rows(M, c.pitch) if full else None
        plg, nlg = (torch.full((M + SPARE,), float("nan"), device="cuda") for _ in range(2)) if full else (None, None)
        coef = torch.full((2 * M + SPARE,), float("nan"), device="cuda") if full else None
        tg = dev(tg0) if c.tg and (full or c.ln) else None           # (cr_head_fwd_bwd, bare: the forward alone; _ln keeps its form)
        kw = dict(d_seq_emb=ds, ldd=c.pitch if full else 0, table_grad=tg, pos_logits=plg, neg_logits=nlg, coef_out=coef)
        if c.ln:
            dx, slabs = nan_rows(M, c.pitch), torch.full((c.n_slabs, stride), float("nan"), device="cuda")
            ops.head_fwd_bwd_ln(sd, c.pitch, tabd, posd, negd, M, D, state, xd, c.pitch, gd, dx, c.pitch, slabs, slabs[0, D:], stride, c.n_slabs, **kw)
        else:
            ops.head_fwd_bwd(sd, c.pitch, tabd, posd, negd, M, D, state, **kw)
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        # the snapshot of the last workgroup to finish: the totals, the step number, the ticket re-armed (castrec.h, state block)
        assert tuple(st[8:11]) == tuple(st[0:3]) and st[8:12].view(np.uint32)[3] == 7 and st[12:13].view(np.uint32)[0] == 0
        got[tag + ".state"] = st[:3].copy()
        if c.ln:
            got[tag + ".dx"] = written(dx, M, D)
            sl = slabs.cpu().numpy()
            assert np.isfinite(sl[:, :2 * D]).all() and np.isnan(sl[:, 2 * D:]).all()
            rps = -(-M // c.n_slabs)
            for w in range(c.n_slabs):
                if w * rps >= M:
                    assert not sl[w, :2 * D].any(), "the slab of a workgroup without rows must be zeros"
            got[tag + ".slabs"] = sl[:, :2 * D].copy()
        if full:
            got["full.d_seq_emb"] = written(ds, M, D)
            for k, b in (("pl", plg), ("nl", nlg)):
                g = b.cpu().numpy()
                assert np.isfinite(g[:M]).all() and np.isnan(g[M:]).all()
                got["full." + k] = g[:M].copy()
            g = coef.cpu().numpy()
            assert np.isfinite(g[:2 * M]).all() and np.isnan(g[2 * M:]).all()
            got["full.coef"] = g[:2 * M].reshape(2, M).copy()
        if tg is not None:
            g = tg.cpu().numpy()
            named = np.zeros(V, bool)
            named[P.pos[P.pos != 0]] = True                # a row counts where pos != 0; its neg id counts where that is not 0 either
            named[P.neg[(P.pos != 0) & (P.neg != 0)]] = True
            assert not named[0] and np.array_equal(g[~named].view(np.int32), tg0[~named].view(np.int32)), "row 0 or a row no id names moved"
            got[tag + ".table_grad"] = g
    got["tg0"] = tg0
    return got


def check(c, got):
    P = R.problem(c.M, c.D)
    W = P.ln if c.ln else P.plain
    D = c.D
    err = {}
    for tag in ("full", "bare"):
        st = got[tag + ".state"]
        err[tag + ".loss"] = abs(st[0] - W.loss) / abs(W.loss)
        assert st[1] == W.auc and st[2] == W.n
        if c.ln:
            err[tag + ".dx"] = relerr(got[tag + ".dx"], P.ln.dx)
            tot = got[tag + ".slabs"].astype(np.float64).sum(0)
            err[tag + ".dgamma"], err[tag + ".dbeta"] = relerr(tot[:D], P.ln.dgamma), relerr(tot[D:], P.ln.dbeta)
        if tag + ".table_grad" in got:
            err[tag + ".table_grad"] = relerr(got[tag + ".table_grad"], got["tg0"].astype(np.float64) + W.table_grad)
    err["pl"], err["nl"] = relerr(got["full.pl"], W.pl), relerr(got["full.nl"], W.nl)
    err["d_seq_emb"], err["coef"] = relerr(got["full.d_seq_emb"], W.d_seq_emb), relerr(got["full.coef"], W.coef)
    print({k: "%.2e" % v for k, v in err.items()})
    bound = {"loss": 2e-6, "pl": 2e-6, "nl": 2e-6, "d_seq_emb": 3e-6, "table_grad": 3e-6, "coef": 3e-6, "dx": 2e-5, "dgamma": 5e-6, "dbeta": 5e-6}
    bad = {k: v for k, v in err.items() if not v < bound[k.split(".")[-1]]}
    assert not bad, bad


HEAD_SHAPES = [(50, 50), (72, 72), (136, 140), (260, 264)]
# D, pitch, rows of the pipeline case (two workgroups), table_grad
LN_SHAPES = [(50, 52, 261, True), (25, 25, 261, False), (72, 72, 133, True), (260, 260, 69, True), (130, 130, 69, False),
             (48, 52, 261, False), (72, 76, 133, False), (132, 132, 69, False), (256, 256, 69, False),
             (24, 26, 261, False), (48, 50, 133, False), (70, 70, 69, False)]


@pytest.mark.parametrize("M", [261, 5])
@pytest.mark.parametrize("D,pitch", HEAD_SHAPES)
def test_head(ops, D, pitch, M):
    c = case(False, D, pitch, M, tg=True)
    check(c, run(ops, c))


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("D,pitch,M,tg", LN_SHAPES)
def test_head_ln(ops, D, pitch, M, tg, small):
    c = case(True, D, pitch, 5, 4, tg) if small else case(True, D, pitch, M, 2, tg)
    check(c, run(ops, c))

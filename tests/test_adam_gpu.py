"""cr_adam_step, cr_reduce_slabs and cr_l2_penalty (csrc/cr_adam.hip) against the fp64 reference of tests/adam_ref.py: every kind of
workgroup of the Adam launch (dense blocks, lazy rows, occurrence-index units, the bitmap sweep, the plain sweep with its head and tail,
the id-ring copy) and every k_adam instantiation, p, m and v element by element under the reference's bounds (derived there; checked
on the CPU by tests/test_adam_host.py, which also shows that these comparisons reject a wrong step).  Every buffer the launch writes
sits between guard elements that must come back unchanged; moments start random, not zero.

What reaches what (k_adam<STREAM, LPR, VEC>; a kernel trace of the streaming cases alone lists the three <true, ...> forms):
  <false, 0, 1>   every test without an index              <true, 0, 1>    test_streaming_plain_sweep
  <false, 16, 1>  test_occurrence_index_step[9-*]          <false, 32, 1>  [17-*]          <false, 64, 1>  [33-*]
  <false, 16, 2>  [6-*]                                    <false, 32, 2>  [50-*]          <false, 64, 2>  [102-*]
  <false, 16, 4>  [20-*]                                   <false, 32, 4>  [100-*], [128-*], test_occurrence_index_large_table
  <false, 64, 4>  [256-*]                                  <true, 32 | 64, 4>  test_streaming_occurrence_index_step[128 | 256]
  dense block, 16-byte columns / scalar columns   test_dense_blocks[n_dense 256, 1027 / 1, 3, 255, 257 (last block), 1027 (last block)]
  lazy rows                                       test_lazy_rows (scalar head of the sweep behind them: [41-7-*])
  unit workgroups, bitmap sweep                   test_occurrence_index_step: shifts D = 128, 256; divisions D = 20, 100; scalar D = 6, 9, 17, 33,
                                                  50, 102; its loop twice: test_occurrence_index_large_table
  plain sweep: first group                        test_plain_sweep_small[4 ..]; unrolled loop, remainder loop: test_plain_sweep_all_three_loops
                                                  (U = 2), test_streaming_plain_sweep (U = 4); tail: n_table % 4 != 0 throughout; head: test_lazy_rows[41-7-*]
  id ring, 16-byte / element copy                 test_id_ring[4000-0-0, 4000-1000-0], test_occurrence_index_step (2nd launch) / the other test_id_ring cases"""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import adam_ref as A
from adam_ref import Buf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


def geometry(D):
    from castrec_amd import lib as L
    ng, ent = C.c_int(), C.c_int()
    assert L.lib.cr_tgrad_geometry(D, C.byref(ng), C.byref(ent)) == 1
    return ng.value, ent.value


def run(ops, c, tg_ring=False):
    """One launch of cr_adam_step on case c (adam_ref.make_case), everything checked; returns the fp32 p, m, v and the lazy flags."""
    from castrec_amd import lib as L
    nt, nd = c.n_table, c.n_dense
    ref = A.reference(c)
    P, M, V = Buf(c.p0, 7.5), Buf(c.m0, 7.5), Buf(c.v0, 7.5)
    TG = Buf(c.table_grad, 3.25) if c.table_grad is not None else None
    SL = Buf(c.slabs, np.nan) if nd else None
    counts = torch.from_numpy(c.slab_counts).cuda() if c.slab_counts is not None else None
    st = np.zeros(16, np.float32)
    sums, decoy = [c.loss_sum, c.auc_sum, c.n_target], [-1.0, -2.0, 1.0]
    st[0:3] = sums if c.stats_mode == "local" else decoy
    st[3], st[7], st[12:16] = 0.5, c.state7, [11.0, 12.0, 13.0, 14.0]
    st.view(np.int32)[4] = c.t + (7 if c.stats_mode == "self" else 0)        # (self-advancing: the step number comes from the snapshot)
    if c.stats_mode == "self":
        st[8:11] = sums
        st.view(np.int32)[11] = c.t
    ST = Buf(st, -9.0)
    EXT = Buf(np.array(sums, np.float32), -9.0) if c.stats_mode == "external" else None
    kw = {}
    if c.stats_mode == "external":
        kw.update(stats=EXT.view)
    elif c.stats_mode == "self":
        kw.update(stats=ST.view[8:11], step_snapshot=ST.view[11:12])
    FL = None
    if c.lazy is not None:
        FL = Buf(c.lazy.flags0.view(np.int32), -3)
        kw.update(lazy_ids=torch.from_numpy(c.lazy.ids).cuda(), lazy_rows=c.lazy.rows, lazy_D=c.lazy.D, lazy_flags=FL.view)
    ring = c.ring
    keep = []
    if c.tg is not None:
        from index_harness import build_index
        t = c.tg
        ng, ent = geometry(t["D"])
        lay, ix = build_index(t["M"], t["V"], t["T_pos"], t["seq"], t["pos"], t["neg"], ng=ng, ent=ent)
        d_ix = None
        if tg_ring:                                       # a slot = the batch's ids, then its index; the running step's slot holds the index
            off = 3 * t["M"]
            assert off % 4 == 0 and ring is None
            rs = np.random.RandomState(c.t)
            data = rs.randint(1, t["V"], (3, off + lay.total_words)).astype(np.int32)
            data[:, off:] = -7
            data[c.t % 3, off:] = ix
            ring = types.SimpleNamespace(slots=3, slot_elems=off + int(lay.total_words), copy_elems=off, misalign=0, data=data)
        else:
            d_ix = torch.from_numpy(ix).cuda()
        dv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        rows, rows2, emb, coef = dv(t["rows"]), dv(t["rows2"]), dv(t["emb"]), dv(t["coef"])
        part = torch.full((lay.cap_blocks, (t["D"] + 3) // 4 * 4), float("nan"), device="cuda")
        tickets = torch.zeros(lay.cap_blocks, dtype=torch.int32, device="cuda")
        keep += [d_ix, rows, rows2, emb, coef, part]
    RING = DST = None
    if ring is not None:
        RING = torch.from_numpy(ring.data.reshape(-1)).cuda()
        dst0 = np.full(ring.slot_elems, -5, np.int32)
        DST = Buf(dst0, -6, shift=ring.misalign)
        kw.update(ids_ring=RING, ids_ring_slots=ring.slots, ids_slot_elems=ring.slot_elems, ids_dst=DST.view, ids_copy_elems=ring.copy_elems)
    if c.tg is not None:
        g = L.TgradDesc(d_ix.data_ptr() if d_ix is not None else None, RING.data_ptr() if tg_ring else None, 3 if tg_ring else 0,
                        ring.slot_elems if tg_ring else 0, 3 * t["M"] if tg_ring else 0, ST.view.data_ptr() + 16, lay, rows.data_ptr(),
                        rows2.data_ptr() if rows2 is not None else None, t["D"], t["scale"], emb.data_ptr(), t["D"], coef.data_ptr(), t["D"],
                        part.data_ptr(), tickets.data_ptr())
        kw.update(tg=g)
    ops.adam_step(P.view, M.view, V.view, TG.view if TG is not None else None, SL.view if SL is not None else None, nt, nd, c.n_slabs, c.lr,
                  ST.view, beta1=c.beta1, beta2=c.beta2, eps=c.eps, l2=c.l2, n_l2=c.n_l2, slab_counts=counts, **kw)
    torch.cuda.synchronize()

    got = dict(p=P.back(), m=M.back(), v=V.back())
    ratio, which, i = A.worst_ratio(got, ref)
    print("worst error / bound: %.3f at %s[%d]" % (ratio, which, i))
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert ratio <= 1.0, (ratio, which, i, got[which][i], getattr(ref, which)[i])
    if TG is not None:
        tg_back = TG.back()
        assert (tg_back[ref.grad_zeroed] == 0.0).all()                                   # used: zeroed for the next step
        assert np.array_equal(tg_back[~ref.grad_zeroed], c.table_grad[~ref.grad_zeroed])   # a lazy row not listed: kept
    if SL is not None:
        SL.back()
    s = ST.back()
    assert s[5] == pytest.approx(ref.state5, rel=A.STATE_RTOL) and s[6] == pytest.approx(ref.state6, rel=A.STATE_RTOL), (s[5], s[6])
    if ref.state04 is None:
        assert np.array_equal(s[:5].view(np.int32), st[:5].view(np.int32))
    else:
        assert (s[:4] == 0.0).all() and int(s.view(np.int32)[4]) == ref.state04[4]
    assert np.array_equal(s[7:].view(np.int32), st[7:].view(np.int32))
    if EXT is not None:
        EXT.back()
    flags = None
    if FL is not None:
        flags = FL.back().view(np.uint32)
        assert np.array_equal(flags, ref.lazy_flags)
    if DST is not None:
        c2 = copy.copy(c)
        c2.ring = ring
        assert np.array_equal(DST.back(), A.ring_copy_reference(c2, dst0))
        assert np.array_equal(RING.cpu().numpy(), ring.data.reshape(-1))
    if c.tg is not None:
        assert int(tickets.abs().sum()) == 0              # every launch leaves the slices' tickets zero
    del keep
    return got, flags


# ---- the plain sweep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_table", [0, 1, 3, 4, 5, 301, 4099])
def test_plain_sweep_small(ops, n_table):
    """No 16-byte group at all, one, one and a scalar tail, several blocks' worth: n_table % 4 in {0, 1, 3}."""
    run(ops, A.make_case(n_table, n_table, 130))


def test_table_only(ops):
    run(ops, A.make_case(7, 1027, 0))


def test_plain_sweep_all_three_loops(ops):
    """1024 blocks of 1024 threads (the cap): a thread's first group outside the loop, the U = 2 loop once, the remainder loop on the
    first 1000 threads of block 0, the scalar tail of 3."""
    run(ops, A.make_case(8, 4 * (3 * 2 ** 20 + 1000) + 3, 130))


@pytest.mark.parametrize("which", range(6))
def test_l2_boundary(ops, which):
    """l2 on the first n_l2 elements: none, inside the first 16-byte group, inside the scalar tail, the table exactly, into the dense
    section, everything; state[7] joins the loss exactly when n_l2 > 0."""
    nt, nd = 303, 130
    n_l2 = [0, 2, nt - 1, nt, nt + 100, nt + nd][which]
    run(ops, A.make_case(10 + which, nt, nd, l2=0.05, n_l2=n_l2))


# ---- dense blocks ---------------------------------------------------------------------------------------------
def _dense_case(n_dense, n_slabs):
    counts = {1027: [n_slabs, 0, 1, n_slabs, max(n_slabs // 2, 1)], 257: [1, n_slabs], 256: [max(n_slabs // 2, 1)]}.get(n_dense)
    return A.make_case(n_dense + n_slabs, 5, n_dense, n_slabs=n_slabs, slab_counts=counts, l2=0.05, n_l2=5 + n_dense // 2)


@pytest.mark.parametrize("n_slabs", [1, 15, 16, 17, 255, 256])
@pytest.mark.parametrize("n_dense", [1, 3, 255, 256, 257, 1027])
def test_dense_blocks(ops, n_dense, n_slabs):
    """Slab sums at the wave-share edges (a wave takes slabs w, w + 16, ...), 16-byte and scalar column groups, blocks that count 0, 1,
    some and all slabs -- the slabs a block does not count are NaN and must not be read."""
    run(ops, _dense_case(n_dense, n_slabs))


@pytest.mark.parametrize("n_slabs", [1, 15, 16, 17, 255, 256])
@pytest.mark.parametrize("n_dense", [1, 3, 255, 256, 257, 1027])
def test_reduce_slabs_is_exact(ops, n_dense, n_slabs):
    """cr_reduce_slabs on the same slabs: the sums are exact in fp32 (dyadic entries), so every order gives the same bits."""
    c = _dense_case(n_dense, n_slabs)
    want = A.reference(c).G[c.n_table:].astype(np.float32)
    SL, OUT = Buf(c.slabs, np.nan), Buf(np.full(n_dense, 5.0, np.float32), 7.5)
    ST, STATS = Buf(np.arange(16, dtype=np.float32) + 0.5, -9.0), Buf(np.zeros(3, np.float32), -9.0)
    counts = torch.from_numpy(c.slab_counts).cuda() if c.slab_counts is not None else None
    ops.reduce_slabs(SL.view, n_slabs, n_dense, OUT.view, state=ST.view, stats_out=STATS.view, slab_counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(OUT.back(), want)
    assert np.array_equal(STATS.back(), [0.5, 1.5, 2.5]) and np.array_equal(ST.back(), np.arange(16, dtype=np.float32) + 0.5)
    SL.back()
    OUT2 = Buf(np.full(n_dense, 5.0, np.float32), 7.5)
    ops.reduce_slabs(SL.view, n_slabs, n_dense, OUT2.view, slab_counts=counts)       # without the statistics copy
    torch.cuda.synchronize()
    assert np.array_equal(OUT2.back(), want)


# ---- scalars --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_target,t,mode", [(0.0, 3, "local"), (37.0, 3, "local"), (16.0, 1, "local"), (16.0, 2, "local"), (16.0, 1000, "local"),
                                             (16.0, 200000, "local"), (16.0, 3, "external"), (16.0, 3, "self"), (37.0, 200000, "self"),
                                             (0.0, 2, "external")])
def test_scalars(ops, n_target, t, mode):
    """n_target = 0 (loss and AUC 0, a pure momentum step) and a count whose reciprocal is not exact; step numbers up to where b1^t
    underflows; the sums from state, from a separate buffer, from the snapshot with the kernel ending the step.  n_table % 4 == 3."""
    run(ops, A.make_case(int(n_target) + t % 1000, 303, 130, n_target=n_target, t=t, stats_mode=mode, l2=0.05, n_l2=303))


# ---- lazy rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ids", [1, 1000])
@pytest.mark.parametrize("rows,D", [(41, 7), (40, 50), (9, 256)])
def test_lazy_rows(ops, rows, D, n_ids):
    """Listed rows once (duplicates, id 0, id = rows and a negative id in the list), the other lazy rows and their gradient untouched,
    the positional tail behind the lazy region swept ((41, 7): from an end that is no multiple of 4 -- the scalar head); a second
    step on the first one's results: its flags are still in place and do not block it."""
    rs = np.random.RandomState(rows + n_ids)
    nt = rows * D + 5 * D + (2 if D % 4 == 0 else 0)
    lists = []
    for step in range(2):
        ids = rs.randint(1, rows, n_ids).astype(np.int32)
        if n_ids > 8:
            ids[ids % 3 == step] = ids[0]                 # a third of the rows is not listed
            ids[[1, 5, 17, 100]] = [0, rows, -3, ids[0]]
        lists.append(ids)
    c = A.make_case(rows * D + n_ids, nt, 130, t=3, l2=0.05, n_l2=nt - 3, lazy=(rows, D, lists[0]))
    got, flags = run(ops, c)
    c2 = A.make_case(rows * D + n_ids + 1, nt, 130, t=4, l2=0.05, n_l2=nt - 3, lazy=(rows, D, lists[1]))
    c2.p0, c2.m0, c2.v0 = got["p"], got["m"], got["v"]
    c2.lazy.flags0 = flags.copy()
    got2, flags2 = run(ops, c2)
    both = np.intersect1d(lists[0][(lists[0] > 0) & (lists[0] < rows)], lists[1][(lists[1] > 0) & (lists[1] < rows)])
    assert len(both) > 0 or n_ids == 1
    assert (flags2[both] == 4).all()


# ---- the occurrence index -------------------------------------------------------------------------------------
# hidden size -> (LPR, VEC) of tg_shape.  (100 is a multiple of 4 and so a second <32, 4>, its D / 4 = 25 no power of two: the division
# form of the bitmap sweep at that width; 102 is the <64, 2> size.)
TG_SHAPES = {9: (16, 1), 17: (32, 1), 33: (64, 1), 6: (16, 2), 50: (32, 2), 102: (64, 2), 20: (16, 4), 128: (32, 4), 100: (32, 4), 256: (64, 4)}


@pytest.mark.parametrize("T_pos", [0, 25])
@pytest.mark.parametrize("D", sorted(TG_SHAPES))
def test_occurrence_index_step(ops, D, T_pos):
    """One hidden size per k_adam<., LPR, VEC> (tg_shape: VEC 4 / 2 / 1 for D % 4 == 0 / even / odd, LPR by D -- the geometry query gives
    1024 / LPR lane groups and 8 occurrences per group at VEC 4, 16 otherwise): the listed rows from the gather, in place, the others
    from the bitmap sweep (D / 4 a power of two: shifts; else divisions; D % 4 != 0: scalar), l2 on both; the boundary at the table's
    end and 8 elements into the dense section; the second launch reads the index out of a ring slot and moves the next slot's ids."""
    lpr, vec = TG_SHAPES[D]
    assert geometry(D) == (1024 // lpr, 8 if vec == 4 else 16) and vec == (4 if D % 4 == 0 else 2 if D % 2 == 0 else 1)
    V = 300
    nt = (V + T_pos) * D
    tg = A.make_tg(D + T_pos, D, V, T_pos)
    _, listed = A.tg_gradient(tg)
    assert 60 <= listed[:V].sum() <= 110
    run(ops, A.make_case(D, nt, 130, l2=0.05, n_l2=nt, t=3, tg=tg))
    run(ops, A.make_case(D + 1, nt, 130, l2=0.05, n_l2=nt + 8, t=4 + D % 3, tg=tg), tg_ring=True)


def test_occurrence_index_large_table(ops):
    """n_table / 4 > 4 * 2^20: the bitmap sweep's loop (four groups per thread and pass, 1024 blocks) runs twice on the first threads."""
    D, V = 128, 140000
    tg = A.make_tg(5, D, V, 0, listed=60, rows2=False)
    run(ops, A.make_case(9, V * D, 130, l2=0.05, n_l2=V * D, tg=tg))


# ---- the id ring ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_elems,copy_elems,misalign", [(4000, 0, 0), (4000, 1000, 0), (4000, 1001, 0), (4001, 0, 0), (4001, 1000, 0),
                                                            (4001, 1001, 0), (4000, 0, 1), (4000, 1000, 1)])
@pytest.mark.parametrize("t", [3, 4, 5])
def test_id_ring(ops, slot_elems, copy_elems, misalign, t):
    """The next step's ids out of slot (t + 1) mod 3: 16-byte copies where slot, count and both pointers allow, element copies
    otherwise (an odd slot, an odd count, a destination off 16 bytes); what lies behind the copied words stays."""
    run(ops, A.make_case(t + copy_elems, 301, 130, t=t, ring=dict(slots=3, slot_elems=slot_elems, copy_elems=copy_elems, misalign=misalign)))


# ---- the l2 penalty -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 1025, 170850])
def test_l2_penalty(ops, n):
    """state[7] = scale * sum(p^2): a thread's serial chain of n / 1024 fmas, then the ten-level tree, then the product --
    (n / 1024 + 11) roundings of partial sums of non-negative terms, each at most the total."""
    rs = np.random.RandomState(n)
    p = rs.standard_normal(n).astype(np.float32)
    scale = 0.025
    Pb, ST = Buf(p, np.nan), Buf(np.arange(16, dtype=np.float32), -9.0)
    ops.l2_penalty(Pb.view, n, scale, ST.view)
    torch.cuda.synchronize()
    s = ST.back()
    want = float(np.float32(scale)) * float((p.astype(np.float64) ** 2).sum())
    err, bound = abs(float(s[7]) - want), (n / 1024 + 11) * 2.0 ** -24 * want
    print("error %.3g, bound %.3g" % (err, bound))
    assert err <= bound
    assert np.array_equal(np.delete(s, 7), np.delete(np.arange(16, dtype=np.float32), 7))
    Pb.back()


# ---- the streaming instantiations -----------------------------------------------------------------------------
def test_streaming_plain_sweep(ops, monkeypatch):
    """k_adam<true, 0, 1>: four groups in flight -- the first group, the U = 4 loop once, the remainder loop, a scalar tail of 1."""
    monkeypatch.setenv("CASTREC_ADAM_STREAM", "1")
    run(ops, A.make_case(20, 4 * (5 * 2 ** 20 + 1000) + 1, 130))


@pytest.mark.parametrize("D", [128, 256])
def test_streaming_occurrence_index_step(ops, D, monkeypatch):
    """k_adam<true, 32, 4> and k_adam<true, 64, 4>: the bitmap sweep with streaming accesses (chosen by size; forced here)."""
    monkeypatch.setenv("CASTREC_ADAM_STREAM", "1")
    V, T_pos = 300, 25
    nt = (V + T_pos) * D
    run(ops, A.make_case(D, nt, 130, l2=0.05, n_l2=nt + 8, tg=A.make_tg(D, D, V, T_pos)))

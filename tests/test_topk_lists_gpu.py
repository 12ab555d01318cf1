"""Top-K over per-query candidate lists on the GPU (castrec.h cr_score_topk_lists; index.search(cand_off=, cand_ids=), ItemIndex.search /
Engine.topk / Model.recommend / Model.similar_items(candidates=)).  One property carries everything: a search of per-row lists returns
the ids, score bits and ranks of the existing full search (topk_harness.search: cr_score_topk, never the code under test) on the same
source at the same precision with the complement of the row's list excluded."""
import ctypes

import numpy as np
import pytest
import torch

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd import ops as O
from castrec_amd.index import ItemIndex, candidate_csr
import topk_harness as H
from topk_harness import same_bits as _same

pytestmark = pytest.mark.gpu
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16
DS = [8, 20, 50, 64, 128, 256]                 # NK 1, 1, 2, 2, 4, 8, with masked columns at 8, 20, 50
VS = [100, 3417]
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 200, -1, 5]          # wave and round edges, several folds, -1: every item, fewer than K


def lists(Q, K, rows, tg, prec, table=None, index=None, iprec=None, V=None, ld=None):
    """cr_score_topk_lists through ops.score_topk_lists, rows taken as they are (any order, any int32): numpy (ids, scores, rank or
    None).  The outputs hold -7 / 123.0 / -7 beforehand, as topk_harness.search's: what the kernels leave unwritten shows."""
    B, D = Q.shape
    ld = ld or D
    q = torch.zeros(B, ld, dtype=torch.float32, device="cuda")
    q[:, :D] = torch.from_numpy(Q)
    if table is not None:
        V = table.shape[0]
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32) if off[-1] else None
    ids = torch.from_numpy(flat).cuda() if flat is not None else None
    tgt = torch.from_numpy(np.asarray(tg, np.int32)).cuda() if tg is not None else None
    ws = torch.empty(O.topk_lists_workspace_bytes(B, int(np.diff(off).max()), D, K), dtype=torch.uint8, device="cuda")
    out_i = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    out_s = torch.full((B, K), 123.0, dtype=torch.float32, device="cuda")
    rk = torch.full((B,), -7, dtype=torch.int32, device="cuda") if tg is not None else None
    if index is None:
        O.score_topk_lists(q, ld, table, B, K, prec, off, ids, tgt, ws, out_i, out_s, rk)
    else:
        O.score_topk_lists(q, ld, (V, D), B, K, prec, off, ids, tgt, ws, out_i, out_s, rk, index=index, index_precision=iprec)
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_s.cpu().numpy(), (rk.cpu().numpy() if rk is not None else None)


def complement(rows, V):
    """Per row: every id of 1 .. V-1 the row does not name -- the exclusion list that restricts the full search to the row's list."""
    return [sorted(set(range(1, V)) - set(int(i) for i in r)) for r in rows]


def make_table(rs, V, D):
    """A table whose row 0 is not zero and in which several rows are copies of one another (equal scores inside a list)."""
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    T[40] = T[20]
    T[60] = T[20]
    T[V - 1] = T[17] = T[16]
    return T


def make_rows(rs, V, lens):
    """One shuffled row of distinct ids per length (-1: all of 1 .. V-1; capped there); every third non-empty row holds V - 1, the
    table's last row, and rows of five or more hold the copies 16, 17, 20, 60."""
    rows = []
    for b, n in enumerate(lens):
        n = V - 1 if n < 0 else min(n, V - 1)
        must = ([V - 1] if b % 3 == 0 and n >= 1 else []) + ([16, 17, 20, 60] if n >= 5 else [])
        rest = rs.choice([i for i in range(1, V) if i not in must], n - len(must), replace=False).tolist()
        rows.append(rs.permutation(must + rest).astype(np.int64).tolist())
    return rows


def make_targets(rs, Q, T, rows, V):
    """Targets by row, cycling: inside the list, outside it, 0, V + 2, the list's best, its worst (fp64 scores decide which)."""
    S = Q.astype(np.float64) @ T.astype(np.float64).T
    tg = np.zeros(len(rows), np.int32)
    for b, r in enumerate(rows):
        kind = b % 6
        outside = sorted(set(range(1, V)) - set(r))
        if kind == 0 and r:
            tg[b] = r[rs.randint(len(r))]
        elif kind == 1 and outside:
            tg[b] = outside[rs.randint(len(outside))]
        elif kind == 2:
            tg[b] = 0
        elif kind == 3:
            tg[b] = V + 2
        elif r:
            tg[b] = r[int(np.argmax(S[b, r]))] if kind == 4 else r[int(np.argmin(S[b, r]))]
    return tg


def sources(T):
    """(name, precision, keyword arguments of the search) for every source and every precision it serves."""
    t = H.table_in_nan_buffer(T)
    V, D = T.shape
    split, plain = O.topk_index_build(t, SPLIT), O.topk_index_build(t, PLAIN)
    return [("table", SPLIT, dict(table=t)), ("table", PLAIN, dict(table=t)),
            ("split index", SPLIT, dict(index=split, iprec=SPLIT, V=V)), ("split index", PLAIN, dict(index=split, iprec=SPLIT, V=V)),
            ("plain index", PLAIN, dict(index=plain, iprec=PLAIN, V=V))]


@pytest.mark.parametrize("D", DS)
def test_lists_search_is_the_full_search_restricted(D):
    rs = np.random.RandomState(300 + D)
    checked_fp64 = False
    for V in VS:
        T = make_table(rs, V, D)
        srcs = sources(T)
        for B, K, lens in ((1, 128, [65]), (5, 10, LENS[1::2]), (37, 1, LENS * 4), (37, 10, LENS * 4)):
            lens = lens[:B]
            Q = rs.standard_normal((B, D)).astype(np.float32)
            Q[0] = 30 * T[20]                                               # the copies of row 20 lead row 0's scores
            rows = make_rows(rs, V, lens)
            tg = make_targets(rs, Q, T, rows, V)
            excl = complement(rows, V)
            for name, prec, kw in srcs:
                what = (D, V, B, K, name, prec)
                want = H.search(Q, K, excl, tg, prec, **kw)
                got = lists(Q, K, rows, tg, prec, **kw)
                _same(want, got, what)
                for b, r in enumerate(rows):
                    n = min(K, len(r))
                    assert np.all(got[0][b, n:] == 0) and np.all(np.isneginf(got[1][b, n:])), what       # filler; an empty row is all filler
                    assert set(got[0][b, :n].tolist()) <= set(r) and (got[2][b] >= 0) == (tg[b] in r), what
                if B == 5:
                    _same(got, lists(Q, K, rows, tg, prec, **kw), what + ("a second call",))
                    _same(want[:2] + (None,), lists(Q, K, rows, None, prec, **kw), what + ("no targets",))
                    _same(want, lists(Q, K, rows, tg, prec, ld=D + 3, **kw), what + ("a pitch above D",))
                    if prec == SPLIT and name == "table" and not checked_fp64:
                        H.check_fp64(Q, T, K, excl, got[0], got[1])
                        checked_fp64 = True
    assert checked_fp64


def test_ineligible_ids_are_not_read_and_order_does_not_matter():
    """0, V, V + 2 and -1 inside a row: not eligible, and their rows (NaNs behind the table, whatever lies before it) are not read; the
    same row ascending, descending and shuffled gives the same bits."""
    rs = np.random.RandomState(11)
    V, D, B, K = 100, 50, 4, 10
    T = make_table(rs, V, D)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    base = rs.choice(np.arange(1, V), 40, replace=False).tolist() + [V - 1]
    base = sorted(set(base))
    junk = [0, V, V + 2, -1]
    rows = [base, base[::-1], rs.permutation(base).tolist(), rs.permutation(base + junk).tolist()]
    Q[:] = Q[0]                                                             # one query: the four rows must agree
    tg = np.array([base[3]] * B, np.int32)
    for name, prec, kw in sources(T):
        want = H.search(Q, K, complement(rows, V), tg, prec, **kw)
        got = lists(Q, K, rows, tg, prec, **kw)
        _same(want, got, (name, prec))
        for b in range(1, B):
            _same(tuple(x[:1] for x in got), tuple(x[b:b + 1] for x in got), (name, prec, "row", b))
        only_junk = lists(Q, K, [junk, [], [0], [V]], np.array([0, V, V + 2, 5], np.int32), prec, **kw)
        assert np.all(only_junk[0] == 0) and np.all(np.isneginf(only_junk[1])) and np.all(only_junk[2] == -1), (name, prec)
    # every list empty: cand_ids may be NULL
    e = lists(Q, K, [[], [], [], []], tg, SPLIT, table=H.table_in_nan_buffer(T))
    assert np.all(e[0] == 0) and np.all(np.isneginf(e[1])) and np.all(e[2] == -1)


def test_equal_scores_inside_a_list_and_at_the_kth_place():
    rs = np.random.RandomState(4)
    V, D, B = 100, 50, 4
    T = make_table(rs, V, D)                                                # 20 = 40 = 60 and 16 = 17 = V - 1
    Q = rs.standard_normal((B, D)).astype(np.float32)
    Q[0] = Q[2] = 30 * T[20]
    Q[1] = Q[3] = 30 * T[16]
    others = [i for i in range(1, V - 1) if i not in (16, 17, 20, 40, 60)]
    rows = [[60, 20] + rs.choice(others, 30, replace=False).tolist(),       # 40 stays outside the list
            [99, 17, 16] + rs.choice(others, 30, replace=False).tolist(),
            [60, 40] + rs.choice(others, 70, replace=False).tolist(),       # 20 itself is no candidate
            [99, 17] + rs.choice(others, 3, replace=False).tolist()]
    tg = np.array([60, 99, 60, 17], np.int32)
    for name, prec, kw in sources(T):
        for K in (1, 2, 10):
            want = H.search(Q, K, complement(rows, V), tg, prec, **kw)
            got = lists(Q, K, rows, tg, prec, **kw)
            _same(want, got, (name, prec, K))
            assert got[0][:, 0].tolist() == [20, 16, 40, 17] and got[2].tolist() == [1, 2, 1, 0], (name, prec, K, got)
            if K >= 2:                                                      # the tie at the K-th place goes to the smaller id
                assert got[0][:, 1].tolist() == [60, 17, 60, 99] and np.array_equal(got[1][:, 0], got[1][:, 1]), (name, prec, K, got)


@pytest.mark.parametrize("K", [10, 128])
def test_segmented_lists(K):
    """A long list at a small batch is cut into segments; the short row leaves two of its three segments empty; the target in the first
    and in the last segment."""
    rs = np.random.RandomState(21 + K)
    B, V, D = 2, 6000, 20
    assert L.lib.cr_topk_lists_segments(B, 5000) == 3
    T = make_table(rs, V, D)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    rows = make_rows(rs, V, [5000, 70])
    excl = complement(rows, V)
    srcs = sources(T)
    for tg in (np.array([rows[0][5], rows[1][69]], np.int32), np.array([rows[0][4990], rows[1][0]], np.int32),
               np.array([excl[0][0], V + 2], np.int32)):
        for name, prec, kw in (srcs[0], srcs[3], srcs[4]):
            want = H.search(Q, K, excl, tg, prec, **kw)
            got = lists(Q, K, rows, tg, prec, **kw)
            _same(want, got, (K, name, prec, tg))
            _same(got, lists(Q, K, rows, tg, prec, **kw), (K, name, prec, "a second call"))
            assert np.all(got[0][1, 70:] == 0) and np.all(got[0][:, :min(K, 70)] > 0)
    got = lists(Q, K, rows, None, SPLIT, **srcs[2][2])
    _same(H.search(Q, K, excl, None, SPLIT, **srcs[2][2]), got, (K, "no targets, split index"))
    H.check_fp64(Q, T, K, excl, got[0], got[1])


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
def test_model_recommend_similar_items_and_index_search_with_candidates(tmp_path):
    itemnum, B, T, k = 500, 9, 20, 12
    m = H.model("cast_1", itemnum=itemnum)
    rs = np.random.RandomState(5)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    every = np.arange(1, itemnum + 1)
    hist = [set(r[r != 0].tolist()) for r in seq.astype(np.int64)]
    cand = [rs.choice(every, n, replace=False).tolist() for n in (101, 0, 1, 16, 65, 200, itemnum, 5, 101)]
    cand[0][7] = sorted(hist[0])[0]                                         # a candidate of row 0's history
    cand[3] = cand[3] + cand[3][:4]                                         # duplicates: candidate_csr makes the row unique
    cset = [set(r) for r in cand]
    tg = np.array([sorted(cset[b] - hist[b])[0] if cset[b] - hist[b] else 1 for b in range(B)], np.int32)
    tg[0] = cand[0][7]                                                      # a target in the history: -1
    tg[4] = sorted(set(every.tolist()) - cset[4])[0]                        # a target outside the row's list: -1
    kw = dict(k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, targets=tg)
    full = [sorted(hist[b] | (set(every.tolist()) - cset[b])) for b in range(B)]
    ix = m.build_item_index()
    want = m.recommend(None, seq, exclude=full, **kw)                       # existing code: the yardstick
    a = m.recommend(None, seq, candidates=cand, exclude="history", **kw)
    _same(want, a, "candidates=rows, the table")
    _same(want, m.recommend(None, seq, candidates=cand, **kw), "exclude='history' is the default")
    _same(want, m.recommend(None, seq, candidates=cand, index=ix, **kw), "candidates=rows, index=ix")
    _same(want, m.recommend(None, seq, candidates=(c for c in cand), exclude=[sorted(h) for h in hist], **kw), "a generator; exclude as rows")
    assert a[2][0] == a[2][1] == a[2][4] == -1 and a[2][5] >= 0 and np.all(a[0][1] == 0)
    for b in range(B):
        got = set(a[0][b].tolist()) - {0}
        assert got <= cset[b] and not (got & hist[b])
    none = m.recommend(None, seq, candidates=cand, exclude=None, **kw)      # without the history exclusion
    _same(m.recommend(None, seq, exclude=[sorted(set(every.tolist()) - c) for c in cset], **kw), none, "exclude=None")
    assert none[2][0] >= 0
    assert np.array_equal(m.recommend(None, seq, k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, candidates=cand, return_scores=False), a[0])

    # the prebuilt (off, ids) form: the caller's CSR, ids on the device; exclusions cannot be subtracted from it
    off, flat = candidate_csr(cand, B, itemnum + 1, exclude=[sorted(h) for h in hist])
    pre = (off, torch.from_numpy(flat).cuda())
    _same(want, m.recommend(None, seq, candidates=pre, exclude=None, **kw), "prebuilt, the table")
    _same(want, m.recommend(None, seq, candidates=pre, exclude=None, index=ix, **kw), "prebuilt, index=ix")
    with pytest.raises(ValueError, match="exclude"):
        m.recommend(None, seq, candidates=pre, **kw)                        # exclude='history' by default

    # one filter per call
    sub = ix.subset(cand[0])
    for bad in (dict(allow=cand[0]), dict(allow=sub), dict(index=sub)):
        with pytest.raises(ValueError, match="one filter per call"):
            m.recommend(None, seq, candidates=cand, **bad, **kw)
    with pytest.raises(ValueError, match="one filter per call"):
        m.similar_items([1, 2], candidates=[[3], [4]], allow=cand[0])
    with pytest.raises(ValueError, match="one filter per call"):
        ix.search(np.zeros((1, 50), np.float32), 3, candidates=[[1, 2]], allow=[1, 2, 3])
    with pytest.raises(ValueError):
        m.recommend(None, seq, candidates=cand[:-1], **kw)                  # a row too few
    with pytest.raises(ValueError):
        m.recommend(None, seq, candidates=[[0]] * B, **kw)
    with pytest.raises(ValueError):
        m.recommend(None, seq, candidates=[[itemnum + 1]] * B, **kw)

    # similar items among each item's own candidates: never the item itself
    items = np.array([1, cand[0][3], itemnum, 16], np.int64)
    sc = [cand[0] + [1], cand[0], cand[4] + [itemnum], [16, 17]]
    E = m.get_params()["item_emb"].cpu()[torch.from_numpy(items)]
    ref = ix.search(E, 10, exclude=[sorted((set(every.tolist()) - set(c)) | {int(i)}) for c, i in zip(sc, items)])
    _same(ref, m.similar_items(items, 10, candidates=sc), "similar_items(candidates=), the table")
    _same(ref, m.similar_items(items, 10, candidates=sc, index=ix), "similar_items(candidates=, index=)")
    assert ref[0][3].tolist() == [17] + [0] * 9

    # ItemIndex.search on a loaded index: no model, no table
    back = ItemIndex.load(ix.save(str(tmp_path / "items.npz")))
    Q = rs.standard_normal((B, 50)).astype(np.float32)
    excl = [sorted(h) for h in hist]
    ref = back.search(Q, k, exclude=full, targets=tg)
    _same(ref, back.search(Q, k, candidates=cand, exclude=excl, targets=tg), "ItemIndex.search(candidates=)")
    _same(ref, back.search(torch.from_numpy(Q).cuda(), k, candidates=pre, targets=tg), "ItemIndex.search(candidates=prebuilt)")
    _same(back.search(Q, k, exclude=full, targets=tg, precision="bf16"),
          back.search(Q, k, candidates=cand, exclude=excl, targets=tg, precision="bf16"), "a plain search of a split index")
    _same(ref[:2], back.search(Q, k, candidates=cand, exclude=excl), "no targets")
    eng = m._eval_engine(B, False)                                          # Engine.topk: device tensors
    top, scr, rk = eng.topk(k, None, None, tg, index=ix, candidates=pre)
    _same(want, (top.cpu().numpy(), scr.cpu().numpy(), rk.cpu().numpy()), "Engine.topk(candidates=)")

    # a training step makes the index stale, with candidates as without
    pos = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    neg = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    m.train_step(None, seq, pos, neg, ts, hrs, dys)
    with pytest.raises(RuntimeError, match="stale index"):
        m.recommend(None, seq, candidates=cand, index=ix, **kw)
    with pytest.raises(RuntimeError, match="stale index"):
        m.similar_items(items, candidates=sc, index=ix)
    fresh = m.recommend(None, seq, candidates=cand, **kw)                   # from the current table
    _same(fresh, m.recommend(None, seq, candidates=cand, index=m.build_item_index(), **kw), "after the step")
    assert not np.array_equal(fresh[1], a[1])


def test_candidates_none_is_the_existing_code_path():
    itemnum, B, T, k = 500, 6, 20, 10
    m = H.model("cast_1", itemnum=itemnum)
    rs = np.random.RandomState(6)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    tg = rs.randint(1, itemnum + 1, B).astype(np.int32)
    kw = dict(k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, targets=tg)
    ix = m.build_item_index()
    _same(m.recommend(None, seq, **kw), m.recommend(None, seq, candidates=None, **kw), "recommend")
    _same(m.recommend(None, seq, index=ix, **kw), m.recommend(None, seq, index=ix, candidates=None, **kw), "recommend(index=)")
    _same(m.similar_items([1, 7, itemnum], 10), m.similar_items([1, 7, itemnum], 10, candidates=None), "similar_items")
    Q = rs.standard_normal((B, 50)).astype(np.float32)
    _same(ix.search(Q, k, targets=tg), ix.search(Q, k, targets=tg, candidates=None), "ItemIndex.search")
    assert ctypes.sizeof(L.TopkListsDesc) == ctypes.sizeof(L.TopkDesc)

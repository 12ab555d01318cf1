"""Cosine item indexes on the GPU (castrec.h CR_INDEX_COSINE; ItemIndex / ItemSubset metric="cosine"; Model.build_item_index /
refresh_item_index / similar_items(metric=)).  The writers' bytes are compared with tests/topk_cosine_ref.py through
topk_index_ref.build_blob -- byte equality, into poisoned and guarded buffers -- for the build and for every path that writes rows
(gather from the table, subset of an index, update from the table and from raw rows, sync, rebuild); the search of such an index is
held to fp64 on the rows it stores and to the fp64 cosine ranking; the model level returns cosines."""
import types

import numpy as np
import pytest
import torch

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd import ops as O
from castrec_amd.index import ItemIndex, ItemSubset
import topk_cosine_ref as C
import topk_harness as H
from topk_index_ref import build_blob, index_bytes

pytestmark = pytest.mark.gpu
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16
NAME = {SPLIT: "bf16x3", PLAIN: "bf16"}
GUARD = 256                                  # bytes of 0xA5 on either side of a blob: a store outside the blob shows


def _table(V, D, seed=0):
    """Normal rows scaled per row by 10^-3 .. 10^3; row 0 zero, and one more zero row where there is room."""
    rs = np.random.RandomState(1000 * V + D + seed)
    T = (rs.standard_normal((V, D)) * 10.0 ** rs.uniform(-3, 3, (V, 1))).astype(np.float32)
    T[0] = 0
    if V > 4:
        T[V // 2] = 0
    return T


def _cos_blob(T, prec):
    return build_blob(C.normalise(T), prec)


def _poisoned(nbytes):
    """0xA5 everywhere: (whole buffer, the blob's view).  What a writer leaves unwritten, or writes outside, shows."""
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _guarded(blob):
    buf, view = _poisoned(blob.size)
    view.copy_(torch.from_numpy(blob).cuda())
    return buf, view


def _check(buf, want, what):
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + want.size:] == 0xA5), (what, "a store outside the blob")
    bad = np.nonzero(got[GUARD:GUARD + want.size] != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:8] // 16)


def _dev_i32(a):
    return torch.from_numpy(np.asarray(a, np.int64).astype(np.int32)).cuda()


# ---- 5. build bytes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 20, 50, 64, 100, 256])
@pytest.mark.parametrize("V", [2, 17, 37])
def test_built_blob_equals_the_numpy_restatement(V, D):
    """Every NK (1, 1, 2, 2, 4, 8), D % 8 != 0 (the last row's partial chunk is re-read column by column), V % 16 != 0."""
    T = _table(V, D)
    t = H.table_in_nan_buffer(T)
    for prec in (SPLIT, PLAIN):
        want = _cos_blob(T, prec)
        assert want.size == index_bytes(V, D, prec) == O.topk_index_bytes(V, D, prec)
        buf, blob = _poisoned(want.size)
        O.topk_index_build(t, prec, out=blob, metric="cosine")
        _check(buf, want, (V, D, prec, "build"))
        buf2, blob2 = _poisoned(want.size)
        O.topk_index_build(t, prec, out=blob2, metric="cosine")
        torch.cuda.synchronize()
        assert torch.equal(blob, blob2)
        assert not np.array_equal(want, build_blob(T, prec))               # (it is not the dot index)


# ---- 9. dot is untouched (one assertion, beside a cosine build of the same table on the same run) ----------------------------------------
def test_a_dot_build_on_the_same_run_has_its_old_bytes():
    T = _table(37, 50)
    t = torch.from_numpy(T).cuda()
    for prec in (SPLIT, PLAIN):
        cos, dot = ItemIndex.build(t, NAME[prec], metric="cosine"), ItemIndex.build(t, NAME[prec])
        assert (cos.metric, dot.metric) == ("cosine", "dot")
        assert np.array_equal(dot.blob.cpu().numpy(), build_blob(T, prec))
        assert np.array_equal(cos.blob.cpu().numpy(), _cos_blob(T, prec))


# ---- 6. one set of bytes, every path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 50, 256])
def test_gathered_subsets_have_the_bytes_of_a_cosine_build_on_the_gathered_table(D):
    V = 37
    T = _table(V, D)
    t = H.table_in_nan_buffer(T)
    rs = np.random.RandomState(D)
    ids = rs.permutation(np.arange(1, V - 1))[:20].tolist() + [V - 1]       # a duplicate-free shuffle that holds the last row
    rs.shuffle(ids)
    G = np.concatenate([np.zeros((1, D), np.float32), T[sorted(ids)]])      # the gathered table {0; rows in ascending id order}
    for prec in (SPLIT, PLAIN):
        ref = ItemIndex.build(torch.from_numpy(G).cuda(), NAME[prec], metric="cosine")
        assert np.array_equal(ref.blob.cpu().numpy(), _cos_blob(G, prec))
        tab = ItemSubset.build(t, ids, NAME[prec], metric="cosine")
        ix = ItemIndex.build(t, NAME[prec], metric="cosine")
        sub = ix.subset(ids)
        for s, what in ((tab, "ItemSubset.build"), (sub, "ix.subset")):
            assert s.metric == s.index.metric == "cosine" and s.ids.cpu().tolist() == [0] + sorted(ids), what
            assert torch.equal(s.index.blob, ref.blob), (D, prec, what)
        # the C entry into a guarded buffer; from an index source the flag is accepted and ignored
        want = _cos_blob(G, prec)
        d_ids = _dev_i32(sorted(ids))
        for kw, what in ((dict(table=t, metric="cosine"), "table"), (dict(index=ix.blob, index_precision=prec, V=V, D=D, metric="cosine"), "index, flag"),
                         (dict(index=ix.blob, index_precision=prec, V=V, D=D), "index, no flag")):
            buf, out = _poisoned(want.size)
            O.topk_index_gather(d_ids, prec, out=out, **kw)
            _check(buf, want, (D, prec, what))


@pytest.mark.parametrize("D", [20, 50, 256])
def test_update_and_rebuild_end_as_a_fresh_cosine_build(D):
    V = 37
    A, Bt = _table(V, D), _table(V, D, seed=7)
    Bt[V // 2] = 1.5                                                        # a zero row becomes a row, a row becomes zero
    Bt[3] = 0
    tB = H.table_in_nan_buffer(Bt)
    rs = np.random.RandomState(D + 1)
    ids = [V - 1, 3, V // 2] + rs.randint(1, V, 9).tolist()                 # the last row, both zero-row changes, duplicates
    named = sorted(set(ids))
    M = A.copy()
    M[named] = Bt[named]
    for prec in (SPLIT, PLAIN):
        start, want = _cos_blob(A, prec), _cos_blob(M, prec)
        assert not np.array_equal(start, want)
        for form in ("table", "rows"):
            buf, blob = _guarded(start)
            ix = ItemIndex(V, D, NAME[prec], blob, metric="cosine")
            if form == "table":
                ix.update(ids, table=tB)
            else:
                ix.update(ids, rows=H.table_in_nan_buffer(Bt[ids]))       # raw rows, in list order
            _check(buf, want, (D, prec, form))                              # rows that are not listed keep their bytes
        buf, blob = _guarded(start)
        ItemIndex(V, D, NAME[prec], blob, metric="cosine").rebuild(tB)
        _check(buf, _cos_blob(Bt, prec), (D, prec, "rebuild"))
        # a dot index of the same tables is still written as a dot index
        buf, blob = _guarded(build_blob(A, prec))
        ItemIndex(V, D, NAME[prec], blob).update(ids, table=tB)
        _check(buf, build_blob(M, prec), (D, prec, "dot update"))


SINCE = 5


@pytest.mark.parametrize("V,D", [(37, 20), (37, 50), (37, 256), (3417, 50)])
def test_sync_rewrites_the_flagged_tiles_as_a_cosine_build(V, D):
    A, Bt = _table(V, D), _table(V, D, seed=7)
    tB = H.table_in_nan_buffer(Bt)
    rs = np.random.RandomState(V + D)
    flags = rs.choice(np.array([0, SINCE - 1, SINCE, SINCE + 1], np.int32), V, p=[0.9, 0.04, 0.03, 0.03]).astype(np.int32)
    flags[V - 1] = SINCE
    hit = sorted(set((np.nonzero(flags >= SINCE)[0] // 16).tolist()))
    if V > 1000:
        assert 0 < len(hit) < (V + 15) // 16                                # untouched tiles exist
    M = A.copy()
    for tile in hit:
        M[16 * tile:16 * tile + 16] = Bt[16 * tile:16 * tile + 16]
    fbuf = torch.full((V + 64,), SINCE + 1, dtype=torch.int32, device="cuda")  # what follows the flags says "touched": not read
    fbuf[:V] = torch.from_numpy(flags).cuda()
    for prec in (SPLIT, PLAIN):
        buf, blob = _guarded(_cos_blob(A, prec))
        ItemIndex(V, D, NAME[prec], blob, metric="cosine").sync(tB, fbuf[:V], SINCE)
        _check(buf, _cos_blob(M, prec), (V, D, prec, "sync"))               # tiles without a flagged row keep their bytes


# ---- 7. scale invariance on the device -----------------------------------------------------------------------------------------------------
def test_a_power_of_two_per_row_changes_no_byte_on_the_device():
    V, D = 37, 50
    T = _table(V, D)
    s = 2.0 ** np.random.RandomState(1).randint(-10, 11, (V, 1))
    T2 = (T * s).astype(np.float32)
    assert np.array_equal(T2.astype(np.float64), T.astype(np.float64) * s)
    for prec in ("bf16x3", "bf16"):
        a = ItemIndex.build(torch.from_numpy(T).cuda(), prec, metric="cosine")
        b = ItemIndex.build(torch.from_numpy(T2).cuda(), prec, metric="cosine")
        assert torch.equal(a.blob, b.blob)
        assert not torch.equal(ItemIndex.build(torch.from_numpy(T).cuda(), prec).blob, ItemIndex.build(torch.from_numpy(T2).cuda(), prec).blob)


# ---- 8. search -------------------------------------------------------------------------------------------------------------------------------
def _complement(rows, V):
    return [sorted(set(range(1, V)) - set(int(i) for i in r)) for r in rows]


@pytest.mark.parametrize("D", [20, 64, 256])
def test_search_of_a_cosine_index(D):
    V, B, K = 3417, 33, 10
    rs = np.random.RandomState(D)
    T = _table(V, D)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = H.excl_lists(rs, B, V, 20)
    tg = H.targets(rs, B, V, excl)
    ix = ItemIndex.build(torch.from_numpy(T).cuda(), metric="cosine")
    stored = C.stored_rows(ix.blob.cpu().numpy(), V, D, SPLIT)
    ids, scores, rank = ix.search(Q, K, exclude=excl, targets=tg)
    H.check_fp64(Q, stored, K, excl, ids, scores)                          # the scores are dot products with the stored rows
    # ... and the ids are the fp64 cosine top-K, up to the items within the harness's tolerance of the K-th score
    T64 = T.astype(np.float64)
    n = np.sqrt((T64 * T64).sum(1, keepdims=True))
    Y = np.divide(T64, n, out=np.zeros_like(T64), where=n > 0)
    S = Q.astype(np.float64) @ Y.T                                         # cos(q, x) ||q||: the cosine order within a row
    Ab = np.abs(Q.astype(np.float64)) @ np.abs(Y).T
    for b in range(B):
        ex = set(int(e) for e in excl[b]) | {0}
        elig = np.array([i for i in range(V) if i not in ex])
        n_real = min(K, elig.size)
        if n_real == 0:
            continue
        tol = H.REL * float(Ab[b, 1:].max())
        order = elig[np.lexsort((elig, -S[b, elig]))]
        kth = S[b, order[n_real - 1]]
        got = set(ids[b, :n_real].tolist())
        sure = set(order[:n_real][S[b, order[:n_real]] > kth + 2 * tol].tolist())
        assert sure <= got, (b, sure - got)
        assert all(S[b, i] >= kth - 2 * tol for i in got), b
    # allow= and candidates=: the bits of the full search restricted to those items
    allow = rs.choice(np.arange(1, V), 700, replace=False).tolist() + [V - 1]
    full = [list(e) + c for e, c in zip(excl, _complement([allow] * B, V))]
    H.same_bits(ix.search(Q, K, exclude=full, targets=tg), ix.search(Q, K, exclude=excl, targets=tg, allow=allow), (D, "allow="))
    rows = [rs.choice(np.arange(1, V), rs.randint(1, 300), replace=False).tolist() for _ in range(B)]
    rows[0] = rows[0] + [int(tg[0])]
    full = [list(e) + c for e, c in zip(excl, _complement(rows, V))]
    H.same_bits(ix.search(Q, K, exclude=full, targets=tg), ix.search(Q, K, exclude=excl, targets=tg, candidates=rows), (D, "candidates="))


# ---- 10. model level -------------------------------------------------------------------------------------------------------------------------
def _fp64_cosines(table):
    T64 = table.astype(np.float64)
    n = np.sqrt((T64 * T64).sum(1, keepdims=True))
    Y = np.divide(T64, n, out=np.zeros_like(T64), where=n > 0)
    return Y @ Y.T, np.abs(Y) @ np.abs(Y).T


def _check_similar(items, top, sc, Cm, Am, k, what, among=None):
    """top / sc against the fp64 cosines Cm: the item itself absent, scores within 2^-15 + REL sum |y_q y_i| of the cosine and inside
    [-1, 1] by that margin, and the ids the fp64 top-k up to items within that tolerance of the k-th (check_fp64's tie rule)."""
    V = Cm.shape[0]
    assert top.shape == sc.shape == (len(items), k) and sc.dtype == np.float32
    assert np.all(np.abs(sc) <= 1 + 2.0 ** -15), (what, float(np.abs(sc).max()))
    for r, it in enumerate(items):
        elig = np.array(sorted((set(range(1, V)) if among is None else set(among[r] if isinstance(among[0], (list, tuple, np.ndarray)) else among)) - {it}))
        n_real = min(k, elig.size)
        got = top[r, :n_real].astype(np.int64)
        assert it not in top[r].tolist() and len(set(got.tolist())) == n_real and set(got.tolist()) <= set(elig.tolist()), (what, r)
        assert np.all(top[r, n_real:] == 0) and np.all(np.isneginf(sc[r, n_real:])), (what, r)
        tol = 2.0 ** -15 + H.REL * float(Am[it, 1:].max())
        assert np.all(np.abs(sc[r, :n_real] - Cm[it, got]) <= 2.0 ** -15 + H.REL * Am[it, got]), (what, r, np.abs(sc[r, :n_real] - Cm[it, got]).max())
        order = elig[np.lexsort((elig, -Cm[it, elig]))]
        kth = Cm[it, order[n_real - 1]]
        sure = set(order[:n_real][Cm[it, order[:n_real]] > kth + 2 * tol].tolist())
        assert sure <= set(got.tolist()), (what, r, sure - set(got.tolist()))
        assert np.all(Cm[it, got] >= kth - 2 * tol), (what, r)


def test_similar_items_returns_cosines():
    itemnum = 500
    m = H.model("sasrec", itemnum=itemnum)
    table = m.get_params()["item_emb"].cpu().numpy()
    Cm, Am = _fp64_cosines(table)
    items = [1, 7, 250, itemnum]
    top, sc = m.similar_items(items, 5, metric="cosine")
    _check_similar(items, top, sc, Cm, Am, 5, "metric=cosine")
    # metric=None without an index is still the dot product
    H.same_bits(m.similar_items(items, 5), m.similar_items(items, 5, metric="dot"), "metric=None is dot")
    cos_ix, dot_ix = m.build_item_index(metric="cosine"), m.build_item_index()
    assert (cos_ix.metric, dot_ix.metric) == ("cosine", "dot")
    H.same_bits((top, sc), m.similar_items(items, 5, index=cos_ix), "index=cosine index, metric=None")
    H.same_bits((top, sc), m.similar_items(items, 5, index=cos_ix, metric="cosine"), "index=cosine index, metric=cosine")
    with pytest.raises(ValueError, match="dot.*cosine|cosine.*dot"):
        m.similar_items(items, 5, index=cos_ix, metric="dot")
    with pytest.raises(ValueError, match="dot.*cosine|cosine.*dot"):
        m.similar_items(items, 5, index=dot_ix, metric="cosine")
    with pytest.raises(ValueError, match="metric"):
        m.similar_items(items, 5, metric="l2")
    # allow= ids without an index: the subset is built with the metric; an ItemSubset carries its own
    allow = list(range(3, itemnum, 3)) + [itemnum]
    a = m.similar_items(items, 5, allow=allow, metric="cosine")
    _check_similar(items, a[0], a[1], Cm, Am, 5, "allow=", among=allow)
    sub = cos_ix.subset(allow)
    H.same_bits(a, m.similar_items(items, 5, allow=sub), "allow=cosine ItemSubset")
    H.same_bits(a, m.similar_items(items, 5, allow=allow, index=cos_ix), "allow= out of the cosine index")
    with pytest.raises(ValueError, match="dot.*cosine|cosine.*dot"):
        m.similar_items(items, 5, allow=sub, metric="dot")
    # candidates= without an index: a cosine index is built for the call
    cand = [list(range(1 + r, itemnum, 7)) + [it] for r, it in enumerate(items)]
    c = m.similar_items(items, 5, candidates=cand, metric="cosine")
    _check_similar(items, c[0], c[1], Cm, Am, 5, "candidates=", among=cand)
    H.same_bits(c, m.similar_items(items, 5, candidates=cand, index=cos_ix), "candidates=, index=cosine index")
    # a query row of norm 0 gets scores 0
    P = {n: v.cpu().numpy() for n, v in m.get_params().items()}
    P["item_emb"][7] = 0
    m.load_params(P)
    z = m.similar_items([7, 1], 5, metric="cosine")
    assert np.all(z[1][0] == 0) and np.all(z[1][1] != 0)
    # recommend takes a cosine index
    rs = np.random.RandomState(0)
    seq, ts, hrs, dys = H.inputs(rs, 4, 20, itemnum)
    cos_ix = m.build_item_index(metric="cosine")
    top, scr = m.recommend(None, seq, k=5, index=cos_ix)
    eng = m._eval_engine(4, False)                                       # (Engine.topk's queries: the last position of every sequence)
    want = cos_ix.search(eng.seq_emb[eng.T - 1::eng.T][:, :eng.D].contiguous(), 5, exclude=[r[r != 0] for r in seq.astype(np.int64)])
    H.same_bits((top, scr), want, "recommend(index=cosine index)")


ITEMNUM, T_, D_, B_, N_ = 2000, 20, 16, 8, 32


def _model(**kw):
    """The smallest model the whole-model tests train: SASRec, one block, D 16, 2000 items."""
    from castrec_amd.models import build_model
    args = dict(maxlen=T_, hidden_units=D_, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-2, max_bins=20,
                num_context_blocks=1, seed=1, ce_negatives=N_)
    args.update(kw)
    return build_model("sasrec", 10, ITEMNUM, 0, types.SimpleNamespace(**args))


def _train(m, seeds):
    for s in seeds:
        rs = np.random.RandomState(s)
        seq, pos, neg = (rs.randint(1, ITEMNUM + 1, (B_, T_)).astype(np.int32) for _ in range(3))
        for a in (seq, pos, neg):
            a[:, :3] = 0
        m.train_step(None, seq, pos, neg)


def test_row_sparse_training_syncs_a_cosine_index(tmp_path, monkeypatch):
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    m = _model(loss="sampled_ce", row_sparse_adam=True)
    ix = m.build_item_index(metric="cosine")
    first, token = ix.save(str(tmp_path / "first.npz")), ix.token
    before, ptr = ix.blob.clone(), ix.blob.data_ptr()
    assert np.array_equal(before.cpu().numpy(), _cos_blob(m.get_params()["item_emb"].cpu().numpy(), ix.prec))
    _train(m, (1, 2, 3))
    assert m._train.lazy_adam
    assert m.refresh_item_index(ix) == "sync"
    fresh = m.build_item_index(metric="cosine")
    assert ix.metric == "cosine" and ix.blob.data_ptr() == ptr and not torch.equal(ix.blob, before) and torch.equal(ix.blob, fresh.blob)
    assert np.array_equal(ix.blob.cpu().numpy(), _cos_blob(m.get_params()["item_emb"].cpu().numpy(), ix.prec))
    assert not torch.equal(ix.blob, m.build_item_index().blob)
    # the delta -- raw rows -- applied where no table is: a saved-and-loaded copy of the first index
    ids, rows, _ = m.item_delta(token)
    far = ItemIndex.load(first)
    assert far.metric == "cosine" and torch.equal(far.blob, before)
    far.update(ids, rows=rows)
    assert torch.equal(far.blob, fresh.blob)


def test_dense_training_rebuilds_a_cosine_index(monkeypatch):
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    m = _model()
    ix = m.build_item_index(metric="cosine")
    ptr, before = ix.blob.data_ptr(), ix.blob.clone()
    _train(m, (1, 2, 3))
    assert not m._train.lazy_adam
    assert m.refresh_item_index(ix) == "rebuild"
    assert ix.blob.data_ptr() == ptr and not torch.equal(ix.blob, before)
    assert torch.equal(ix.blob, m.build_item_index(metric="cosine").blob) and ix.metric == "cosine"

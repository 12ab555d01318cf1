"""Shared candidate subsets on the GPU (castrec.h cr_topk_index_gather; castrec_amd.index.ItemSubset, ItemIndex.subset / search(allow=);
Model.recommend(allow=), similar_items(allow=)).  Two properties carry everything: the gathered sub-index is, byte for byte, the index
cr_topk_index_build makes of the gathered table, and a search of it returns the ids, score bits and ranks of the full search with the
subset's complement excluded."""
import numpy as np
import pytest
import torch

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd import ops as O
from castrec_amd.index import ItemIndex, ItemSubset, subset_ids
import topk_harness as H
import topk_index_ref as R
from topk_harness import same_bits as _same

pytestmark = pytest.mark.gpu
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16
NAME = {SPLIT: "bf16x3", PLAIN: "bf16"}
DS = [8, 20, 50, 64, 128, 256]                 # NK 1, 1, 2, 2, 4, 8
VS = [100, 3417]
NS = [1, 15, 16, 37]                           # n + 1 = 2; exactly one tile; one row into a second tile; a ragged third tile


def _pick(rs, V, n):
    """n ids with V - 1, 1 and both sides of a source tile boundary among them (n = 1: the last row alone)."""
    if n == 1:
        return [V - 1]
    must = [1, 15, 16, 17, V - 1]
    rest = rs.choice([i for i in range(2, V - 1) if i not in must], n - len(must), replace=False)
    return rs.permutation(must + rest.tolist()).tolist()


def _gather_checked(ids_dev, prec, want, what, **src):
    """topk_index_gather into stale bytes with a guard behind: the whole blob is written, padding included, and nothing past it."""
    n = want.size
    out = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    O.topk_index_gather(ids_dev, prec, out=out[:n], **src)
    again = O.topk_index_gather(ids_dev, prec, **src)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want), (what, np.nonzero(got[:n] != want)[0][:8])
    assert np.all(got[n:] == 0xA5), (what, "the gather wrote past the blob")
    assert np.array_equal(again.cpu().numpy(), want), what


@pytest.mark.parametrize("D", DS)
def test_gathered_sub_index_has_the_bytes_of_a_build_on_the_gathered_table(D):
    rs = np.random.RandomState(100 + D)
    for V in VS:
        T = rs.standard_normal((V, D)).astype(np.float32)                   # row 0 is NOT zero: local row 0 must be written as +0
        T[1, 0] = -0.0
        t = H.table_in_nan_buffer(T)
        ix = {p: O.topk_index_build(t, p) for p in (SPLIT, PLAIN)}
        for n in NS:
            for ids in ([_pick(rs, V, n)] + ([[1], [16]] if n == 1 else [])):
                m = subset_ids(ids, V)
                ids_dev = torch.from_numpy(m).cuda()[1:]
                G = np.concatenate([np.zeros((1, D), np.float32), T[m[1:]]])
                g = torch.cat([torch.zeros(1, D, device="cuda"), t[ids_dev.long()]])
                for prec in (SPLIT, PLAIN):
                    want = R.build_blob(G, prec)
                    assert want.size == O.topk_index_bytes(n + 1, D, prec)
                    assert np.array_equal(O.topk_index_build(g, prec).cpu().numpy(), want)
                    _gather_checked(ids_dev, prec, want, (D, V, n, prec, "from the table"), table=t)
                    _gather_checked(ids_dev, prec, want, (D, V, n, prec, "from an index"), index=ix[prec], index_precision=prec, V=V, D=D)
                _gather_checked(ids_dev, PLAIN, R.build_blob(G, PLAIN), (D, V, n, "plain out of a split index"),
                                index=ix[SPLIT], index_precision=SPLIT, V=V, D=D)
        with pytest.raises(RuntimeError, match="plain"):                    # a plain index has no lo plane to give
            O.topk_index_gather(ids_dev, SPLIT, index=ix[PLAIN], index_precision=PLAIN, V=V, D=D)
        # every item: the full index (of a table whose padding row is zero, as an item table's is)
        T0 = T.copy()
        T0[0] = 0.0
        t0 = H.table_in_nan_buffer(T0)
        every = torch.arange(1, V, dtype=torch.int32, device="cuda")
        for prec in (SPLIT, PLAIN):
            full = O.topk_index_build(t0, prec)
            want = full.cpu().numpy()
            assert np.array_equal(want, R.build_blob(T0, prec))
            _gather_checked(every, prec, want, (D, V, "every item, table"), table=t0)
            _gather_checked(every, prec, want, (D, V, "every item, index"), index=full, index_precision=prec, V=V, D=D)


def _case(rs, V, ids, B):
    """Exclusion rows and targets (global ids) for a subset `ids`: ids inside and outside it, 0, ids >= V, duplicates; targets inside,
    outside, excluded.  Returns (exclude, exclude united with the complement, targets, the rows whose rank must be -1)."""
    inside = sorted(set(ids))
    outside = [i for i in range(1, V) if i not in set(inside)]
    excl = [[] for _ in range(B)]
    excl[1] = rs.choice(inside, min(3, len(inside)), replace=False).tolist() + rs.choice(outside, 5).tolist() + [0, V, V + 7]
    excl[1] += excl[1][:2]
    excl[3] = inside[: max(0, len(inside) - 3)] + outside[:4]             # fewer than K eligible
    excl[4] = rs.choice(outside, 6).tolist()
    tg = np.array([inside[rs.randint(len(inside))] for _ in range(B)], np.int32)
    tg[0] = inside[-1]
    tg[1] = outside[rs.randint(len(outside))]                               # outside the subset: -1
    excl[2] = [int(tg[2]), outside[0]]                                      # an excluded target: -1
    tg[3] = inside[-1]                                                      # survives row 3's exclusions
    full = [sorted(set(r) | set(outside)) for r in excl]
    return excl, full, tg, (1, 2)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("V", VS)
def test_subset_search_is_the_full_search_restricted(D, V):
    rs = np.random.RandomState(D * 13 + V)
    B, K = 5, 10
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    T[0] = 0.0
    t = torch.from_numpy(T).cuda()
    Q = rs.standard_normal((B, D)).astype(np.float32)
    for prec in (SPLIT, PLAIN):
        ix = ItemIndex.build(t, NAME[prec], version=5)
        for n in NS:
            ids = _pick(rs, V, n)
            excl, full, tg, minus = _case(rs, V, ids, B)
            want = ix.search(Q, K, exclude=full, targets=tg)                # existing code: the yardstick
            sub = ix.subset(ids + ids[:1])
            assert (sub.parent_V, sub.D, sub.precision, sub.version, sub.index.V) == (V, D, NAME[prec], 5, n + 1)
            assert sub.ids.is_cuda and sub.ids.dtype == torch.int32 and sub.ids.cpu().tolist() == [0] + sorted(ids)
            got = sub.search(Q, K, exclude=excl, targets=tg)
            _same(want, got, (D, V, n, prec, "subset of the index"))
            assert all(got[2][b] == -1 for b in minus) and got[2][0] >= 0 and got[2][3] >= 0
            assert set(got[0].ravel().tolist()) <= set(ids) | {0}
            if n < K:                                                       # K > n: the tail is id 0, score -inf
                assert np.all(got[0][:, n:] == 0) and np.all(np.isneginf(got[1][:, n:]))
                assert set(got[0][0, :n].tolist()) == set(got[0][4, :n].tolist()) == set(ids)
            assert np.all(got[0][3, 3:] == 0) and np.all(np.isneginf(got[1][3, 3:])) and np.all(got[0][3, :min(3, n)] > 0)
            tab = ItemSubset.build(t, ids, NAME[prec])                      # the table form: no index at all
            assert torch.equal(tab.index.blob, sub.index.blob) and torch.equal(tab.ids, sub.ids) and tab.version is None
            _same(want, tab.search(Q, K, exclude=excl, targets=tg), (D, V, n, prec, "subset of the table"))
            _same(want, ix.search(Q, K, exclude=excl, targets=tg, allow=ids), (D, V, n, prec, "allow="))
            _same(ix.search(Q, K, exclude=full), sub.search(torch.from_numpy(Q).cuda(), K, exclude=excl), (D, V, n, prec, "no targets"))
            _same(ix.search(Q, K, exclude=[full[0]] * B, targets=tg), sub.search(Q, K, targets=tg), (D, V, n, prec, "no exclusions"))
    split = ItemIndex.build(t)
    sub = split.subset(ids)                                                 # a plain search of a split subset
    _same(split.search(Q, K, exclude=full, targets=tg, precision="bf16"), sub.search(Q, K, exclude=excl, targets=tg, precision="bf16"),
          (D, V, "plain search of a split subset"))


def test_subset_refusals():
    t = torch.randn(100, 50, device="cuda")
    ix = ItemIndex.build(t)
    for bad in ([], [0], [100], [-1], [5, 100]):
        with pytest.raises(ValueError):
            ix.subset(bad)
        with pytest.raises(ValueError):
            ItemSubset.build(t, bad)
        with pytest.raises(ValueError):
            ix.search(np.zeros((1, 50), np.float32), 3, allow=bad)
    with pytest.raises(RuntimeError, match="plain"):
        ItemIndex.build(t, "bf16").subset([1, 2]).search(np.zeros((1, 50), np.float32), 3, precision="bf16x3")


def test_duplicate_rows_inside_the_subset_tie_towards_the_smaller_global_id():
    rs = np.random.RandomState(4)
    V, D, B, K = 100, 50, 5, 10
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    T[0] = 0.0
    T[60] = T[40] = T[20]                                                   # 40 stays outside the subset
    T[99] = T[17] = T[16]
    Q = rs.standard_normal((B, D)).astype(np.float32)
    Q[0] = 30 * T[20]
    Q[1] = 30 * T[16]
    ids = [99, 60, 20, 17, 16] + rs.choice([i for i in range(1, 99) if i not in (16, 17, 20, 40, 60)], 32, replace=False).tolist()
    outside = sorted(set(range(1, V)) - set(ids))
    t = torch.from_numpy(T).cuda()
    ix = ItemIndex.build(t)
    tg = np.array([60, 99, 20, 17, 16], np.int32)
    want = ix.search(Q, K, exclude=[outside] * B, targets=tg)
    for sub in (ix.subset(ids), ItemSubset.build(t, ids)):
        got = sub.search(Q, K, targets=tg)
        _same(want, got, "ties")
        assert got[0][0, :2].tolist() == [20, 60] and got[1][0, 0] == got[1][0, 1] and got[2][0] == 1
        assert got[0][1, :3].tolist() == [16, 17, 99] and got[1][1, 0] == got[1][1, 2] and got[2][1] == 2


def test_subset_search_against_fp64_brute_force():
    """The returned set against an fp64 ranking of the subset's rows, with the tolerance rule of the full search (DESIGN.md section 10:
    1e-5 of sum_i |q_i t_i|): every score within it, everything surely in the top K returned, nothing surely outside it returned."""
    rs = np.random.RandomState(9)
    V, D, B, K = 100, 50, 5, 10
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    T[0] = 0.0
    Q = rs.standard_normal((B, D)).astype(np.float32)
    ids = _pick(rs, V, 37)
    excl = [[], ids[:5], [3, 0, 200], ids[:30], ids[5:9]]
    t = torch.from_numpy(T).cuda()
    outside = set(range(1, V)) - set(ids)                                   # eligible: the subset's items the row does not exclude
    for sub in (ItemIndex.build(t).subset(ids), ItemSubset.build(t, ids)):
        got_i, got_s = sub.search(Q, K, exclude=excl)
        H.check_fp64(Q, T, K, [set(r) | outside for r in excl], got_i, got_s)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
def test_model_recommend_and_similar_items_with_allow(tmp_path):
    itemnum, B, T, k = 500, 9, 20, 12
    m = H.model("cast_1", itemnum=itemnum)
    rs = np.random.RandomState(5)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    allow = rs.choice(np.arange(1, itemnum + 1), 120, replace=False).tolist() + [1, itemnum, 15, 16, 17]
    allow[7] = int(seq[0][seq[0] != 0][0])                                  # an allowed item of row 0's history
    inside = set(allow)
    outside = sorted(set(range(1, itemnum + 1)) - inside)
    hist = [set(r[r != 0].tolist()) for r in seq.astype(np.int64)]
    tg = np.array([sorted(inside - hist[b])[3 * b] for b in range(B)], np.int32)       # allowed and not in the row's history
    tg[1] = outside[0]                                                      # a target outside the subset
    tg[0] = allow[7]                                                        # a target in the history
    kw = dict(k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, targets=tg)
    ix = m.build_item_index()
    sub = ix.subset(allow)
    assert sub.version == ix.version is not None and sub.parent_V == itemnum + 1
    # the full search with (history united with the complement) excluded: existing code
    want = m.recommend(None, seq, exclude=[sorted(h | set(outside)) for h in hist], **kw)
    a = m.recommend(None, seq, allow=allow, **kw)
    _same(want, a, "allow=ids, no index")
    _same(a, m.recommend(None, seq, allow=allow, index=ix, **kw), "allow=ids, index=ix")
    _same(a, m.recommend(None, seq, allow=sub, **kw), "allow=ItemSubset")
    _same(a, m.recommend(None, seq, allow=iter(allow), exclude="history", **kw), "an iterator; exclude='history' spelled out")
    _same(a, m.recommend(None, seq, index=sub, **kw), "index=ItemSubset")
    assert a[2][0] == a[2][1] == -1 and np.all(a[2][2:] >= 0)
    for b in range(B):
        got = set(a[0][b].tolist())
        assert got <= inside and not (got & hist[b]) and 0 not in got
    none = m.recommend(None, seq, allow=allow, exclude=None, **kw)          # without the history exclusion
    _same(m.recommend(None, seq, exclude=[outside] * B, **kw), none, "allow=ids, exclude=None")
    assert none[2][0] >= 0
    ids_only = m.recommend(None, seq, k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, allow=sub, return_scores=False)
    assert np.array_equal(ids_only, a[0])

    # similar items among the allowed ones: never the item itself, never an id outside the subset
    items = np.array([1, allow[3], outside[1], itemnum], np.int64)
    ref = None
    for use_index, al in ((None, allow), (ix, allow), (None, sub), (ix, sub)):
        sid, ssc = m.similar_items(items, k=10, index=use_index, allow=al)
        assert sid.shape == ssc.shape == (4, 10)
        for r, it in enumerate(items):
            assert it not in sid[r] and set(sid[r].tolist()) <= inside and len(set(sid[r].tolist())) == 10
        ref = ref or (sid, ssc)
        _same(ref, (sid, ssc), "similar_items(allow=)")
    _same(ref, ix.search(m.get_params()["item_emb"].cpu()[torch.from_numpy(items)], 10,
                         exclude=[sorted(set(outside) | {int(i)}) for i in items]), "similar_items against the full search")

    # save / load on the device: equal arrays; version None after a load
    p = sub.save(str(tmp_path / "allowed.npz"))
    back = ItemSubset.load(p)
    assert back.index.blob.is_cuda and back.ids.is_cuda and back.version is None and back.parent_V == itemnum + 1
    assert torch.equal(back.index.blob, sub.index.blob) and torch.equal(back.ids, sub.ids)
    Q = rs.standard_normal((B, 50)).astype(np.float32)
    _same(sub.search(Q, k, exclude=[list(h) for h in hist], targets=tg), back.search(Q, k, exclude=[list(h) for h in hist], targets=tg), "loaded")
    _same(a, m.recommend(None, seq, allow=back, **kw), "allow=a loaded ItemSubset")
    with pytest.raises(ValueError, match="format"):
        ItemIndex.load(p)
    with pytest.raises(ValueError):
        m.recommend(None, seq, allow=[0, 5], **kw)
    with pytest.raises(ValueError):
        m.recommend(None, seq, allow=[itemnum + 1], **kw)
    other = H.model("cast_1", itemnum=itemnum + 1)
    with pytest.raises(ValueError):
        other.recommend(None, seq, allow=sub, **kw)

    # a training step makes the subset stale, as it does the index it came from
    pos = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    neg = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    m.train_step(None, seq, pos, neg, ts, hrs, dys)
    for call in (lambda: m.recommend(None, seq, allow=sub, **kw), lambda: m.recommend(None, seq, allow=allow, index=ix, **kw),
                 lambda: m.similar_items(items, allow=sub), lambda: m.recommend(None, seq, index=sub, **kw)):
        with pytest.raises(RuntimeError, match="stale index"):
            call()
    fresh = m.recommend(None, seq, allow=allow, **kw)                       # gathered from the current table
    _same(fresh, m.recommend(None, seq, allow=m.build_item_index().subset(allow), **kw), "after the step")
    assert not np.array_equal(fresh[1], a[1])


def test_allow_none_is_the_existing_code_path():
    itemnum, B, T, k = 500, 6, 20, 10
    m = H.model("cast_1", itemnum=itemnum)
    rs = np.random.RandomState(6)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    tg = rs.randint(1, itemnum + 1, B).astype(np.int32)
    kw = dict(k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, targets=tg)
    ix = m.build_item_index()
    _same(m.recommend(None, seq, **kw), m.recommend(None, seq, allow=None, **kw), "recommend")
    _same(m.recommend(None, seq, index=ix, **kw), m.recommend(None, seq, index=ix, allow=None, **kw), "recommend(index=)")
    items = [1, 7, itemnum]
    _same(m.similar_items(items, 10), m.similar_items(items, 10, allow=None), "similar_items")
    _same(m.similar_items(items, 10, index=ix), m.similar_items(items, 10, index=ix, allow=None), "similar_items(index=)")
    Q = rs.standard_normal((B, 50)).astype(np.float32)
    excl = [rs.randint(0, itemnum + 3, 10).tolist() for _ in range(B)]
    _same(ix.search(Q, k, exclude=excl, targets=tg), ix.search(Q, k, exclude=excl, targets=tg, allow=None), "ItemIndex.search")
    _same(ix.search(Q, k), ix.search(Q, k, allow=None), "ItemIndex.search, queries alone")
    eng = m._eval_engine(B, False)
    a = eng.topk(k, None, None, tg, index=ix)
    b = eng.topk(k, None, None, tg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))

"""Keeping an item index in step with training, on the GPU (castrec.h cr_topk_index_update, cr_topk_index_sync; ItemIndex.update / sync
/ rebuild; Model.refresh_item_index / item_delta; util.evaluate_full(use_index=ItemIndex)).  Everything is byte equality against
tests/topk_index_ref.py: a row's groups depend on that row alone, so the expected blob after an update is build_blob of the table
that has B's rows where the list (or, for sync, a flagged tile) names them and A's elsewhere."""
import types

import numpy as np
import pytest
import torch

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd import ops as O
from castrec_amd.index import ItemIndex
import topk_harness as H
import topk_index_ref as R
from topk_index_ref import build_blob, group_offset, index_bytes

pytestmark = pytest.mark.gpu
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16
GUARD = 256                                  # bytes of 0xA5 on either side of a blob: a store outside the blob shows


def _tables(V, D):
    """A and B: two tables that differ in every element."""
    rs = np.random.RandomState(1000 * V + D)
    A = rs.standard_normal((V, D)).astype(np.float32)
    Bt = (rs.standard_normal((V, D)) + 3.0 * np.sign(A)).astype(np.float32)
    assert np.all(A != Bt)
    return A, Bt


def _guarded(blob):
    """The numpy blob on the device between guard bytes: (whole buffer, the blob's view)."""
    buf = torch.full((blob.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + blob.size] = torch.from_numpy(blob).cuda()
    return buf, buf[GUARD:GUARD + blob.size]


def _check(buf, want, what):
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + want.size:] == 0xA5), (what, "a store outside the blob")
    bad = np.nonzero(got[GUARD:GUARD + want.size] != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:8] // 16)


def _dev_i32(a):
    return torch.from_numpy(np.asarray(a, np.int64).astype(np.int32)).cuda()


def _lists(V, rs):
    """n = 1; n = 17 (the second wave partly filled); and the last row (its column-by-column re-read), row 0, duplicates and the ids
    that are skipped: -1, V and 2^31 - 1 -- ending in a named row, so that the packed source's last row is one that is read."""
    dup = int(rs.randint(0, V))
    return [[V - 1], rs.randint(0, V, 17).tolist(), [V - 1, 0, dup, dup, -1, V, 2 ** 31 - 1, V // 2, dup, V - 1]]


@pytest.mark.parametrize("D", [8, 20, 50, 64, 100, 256])
@pytest.mark.parametrize("V", [2, 17, 37])
def test_update_rewrites_exactly_the_listed_rows(V, D):
    """Every NK (1, 1, 2, 2, 4, 8), D % 8 != 0, a last tile that is not full; both precisions; the table form and the packed form."""
    A, Bt = _tables(V, D)
    rs = np.random.RandomState(V + D)
    tB = H.table_in_nan_buffer(Bt)
    for prec in (SPLIT, PLAIN):
        start = build_blob(A, prec)
        assert start.size == index_bytes(V, D, prec)
        for ids in _lists(V, rs):
            named = sorted(set(i for i in ids if 0 <= i < V))
            M = A.copy()
            M[named] = Bt[named]
            want = build_blob(M, prec)
            d_ids = _dev_i32(ids)
            packed = np.full((len(ids), D), 7.0, np.float32)              # (the rows of skipped ids are not read: anything)
            for j, i in enumerate(ids):
                if 0 <= i < V:
                    packed[j] = Bt[i]
            for src, pk in ((tB, False), (H.table_in_nan_buffer(packed), True)):
                buf, blob = _guarded(start)
                O.topk_index_update(blob, V, D, prec, d_ids, src, pk)
                _check(buf, want, (V, D, prec, ids, pk))
            # the padding stays +0: rows >= V of the last tile, columns >= D of the last k-step
            t, NK = (V - 1) // 16, R.tk_nk(D)
            for h in range(R.planes(prec)):
                for lane in range(64):
                    g = want[group_offset(V, D, h, t, NK - 1, lane):][:16].view(np.uint16)
                    row, col = 16 * t + (lane & 15), 32 * (NK - 1) + 8 * (lane >> 4)
                    assert np.all(g[[row >= V or col + j >= D for j in range(8)]] == 0)


def test_update_checks_its_tensors():
    A, _ = _tables(17, 20)
    blob, t = torch.from_numpy(build_blob(A, SPLIT)).cuda(), torch.from_numpy(A).cuda()
    ids = _dev_i32([1, 2])
    with pytest.raises(TypeError):
        O.topk_index_update(blob, 17, 20, SPLIT, ids.long(), t, False)
    with pytest.raises(TypeError):
        O.topk_index_update(blob, 17, 20, SPLIT, ids, t.double(), False)
    with pytest.raises(TypeError):
        O.topk_index_update(blob.cpu(), 17, 20, SPLIT, ids, t, False)
    with pytest.raises(ValueError):
        O.topk_index_update(blob, 17, 20, SPLIT, ids, t, True)             # packed rows are [n, D]
    with pytest.raises(ValueError):
        O.topk_index_update(blob, 17, 20, SPLIT, ids, t[:, ::2], False)
    with pytest.raises(ValueError):
        O.topk_index_update(blob, 17, 20, PLAIN, ids, t, False)            # the split blob is no plain index
    with pytest.raises(ValueError):
        O.topk_index_update(blob, 17, 20, SPLIT, ids[:0], t, False)
    with pytest.raises(TypeError):
        O.topk_index_sync(blob, t, SPLIT, torch.zeros(17, device="cuda"), 1)
    with pytest.raises(ValueError):
        O.topk_index_sync(blob, t, SPLIT, torch.zeros(18, dtype=torch.int32, device="cuda"), 1)
    assert np.array_equal(blob.cpu().numpy(), build_blob(A, SPLIT))


SINCE = 5


def _flag_patterns(V, rs):
    mixed = rs.choice(np.array([0, SINCE - 1, SINCE, SINCE + 1], np.int32), V, p=[0.9, 0.04, 0.03, 0.03]).astype(np.int32)
    mixed[V // 3] = -1                                                   # compared as unsigned: 2^32 - 1 >= since
    last = np.zeros(V, np.int32)
    last[V - 1] = SINCE
    return {"none": np.full(V, SINCE - 1, np.int32), "zero": np.zeros(V, np.int32), "all": np.full(V, SINCE, np.int32),
            "last partial tile": last, "mixed": mixed}


@pytest.mark.parametrize("D", [20, 50, 256])
@pytest.mark.parametrize("V", [17, 37, 3417])
def test_sync_rewrites_exactly_the_flagged_tiles(V, D):
    A, Bt = _tables(V, D)
    rs = np.random.RandomState(V * 3 + D)
    tB = H.table_in_nan_buffer(Bt)
    for prec in (SPLIT, PLAIN):
        start, full = build_blob(A, prec), build_blob(Bt, prec)
        for name, flags in _flag_patterns(V, rs).items():
            hit = np.nonzero(flags.view(np.uint32) >= SINCE)[0]
            M = A.copy()
            for t in sorted(set((hit // 16).tolist())):
                M[16 * t:16 * t + 16] = Bt[16 * t:16 * t + 16]
            want = build_blob(M, prec)
            if name in ("none", "zero"):
                assert np.array_equal(want, start)
            if name == "all":
                assert np.array_equal(want, full)
            # the flags end at V: what follows them on the device says "touched", and must not be read
            fbuf = torch.full((V + 64,), SINCE + 1, dtype=torch.int32, device="cuda")
            fbuf[:V] = torch.from_numpy(flags).cuda()
            buf, blob = _guarded(start)
            O.topk_index_sync(blob, tB, prec, fbuf[:V], SINCE)
            _check(buf, want, (V, D, prec, name))
    # since = 0: every row counts, the result is the build's
    buf, blob = _guarded(build_blob(A, SPLIT))
    O.topk_index_sync(blob, tB, SPLIT, torch.zeros(V, dtype=torch.int32, device="cuda"), 0)
    _check(buf, build_blob(Bt, SPLIT), (V, D, "since 0"))


def test_update_forms_64_bit_offsets():
    """D = 256, bf16x3, V = 4 200 005: a 4.3 GB blob whose lo plane starts beyond 2^31 bytes and ends beyond 2^32.  A zeroed blob, no
    table of that size: a packed update of three rows, read back group by group."""
    V, D = 4_200_005, 256
    nb = index_bytes(V, D, SPLIT)
    assert group_offset(V, D, 1, 0, 0, 0) > 2 ** 31 and nb > 2 ** 32 and nb == O.topk_index_bytes(V, D, SPLIT)
    rows = [1, V // 2, V - 1]
    X = np.random.RandomState(9).standard_normal((3, D)).astype(np.float32)
    small = build_blob(X, SPLIT)                                         # the same rows as local rows 0, 1, 2 of a 3-row table
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    O.topk_index_update(blob, V, D, SPLIT, _dev_i32(rows), torch.from_numpy(X).cuda(), True)
    torch.cuda.synchronize()
    words = 0
    for j, r in enumerate(rows):
        for h in range(2):
            for ks in range(8):
                for lg in range(4):
                    o = group_offset(V, D, h, r >> 4, ks, 16 * lg + (r & 15))
                    want = small[group_offset(3, D, h, 0, ks, 16 * lg + j):][:16]
                    lo, hi = (16 if r & 15 else 0), (16 if (r & 15) < 15 else 0)         # the neighbouring lanes' groups
                    got = blob[o - lo:o + 16 + hi].cpu().numpy()
                    assert np.array_equal(got[lo:lo + 16], want), (r, h, ks, lg)
                    assert not got[:lo].any() and not got[lo + 16:].any(), (r, h, ks, lg, "a neighbouring group was written")
                    words += int(np.count_nonzero(want.view(np.int64)))
    assert words > 3 * 2 * 32                                            # (real data: most 8-byte words are non-zero)
    assert int(torch.count_nonzero(blob.view(torch.int64))) == words     # ... and nothing else in 4.3 GB was written
    del blob
    torch.cuda.empty_cache()


def test_search_after_update_has_the_bits_of_a_fresh_index():
    V, D, B, K = 3417, 50, 33, 10
    A, Bt = _tables(V, D)
    rs = np.random.RandomState(4)
    ids = rs.choice(np.arange(1, V), 500, replace=False)
    ids[0], ids[1] = V - 1, 1
    M = A.copy()
    M[ids] = Bt[ids]
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = H.excl_lists(rs, B, V, 20)
    tg = H.targets(rs, B, V, excl)
    tM = torch.from_numpy(M).cuda()
    for prec in ("bf16x3", "bf16"):
        fresh = ItemIndex.build(tM, prec)
        want = fresh.search(Q, K, exclude=excl, targets=tg)
        for form in ("table", "rows", "tensor ids"):
            ix = ItemIndex.build(torch.from_numpy(A).cuda(), prec)
            ptr = ix.blob.data_ptr()
            assert not torch.equal(ix.blob, fresh.blob)
            if form == "table":
                ix.update(ids, table=tM, version=7)
            elif form == "rows":
                ix.update(ids.tolist(), rows=Bt[ids], version=7)
            else:
                ix.update(_dev_i32(ids), rows=torch.from_numpy(Bt[ids]).cuda(), version=7)
            assert ix.version == 7 and ix.blob.data_ptr() == ptr and torch.equal(ix.blob, fresh.blob)
            H.same_bits(ix.search(Q, K, exclude=excl, targets=tg), want, (prec, form))
        with pytest.raises(ValueError):
            ix.update(_dev_i32([1, V]), table=tM)
        ix.rebuild(torch.from_numpy(A).cuda())
        assert ix.version is None and ix.blob.data_ptr() == ptr and np.array_equal(ix.blob.cpu().numpy(), build_blob(A, ix.prec))


# ---- end to end: a model that trains, an index that follows -------------------------------------------------------------------
ITEMNUM, T_, D_, B_, N_ = 2000, 20, 16, 8, 32


def _model(**kw):
    """The smallest model the whole-model tests train: SASRec, one block, D 16, 2000 items."""
    from castrec_amd.models import build_model
    args = dict(maxlen=T_, hidden_units=D_, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-2, max_bins=20,
                num_context_blocks=1, seed=1, ce_negatives=N_)
    args.update(kw)
    return build_model("sasrec", 10, ITEMNUM, 0, types.SimpleNamespace(**args))


def _batch(seed):
    rs = np.random.RandomState(seed)
    seq, pos, neg = (rs.randint(1, ITEMNUM + 1, (B_, T_)).astype(np.int32) for _ in range(3))
    for b in range(B_):
        k = rs.randint(0, T_ // 2) if b else 3
        for a in (seq, pos, neg):
            a[b, :k] = 0
    return seq, pos, neg


def _train(m, seeds):
    for s in seeds:
        seq, pos, neg = _batch(s)
        m.train_step(None, seq, pos, neg)


def _same_recommendations(m, ix):
    seq = _batch(99)[0]
    tg = np.random.RandomState(5).randint(1, ITEMNUM + 1, B_).astype(np.int32)
    H.same_bits(m.recommend(None, seq, k=10, targets=tg, index=ix), m.recommend(None, seq, k=10, targets=tg), "recommend")


@pytest.mark.parametrize("loss", ["sampled_ce", "bce"])
def test_row_sparse_training_syncs_the_index(loss, tmp_path, monkeypatch):
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    m = _model(loss=loss, row_sparse_adam=True)
    ix = m.build_item_index()
    first, token = ix.save(str(tmp_path / "first.npz")), ix.token
    before, ptr = ix.blob.clone(), ix.blob.data_ptr()
    table0 = m.get_params()["item_emb"].cpu().numpy()
    _train(m, (1, 2, 3))
    assert m._train.lazy_adam and m._train.step_number() == 4
    with pytest.raises(RuntimeError, match="stale index"):
        m.recommend(None, _batch(99)[0], index=ix)                       # nothing refreshes by itself
    assert m.refresh_item_index(ix) == "sync"
    fresh = m.build_item_index()
    assert ix.blob.data_ptr() == ptr and not torch.equal(ix.blob, before) and torch.equal(ix.blob, fresh.blob)
    assert ix.version == fresh.version and ix.token == fresh.token and ix.token.step == 4
    _same_recommendations(m, ix)

    # the delta, applied where no table is: a saved-and-loaded copy of the first index
    ids, rows, now = m.item_delta(token)
    table = m.get_params()["item_emb"].cpu().numpy()
    moved = np.nonzero((table != table0).any(1))[0]
    assert ids.dtype == torch.int32 and ids.is_cuda and 0 < ids.numel() < ITEMNUM and rows.shape == (ids.numel(), D_)
    assert 0 < moved.size and set(moved.tolist()) <= set(ids.tolist()) and 0 not in ids.tolist() and now == ix.token
    assert np.array_equal(rows.cpu().numpy(), table[ids.cpu().numpy()])
    far = ItemIndex.load(first)
    assert torch.equal(far.blob, before)
    far.update(ids, rows=rows)
    assert torch.equal(far.blob, fresh.blob)

    # one more step, a second sync from the new token; then a load: the flags say nothing about it
    _train(m, (4,))
    assert m.refresh_item_index(ix) == "sync" and torch.equal(ix.blob, m.build_item_index().blob)
    P = {n: v.cpu().numpy() for n, v in m.get_params().items()}
    P["item_emb"] = P["item_emb"] + np.float32(0.25)
    m.load_params(P)
    with pytest.raises(RuntimeError, match="table epoch"):
        m.item_delta(ix.token)
    assert m.refresh_item_index(ix) == "rebuild"
    assert ix.blob.data_ptr() == ptr and torch.equal(ix.blob, m.build_item_index().blob)
    _same_recommendations(m, ix)
    m.load_params({n: v.cpu().numpy() for n, v in m.get_params().items()})           # the same values: still a load
    assert m.refresh_item_index(ix) == "rebuild" and torch.equal(ix.blob, m.build_item_index().blob)


def test_dense_training_rebuilds_in_place(monkeypatch):
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    m = _model()
    ix = m.build_item_index()
    ptr, before = ix.blob.data_ptr(), ix.blob.clone()
    _train(m, (1, 2, 3))
    assert not m._train.lazy_adam
    with pytest.raises(RuntimeError, match="dense Adam"):
        m.item_delta(ix.token)
    assert m.refresh_item_index(ix) == "rebuild"
    assert ix.blob.data_ptr() == ptr and not torch.equal(ix.blob, before) and torch.equal(ix.blob, m.build_item_index().blob)
    assert ix.token.step is None
    _same_recommendations(m, ix)


def test_evaluate_full_refreshes_the_index_it_is_given(monkeypatch):
    from castrec_amd import util as U
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    rs = np.random.RandomState(3)
    usernum = 40
    User = {}
    for u in range(1, usernum + 1):
        n = rs.randint(3, 30)
        ts = 1_000_000_000 + 3600 * np.cumsum(rs.randint(1, 50, n))
        User[u] = [(int(rs.randint(1, ITEMNUM + 1)), 4.0, int(ts[j])) for j in range(n)]
    dataset = U.partition(User, usernum, ITEMNUM)
    m = _model(loss="sampled_ce", row_sparse_adam=True)
    args = types.SimpleNamespace(maxlen=T_, bin_in_hours=24, max_bins=20, log_scale=False, test_model=None, test_seq_len=None)
    ix = m.build_item_index()
    _train(m, (1, 2))                                                     # the index is stale now: evaluate_full brings it in step
    for fn in (U.evaluate_full, U.evaluate_valid_full):
        a, b, c = fn(m, dataset, args, use_index=ix), fn(m, dataset, args, use_index=True), fn(m, dataset, args)
        assert a == b == c and 0.0 <= a[1] <= 1.0, (a, b, c)
    assert ix.version == m._param_version and torch.equal(ix.blob, m.build_item_index().blob)

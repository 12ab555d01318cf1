"""Item index on the GPU (castrec.h cr_topk_index_build, cr_topk_desc.index; castrec_amd.index.ItemIndex; Model.build_item_index,
recommend(index=), similar_items; util.evaluate_full(use_index=True)).  The two properties everything else rests on: the built blob is
the numpy restatement of the layout byte for byte, and a search of the index returns the bits of the search of its table."""
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
from topk_harness import REL, same_bits as _same, search as _search

pytestmark = pytest.mark.gpu
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16
DS = [8, 20, 50, 64, 128, 256]


@pytest.mark.parametrize("D", DS)
def test_built_blob_equals_the_numpy_layout(D):
    rs = np.random.RandomState(D)
    for V in (1, 2, 17, 65):
        T = rs.standard_normal((V, D)).astype(np.float32)
        T[0, 0] = -0.0
        t = H.table_in_nan_buffer(T)
        for prec in (SPLIT, PLAIN):
            want = R.build_blob(T, prec)
            n = O.topk_index_bytes(V, D, prec)
            assert n == want.size
            out = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")        # stale bytes: the build writes the padding too
            O.topk_index_build(t, prec, out=out[:n])
            again = O.topk_index_build(t, prec)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], want), (V, D, prec, np.nonzero(got[:n] != want)[0][:8])
            assert np.all(got[n:] == 0xA5), "the build wrote past the blob"
            assert np.array_equal(again.cpu().numpy(), want)
        if V == 17:                                                                      # CR_PREC_F32 names the split index
            assert torch.equal(O.topk_index_build(t, L.PREC_F32), O.topk_index_build(t, SPLIT))


def _compare_all(T, Q, K, excl, tg, what):
    """Table against index in both precisions, and a plain search of the split index."""
    t = torch.from_numpy(T).cuda()
    V = T.shape[0]
    ix_split, ix_plain = O.topk_index_build(t, SPLIT), O.topk_index_build(t, PLAIN)
    ref_split = _search(Q, K, excl, tg, SPLIT, table=t)
    ref_plain = _search(Q, K, excl, tg, PLAIN, table=t)
    _same(ref_split, _search(Q, K, excl, tg, SPLIT, index=ix_split, iprec=SPLIT, V=V), what + ("split",))
    _same(ref_plain, _search(Q, K, excl, tg, PLAIN, index=ix_plain, iprec=PLAIN, V=V), what + ("plain",))
    _same(ref_plain, _search(Q, K, excl, tg, PLAIN, index=ix_split, iprec=SPLIT, V=V), what + ("plain of split",))
    return ref_split


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("V", [2, 17, 65, 3417])
def test_indexed_search_is_bit_identical(D, V):
    """V: one item; a partial tile; a partial round (of 64); two chunks with a partial last tile."""
    rs = np.random.RandomState(D * 11 + V)
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    for B, K in ((1, 1), (17, 10), (70, 128)):
        Q = rs.standard_normal((B, D)).astype(np.float32)
        excl = H.excl_lists(rs, B, V, 40)                   # empty, duplicates, 0, ids >= V, nearly everything
        tg = H.targets(rs, B, V, excl)
        ids, _, rk = _compare_all(T, Q, K, excl, tg, (D, V, B, K))
        assert np.all(ids[:, 0] != -7) and np.all(rk != -7)
        if B > 4:
            assert rk[1] == rk[2] == rk[3] == rk[4] == -1
        ids, _, _ = _compare_all(T, Q, K, None, None, (D, V, B, K, "no exclusions"))
        assert np.all((ids >= 0) & (ids < V))


def test_indexed_search_is_bit_identical_on_ties():
    rs = np.random.RandomState(2)
    D, V, B, K = 50, 3000, 5, 30
    base = rs.standard_normal((V // 3, D)).astype(np.float32)
    T = np.repeat(base, 3, axis=0)[:V]                                                   # rows 3j, 3j + 1, 3j + 2 equal
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = [rs.randint(1, V, 20).tolist() for _ in range(B)]
    ids, sc, rk = _compare_all(T, Q, K, excl, rs.randint(1, V, B), ("ties",))
    bits = sc.view(np.uint32)
    assert np.any(bits[:, :-1] == bits[:, 1:])                                           # the run did meet ties


def test_indexed_search_is_bit_identical_on_many_chunks():
    rs = np.random.RandomState(6)
    V, D, B, K = 100003, 50, 33, 100
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = [rs.randint(0, V + 5, rs.randint(0, 60)).tolist() for _ in range(B)]
    tg = rs.randint(1, V, B)
    tg[0], tg[1] = V - 1, 1
    _compare_all(T, Q, K, excl, tg, ("many chunks",))


def test_offsets_beyond_4_gib():
    V, D, B, K = 4_194_321, 256, 7, 10                                                   # a 4.29 GB table, a 4.29 GB split index
    if torch.cuda.mem_get_info()[0] < 16 * 10 ** 9:
        pytest.skip("needs 16 GB of free device memory")
    assert O.topk_index_bytes(V, D, SPLIT) > 2 ** 32
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
    Q = torch.randn(B, D, device="cuda", generator=g)
    t[V - 3] = Q[0] * 0.5                                   # rows of the last tile that must reach the lists: lo plane, highest offsets
    t[V - 1] = Q[1] * 0.5
    excl = [[], [5, V - 2], [V - 1], [], [1, 2, 3], [], [V - 5]]
    tg = np.array([V - 1, V - 2, V - 3, V - 16, V - 17, 1, V - 5], np.int32)
    ix = O.topk_index_build(t, SPLIT)
    ref = _search(Q, K, excl, tg, SPLIT, table=t)
    assert ref[0][0, 0] == V - 3 and ref[0][1, 0] == V - 1 and ref[2][1] == -1 and ref[2][6] == -1 and ref[2][0] >= 0
    _same(ref, _search(Q, K, excl, tg, SPLIT, index=ix, iprec=SPLIT, V=V), ("4 GiB", "split"))
    _same(_search(Q, K, excl, tg, PLAIN, table=t), _search(Q, K, excl, tg, PLAIN, index=ix, iprec=SPLIT, V=V), ("4 GiB", "plain of split"))


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
def test_item_index_search_save_load(tmp_path):
    rs = np.random.RandomState(8)
    V, D, B, K = 517, 50, 9, 20
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = H.excl_lists(rs, B, V, 30)
    tg = rs.randint(1, V, B).astype(np.int32)
    t = torch.from_numpy(T).cuda()
    ix = ItemIndex.build(t)
    assert (ix.V, ix.D, ix.precision, ix.version) == (V, D, "bf16x3", None) and ix.blob.is_cuda
    assert np.array_equal(ix.blob.cpu().numpy(), R.build_blob(T, SPLIT))
    ids, sc, rk = ix.search(Q, K, exclude=excl, targets=tg)
    ref = _search(Q, K, excl, tg, SPLIT, table=t)
    _same(ref, (ids, sc, rk), ("ItemIndex.search",))
    ids2, sc2 = ix.search(torch.from_numpy(Q).cuda(), K)                                 # device queries, no exclusions, no targets
    _same(_search(Q, K, None, None, SPLIT, table=t)[:2], (ids2, sc2), ("device queries",))
    p = ix.save(str(tmp_path / "items.npz"))
    back = ItemIndex.load(p)
    assert back.blob.is_cuda and back.version is None and torch.equal(back.blob, ix.blob)
    _same(ref, back.search(Q, K, exclude=excl, targets=tg), ("loaded",))
    plain = ItemIndex.build(t, "bf16")
    assert plain.blob.numel() * 2 == ix.blob.numel()
    _same(_search(Q, K, excl, tg, PLAIN, table=t), plain.search(Q, K, exclude=excl, targets=tg), ("plain ItemIndex",))
    _same(_search(Q, K, excl, tg, PLAIN, table=t), ix.search(Q, K, exclude=excl, targets=tg, precision="bf16"), ("plain search of split",))
    with pytest.raises(RuntimeError, match="plain"):
        plain.search(Q, K, precision="bf16x3")
    with pytest.raises(ValueError):
        ix.search(Q[:, :40], K)


def test_model_recommend_similar_items_and_staleness():
    itemnum, B, T, k = 300, 9, 20, 25
    m = H.model("cast_1", itemnum=itemnum)
    rs = np.random.RandomState(1)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    tg = rs.randint(1, itemnum + 1, B).astype(np.int32)
    kw = dict(k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, targets=tg)
    ix = m.build_item_index()
    assert (ix.V, ix.D, ix.precision) == (itemnum + 1, 50, "bf16x3") and ix.version is not None
    ref = m.recommend(None, seq, **kw)
    got = m.recommend(None, seq, index=ix, **kw)
    for a, b in zip(ref, got):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)

    # similar items: never the item itself; agrees with an fp64 ranking of the table's rows outside the tolerance band
    items = np.array([1, 2, 57, itemnum], np.int64)
    Tt = m.get_params()["item_emb"].cpu().numpy().astype(np.float64)
    for use in (None, ix):
        sid, ssc = m.similar_items(items, k=10, index=use)
        assert sid.shape == ssc.shape == (4, 10)
        S = Tt[items] @ Tt.T
        A = np.abs(Tt[items]) @ np.abs(Tt).T
        for r, it in enumerate(items):
            assert it not in sid[r] and 0 not in sid[r] and len(set(sid[r].tolist())) == 10
            assert np.all(np.abs(ssc[r] - S[r, sid[r]]) <= REL * A[r, sid[r]])
            elig = np.array([i for i in range(1, itemnum + 1) if i != it])
            order = elig[np.lexsort((elig, -S[r, elig]))]
            tol = REL * A[r, 1:].max()
            kth = S[r, order[9]]
            sure = set(order[:10][S[r, order[:10]] > kth + 2 * tol].tolist())
            assert sure <= set(sid[r].tolist())
            assert np.all(S[r, sid[r]] >= kth - 2 * tol)
    with pytest.raises(ValueError):
        m.similar_items([0])

    # a training step makes the index stale; a rebuilt one works; a loaded one (version None) is the caller's responsibility
    other = H.model("cast_1", itemnum=itemnum + 1)
    with pytest.raises(ValueError):
        other.recommend(None, seq, index=ix, **kw)
    pos = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    neg = rs.randint(1, itemnum + 1, seq.shape).astype(np.int32) * (seq != 0)
    m.train_step(None, seq, pos, neg, ts, hrs, dys)
    with pytest.raises(RuntimeError, match="stale index"):
        m.recommend(None, seq, index=ix, **kw)
    with pytest.raises(RuntimeError, match="stale index"):
        m.similar_items(items, index=ix)
    ix2 = m.build_item_index()
    assert not torch.equal(ix2.blob, ix.blob)
    ref = m.recommend(None, seq, **kw)
    got = m.recommend(None, seq, index=ix2, **kw)
    for a, b in zip(ref, got):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    m.load_params({n: v.cpu().numpy() for n, v in m.get_params().items()})
    with pytest.raises(RuntimeError, match="stale index"):
        m.recommend(None, seq, index=ix2, **kw)
    ix2.version = None
    m.recommend(None, seq, index=ix2, **kw)


def test_evaluate_full_with_an_index_returns_the_same_pair():
    from castrec_amd import util as U
    rs = np.random.RandomState(3)
    usernum, itemnum = 40, 300
    User = {}
    for u in range(1, usernum + 1):
        n = rs.randint(3, 30)
        ts = 1_000_000_000 + 3600 * np.cumsum(rs.randint(1, 50, n))
        User[u] = [(int(rs.randint(1, itemnum + 1)), 4.0, int(ts[j])) for j in range(n)]
    dataset = U.partition(User, usernum, itemnum)
    m = H.model("cast_1", itemnum=itemnum)
    args = types.SimpleNamespace(maxlen=20, bin_in_hours=24, max_bins=20, log_scale=False, test_model=None, test_seq_len=None)
    for fn in (U.evaluate_full, U.evaluate_valid_full):
        a = fn(m, dataset, args)
        b = fn(m, dataset, args, use_index=True)
        assert a == b and 0.0 <= a[1] <= 1.0, (a, b)


def test_main_cli_eval_index_logs_the_same_full_ranking(tmp_path, monkeypatch, caplog):
    import json
    import logging
    import os
    import re
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    lines = []
    for extra in ([], ["--eval_index"]):
        caplog.clear()
        rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t" + str(len(extra)), "--model", "cast_1", "--maxlen", "12",
                       "--batch_size", "4", "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20",
                       "--eval_full_ranking"] + extra)
        assert rc == 0
        assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
        full = re.findall(r"full ranking: valid \(NDCG@10: (\S+), HR@10: (\S+)\), test \(NDCG@10: (\S+), HR@10: (\S+)\)", caplog.text)
        assert len(full) == 2, caplog.text[-2000:]
        lines.append(full)
    assert lines[0] == lines[1]                             # same seed, same steps, same ranks: the index changes no metric
    root = tmp_path / "saved_models" / "synthetic_tiny"
    flags = sorted(json.loads((root / d / "params.txt").read_text())["eval_index"] for d in os.listdir(root))
    assert flags == [False, True]

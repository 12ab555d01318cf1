"""Full-catalogue top-K on the GPU (castrec.h cr_score_topk, Engine.topk, Model.recommend, util.evaluate_full) against fp64 numpy
and against the independent candidate path (predict / cr_test_logits)."""
import types

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

import topk_harness as H
from topk_harness import REL

pytestmark = pytest.mark.gpu
KMAX = L.CR_TOPK_MAX


@pytest.mark.parametrize("D", [20, 50, 64, 128, 256])
@pytest.mark.parametrize("V", [1, 100, 3416, 100003])
def test_topk_against_fp64(D, V):
    rs = np.random.RandomState(D * 7 + V)
    for B, K in ((1, 1), (7, 10), (128, 100), (300, KMAX)):
        if V == 100003 and B > 7 and D not in (50, 256):
            B = 33                                                           # (host reference time)
        Q = rs.standard_normal((B, D)).astype(np.float32)
        T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
        excl = H.excl_lists(rs, B, V, 40) if V <= 3416 else [rs.randint(0, V, rs.randint(0, 60)).tolist() for _ in range(B)]
        ids, sc, _ = H.search(Q, K, excl, None, L.PREC_BF16X3, table=T)
        H.check_fp64(Q, T, K, excl, ids, sc)


def test_topk_large_table_and_pitch():
    rs = np.random.RandomState(5)
    V, D, B, K = 2_000_000, 256, 7, 100                                     # 2 GB table (above the 256 MB Infinity Cache)
    T = (0.05 * rs.standard_normal((V, D))).astype(np.float32)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = [rs.randint(1, V, 30).tolist() for _ in range(B)]
    ids, sc, _ = H.search(Q, K, excl, None, L.PREC_BF16X3, table=T, ld=300)
    H.check_fp64(Q, T, K, excl, ids, sc)


def test_plain_bf16_bound():
    rs = np.random.RandomState(9)
    for D in (50, 128):
        Q = rs.standard_normal((33, D)).astype(np.float32)
        T = (0.1 * rs.standard_normal((5000, D))).astype(np.float32)
        ids, sc, _ = H.search(Q, 10, None, None, L.PREC_BF16, table=T)
        # bf16 operands: |err| <= 2 * 2^-8 * sum |q_i t_i| per score; checked against that bound, relative to the score scale
        H.check_fp64(Q, T, 10, None, ids, sc, rel=2 ** -6)
        i2, s2, _ = H.search(Q, 10, None, None, L.PREC_F32, table=T)              # CR_PREC_F32 takes the bf16x3 products
        i3, s3, _ = H.search(Q, 10, None, None, L.PREC_BF16X3, table=T)
        np.testing.assert_array_equal(i2, i3); np.testing.assert_array_equal(s2, s3)


def test_ties_go_to_the_smaller_id():
    rs = np.random.RandomState(2)
    D, V = 50, 3000
    base = rs.standard_normal((V // 3, D)).astype(np.float32)
    T = np.repeat(base, 3, axis=0)[:V]                                     # rows 3j, 3j+1, 3j+2 equal
    Q = rs.standard_normal((5, D)).astype(np.float32)
    ids, sc, _ = H.search(Q, 30, None, None, L.PREC_BF16X3, table=T)
    for b in range(5):
        for k in range(29):
            assert sc[b, k] > sc[b, k + 1] or (sc[b, k] == sc[b, k + 1] and ids[b, k] < ids[b, k + 1]), (b, k)
        # an item is returned only with every equal-scored row of smaller id (other than the padding row 0) returned before it
        got = set(ids[b].tolist())
        for i in ids[b]:
            j0 = (i // 3) * 3
            for j in range(max(1, j0), i):
                assert j in got, (b, i, j)


def _host_rank(ids, scores, t):
    """rank of t from the kernel's own scores of every eligible item (K >= number of eligible items)."""
    n = np.isfinite(scores) & (ids != 0)
    s_t = scores[n][ids[n] == t]
    assert len(s_t) == 1
    s_t = s_t[0]
    oth = n & (ids != t)
    return int(np.sum(scores[oth] > s_t) + np.sum((scores[oth] == s_t) & (ids[oth] < t)))


def test_ranks_exact_on_small_tables_and_bounded_on_large():
    rs = np.random.RandomState(11)
    for D, V in ((50, 100), (20, 120), (128, 90)):
        B = 40
        T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
        T[7] = T[3]; T[8] = T[3]                                            # ties
        Q = rs.standard_normal((B, D)).astype(np.float32)
        excl = H.excl_lists(rs, B, V, 20)
        excl = [r if b % 4 != 3 else r[:10] for b, r in enumerate(excl)]
        tg = rs.randint(1, V, B)
        tg[0] = 3; tg[1] = 8
        excl[2] = excl[2] + [int(tg[2])]                                     # an excluded target
        ids, sc, rk = H.search(Q, KMAX, excl, tg, L.PREC_BF16X3, table=T)
        for b in range(B):
            ex = set(excl[b])
            if tg[b] in ex:
                assert rk[b] == -1
                continue
            assert rk[b] == _host_rank(ids[b], sc[b], tg[b]), (D, V, b)
    V, D, B = 100003, 64, 50
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = [rs.randint(1, V, 50).tolist() for _ in range(B)]
    tg = rs.randint(1, V, B)
    _, _, rk = H.search(Q, 10, excl, tg, L.PREC_BF16X3, table=T)
    S = Q.astype(np.float64) @ T.astype(np.float64).T
    for b in range(B):
        ex = set(excl[b]) | {0}
        if tg[b] in ex:
            assert rk[b] == -1
            continue
        el = np.ones(V, bool); el[list(ex)] = False; el[tg[b]] = False
        tol = REL * (np.abs(Q[b].astype(np.float64)) @ np.abs(T.astype(np.float64)).T).max() * 2
        lo = int(np.sum(S[b, el] > S[b, tg[b]] + tol))
        hi = int(np.sum(S[b, el] >= S[b, tg[b]] - tol))
        assert lo <= rk[b] <= hi, (b, lo, rk[b], hi)


def test_deterministic():
    rs = np.random.RandomState(4)
    V, D, B = 200003, 50, 300
    T = (0.1 * rs.standard_normal((V, D))).astype(np.float32)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    excl = [rs.randint(1, V, 30).tolist() for _ in range(B)]
    tg = rs.randint(1, V, B)
    a = H.search(Q, 100, excl, tg, L.PREC_BF16X3, table=T)
    b = H.search(Q, 100, excl, tg, L.PREC_BF16X3, table=T)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sasrec", "cast_1", "cast_9"])
def test_recommend_matches_predict_over_all_items(name):
    itemnum, B, T, k = 500, 9, 20, 25
    m = H.model(name)
    rs = np.random.RandomState(1)
    seq, ts, hrs, dys = H.inputs(rs, B, T, itemnum)
    ids, sc = m.recommend(list(range(B)), seq, k=k, timeseq=ts, hours_seq=hrs, days_seq=dys)
    allc = np.arange(1, itemnum + 1, dtype=np.int32)
    lg, _ = m.predict(None, list(range(B)), seq, allc, timeseq=ts, hours_seq=hrs, days_seq=dys, want_attention=False)
    for b in range(B):
        hist = set(seq[b][seq[b] != 0].tolist())
        keep = np.array([i not in hist for i in allc])
        cand, s = allc[keep], lg[b][keep].astype(np.float64)
        order = np.lexsort((cand, -s))
        ref_i, ref_s = cand[order[:k]], s[order[:k]]
        scale = np.abs(s).max()
        np.testing.assert_allclose(sc[b], ref_s, rtol=0, atol=3e-5 * scale)             # bf16x3 against exact fp32: 2^-16 of sum |q_i t_i|
        kth = ref_s[-1]
        sure = set(ref_i[ref_s > kth + 6e-5 * scale].tolist())
        assert sure <= set(ids[b].tolist()) and not (set(ids[b].tolist()) & hist)
    # exclude=None and explicit lists; ids only
    ids2 = m.recommend(None, seq, k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, exclude=None, return_scores=False)
    assert ids2.shape == (B, k) and (ids2 > 0).all()
    ids3, _ = m.recommend(None, seq, k=k, timeseq=ts, hours_seq=hrs, days_seq=dys, exclude=[r[r != 0] for r in seq])
    np.testing.assert_array_equal(ids3, ids)


def test_evaluate_full_equals_a_host_full_ranking_evaluator():
    from castrec_amd import synth
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
    for fn, mode in ((U.evaluate_full, "test"), (U.evaluate_valid_full, "valid")):
        np.random.seed(7)
        st = np.random.get_state()
        got = fn(m, dataset, args)
        assert all(np.array_equal(x, y) for x, y in zip(st, np.random.get_state()))
        train, valid, test = dataset[:3]
        min_td, max_td = U.get_delta_range(train)
        ndcg = ht = 0.0
        n = 0
        allc = np.arange(1, itemnum + 1, dtype=np.int32)
        for u in range(1, usernum + 1):
            r = U._eval_inputs(train, valid, test, u, mode, args, itemnum, min_td, max_td, draw=False)
            if r is None:
                continue
            n += 1
            seq, ts, hrs, dys, (t, rated) = r
            lg, _ = m.predict(None, [u], seq[None], allc, timeseq=ts[None], hours_seq=hrs[None], days_seq=dys[None],
                              want_attention=False)
            s = lg[0].astype(np.float64)
            el = np.array([(i not in rated) and i != t for i in allc])
            rank = int(np.sum(s[el] > s[t - 1]) + np.sum((s[el] == s[t - 1]) & (allc[el] < t)))
            if rank < 10:
                ndcg += 1 / np.log2(rank + 2); ht += 1
        # the two paths differ only in arithmetic (bf16x3 vs exact fp32): near-ties may move one user across the cut
        assert abs(got[1] - ht / n) <= 1.0 / n + 1e-12 and abs(got[0] - ndcg / n) <= 1.0 / n + 1e-12, (mode, got, (ndcg / n, ht / n))

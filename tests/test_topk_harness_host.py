"""topk_harness.check_fp64 and same_bits can fail (no GPU, no native library): on D = 8, V = 17, B = 3, K = 4 with exclusions, the top-K
built in fp64 numpy passes, and each way a search can be wrong -- an excluded id, the filler id 0 too early, two entries out of order, a
surely-better item dropped, a score off by ten times the bound, one different bit -- is refused."""
import numpy as np
import pytest

from topk_harness import REL, check_fp64, same_bits

D, V, B, K = 8, 17, 3, 4
EXCL = [[], [3, 3, 0, 40, 5], list(range(1, 15))]            # none; duplicates, 0 and an id past the table; two eligible items left


def _case():
    rs = np.random.RandomState(0)
    Q = rs.standard_normal((B, D)).astype(np.float32)
    T = rs.standard_normal((V, D)).astype(np.float32)
    S = Q.astype(np.float64) @ T.astype(np.float64).T
    A = np.abs(Q.astype(np.float64)) @ np.abs(T.astype(np.float64)).T
    ids = np.zeros((B, K), np.int32)
    sc = np.full((B, K), -np.inf, np.float32)
    for b in range(B):
        elig = np.array([i for i in range(1, V) if i not in EXCL[b]])
        order = elig[np.lexsort((elig, -S[b, elig]))][:K]
        ids[b, :len(order)], sc[b, :len(order)] = order, S[b, order]
    return Q, T, S, A, ids, sc


def _refused(Q, T, ids, sc):
    with pytest.raises(AssertionError):
        check_fp64(Q, T, K, EXCL, ids, sc)


def test_check_fp64_passes_the_fp64_answer_and_refuses_every_mutant():
    Q, T, S, A, ids, sc = _case()
    check_fp64(Q, T, K, EXCL, ids, sc)
    assert np.all(ids[:2] > 0) and ids[2].tolist()[2:] == [0, 0]            # two full rows, one that runs out of eligible items
    tol = REL * A[:, 1:].max(axis=1)

    i, s = ids.copy(), sc.copy()                                            # an excluded id returned
    four = sorted(ids[1, :3].tolist() + [3], key=lambda j: -S[1, j])        # (in its place by score: nothing else is wrong)
    i[1], s[1] = four, S[1, four]
    _refused(Q, T, i, s)
    i, s = ids.copy(), sc.copy()                                            # id 0 before the list is exhausted
    i[0, 3], s[0, 3] = 0, -np.inf
    _refused(Q, T, i, s)
    i, s = ids.copy(), sc.copy()                                            # two entries swapped: the scores increase
    assert s[0, 1] > s[0, 2]
    i[0, [1, 2]], s[0, [1, 2]] = ids[0, [2, 1]], sc[0, [2, 1]]
    _refused(Q, T, i, s)
    i, s = ids.copy(), sc.copy()                                            # a surely-better item dropped for the next best one
    assert S[0, ids[0, 0]] > S[0, ids[0, 3]] + 2 * tol[0]
    rest = [j for j in range(1, V) if j not in ids[0]]
    nxt = rest[int(np.argmax(S[0, rest]))]
    i[0], s[0] = np.r_[ids[0, 1:], nxt], np.r_[sc[0, 1:], S[0, nxt]]
    _refused(Q, T, i, s)
    i, s = ids.copy(), sc.copy()                                            # a score off by ten times its bound
    s[0, 0] += 10 * REL * A[0, ids[0, 0]]
    _refused(Q, T, i, s)


def test_same_bits_passes_equal_results_and_refuses_a_bit_a_dtype_a_none_and_a_length():
    _, _, _, _, ids, sc = _case()
    rk = np.array([2, -1, 0], np.int32)
    same_bits((ids, sc, rk), (ids.copy(), sc.copy(), rk.copy()), "equal")
    same_bits((ids, sc, None), (ids, sc, None), "no rank on either side")
    same_bits((ids, sc), (ids, sc), "pairs")
    last_bit = sc.copy()
    last_bit.view(np.uint32)[0, 0] ^= 1
    assert last_bit[0, 0] != sc[0, 0] and abs(last_bit[0, 0] - sc[0, 0]) <= 2 ** -22 * abs(sc[0, 0])
    zero, minus_zero = np.zeros(1, np.float32), -np.zeros(1, np.float32)
    assert zero == minus_zero
    for a, b in (((ids, sc, rk), (ids, last_bit, rk)),                      # a score differing in its last bit
                 ((ids, sc, None), (ids, sc, rk)),                          # a rank of None against an array
                 ((ids, sc, rk), (ids, sc)),                                # another length
                 ((ids, sc, rk), (ids.astype(np.int64), sc, rk)),           # equal values of another dtype
                 ((ids, zero), (ids, minus_zero))):                         # equal floats of other bits
        with pytest.raises(AssertionError):
            same_bits(a, b, "mutant")

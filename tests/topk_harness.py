"""What the six test_topk* modules share: one marshalling of cr_score_topk into poisoned outputs, the bit comparison and the fp64 check
of a returned top-K, the generators of exclusion lists, targets, models and model inputs, and the host tests' "this call is refused".
castrec_amd and torch are imported inside the functions: check_fp64 and same_bits run without the native library
(test_topk_harness_host.py)."""
import types

import numpy as np

REL = 1e-5                       # bf16x3 against the fp64 dot, relative to sum_i |q_i t_i| (the scale of a dot product's rounding)


def _ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import lib as L
    from castrec_amd import ops as O
    return L, O


def search(Q, K, excl, tg, prec, table=None, index=None, iprec=None, V=None, ld=None):
    """cr_score_topk on the table (numpy or CUDA) or on an index of a [V, D] table: numpy (ids, scores, rank or None).  Q [B, D] numpy
    or CUDA (numpy for a pitch ld > D); excl: None or one id list per row.  The outputs hold -7 / 123.0 / -7 beforehand: what the
    kernels leave unwritten shows."""
    import torch
    _, O = _ops()
    B, D = Q.shape
    ld = ld or D
    if torch.is_tensor(Q):
        q = Q
    else:
        q = torch.zeros(B, ld, dtype=torch.float32, device="cuda")
        q[:, :D] = torch.from_numpy(Q)
    if table is not None:
        table = table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table, np.float32)).cuda()
        V = table.shape[0]
    off = ids = None
    if excl is not None:
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in excl])
        flat = np.concatenate([np.asarray(r, np.int32) for r in excl]) if off[-1] else np.zeros(1, np.int32)
        ids = torch.from_numpy(flat.astype(np.int32)).cuda()
    tgt = torch.from_numpy(np.asarray(tg, np.int32)).cuda() if tg is not None else None
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    out_i = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    out_s = torch.full((B, K), 123.0, dtype=torch.float32, device="cuda")
    rk = torch.full((B,), -7, dtype=torch.int32, device="cuda") if tg is not None else None
    if index is None:
        O.score_topk(q, ld, table, B, K, prec, off, ids, tgt, ws, out_i, out_s, rk)
    else:
        O.score_topk(q, ld, (V, D), B, K, prec, off, ids, tgt, ws, out_i, out_s, rk, index=index, index_precision=iprec)
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_s.cpu().numpy(), (rk.cpu().numpy() if rk is not None else None)


def table_in_nan_buffer(T):
    """The table on the device, followed directly by NaNs: anything read past its end shows."""
    import torch
    V, D = T.shape
    buf = torch.full((V * D + 1024,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:V * D] = torch.from_numpy(T.reshape(-1)).cuda()
    return buf[:V * D].view(V, D)


def same_bits(a, b, what):
    """Two results (ids, scores[, rank]) of equal length: None against None, else equal dtypes, shapes and bit patterns."""
    assert len(a) == len(b), (what, len(a), len(b))
    for x, y, name in zip(a, b, ("ids", "scores", "rank")):
        if x is None or y is None:
            assert x is None and y is None, (what, name, x, y)
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        bx, by = (v.view(np.uint32) if v.dtype == np.float32 else v for v in (x, y))
        assert np.array_equal(bx, by), (what, name, np.argwhere(bx != by)[:5], x, y)


def check_fp64(Q, T, K, excl, ids, scores, rel=REL):
    """A returned top-K against the fp64 ranking of row b's eligible items (not 0, not in excl[b]): the tail past the eligible items
    is id 0 / -inf; the ids are distinct and eligible; the scores do not increase and lie within rel * sum_i |q_i t_i| of the fp64
    dot; with tol = rel * max_i>0 A[b, i], everything more than 2 tol above the K-th fp64 score is returned and nothing more than
    2 tol below it."""
    S = Q.astype(np.float64) @ T.astype(np.float64).T                      # [B, V]
    A = np.abs(Q.astype(np.float64)) @ np.abs(T.astype(np.float64)).T      # sum_i |q_i t_i|
    B, V = S.shape
    for b in range(B):
        ex = set(int(e) for e in (excl[b] if excl is not None else ())) | {0}
        mask = np.ones(V, bool)
        mask[[e for e in ex if 0 <= e < V]] = False
        elig = np.nonzero(mask)[0]
        tol = rel * max(1e-30, float(A[b, 1:].max()) if V > 1 else 1.0)
        n_real = min(K, len(elig))
        got_i, got_s = ids[b], scores[b]
        assert np.all(got_i[n_real:] == 0) and np.all(np.isneginf(got_s[n_real:])), (b, got_i, got_s)
        gi = got_i[:n_real].astype(np.int64)
        assert len(set(gi.tolist())) == n_real and not (set(gi.tolist()) & ex) and np.all(gi < V), (b, gi)
        assert np.all(np.diff(got_s[:n_real]) <= 0), (b, got_s)
        assert np.all(np.abs(got_s[:n_real] - S[b, gi]) <= rel * A[b, gi]), (b, np.abs(got_s[:n_real] - S[b, gi]) / A[b, gi])
        if n_real == 0:
            continue
        order = elig[np.lexsort((elig, -S[b, elig]))]
        kth = S[b, order[n_real - 1]]
        sure = set(order[:n_real][S[b, order[:n_real]] > kth + 2 * tol].tolist())
        assert sure <= set(gi.tolist()), (b, sure - set(gi.tolist()))
        for i in gi:                                                         # anything else is within the tolerance of the K-th
            assert S[b, i] >= kth - 2 * tol, (b, i, S[b, i], kth)


def excl_lists(rs, B, V, n_max):
    out = []
    for b in range(B):
        kind = b % 4
        if kind == 0:
            out.append([])
        elif kind == 1:
            r = rs.randint(0, V + 3, rs.randint(1, n_max + 1)).tolist()         # ids past the table, 0
            out.append(r + r[:2] + [0])                                      # duplicates
        elif kind == 2:
            out.append(rs.randint(1, max(2, V), rs.randint(1, n_max + 1)).tolist())
        else:
            out.append(list(range(1, V))[: max(0, V - 3)])                   # fewer than K eligible when K > 2
    return out


def targets(rs, B, V, excl):
    tg = rs.randint(1, max(2, V), B).astype(np.int32)
    tg[0] = V - 1
    if B > 4:
        tg[1], tg[3], tg[4] = 0, V + 2, V
        tg[2] = max(1, V - 2)
        excl[2] = list(excl[2]) + [int(tg[2])]                                           # an excluded target
    return tg


def model(name, itemnum=500, D=50, T=20, seed=0):
    from castrec_amd.models import build_model
    args = types.SimpleNamespace(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3,
                                 max_bins=20, bin_in_hours=24, num_context_blocks=2, log_scale=False, input_context=False)
    m = build_model(name, 20, itemnum, 5.0, args)
    rs = np.random.RandomState(seed)
    P = m.get_params()
    m.load_params({k: v.cpu().numpy() + 0.1 * rs.standard_normal(tuple(v.shape)).astype(np.float32) for k, v in P.items()})
    return m


def inputs(rs, B, T, itemnum, max_bins=20):
    seq = rs.randint(1, itemnum + 1, (B, T)).astype(np.int32)
    for b in range(B):
        seq[b, : rs.randint(0, T - 2)] = 0
    ts = (rs.randint(0, max_bins + 1, (B, T)) * (seq != 0)).astype(np.int32)
    hrs = (rs.randint(1, 25, (B, T)) * (seq != 0)).astype(np.int32)
    dys = (rs.randint(1, 8, (B, T)) * (seq != 0)).astype(np.int32)
    return seq, ts, hrs, dys


def rejects(call, *words):
    """call = (entry point, *arguments): the C entry point returns -1 before any HIP call (fake pointers are never dereferenced) and
    cr_last_error starts with its name and holds every one of `words`.  Returns the message."""
    L, _ = _ops()
    rc = getattr(L.lib, call[0])(*call[1:])
    msg = L.lib.cr_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(call[0] + ":"), msg
    for w in words:
        assert w in msg, msg
    return msg

"""Row-sparse Adam for the sampled losses: the second id list of cr_adam_step against tests/adam_ref.py and
against one launch on the joined list; one engine step against the engine's own gradient; skipped rows stay frozen eagerly, under a
graph and on the fed path, with the graph's Adam following each step's draw; construction; the CLI; training.  Every tolerance is
adam_ref's own bound (worst_ratio <= 1) or exact equality."""
import math
import os
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


@pytest.fixture(scope="module")
def E():
    import castrec_amd  # noqa: F401
    from castrec_amd import engine
    return engine


# ---- 1. the second list at op level -------------------------------------------------------------------------------------------
def _launch(ops, c, lists):
    """One launch of cr_adam_step on case c with the lazy ids handed over as `lists` (one array, or two: lazy_ids and lazy_ids2);
    returns p, m, v, table_grad, flags after it.  Guards around every array the launch writes."""
    P, M, V, TG, SL = Buf(c.p0, 7.5), Buf(c.m0, 7.5), Buf(c.v0, 7.5), Buf(c.table_grad, 3.25), Buf(c.slabs, np.nan)
    st = np.zeros(16, np.float32)
    st[0:3] = [c.loss_sum, c.auc_sum, c.n_target]
    st.view(np.int32)[4] = c.t
    ST = Buf(st, -9.0)
    FL = Buf(c.lazy.flags0.view(np.int32), -3)
    ID = [Buf(np.asarray(x, np.int32), -4) for x in lists]
    kw = dict(lazy_ids=ID[0].view, lazy_rows=c.lazy.rows, lazy_D=c.lazy.D, lazy_flags=FL.view)
    if len(ID) > 1:
        kw.update(lazy_ids2=ID[1].view)
    ops.adam_step(P.view, M.view, V.view, TG.view, SL.view, c.n_table, c.n_dense, c.n_slabs, c.lr, ST.view, beta1=c.beta1, beta2=c.beta2,
                  eps=c.eps, l2=c.l2, n_l2=c.n_l2, **kw)
    torch.cuda.synchronize()
    for b, x in zip(ID, lists):
        assert np.array_equal(b.back(), x)                    # the lists are read only
    SL.back(), ST.back()
    return dict(p=P.back(), m=M.back(), v=V.back()), TG.back(), FL.back().view(np.uint32)


def _two_lists(rows, n1, n2, seed):
    """Ids of rows with id % 4 != 1 only (rows 1, 5, 9, ... are in neither list); list 2 repeats one of its own ids, holds one of list
    1's, and the ids 0, rows and -3 -- as far as its length allows (one id: the id of list 1)."""
    rs = np.random.RandomState(seed)
    pool = np.array([i for i in range(1, rows) if i % 4 != 1], np.int32)
    ids = pool[rs.randint(0, len(pool), n1)]
    ids2 = pool[rs.randint(0, len(pool), n2)]
    ids2[0] = ids[0]                                              # across the lists
    if n2 >= 6:
        fresh = np.setdiff1d(pool, ids)                           # (a row of list 2 alone, twice)
        ids2[1] = ids2[2] = fresh[0] if len(fresh) else pool[-1]
        ids2[3:6] = [0, rows, -3]
    return ids.astype(np.int32), ids2.astype(np.int32)


@pytest.mark.parametrize("rows,D,n1,n2", [(41, 7, 130, 1), (41, 7, 3, 37), (300, 64, 130, 256), (97, 256, 64, 64)])
def test_second_list_at_op_level(ops, rows, D, n1, n2):
    """The reference takes the joined list; the launch takes the two lists apart, then the joined list as lazy_ids alone: the same bits.
    (41, 7): the dense tail behind the lazy region starts at element 287, no multiple of 4 -- the sweep's scalar head."""
    ids, ids2 = _two_lists(rows, n1, n2, rows + n1 + n2)
    both = np.concatenate([ids, ids2])
    ok = lambda x: x[(x > 0) & (x < rows)]
    assert np.intersect1d(ok(ids), ok(ids2)).size >= 1
    if n2 >= 6:
        assert (np.unique(ok(ids2), return_counts=True)[1] > 1).any() and {0, rows, -3} <= set(ids2.tolist())
    unlisted = np.setdiff1d(np.arange(1, rows), both)
    assert unlisted.size >= 1
    nt = rows * D + 5 * D
    c = A.make_case(rows * D + n1 + n2, nt, 130, t=3, l2=0.05, n_l2=nt - 3, lazy=(rows, D, both))
    ref = A.reference(c)
    got, tg, flags = _launch(ops, c, [ids, ids2])
    ratio, which, i = A.worst_ratio(got, ref)
    print("worst error / bound: %.3f at %s[%d]" % (ratio, which, i))
    assert ratio <= 1.0, (ratio, which, i, got[which][i], getattr(ref, which)[i])
    # unlisted rows (and row 0): bits kept, gradient kept; claimed rows and the swept tail: gradient zeroed; the flags
    keep = ~ref.updated[:nt]
    assert keep.reshape(-1)[:rows * D].reshape(rows, D)[np.r_[0, unlisted]].all()
    for k, x0 in (("p", c.p0), ("m", c.m0), ("v", c.v0)):
        assert np.array_equal(got[k][:nt][keep].view(np.int32), x0[:nt][keep].view(np.int32)), k
    assert np.array_equal(tg[~ref.grad_zeroed].view(np.int32), c.table_grad[~ref.grad_zeroed].view(np.int32))
    assert (tg[ref.grad_zeroed] == 0.0).all()
    assert np.array_equal(flags, ref.lazy_flags)
    # the joined list in one piece
    one, tg1, flags1 = _launch(ops, c, [both])
    for k in got:
        assert np.array_equal(got[k].view(np.int32), one[k].view(np.int32)), k
    assert np.array_equal(tg.view(np.int32), tg1.view(np.int32)) and np.array_equal(flags, flags1)


# ---- the small engines ----------------------------------------------------------------------------------------------------------
ITEMNUM, T_, D_, B_, N_ = 2000, 20, 16, 8, 32


def _hp(E, **kw):
    d = dict(maxlen=T_, hidden_units=D_, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=3, ce_negatives=N_, max_bins=20)
    d.update(kw)
    return E.Hyper(**d)


def _batch(seed, lo=1, hi=400, neg=(1000, 1400), B=B_, T=T_):
    """seq / pos from lo .. hi, neg from its own range, left padding of 0 .. T / 2 per sequence; context ids for the cast models."""
    rs = np.random.RandomState(seed)
    seq, pos = rs.randint(lo, hi + 1, (B, T)), rs.randint(lo, hi + 1, (B, T))
    ng = rs.randint(neg[0], neg[1] + 1, (B, T))
    time, hours, days = rs.randint(0, 21, (B, T)), rs.randint(0, 24, (B, T)), rs.randint(0, 7, (B, T))
    for b in range(B):
        k = rs.randint(0, T // 2) if b else 3                     # (the first sequence always has padding)
        for a in (seq, pos, ng, time, hours, days):
            a[b, :k] = 0
    return tuple(a.astype(np.int32) for a in (seq, pos, ng, time, hours, days))


def _touched(seq, pos, samples):
    t = np.unique(np.concatenate([np.asarray(seq).reshape(-1), np.asarray(pos).reshape(-1), np.asarray(samples).reshape(-1)]))
    return t[t != 0]


def _item_rows(eng, x):
    """[itemnum + 1, D] host copy of the item section of a flat parameter-sized tensor"""
    return x[:(eng.itemnum + 1) * eng.D].detach().cpu().numpy().reshape(eng.itemnum + 1, eng.D).copy()


# ---- 2. one engine step against the engine's own gradient ---------------------------------------------------------------------
ENGINES = {"sampled_ce": ("sasrec", dict(loss="sampled_ce")), "gbce": ("sasrec", dict(loss="gbce")),
           "popularity": ("sasrec", dict(loss="sampled_ce", ce_proposal="popularity")),
           "cast_1": ("cast_1", dict(loss="sampled_ce", hidden_units=50, num_blocks=2))}


@pytest.mark.parametrize("which", sorted(ENGINES))
def test_one_engine_step_moves_exactly_the_touched_rows(E, which):
    model, kw = ENGINES[which]
    hp = _hp(E, **kw)
    eng = E.Engine(model, 10, ITEMNUM, hp, B_, training=True, row_sparse_adam=True)
    V, D, lay = ITEMNUM + 1, eng.D, eng.layout
    assert lay.entries["item_emb"][0] == 0 and lay.n_table >= V * D
    if which == "popularity":
        eng.set_item_weights(np.random.RandomState(1).uniform(0.5, 4.0, V))
    # moments that are not zero, so that their decay counts (a step number to go with them)
    rs = np.random.RandomState(2)
    eng.Mom.copy_(torch.from_numpy(rs.uniform(-1e-2, 1e-2, lay.n_total).astype(np.float32)))
    eng.Vel.copy_(torch.from_numpy(rs.uniform(0, 1e-4, lay.n_total).astype(np.float32)))
    batch = _batch(5)
    seq, pos, neg = batch[:3]
    eng.set_batch(*batch)
    eng.set_step(3)
    eng.launch_step(apply=False)
    torch.cuda.synchronize()
    nt = lay.n_table
    p0, m0, v0, g0 = (x[:nt].detach().cpu().numpy().copy() for x in (eng.P, eng.Mom, eng.Vel, eng.Gt))
    samples = eng.samples.cpu().numpy().copy()
    flags0 = eng.lazy_flags.cpu().numpy().copy()
    st = eng.state.cpu().numpy()
    n_target, t = float(st[10]), int(st.view(np.int32)[11])
    assert t == 3 and n_target == float((pos != 0).sum()) and (flags0 == 0).all()
    touched = _touched(seq, pos, samples)
    only_neg = np.setdiff1d(np.unique(neg), np.r_[0, touched])
    assert samples.min() >= 1 and samples.max() <= ITEMNUM and only_neg.size > 100
    # the premise: no gradient outside seq | pos | samples
    g_rows = g0[:V * D].reshape(V, D)
    nz = np.flatnonzero((g_rows != 0).any(1))
    assert nz.size > 0 and np.isin(nz, touched).all(), np.setdiff1d(nz, touched)[:10]

    eng._run([eng._adam], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(eng.samples.cpu().numpy(), samples)
    got = {k: x[:nt].detach().cpu().numpy() for k, x in (("p", eng.P), ("m", eng.Mom), ("v", eng.Vel))}
    assert (eng.Gt[:V * D].cpu().numpy() == 0.0).all()
    # the reference on the snapshots: the listed rows as the engine lists them (seq | pos, then the samples); rows outside have bound 0
    c = A.make_case(0, nt, 0, n_target=n_target, t=t, lr=float(hp.lr), lazy=(V, D, np.concatenate([seq.reshape(-1), pos.reshape(-1), samples])))
    c.p0, c.m0, c.v0, c.table_grad = p0, m0, v0, g0
    ref = A.reference(c)
    assert np.array_equal(np.flatnonzero(ref.updated[:V * D].reshape(V, D).all(1)), touched) and ref.updated[V * D:].all()
    ratio, name, i = A.worst_ratio(got, ref)
    print("worst error / bound: %.3f at %s[%d]" % (ratio, name, i))
    assert ratio <= 1.0, (ratio, name, i, got[name][i], getattr(ref, name)[i])
    rest = np.setdiff1d(np.arange(V), touched)
    assert 0 in rest and np.isin(only_neg, rest).all()
    for k, x0 in (("p", p0), ("m", m0), ("v", v0)):
        a, b = got[k][:V * D].reshape(V, D), x0[:V * D].reshape(V, D)
        assert np.array_equal(a[rest].view(np.int32), b[rest].view(np.int32)), k
        assert (a[touched] != b[touched]).any(1).all(), k          # (every touched row moved: its moments decay at the least)
    want = np.zeros(V, np.int32)
    want[touched] = t
    assert np.array_equal(eng.lazy_flags.cpu().numpy(), want)


# ---- 3. skipped rows stay frozen, eagerly and under a graph ---------------------------------------------------------------------
def _distinct_batch(seed, lo, hi):
    """seq and pos: 2 B T = 320 DISTINCT ids of lo .. hi (a step then touches 316 rows beside its samples: two positions of padding
    in the first sequence), neg from 1400 .. 1999"""
    rs = np.random.RandomState(seed)
    ids = lo + rs.permutation(hi - lo + 1)[:2 * B_ * T_]
    seq, pos = ids[:B_ * T_].reshape(B_, T_).copy(), ids[B_ * T_:].reshape(B_, T_).copy()
    neg = rs.randint(1400, 2000, (B_, T_))
    for a in (seq, pos, neg):
        a[0, :2] = 0
    z = np.zeros_like(seq)
    return tuple(a.astype(np.int32) for a in (seq, pos, neg, z, z, z))


@pytest.mark.parametrize("how", ["train_step", "graph", "fed"])
@pytest.mark.parametrize("loss", ["sampled_ce", "gbce"])
def test_skipped_rows_stay_frozen(E, loss, how):
    hp = _hp(E, loss=loss)
    batches = [_distinct_batch(20 + k, 400 * (k - 1) + 1, 400 * k) for k in (1, 2, 3)]

    def train(eng, how):
        """three steps; after each: (item rows of P, Mom, Vel; samples; flags)"""
        out = []

        def snap():
            torch.cuda.synchronize()
            out.append((_item_rows(eng, eng.P), _item_rows(eng, eng.Mom), _item_rows(eng, eng.Vel), eng.samples.cpu().numpy().copy(),
                        eng.lazy_flags.cpu().numpy().copy() if eng.lazy_adam else None))
        if how != "train_step":
            eng.capture()
            eng.set_step(1)
        if how == "fed":
            eng.enable_feed(n_slots=8)
            assert eng.graph is not None and eng.graph_steps == 1
            eng.feed(*batches[0]); eng.feed(*batches[1])          # the tail of step 1 moves batch 2 into place (cr_ids_ring_next)
            assert eng.train_fed() == 1; snap()
            eng.feed(*batches[2])
            assert eng.train_fed() == 1; snap()
            assert eng.train_fed() == 1; snap()
        else:
            for b in batches:
                eng.train_step(*b); snap()
        assert eng.step_number() == 4
        return out

    eng = E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, row_sparse_adam=True)
    s = train(eng, how)
    tch = [_touched(b[0], b[1], st[3]) for b, st in zip(batches, s)]
    # every step drew its own samples, and the (replayed) Adam launch read THAT draw
    assert len({st[3].tobytes() for st in s}) == 3
    for k, st in enumerate(s, 1):
        assert (st[4][st[3]] == k).all(), k
        want = np.zeros(ITEMNUM + 1, np.int32)
        for j in range(k):
            want[tch[j]] = j + 1
        assert np.array_equal(st[4], want), k                     # (a row's flag: the last step that moved it)
    frozen = np.setdiff1d(tch[0], tch[1])
    assert frozen.size >= 300, frozen.size
    for a in range(3):
        assert np.array_equal(s[1][a][frozen].view(np.int32), s[0][a][frozen].view(np.int32)), "P Mom Vel".split()[a]
    # the dense update moves them on their momentum
    dense = E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True)
    assert not dense.lazy_adam
    d = train(dense, "train_step")
    assert np.array_equal(d[0][3], s[0][3])                       # (the same draw)
    assert (d[1][0][frozen] != d[0][0][frozen]).any()


# ---- 4. construction --------------------------------------------------------------------------------------------------------------
def test_construction(E, monkeypatch):
    monkeypatch.delenv("CASTREC_LAZY_ADAM", raising=False)
    names = lambda e: [x[0] for x in e.fwd + e.bwd] + [e._adam[0]]
    hp = _hp(E)
    M = B_ * T_
    for loss in ("sampled_ce", "gbce"):
        a = E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss=loss, row_sparse_adam=True)
        d = E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss=loss)
        assert names(a) == names(d) and a.n_kernel_launches() == d.n_kernel_launches()
        assert a.lazy_adam is True and a.row_sparse_adam is True and not a.bitwise_reproducible and not a.use_index
        assert d.lazy_adam is False and d.row_sparse_adam is False
        assert a.lazy_ids.numel() == 2 * M and a.lazy_ids.data_ptr() == a.ids_all.data_ptr()
        for ad in (a._adam[2][0]._obj, a._adam_flat[2][0]._obj):
            assert ad.lazy_ids2 == a.samples.data_ptr() and ad.n_lazy_ids2 == N_ and ad.n_lazy_ids == 2 * M and ad.lazy_rows == ITEMNUM + 1
        for ad in (d._adam[2][0]._obj, d._adam_flat[2][0]._obj):
            assert not ad.lazy_ids and not ad.lazy_ids2 and ad.n_lazy_ids2 == 0
    # through Hyper, and the popularity proposal
    h = E.Engine("sasrec", 10, ITEMNUM, _hp(E, loss="sampled_ce", ce_proposal="popularity", row_sparse_adam=True), B_, training=True)
    assert h.lazy_adam and h._adam[2][0]._obj.lazy_ids2 == h.samples.data_ptr()
    assert E.Engine("sasrec", 10, ITEMNUM, _hp(E, loss="gbce", row_sparse_adam=True), B_, training=True, row_sparse_adam=False).lazy_adam is False
    # bce: the engine of lazy_adam=True
    a = E.Engine("cast_1", 10, ITEMNUM, hp, B_, training=True, row_sparse_adam=True)
    b = E.Engine("cast_1", 10, ITEMNUM, hp, B_, training=True, lazy_adam=True)
    assert a.loss == "bce" and a.lazy_adam and b.lazy_adam and names(a) == names(b) and a.n_kernel_launches() == b.n_kernel_launches()
    for e in (a, b):
        ad = e._adam[2][0]._obj
        assert e.lazy_ids.numel() == 3 * M == ad.n_lazy_ids and not ad.lazy_ids2 and ad.n_lazy_ids2 == 0 and not e.use_index
    # refusals
    with pytest.raises(ValueError, match="every item row has a gradient"):
        E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss="ce", row_sparse_adam=True)
    with pytest.raises(ValueError, match="every item row has a gradient"):
        E.Engine("sasrec", 10, ITEMNUM, _hp(E, loss="ce", row_sparse_adam=True), B_, training=True)
    for loss in ("sampled_ce", "gbce"):
        with pytest.raises(ValueError, match="data parallelism"):
            E.Engine("sasrec", 10, ITEMNUM, hp, 4, training=True, loss=loss, row_sparse_adam=True, batch_global=8, row_offset=4 * T_)
        with pytest.raises(ValueError, match="lazy_adam") as ei:
            E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss=loss, lazy_adam=True)
        assert "row_sparse_adam" in str(ei.value)
        with pytest.raises(ValueError, match="lazy_adam"):
            E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss=loss, lazy_adam=True, row_sparse_adam=True)
    monkeypatch.setenv("CASTREC_LAZY_ADAM", "1")
    with pytest.raises(ValueError, match="lazy_adam") as ei:
        E.Engine("sasrec", 10, ITEMNUM, hp, B_, training=True, loss="sampled_ce")
    assert "row_sparse_adam" in str(ei.value)
    monkeypatch.delenv("CASTREC_LAZY_ADAM")
    # eval engines ignore it
    assert E.Engine("sasrec", 10, ITEMNUM, _hp(E, loss="ce", row_sparse_adam=True), B_, training=False).loss == "bce"


def test_model_sizes_its_feed_for_one_step_per_launch(monkeypatch):
    from castrec_amd.models import build_model
    for k in ("CASTREC_LAZY_ADAM", "CASTREC_STEPS_PER_GRAPH", "CASTREC_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    args = dict(maxlen=T_, hidden_units=D_, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3, max_bins=20,
                num_context_blocks=1, seed=1, loss="sampled_ce", ce_negatives=N_)
    m = build_model("sasrec", 10, ITEMNUM, 0, types.SimpleNamespace(row_sparse_adam=True, **args))
    assert m._train is None and m.steps_per_launch == 1 and m.feed_ahead == 1
    d = build_model("sasrec", 10, ITEMNUM, 0, types.SimpleNamespace(**args))
    assert d.steps_per_launch == 4
    # ... and runs at what it said
    b = _batch(7)
    m.feed(None, *b)
    assert m._train.lazy_adam and m._train._feed_ring.shape[0] == 8 and m.steps_per_launch == 1
    auc, loss = m.train_fed()
    assert math.isfinite(loss) and 0 < loss < 3 * math.log(N_ + 1)


# ---- 5. the CLI -------------------------------------------------------------------------------------------------------------------
def test_main_cli_trains_with_sampled_ce_and_row_sparse_adam(tmp_path, monkeypatch, caplog):
    import json
    import logging
    import re
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "cast_1", "--maxlen", "12", "--batch_size", "4",
                   "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20", "--loss", "sampled_ce",
                   "--ce_negatives", "16", "--eval_full_ranking", "--row_sparse_adam"])
    assert rc == 0
    runs = os.listdir(tmp_path / "saved_models" / "synthetic_tiny")
    d = tmp_path / "saved_models" / "synthetic_tiny" / runs[0]
    params = json.loads((d / "params.txt").read_text())
    assert params["loss"] == "sampled_ce" and params["ce_negatives"] == 16 and params["row_sparse_adam"] is True
    assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
    train = [float(x) for x in re.findall(r"TRAIN/loss (\S+)", caplog.text)]
    full = re.findall(r"full ranking: valid \(NDCG@10: (\S+), HR@10: (\S+)\), test \(NDCG@10: (\S+), HR@10: (\S+)\)", caplog.text)
    assert len(train) == 2 and len(full) == 2, caplog.text[-2000:]
    vals = train + [float(x) for row in full for x in row] + [float(x) for x in re.findall(r"\d+\.\d+", (d / "log.txt").read_text())]
    assert all(math.isfinite(v) for v in vals), vals
    assert all(0 < v < 3 * math.log(17) for v in train), train      # (17 candidates per row at most)


# ---- 6. it learns -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_batches():
    """200 batches of the small shape from a seeded synthetic corpus (Zipf item popularity), drawn once for both losses"""
    import castrec_amd  # noqa: F401
    from castrec_amd import synth
    from castrec_amd.sampler import WarpSampler
    c = synth.make_corpus(300, ITEMNUM, 3.0, 0.5, 60, 1.0, 11)
    args = types.SimpleNamespace(maxlen=T_, bin_in_hours=24, max_bins=20, log_scale=False, seed=11)
    smp = WarpSampler(args, c, c.usernum, c.itemnum, batch_size=B_, maxlen=T_, n_workers=1)
    out = []
    for _ in range(200):
        u, seq, pos, neg, ts, rat, hrs, dys, _x = smp.next_batch()
        out.append(tuple(np.array(a, np.int32) for a in (seq, pos, neg)))
    smp.close()
    return out


@pytest.mark.parametrize("loss", ["sampled_ce", "gbce"])
def test_it_learns(E, synth_batches, loss):
    eng = E.Engine("sasrec", 10, ITEMNUM, _hp(E, loss=loss, lr=3e-3), B_, training=True, row_sparse_adam=True)
    eng.capture()
    eng.set_step(1)
    losses = []
    for b in synth_batches:
        eng.train_step(*b)
        losses.append(eng.loss_auc()[0])
    assert all(math.isfinite(x) for x in losses)
    first, last = float(np.mean(losses[:20])), float(np.mean(losses[-20:]))
    print("%s: mean loss of steps 1-20 %.4f, of steps 181-200 %.4f" % (loss, first, last))
    assert last < first, (first, last)

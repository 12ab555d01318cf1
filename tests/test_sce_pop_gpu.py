"""The popularity proposal of the sampled softmax on the GPU: cr_sampled_ce with logq against fp64 on the corrected logits (supplied
samples, per-element bounds as test_sce_gpu.py), a constant proposal against the uniform path, the device draw through the cdf against
its numpy restatement, determinism, padding and all-hits rows; Engine(ce_proposal="popularity") against the oracle with the corrected
loss + autograd in fp64, its refusals and launch list, graph capture with a change of weights, the fed multi-step path, the CLI and
the skewed planted corpus."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import fpmodel as fm

import sce_pop_ref as R
from test_ce_gpu import _batch
from test_sce_gpu import _case, _check, _ops, _ref64
from test_sce_gpu import _run as _run_uniform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import castrec_amd  # noqa: F401
    from castrec_amd import engine
    return engine


_PROPOSALS = {}


def _proposal(V):
    """The Zipf proposal of a table size, from the library's builder (built once per size)."""
    if V not in _PROPOSALS:
        from castrec_amd.proposal import build_proposal
        _PROPOSALS[V] = build_proposal(R.zipf_weights(V, 1.0), V)
    return _PROPOSALS[V]


def _run(h, E_, pos, neg, samples, prec, cdf=None, logq=None, seed=0, step=None, N=None, want_tg=True):
    """test_sce_gpu._run with the proposal's arrays."""
    L, O = _ops()
    M, D = h.shape
    V = E_.shape[0]
    N = len(samples) if samples is not None else N
    hs = torch.from_numpy(h).cuda()
    tab = torch.from_numpy(E_).cuda()
    p = torch.from_numpy(pos).cuda()
    n = torch.from_numpy(neg).cuda()
    smp = torch.from_numpy(samples).cuda() if samples is not None else None
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda")
    if step is not None:
        st[4:5].view(torch.int32)[0] = step - 2 ** 32 if step >= 2 ** 31 else step          # (the uint32 word's bits)
    dh = torch.full((M, D), float("nan"), dtype=torch.float32, device="cuda")
    tg = torch.zeros(V, D, dtype=torch.float32, device="cuda") if want_tg else None
    lse = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    so = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(O.sampled_ce_workspace_bytes(M, N, D), dtype=torch.uint8, device="cuda")
    c = torch.from_numpy(cdf.view(np.int32)).cuda() if cdf is not None else None
    q = torch.from_numpy(logq).cuda() if logq is not None else None
    O.sampled_ce(hs, D, tab, p, st, ws, M, N, precision=prec, neg=n, samples=smp, seed=seed, step=st[4:5], samples_out=so,
                 d_seq_emb=dh, ldd=D, table_grad=tg, lse_out=lse, cdf=c, logq=q)
    torch.cuda.synchronize()
    return dict(dh=dh.cpu().numpy(), tg=tg.cpu().numpy() if want_tg else None, lse=lse.cpu().numpy(), state=st.cpu().numpy(),
                samples=so.cpu().numpy())


CASES = [(D, N, V) for D in (8, 50, 64, 128, 256) for N in (1, 7, 256, 2048) for V in (17, 3417, 100003)]


@pytest.mark.parametrize("D,N,V", CASES)
def test_corrected_sampled_ce_against_fp64(D, N, V):
    L, _ = _ops()
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"scepop%d_%d_%d" % (D, N, V)))
    _, logq = _proposal(V)
    got = _run(h, E_, pos, neg, s, L.PREC_BF16X3, logq=logq)          # (supplied samples: the cdf is not needed)
    ref = R.ref64(h, E_, pos, neg, s, logq)
    _check(got, ref)
    assert np.all(got["dh"][pos == 0] == 0.0)
    assert np.array_equal(got["samples"], s)
    assert np.all(got["tg"][0] == 0.0)
    # the AUC term stays on the raw scores
    sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
    auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
    assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6
    if N == 256 and D == 50:
        # ... and the correction is not a no-op at this skew: the uniform objective's loss is outside the corrected one's bound
        plain = _ref64(h, E_, pos, neg, s)
        assert abs(plain["loss"] - ref["loss"]) > 10 * (4 * ref["e_loss"] + 1e-5)


@pytest.mark.parametrize("D,N,V", [(20, 256, 17), (50, 256, 3417), (128, 2048, 100003), (256, 7, 3417)])
def test_plain_bf16_bound(D, N, V):
    L, _ = _ops()
    h, E_, pos, neg, s = _case(D, V, 151, N, 11 + D + N)
    _, logq = _proposal(V)
    _check(_run(h, E_, pos, neg, s, L.PREC_BF16, logq=logq), R.ref64(h, E_, pos, neg, s, logq, bf16=True))


@pytest.mark.parametrize("V,D,N", [(17, 50, 40), (4097, 64, 256)])
def test_constant_proposal_agrees_with_the_uniform_path(V, D, N):
    """Equal weights over V - 1 = 2^k items: log Q is one constant exactly, so the corrected softmax is the uniform one -- loss and
    gradients agree within the sum of the two paths' bounds, lse_out differs by log(V - 1) on target rows.  (A bias on the candidates
    but not on the target, or of the wrong sign, shifts the loss by log(V - 1) per row instead.)"""
    from castrec_amd.proposal import build_proposal
    L, _ = _ops()
    M = 203
    h, E_, pos, neg, s = _case(D, V, M, N, 77 + V)
    cdf, logq = build_proposal(np.ones(V), V)
    assert np.all(logq[1:] == logq[1]) and logq[1] == np.float32(-math.log(V - 1))
    a = _run(h, E_, pos, neg, s, L.PREC_BF16X3, logq=logq)
    b = _run_uniform(h, E_, pos, neg, s, L.PREC_BF16X3)
    ra, rb = R.ref64(h, E_, pos, neg, s, logq), _ref64(h, E_, pos, neg, s)
    for k, e in (("dh", "e_dh"), ("tg", "e_dE")):
        r = np.abs(a[k] - b[k]) / (4.0 * (ra[e] + rb[e]) + 1e-30)
        assert np.all(r <= 1.0), (k, float(r.max()))
    assert abs(a["state"][0] - b["state"][0]) <= 4.0 * (ra["e_loss"] + rb["e_loss"]) + 2e-6 * abs(rb["loss"]) + 2e-5
    live = ra["ist"]                                     # (a padded row's "target" is row 0, whose correction is 0: no common shift)
    r = np.abs((a["lse"] - b["lse"]) - math.log(V - 1))[live] / (4.0 * (ra["e_lse"] + rb["e_lse"]))[live]
    assert np.all(r <= 1.0), ("lse", float(r.max()))
    assert a["state"][2] == b["state"][2] and a["state"][1] == b["state"][1]


@pytest.mark.parametrize("seed,step,V,N", [(42, 1, 3417, 256), (7, 123456, 17, 300), (0, 2 ** 31 + 5, 10 ** 7, 4096)])
def test_device_draw_matches_the_numpy_restatement(seed, step, V, N):
    L, _ = _ops()
    D, M = 16, 40
    h, E_, pos, neg, _ = _case(D, min(V, 4000), M, 1, 3)
    if V > E_.shape[0]:                                  # (a 10^7-row table: its rows' values do not matter here)
        E_ = np.zeros((V, D), np.float32)
        E_[:4000] = np.random.RandomState(4).standard_normal((4000, D))
    cdf, logq = _proposal(V)
    got = _run(h, E_, pos, neg, None, L.PREC_BF16X3, cdf=cdf, logq=logq, seed=seed, step=step, N=N, want_tg=False)
    want = R.draw(seed, step, cdf, N)
    assert np.array_equal(got["samples"], want)
    assert got["samples"].min() >= 1 and got["samples"].max() <= V - 1
    again = _run(h, E_, pos, neg, None, L.PREC_BF16X3, cdf=cdf, logq=logq, seed=seed, step=step, N=N, want_tg=False)
    assert np.array_equal(again["samples"], got["samples"])
    # the drawn ids give the results of the same ids supplied by the caller, bit for bit
    sup = _run(h, E_, pos, neg, want, L.PREC_BF16X3, logq=logq, want_tg=False)
    for k in ("lse", "dh"):
        assert np.array_equal(got[k].view(np.int32), sup[k].view(np.int32)), k
    assert np.array_equal(got["state"][:3].view(np.int32), sup["state"][:3].view(np.int32))
    nxt = _run(h, E_, pos, neg, None, L.PREC_BF16X3, cdf=cdf, logq=logq, seed=seed, step=step + 1, N=N, want_tg=False)
    assert not np.array_equal(nxt["samples"], got["samples"])
    assert np.array_equal(nxt["samples"], R.draw(seed, step + 1, cdf, N))


@pytest.mark.parametrize("D,V,M,N", [(50, 3417, 1300, 256), (128, 100003, 200, 2048), (8, 17, 77, 300)])
def test_two_calls_give_the_same_bits(D, V, M, N):
    L, _ = _ops()
    h, E_, pos, neg, _ = _case(D, V, M, N, 3)
    cdf, logq = _proposal(V)
    a = _run(h, E_, pos, neg, None, L.PREC_BF16X3, cdf=cdf, logq=logq, seed=9, step=4, N=N)
    b = _run(h, E_, pos, neg, None, L.PREC_BF16X3, cdf=cdf, logq=logq, seed=9, step=4, N=N)
    for k in ("lse", "dh", "state", "samples"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    keep = np.ones(V, bool)
    keep[pos] = False                                    # target rows take float atomics: rounding order may differ
    assert np.array_equal(a["tg"][keep].view(np.int32), b["tg"][keep].view(np.int32))
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=1e-5, atol=1e-6)
    _check(a, R.ref64(h, E_, pos, neg, a["samples"], logq))


def test_padding_rows_and_all_hits_rows():
    L, _ = _ops()
    D, V, M = 32, 50, 96
    rs = np.random.RandomState(2)
    h = rs.standard_normal((M, D)).astype(np.float32) * 0.3
    E_ = rs.standard_normal((V, D)).astype(np.float32)
    _, logq = _proposal(3417)
    logq = np.ascontiguousarray(logq[:V])                # (any correction will do with supplied samples)
    # every sample is the target of every live row: loss 0 and zero gradients exactly, nothing touched
    pos = np.full(M, 7, np.int32)
    pos[::3] = 0
    neg = np.zeros(M, np.int32)
    got = _run(h, E_, pos, neg, np.full(8, 7, np.int32), L.PREC_BF16X3, logq=logq)
    assert got["state"][0] == 0.0 and got["state"][2] == float((pos != 0).sum())
    assert np.all(got["dh"] == 0.0) and np.all(got["tg"] == 0.0)
    # padding rows contribute nothing: the same call with them removed has the same loss and gradients
    s = np.array([3, 9, 9, 7, 20], np.int32)
    pos2 = pos.copy(); pos2[1::5] = 9
    live = pos2 != 0
    a = _run(h, E_, pos2, neg, s, L.PREC_BF16X3, logq=logq)
    b = _run(h[live], E_, pos2[live], neg[live], s, L.PREC_BF16X3, logq=logq)
    assert np.all(a["dh"][~live] == 0.0) and np.all(a["tg"][0] == 0.0)
    np.testing.assert_allclose(a["dh"][live], b["dh"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=1e-5, atol=1e-6)
    assert a["state"][0] == pytest.approx(b["state"][0], rel=1e-6) and a["state"][2] == b["state"][2]
    _check(a, R.ref64(h, E_, pos2, neg, s, logq))
    untouched = np.setdiff1d(np.arange(V), np.concatenate([s, pos2]))
    assert np.all(a["tg"][untouched] == 0.0)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _loss(out, pos, samples, logq):
    """The corrected sampled loss on the oracle's seq_emb and item table, in fp64 (loss / n_target, as Adam sees it)."""
    se, tab = out["seq_emb"], out["item_table"]
    lq = torch.as_tensor(np.asarray(logq, np.float64))
    p = torch.as_tensor(np.asarray(pos).reshape(-1), dtype=torch.long)
    s = torch.as_tensor(np.asarray(samples), dtype=torch.long)
    S = se @ tab[s].t() - lq[s][None, :]
    st = (se * tab[p]).sum(1) - lq[p]
    S = S.masked_fill(s[None, :] == p[:, None], float("-inf"))
    lse = torch.logsumexp(torch.cat([st[:, None], S], 1), 1)
    ist = p != 0
    return ((lse - st) * ist).sum() / ist.sum()


@pytest.mark.parametrize("model", ["sasrec", "cast_1"])
def test_engine_popularity_step_matches_oracle(E, model):
    from test_model_gpu import engine_relu_gates
    rs = np.random.RandomState(zlib.crc32(model.encode()) % 1000)
    B, T, D, H, itemnum, max_bins = 5, 24, 20, 1, 37, 12
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                 lr=1e-3, seed=7)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                   lr=1e-3)
    eng = E.Engine(model, 9, itemnum, hp, B, training=True, n_slabs=7, loss="sampled_ce", ce_negatives=16, ce_proposal="popularity")
    assert eng.loss == "sampled_ce" and eng.ce_proposal == "popularity" and not eng.use_index and not eng.bitwise_reproducible
    w = np.concatenate([[0.0], (rs.randint(0, 50, itemnum) + 1.0) ** 0.75])
    eng.set_item_weights(w)
    cdf, logq = R.build(w)
    assert np.array_equal(eng.item_cdf.cpu().numpy().view(np.uint32), cdf)
    assert np.array_equal(eng.item_logq.cpu().numpy().view(np.int32), logq.view(np.int32))
    P = fm.init_params(model, 9, itemnum, ohp, seed=3)
    P = {k: v + 0.1 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
    eng.load_params(P)
    P = {k: v.double().cpu() for k, v in eng.get_params().items()}
    seq, pos, neg, time, hours, days = _batch(rs, B, T, itemnum, max_bins)
    batch = fm.to_batch(seq, pos, neg, time, hours, days)
    eng.set_batch(seq, pos, neg, time, hours, days)
    eng.set_step(1)
    eng.launch_step(apply=False)
    torch.cuda.synchronize()
    samples = eng.samples.cpu().numpy()
    assert np.array_equal(samples, R.draw(7, 1, cdf, 16))
    gates, care = engine_relu_gates(eng, B, T, None)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    with fm.handed_over_gates(gates, care, check=True):
        out = fm.forward(model, leaves, ohp, batch, None)
    loss = _loss(out, pos, samples, logq)
    loss.backward()
    G = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    st = eng.state.cpu().numpy()
    n = float((pos != 0).sum())
    assert st[2] == n
    assert st[0] / n == pytest.approx(loss.item(), rel=2e-5)
    got = eng.grads()
    gmax = max(float(G[k].abs().max()) for k in G)
    for k in G:
        if k.endswith(".bk"):                            # d loss / d bk == 0 identically: rounding noise on both sides
            continue
        ref = G[k].numpy()
        err = float(np.abs(got[k].cpu().double().numpy() - ref).max())
        assert err < 2e-3 * max(float(np.abs(ref).max()), 1e-3 * gmax), (k, err, float(np.abs(ref).max()))
    # one Adam step on both sides (the same step word: the same samples)
    eng.Gt.zero_()
    eng.set_step(1)
    eng.launch_step(apply=True)
    torch.cuda.synchronize()
    assert np.array_equal(eng.samples.cpu().numpy(), samples)
    lr = hp.lr
    P1 = fm.AdamTF(P, lr=lr).step(dict(P), G)
    now = eng.get_params()
    for k in P:
        if k.endswith(".bk"):
            continue
        d_eng = now[k].double().cpu() - P[k]
        d_orc = P1[k] - P[k]
        big = G[k].abs() > 1e-2 * max(float(G[k].abs().max()), 1e-3 * gmax)
        assert float((d_eng - d_orc).abs().max()) <= 2.0 * lr + 1e-7, k
        if bool(big.any()):
            assert float((d_eng - d_orc)[big].abs().max()) <= 0.02 * lr, k
    assert eng.loss_auc()[0] == pytest.approx(loss.item(), rel=2e-5)


def test_engine_refusals_defaults_and_launch_list(E):
    hp = E.Hyper(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=1)
    assert E.Hyper().ce_proposal == "uniform" and hp.ce_proposal == "uniform" and hp.ce_pop_power == 1.0
    with pytest.raises(ValueError, match="ce_proposal"):
        E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="sampled_ce", ce_proposal="zipf")
    for loss in ("bce", "ce", "gbce"):
        with pytest.raises(ValueError, match="ce_proposal"):
            E.Engine("sasrec", 10, 100, hp, 8, training=True, loss=loss, ce_proposal="popularity")
    hp_p = E.Hyper(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=1, loss="sampled_ce",
                   ce_proposal="popularity")
    ev = E.Engine("sasrec", 10, 100, hp_p, 8, training=False)                 # eval engines ignore the option
    assert ev.ce_proposal == "uniform" and ev.loss == "bce"
    with pytest.raises(RuntimeError, match="popularity"):
        ev.set_item_weights(np.ones(101))
    names = lambda e: [x[0] for x in e.fwd + e.bwd]
    u = E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="sampled_ce", ce_negatives=16)
    p = E.Engine("sasrec", 10, 100, hp_p, 8, training=True, ce_negatives=16)
    assert u.ce_proposal == "uniform" and p.ce_proposal == "popularity" and p.loss == "sampled_ce"
    assert names(u) == names(p) and names(p).count("cr_sampled_ce") == 1 and u.n_kernel_launches() == p.n_kernel_launches()
    assert not hasattr(u, "item_logq")
    assert tuple(p.item_logq.shape) == (101,) and tuple(p.item_cdf.shape) == (101,) and p.item_logq.dtype == torch.float32
    # a training step before the first set_item_weights
    rs = np.random.RandomState(0)
    bt = _planted_batch(rs, 8, 20, 100)
    with pytest.raises(RuntimeError, match="set_item_weights"):
        p.train_step(*bt)
    with pytest.raises(RuntimeError, match="set_item_weights"):
        p.launch_step()
    p.capture()                                          # (recording a graph is not a step)
    with pytest.raises(RuntimeError, match="set_item_weights"):
        p.train_step(*bt)
    with pytest.raises(ValueError, match="item 3 has no mass"):
        p.set_item_weights(np.concatenate([np.ones(3), [0.0], np.ones(97)]))
    with pytest.raises(ValueError, match="shape"):
        p.set_item_weights(np.ones(100))
    with pytest.raises(RuntimeError, match="set_item_weights"):
        p.train_step(*bt)                                # (a refused set of weights is not a proposal)
    p.set_item_weights(np.ones(101))
    p.set_step(1)
    p.train_step(*bt)
    torch.cuda.synchronize()
    assert math.isfinite(p.loss_auc()[0])
    # the model reads the options with defaults: a namespace from before them builds the uniform model
    import types
    from castrec_amd.models import build_model
    args = types.SimpleNamespace(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3,
                                 max_bins=20, num_context_blocks=1, seed=1, loss="sampled_ce", ce_negatives=16)
    m = build_model("sasrec", 10, 100, 0, args)
    assert m.hp.ce_proposal == "uniform"
    with pytest.raises(RuntimeError, match="popularity"):
        m.set_item_counts(np.zeros(101))
    args.ce_proposal, args.ce_pop_power = "popularity", 0.5
    m = build_model("sasrec", 10, 100, 0, args)
    with pytest.raises(ValueError, match="counts"):
        m.set_item_counts(np.zeros(100))
    counts = rs.randint(0, 30, 101)
    m.set_item_counts(counts)                            # before the training engine exists: kept for it
    m.train_step(None, *bt)
    cdf, logq = R.build((counts + 1.0) ** 0.5)
    assert np.array_equal(m._train.item_cdf.cpu().numpy().view(np.uint32), cdf)
    assert np.array_equal(m._train.samples.cpu().numpy(), R.draw(1, 1, cdf, 16))
    m.set_item_counts(counts, power=1.0)                 # ... and afterwards: into the engine's buffers
    m.train_step(None, *bt)
    cdf, _ = R.build(counts + 1.0)
    assert np.array_equal(m._train.samples.cpu().numpy(), R.draw(1, 2, cdf, 16))


def _planted_batch(rs, B, T, itemnum):
    return R.planted_skewed(rs, B, T, itemnum)


def test_captured_graph_follows_new_weights_and_fed_multi_step_path_matches_train_step(E):
    B, T, D, itemnum = 16, 20, 32, 300
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=5, loss="sampled_ce", ce_negatives=64,
                 ce_proposal="popularity")
    batches = [_planted_batch(np.random.RandomState(100 + i), B, T, itemnum) for i in range(8)]
    w1 = R.zipf_weights(itemnum + 1, 1.0)
    w2 = w1[::-1].copy()
    cdf1, _ = R.build(w1)
    cdf2, _ = R.build(w2)
    a = E.Engine("sasrec", 10, itemnum, hp, B, training=True)
    assert a.loss == "sampled_ce" and a.ce_proposal == "popularity"
    a.capture()
    a.set_step(1)
    a.set_item_weights(w1)
    a.enable_feed(n_slots=16, steps_per_graph=4)
    assert a.graph_steps == 4
    ran = 0
    for bt in batches:
        a.feed(*bt)
    while ran < 8:
        ran += a.train_fed()
    torch.cuda.synchronize()
    b = E.Engine("sasrec", 10, itemnum, hp, B, training=True)
    b.capture()
    b.set_step(1)
    b.set_item_weights(w1)
    seen = []
    for bt in batches:
        b.train_step(*bt)
        seen.append(b.samples.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert a.step_number() == b.step_number() == 9
    for k, s in enumerate(seen):
        assert np.array_equal(s, R.draw(5, k + 1, cdf1, 64)), k
    assert np.array_equal(a.samples.cpu().numpy(), seen[-1])
    pa, pb = a.get_params(), b.get_params()
    d = np.concatenate([(pa[k] - pb[k]).abs().reshape(-1).cpu().numpy() for k in pa if not k.endswith(".bk")])
    assert np.quantile(d, 0.999) < 1e-5 and d.max() < 8 * hp.lr, (np.quantile(d, 0.999), d.max())
    assert a.loss_auc()[0] == pytest.approx(b.loss_auc()[0], rel=1e-4)
    # new weights behind a captured graph: the next step draws from the new cdf
    b.set_item_weights(w2)
    b.train_step(*batches[0])
    torch.cuda.synchronize()
    got = b.samples.cpu().numpy()
    assert np.array_equal(got, R.draw(5, 9, cdf2, 64)) and not np.array_equal(got, R.draw(5, 9, cdf1, 64))
    assert math.isfinite(b.loss_auc()[0])


def test_main_cli_trains_with_the_popularity_proposal(tmp_path, monkeypatch, caplog):
    import json
    import logging
    import re
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "cast_1", "--maxlen", "12", "--batch_size", "4",
                   "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20", "--loss", "sampled_ce",
                   "--ce_negatives", "16", "--ce_proposal", "popularity", "--ce_pop_power", "0.75"])
    assert rc == 0
    runs = os.listdir(tmp_path / "saved_models" / "synthetic_tiny")
    d = tmp_path / "saved_models" / "synthetic_tiny" / runs[0]
    params = json.loads((d / "params.txt").read_text())
    assert params["loss"] == "sampled_ce" and params["ce_proposal"] == "popularity" and params["ce_pop_power"] == 0.75
    assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
    eff = re.findall(r"popularity proposal: power (\S+), effective number of items (\S+) of (\d+)", caplog.text)
    assert len(eff) == 1 and float(eff[0][0]) == 0.75 and 1.0 <= float(eff[0][1]) <= float(eff[0][2]), caplog.text[-2000:]
    train = [float(x) for x in re.findall(r"TRAIN/loss (\S+)", caplog.text)]
    assert len(train) == 2, caplog.text[-2000:]
    vals = train + [float(x) for x in re.findall(r"\d+\.\d+", (d / "log.txt").read_text())]
    assert all(math.isfinite(v) for v in vals), vals
    assert all(v > 0 for v in train), train


def test_popularity_training_learns_the_skewed_planted_corpus(E):
    c = R.PLANTED
    rs = np.random.RandomState(0)
    B, T, D, itemnum = c["B"], c["T"], c["D"], c["itemnum"]
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.1, lr=c["lr"], seed=3)
    eng = E.Engine("sasrec", 10, itemnum, hp, B, training=True, loss="sampled_ce", ce_negatives=c["N"], ce_proposal="popularity")
    eng.set_item_weights(R.planted_counts() + 1.0)
    eng.capture()
    eng.set_step(1)
    for _ in range(c["steps"]):
        eng.train_step(*R.planted_skewed(rs, B, T, itemnum))
    torch.cuda.synchronize()
    loss, _ = eng.loss_auc()
    print("loss %.4f" % loss)
    assert loss < R.PLANTED_LOSS, loss
    # full-ranking HR@10 of the next item after each test sequence's last one (chance: 10 / 400)
    ev = E.Engine("sasrec", 10, itemnum, hp, B, training=False, share=eng)
    seq, pos, _ = R.planted_skewed(np.random.RandomState(99), B, T, itemnum)
    ev.forward_eval(seq)
    ids, _, rank = ev.topk(10, targets=pos[:, -1])
    torch.cuda.synchronize()
    hr = float((rank.cpu().numpy() < 10).mean())
    print("HR@10 %.3f" % hr)
    assert hr > R.PLANTED_HR, hr

"""gBCE on the GPU: cr_gbce against fp64 with caller-supplied samples (every element of loss_out, d_seq_emb and table_grad inside 4x the
per-element bound of gbce_ref, which a numpy emulation of the device arithmetic meets at 1x in test_gbce_host.py), rows whose every
sample is a hit, padding, accumulation, the state block, pitch, determinism and the device draw; Engine(loss="gbce") against the
oracle's seq_emb with the gBCE loss + autograd in fp64, the fed multi-step path, the launch list, the refusals, the CLI and the
planted corpus."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import fpmodel as fm

import gbce_ref
import sce_ref
from test_ce_gpu import _batch, _planted
from test_sce_gpu import _case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import castrec_amd  # noqa: F401
    from castrec_amd import engine
    return engine


def _ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import lib as L
    from castrec_amd import ops as O
    return L, O


def _run(h, E_, pos, neg, samples, prec, beta=1.0, tg0=None, state0=None, ld=None, seed=0, step=None, N=None, want_tg=True):
    L, O = _ops()
    M, D = h.shape
    V = E_.shape[0]
    N = len(samples) if samples is not None else N
    ld = ld or D
    hs = torch.zeros(M, ld, dtype=torch.float32, device="cuda")
    hs[:, :D] = torch.from_numpy(h)
    if ld > D:
        hs[:, D:] = float("nan")
    tab = torch.from_numpy(E_).cuda()
    p = torch.from_numpy(pos).cuda()
    n = torch.from_numpy(neg).cuda()
    smp = torch.from_numpy(samples).cuda() if samples is not None else None
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda") if state0 is None else state0.clone()
    if step is not None:
        st[4:5].view(torch.int32)[0] = step - 2 ** 32 if step >= 2 ** 31 else step          # (the uint32 word's bits)
    dh = torch.full((M, D), float("nan"), dtype=torch.float32, device="cuda")
    tg = (torch.zeros(V, D, dtype=torch.float32, device="cuda") if tg0 is None else tg0.clone()) if want_tg else None
    lo = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    so = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(O.gbce_workspace_bytes(M, N, D), dtype=torch.uint8, device="cuda")
    O.gbce(hs, ld, tab, p, st, ws, M, N, beta=beta, precision=prec, neg=n, samples=smp, seed=seed, step=st[4:5], samples_out=so,
           d_seq_emb=dh, ldd=D, table_grad=tg, loss_out=lo)
    torch.cuda.synchronize()
    return dict(dh=dh.cpu().numpy(), tg=tg.cpu().numpy() if want_tg else None, l=lo.cpu().numpy(), state=st.cpu().numpy(),
                samples=so.cpu().numpy())


CASES = [(D, N, V) for D in (8, 20, 50, 64, 128, 256) for N in (1, 7, 256, 2048) for V in (17, 3417, 100003)]


@pytest.mark.parametrize("D,N,V", CASES)
def test_gbce_against_fp64(D, N, V):
    L, _ = _ops()
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"gbce%d_%d_%d" % (D, N, V)))
    betas = (1.0, 0.25) + ((1e-3,) if (D, N, V) == (50, 256, 3417) else ())
    for b in betas:
        got = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=b)
        ref = gbce_ref.ref64(h, E_, pos, neg, s, b)
        print("D %d N %d V %d beta %g: worst dE ratio %.3f of 4" % (D, N, V, b, 4 * gbce_ref.check(got, ref, 4.0)))
        assert np.all(got["dh"][pos == 0] == 0.0) and np.all(got["l"][pos == 0] == 0.0)
        assert np.array_equal(got["samples"], s)
        assert np.all(got["tg"][0] == 0.0)
        sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
        auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
        assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6


@pytest.mark.parametrize("D,N,V", [(20, 256, 17), (50, 256, 3417), (128, 2048, 100003), (256, 7, 3417)])
def test_plain_bf16_bound(D, N, V):
    L, _ = _ops()
    h, E_, pos, neg, s = _case(D, V, 151, N, 11 + D + N)
    for b in (1.0, 0.25):
        gbce_ref.check(_run(h, E_, pos, neg, s, L.PREC_BF16, beta=b), gbce_ref.ref64(h, E_, pos, neg, s, b, bf16=True), 4.0)


def test_pitch_many_rows_and_many_samples():
    """ld > D with NaN in the padding columns, more rows than one part of the sample sweep, N above the part budget's knee."""
    L, _ = _ops()
    h, E_, pos, neg, s = _case(50, 3417, 1237, 4100, 5)
    gbce_ref.check(_run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.3, ld=67), gbce_ref.ref64(h, E_, pos, neg, s, 0.3), 4.0)


def test_all_hit_rows_duplicates_and_padding():
    L, _ = _ops()
    D, V, M = 32, 50, 96
    rs = np.random.RandomState(2)
    h = rs.standard_normal((M, D)).astype(np.float32) * 0.3
    E_ = rs.standard_normal((V, D)).astype(np.float32)
    # every sample is the target of every live row: loss = beta softplus(-z_pos), only the target term in the gradients
    pos = np.full(M, 7, np.int32)
    pos[::3] = 0
    live = pos != 0
    neg = np.zeros(M, np.int32)
    b = 0.4
    got = _run(h, E_, pos, neg, np.full(8, 7, np.int32), L.PREC_BF16X3, beta=b)
    ref = gbce_ref.ref64(h, E_, pos, neg, np.full(8, 7, np.int32), b)
    gbce_ref.check(got, ref, 4.0)
    z = h.astype(np.float64) @ E_[7].astype(np.float64)
    lt = b * (np.maximum(-z, 0) + np.log1p(np.exp(-np.abs(z))))
    np.testing.assert_allclose(got["l"][live], lt[live], rtol=1e-4)
    gt = b * (1.0 / (1.0 + np.exp(-z)) - 1.0)
    np.testing.assert_allclose(got["dh"][live], gt[live, None] * E_[7][None, :], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(got["tg"][7], (gt[live, None] * h[live]).sum(0), rtol=1e-3, atol=1e-5)
    assert np.all(got["tg"][np.arange(V) != 7] == 0.0)
    assert np.all(got["dh"][~live] == 0.0) and np.all(got["l"][~live] == 0.0)
    assert got["state"][2] == float(live.sum())
    # padding rows contribute nothing: the same call with them removed has the same loss and gradients
    s = np.array([3, 9, 9, 7, 20], np.int32)
    pos2 = pos.copy(); pos2[1::5] = 9
    live = pos2 != 0
    a = _run(h, E_, pos2, neg, s, L.PREC_BF16X3, beta=b)
    c = _run(h[live], E_, pos2[live], neg[live], s, L.PREC_BF16X3, beta=b)
    assert np.all(a["dh"][~live] == 0.0) and np.all(a["l"][~live] == 0.0)
    np.testing.assert_allclose(a["dh"][live], c["dh"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["l"][live], c["l"], rtol=1e-6)
    # (the rows meet in other blocks of the item sweep: fp32 sums of sum |g| |h| <= 64 x 0.3 x a few in another order, ~2^-22 of it)
    np.testing.assert_allclose(a["tg"], c["tg"], rtol=1e-5, atol=1e-5)
    assert a["state"][0] == pytest.approx(c["state"][0], rel=1e-6) and a["state"][2] == c["state"][2]
    # a duplicated id: its row of table_grad is twice one copy's contribution (rows that target it drop both copies)
    zz = h.astype(np.float64) @ E_[9].astype(np.float64)
    single = ((1.0 / (1.0 + np.exp(-zz))) * (live & (pos2 != 9))) @ h.astype(np.float64)
    tgt9 = ((pos2 == 9)[:, None] * (b * (1.0 / (1.0 + np.exp(-zz)) - 1.0))[:, None] * h).sum(0)
    ref2 = gbce_ref.ref64(h, E_, pos2, neg, s, b)
    gbce_ref.check(a, ref2, 4.0)
    assert np.all(np.abs(a["tg"][9] - (2 * single + tgt9)) <= 4.0 * ref2["e_dE"][9])     # (the row's own bound: its terms cancel)
    untouched = np.setdiff1d(np.arange(V), np.concatenate([s, pos2]))
    assert np.all(a["tg"][untouched] == 0.0) and np.all(a["tg"][0] == 0.0)


@pytest.mark.parametrize("seed,step,V,N", [(42, 1, 3417, 256), (7, 123456, 17, 300), (0, 2 ** 31 + 5, 10 ** 7, 4096),
                                           (0xDEADBEEF, 9, 2, 7)])
def test_device_draw_matches_the_numpy_restatement(seed, step, V, N):
    L, _ = _ops()
    D, M = 16, 40
    h, E_, pos, neg, _ = _case(D, min(V, 4000), M, 1, 3)
    if V > E_.shape[0]:                                  # (a 10^7-row table: its rows' values do not matter here)
        E_ = np.zeros((V, D), np.float32)
        E_[:4000] = np.random.RandomState(4).standard_normal((4000, D))
    got = _run(h, E_, pos, neg, None, L.PREC_BF16X3, beta=0.5, seed=seed, step=step, N=N, want_tg=False)
    want = gbce_ref.draw(seed, step, V, N)
    assert np.array_equal(got["samples"], want)
    assert got["samples"].min() >= 1 and got["samples"].max() <= V - 1
    # the drawn ids give the results of the same ids supplied by the caller, bit for bit
    sup = _run(h, E_, pos, neg, want, L.PREC_BF16X3, beta=0.5, want_tg=False)
    for k in ("l", "dh"):
        assert np.array_equal(got[k].view(np.int32), sup[k].view(np.int32)), k
    assert np.array_equal(got["state"][:3].view(np.int32), sup["state"][:3].view(np.int32))     # ([4], [11]: the step words differ)
    if V > 2:
        nxt = _run(h, E_, pos, neg, None, L.PREC_BF16X3, beta=0.5, seed=seed, step=step + 1, N=N, want_tg=False)
        assert not np.array_equal(nxt["samples"], got["samples"])
        assert np.array_equal(nxt["samples"], gbce_ref.draw(seed, step + 1, V, N))
        # not the sampled softmax's negatives at the same seed and step
        from test_sce_gpu import _run as _run_sce
        sce = _run_sce(h, E_, pos, neg, None, L.PREC_BF16X3, seed=seed, step=step, N=N, want_tg=False)
        assert np.array_equal(sce["samples"], sce_ref.draw(seed, step, V, N)) and not np.array_equal(sce["samples"], got["samples"])


@pytest.mark.parametrize("D,V,M,N", [(50, 3417, 1300, 256), (128, 100003, 200, 2048), (8, 17, 77, 300)])
def test_two_calls_give_the_same_bits(D, V, M, N):
    L, _ = _ops()
    h, E_, pos, neg, s = _case(D, V, M, N, 3)
    a = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25)
    b = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25)
    for k in ("l", "dh", "state", "samples"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    keep = np.ones(V, bool)
    keep[pos] = False                                    # target rows take float atomics: rounding order may differ
    assert np.array_equal(a["tg"][keep].view(np.int32), b["tg"][keep].view(np.int32))
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=1e-5, atol=1e-6)


def test_table_grad_accumulates_and_untouched_rows_stay():
    L, _ = _ops()
    h, E_, pos, neg, s = _case(64, 3417, 300, 256, 9)
    rs = np.random.RandomState(1)
    pre = torch.from_numpy(rs.standard_normal(E_.shape).astype(np.float32)).cuda()
    got = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25, tg0=pre)
    base = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25)
    pre = pre.cpu().numpy()
    untouched = np.setdiff1d(np.arange(E_.shape[0]), np.concatenate([s, pos[pos != 0]]))
    assert 0 in untouched
    assert np.array_equal(got["tg"][untouched].view(np.int32), pre[untouched].view(np.int32))
    assert np.all(base["tg"][untouched] == 0.0)
    # rows of samples: one += of the same sum, the same bits; target rows: a few atomic adds onto another start, an ulp of ~10 each
    np.testing.assert_allclose(got["tg"], pre + base["tg"], rtol=0, atol=1e-5)


def test_state_block_follows_the_head_contract():
    L, _ = _ops()
    h, E_, pos, neg, s = _case(50, 500, 400, 64, 4)
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda")
    st[0], st[1], st[2] = 1.5, 2.0, 3.0
    st[4:5].view(torch.int32)[0] = 7
    got = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25, state0=st)
    ref = _run(h, E_, pos, neg, s, L.PREC_BF16X3, beta=0.25)
    g, r = got["state"], ref["state"]
    assert g[0] == np.float32(1.5) + r[0] and g[1] == np.float32(2.0) + r[1] and g[2] == 3.0 + r[2]
    assert np.array_equal(g[8:11], g[0:3])
    assert g[11:12].view(np.int32)[0] == 7 and g[4:5].view(np.int32)[0] == 7
    assert g[12:13].view(np.int32)[0] == 0
    assert r[2] == float((pos != 0).sum())


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _gbce_loss(out, pos, samples, beta):
    """The gBCE loss on the oracle's seq_emb and item table, in fp64 (loss / n_target, as Adam sees it)."""
    se, tab = out["seq_emb"], out["item_table"]
    p = torch.as_tensor(np.asarray(pos).reshape(-1), dtype=torch.long)
    s = torch.as_tensor(np.asarray(samples), dtype=torch.long)
    S = se @ tab[s].t()
    st = (se * tab[p]).sum(1)
    live = (s[None, :] != p[:, None]).to(S.dtype)
    sp = torch.nn.functional.softplus
    ist = p != 0
    return ((beta * sp(-st) + (sp(S) * live).sum(1)) * ist).sum() / ist.sum()


@pytest.mark.parametrize("model", ["sasrec", "cast_5"])
def test_engine_gbce_step_matches_oracle(E, model):
    from test_model_gpu import engine_relu_gates
    rs = np.random.RandomState(zlib.crc32(model.encode()) % 1000)
    B, T, D, H, itemnum, max_bins = 5, 24, 20, 1, 37, 12
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                 lr=1e-3, seed=7)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                   lr=1e-3)
    eng = E.Engine(model, 9, itemnum, hp, B, training=True, n_slabs=7, loss="gbce", ce_negatives=16)
    assert eng.loss == "gbce" and not eng.use_index and not eng.bitwise_reproducible and eng.ce_negatives == 16
    assert eng.gbce_t == 0.75 and eng.gbce_beta == pytest.approx(gbce_ref.beta(16, itemnum, 0.75), rel=1e-12)
    assert E.Engine(model, 9, itemnum, hp, B, training=True, loss="gbce", ce_negatives=16, gbce_t=0.0).gbce_beta == 1.0
    assert E.Engine(model, 9, itemnum, hp, B, training=True, loss="gbce", ce_negatives=16, gbce_t=1.0).gbce_beta == \
        pytest.approx(16 / 36, rel=1e-12)
    beta = eng.gbce_beta
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
    assert np.array_equal(samples, gbce_ref.draw(7, 1, itemnum + 1, 16))
    gates, care = engine_relu_gates(eng, B, T, None)

    def oracle(smp):
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
        with fm.handed_over_gates(gates, care, check=True):
            out = fm.forward(model, leaves, ohp, batch, None)
        loss = _gbce_loss(out, pos, smp, beta)
        loss.backward()
        return loss, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}

    loss, G = oracle(samples)
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


def test_fed_multi_step_path_matches_train_step(E):
    B, T, D, itemnum = 16, 20, 32, 300
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=5, loss="gbce", ce_negatives=64, gbce_t=0.5)
    batches = [_planted(np.random.RandomState(100 + i), B, T, itemnum) for i in range(8)]
    a = E.Engine("sasrec", 10, itemnum, hp, B, training=True)
    assert a.loss == "gbce" and a.ce_negatives == 64 and a.gbce_beta == pytest.approx(gbce_ref.beta(64, itemnum, 0.5))
    a.capture()
    a.set_step(1)
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
    seen = []
    for bt in batches:
        b.train_step(*bt)
        seen.append(b.samples.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert a.step_number() == b.step_number() == 9
    # each step drew its own samples: those of step k are the draw at step word k
    for k, s in enumerate(seen):
        assert np.array_equal(s, gbce_ref.draw(5, k + 1, itemnum + 1, 64)), k
    assert len({s.tobytes() for s in seen}) == 8
    assert np.array_equal(a.samples.cpu().numpy(), seen[-1])
    pa, pb = a.get_params(), b.get_params()
    d = np.concatenate([(pa[k] - pb[k]).abs().reshape(-1).cpu().numpy() for k in pa if not k.endswith(".bk")])
    assert np.quantile(d, 0.999) < 1e-5 and d.max() < 8 * hp.lr, (np.quantile(d, 0.999), d.max())
    assert a.loss_auc()[0] == pytest.approx(b.loss_auc()[0], rel=1e-4)


def test_launch_list_and_refusals(E):
    hp = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1)
    assert hp.loss == "bce" and hp.gbce_t == 0.75
    names = lambda e: [x[0] for x in e.fwd + e.bwd]
    g = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="gbce")
    s = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="sampled_ce")
    ng = names(g)
    assert ng.count("cr_gbce") == 1 and "cr_sampled_ce" not in ng and "cr_softmax_ce" not in ng
    assert [n if n != "cr_gbce" else "cr_sampled_ce" for n in ng] == names(s)       # the route of "sampled_ce"
    assert g.ce_negatives == 256 and tuple(g.samples.shape) == (256,) and not g.use_index and not g.bitwise_reproducible
    assert g.gbce_beta == pytest.approx(gbce_ref.beta(256, 500, 0.75))
    for loss in ("bce", "ce", "sampled_ce"):
        e = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss=loss, gbce_t=0.3)
        assert "cr_gbce" not in names(e) and e.loss == loss
    a = E.Engine("cast_1", 10, 500, hp, 64, training=True)
    assert a.loss == "bce" and a.use_index and a.bitwise_reproducible
    assert names(a) == names(E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="bce", ce_negatives=17, gbce_t=0.1))
    hp_g = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1, loss="gbce", ce_negatives=32, gbce_t=0.25)
    e = E.Engine("cast_1", 10, 500, hp_g, 8, training=True)
    assert e.loss == "gbce" and e.ce_negatives == 32 and e.gbce_t == 0.25
    assert E.Engine("cast_1", 10, 500, hp_g, 8, training=True, gbce_t=0.5).gbce_t == 0.5
    assert E.Engine("cast_1", 10, 500, hp_g, 8, training=False).loss == "bce"      # eval engines ignore it
    # refusals
    hp = E.Hyper(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=1)
    with pytest.raises(ValueError, match="lazy_adam"):
        E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="gbce", lazy_adam=True)
    with pytest.raises(ValueError, match="data parallelism"):
        E.Engine("sasrec", 10, 100, hp, 4, training=True, loss="gbce", batch_global=8, row_offset=80)
    with pytest.raises(ValueError, match="hidden_units"):
        E.Engine("sasrec", 10, 100, E.Hyper(maxlen=20, hidden_units=4, num_blocks=1, num_heads=1, seed=1), 8, training=True,
                 loss="gbce")
    for n in (0, 16385):
        with pytest.raises(ValueError, match="ce_negatives"):
            E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="gbce", ce_negatives=n)
    for t in (-0.1, 1.5):
        with pytest.raises(ValueError, match="gbce_t"):
            E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="gbce", gbce_t=t)
    from castrec_amd.models import build_model
    import types
    args = types.SimpleNamespace(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3,
                                 max_bins=20, num_context_blocks=1, seed=1, loss="gbce", ce_negatives=16, gbce_t=0.75)
    m = build_model("sasrec", 10, 100, 0, args)
    with pytest.raises(ValueError, match="data parallelism"):
        m.data_parallel(0, 2)


def test_main_cli_trains_with_gbce_and_logs_finite_numbers(tmp_path, monkeypatch, caplog):
    import json
    import logging
    import re
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "cast_1", "--maxlen", "12", "--batch_size", "4",
                   "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20", "--loss", "gbce",
                   "--ce_negatives", "16", "--gbce_t", "0.5", "--eval_full_ranking"])
    assert rc == 0
    runs = os.listdir(tmp_path / "saved_models" / "synthetic_tiny")
    d = tmp_path / "saved_models" / "synthetic_tiny" / runs[0]
    params = json.loads((d / "params.txt").read_text())
    assert params["loss"] == "gbce" and params["ce_negatives"] == 16 and params["gbce_t"] == 0.5
    assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
    train = [float(x) for x in re.findall(r"TRAIN/loss (\S+)", caplog.text)]
    full = re.findall(r"full ranking: valid \(NDCG@10: (\S+), HR@10: (\S+)\), test \(NDCG@10: (\S+), HR@10: (\S+)\)", caplog.text)
    assert len(train) == 2 and len(full) == 2, caplog.text[-2000:]
    vals = train + [float(x) for row in full for x in row] + [float(x) for x in re.findall(r"\d+\.\d+", (d / "log.txt").read_text())]
    assert all(math.isfinite(v) for v in vals), vals
    assert all(0 < v < 3 * 17 * math.log(2) for v in train), train      # (17 binary terms per row at most, log 2 each at z = 0)


def test_gbce_training_learns_a_planted_corpus(E):
    """The structure and thresholds of test_sampled_ce_training_learns_a_planted_corpus, on gbce_ref.PLANTED_STEPS steps: gBCE first
    settles on the constant-score plateau (loss 2.28 here, ranking at chance) and the fp64 reference of this very objective leaves it
    between steps 450 and 600, so the softmax's 250 steps measure the plateau, not the implementation (250 steps on the GPU: loss
    below the threshold, HR@10 0.078; the reference at 250 steps: loss 2.29, HR@10 0.11).  test_gbce_host.py runs the reference on this
    schedule against the same thresholds."""
    rs = np.random.RandomState(0)
    c = gbce_ref.PLANTED
    B, T, D, itemnum = c["B"], c["T"], c["D"], c["itemnum"]
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.1, lr=c["lr"], seed=3)
    eng = E.Engine("sasrec", 10, itemnum, hp, B, training=True, loss="gbce", ce_negatives=c["N"])
    assert eng.gbce_t == c["t"]
    eng.capture()
    eng.set_step(1)
    for _ in range(gbce_ref.PLANTED_STEPS):
        eng.train_step(*_planted(rs, B, T, itemnum))
    torch.cuda.synchronize()
    loss, _ = eng.loss_auc()
    # half of the loss of an untrained model (every score 0: beta log 2 for the target, log 2 per negative)
    assert loss < 0.5 * (eng.gbce_beta + 64) * math.log(2), loss
    # full-ranking HR@10 of the next item after each test sequence's last one (chance: 10 / 400)
    ev = E.Engine("sasrec", 10, itemnum, hp, B, training=False, share=eng)
    seq, pos, _ = _planted(np.random.RandomState(99), B, T, itemnum)
    ev.forward_eval(seq)
    ids, _, rank = ev.topk(10, targets=pos[:, -1])
    torch.cuda.synchronize()
    hr = float((rank.cpu().numpy() < 10).mean())
    print("planted corpus after %d steps: loss %.4f, HR@10 %.3f" % (gbce_ref.PLANTED_STEPS, loss, hr))
    assert hr > 0.5, hr

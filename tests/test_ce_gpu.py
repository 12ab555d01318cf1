"""Full-catalogue softmax cross-entropy on the GPU: cr_softmax_ce against fp64 (per-element bounds built from the fp64 absolute
products), accumulation, determinism and the state block; Engine(loss="ce") against the oracle's seq_emb with CE + autograd in fp64,
the fed multi-step path, the unchanged default, the refusals, the CLI and a planted corpus that CE training has to learn."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import fpmodel as fm

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


def _case(D, V, M, seed):
    """h [M, D], table [V, D] (row 0 random too: it must not take part), ~30 % padded rows, repeated targets, one target V-1."""
    rs = np.random.RandomState(seed)
    h = rs.standard_normal((M, D)).astype(np.float32) * (1.5 / math.sqrt(D))
    E_ = rs.standard_normal((V, D)).astype(np.float32) * 1.5
    pos = rs.randint(1, V, M).astype(np.int32)
    pos[rs.rand(M) < 0.3] = 0
    live = np.flatnonzero(pos)
    if len(live) > 3:
        pos[live[1]] = pos[live[0]]                      # a repeated target
        pos[live[2]] = V - 1                             # the table's last row
    neg = rs.randint(1, V, M).astype(np.int32)
    neg[pos == 0] = 0
    return h, E_, pos, neg


def _run(h, E_, pos, neg, prec, tg0=None, state0=None, ld=None):
    L, O = _ops()
    M, D = h.shape
    V = E_.shape[0]
    ld = ld or D
    hs = torch.zeros(M, ld, dtype=torch.float32, device="cuda")
    hs[:, :D] = torch.from_numpy(h)
    if ld > D:
        hs[:, D:] = float("nan")                         # the pitch's extra columns must never be read into a score
    tab = torch.from_numpy(E_).cuda()
    p = torch.from_numpy(pos).cuda()
    n = torch.from_numpy(neg).cuda()
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda") if state0 is None else state0.clone()
    dh = torch.full((M, D), float("nan"), dtype=torch.float32, device="cuda")
    tg = torch.zeros(V, D, dtype=torch.float32, device="cuda") if tg0 is None else tg0.clone()
    lse = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(O.softmax_ce_workspace_bytes(M, V, D), dtype=torch.uint8, device="cuda")
    O.softmax_ce(hs, ld, tab, p, st, ws, M, precision=prec, neg=n, d_seq_emb=dh, ldd=D, table_grad=tg, lse_out=lse)
    torch.cuda.synchronize()
    return dict(dh=dh.cpu().numpy(), tg=tg.cpu().numpy(), lse=lse.cpu().numpy(), state=st.cpu().numpy())


def _ref64(h, E_, pos, neg, bf16=False):
    """fp64 results and per-element error bounds.  A score's error bound es_mv = u * sum_i |h_mi E_vi| (u = 2^-15 for the bf16x3
    products, 2^-7 for plain bf16), carried through the p-weighted sums."""
    u = 2.0 ** -7 if bf16 else 2.0 ** -15
    acc = 2.0 ** -7 if bf16 else 2.0 ** -14              # relative bound of the fp32 / bf16-operand sums of the gradients
    h = h.astype(np.float64)
    T = E_[1:].astype(np.float64)
    S = h @ T.T                                          # [M, V-1]
    es = u * (np.abs(h) @ np.abs(T).T)
    mx = S.max(1, keepdims=True)
    Z = np.exp(S - mx)
    lse = mx[:, 0] + np.log(Z.sum(1))
    P = Z / Z.sum(1, keepdims=True)
    ist = pos != 0
    rows = np.arange(len(pos))
    e_lse = (P * es).sum(1) + 2.0 ** -20 * (1.0 + np.abs(lse))
    G = P.copy()
    G[rows[ist], pos[ist] - 1] -= 1.0
    G[~ist] = 0.0
    dh = G @ T
    dE = np.zeros_like(E_, dtype=np.float64)
    dE[1:] = G.T @ h
    # |dp_mv| <= p_mv (es_mv + e_lse_m)
    W = P * (es + e_lse[:, None])
    W[~ist] = 0.0
    Pa = np.abs(G)
    e_dh = W @ np.abs(T) + acc * (Pa @ np.abs(T))
    e_dE = np.zeros_like(dE)
    e_dE[1:] = W.T @ np.abs(h) + acc * (Pa.T @ np.abs(h))
    sp = np.where(ist, S[rows, np.maximum(pos, 1) - 1], 0.0)
    loss = float((lse - sp)[ist].sum())
    e_loss = float((e_lse + np.where(ist, es[rows, np.maximum(pos, 1) - 1], 0.0))[ist].sum())
    sn = np.where(neg > 0, S[rows, np.maximum(neg, 1) - 1], 0.0)
    return dict(lse=lse, e_lse=e_lse, dh=dh, e_dh=e_dh, dE=dE, e_dE=e_dE, loss=loss, e_loss=e_loss, n=float(ist.sum()),
                sp=sp, sn=sn, ist=ist)


def _check(got, ref, scale=4.0):
    assert np.all(np.abs(got["lse"] - ref["lse"]) <= scale * ref["e_lse"]), np.max(np.abs(got["lse"] - ref["lse"]) / ref["e_lse"])
    r = np.abs(got["dh"] - ref["dh"]) / (scale * ref["e_dh"] + 1e-30)
    assert np.all(r <= 1.0), ("dh", float(r.max()), np.unravel_index(np.argmax(r), r.shape))
    r = np.abs(got["tg"][1:] - ref["dE"][1:]) / (scale * ref["e_dE"][1:] + 1e-30)
    assert np.all(r <= 1.0), ("dE", float(r.max()), np.unravel_index(np.argmax(r), r.shape))
    assert abs(got["state"][0] - ref["loss"]) <= scale * ref["e_loss"] + 1e-6 * abs(ref["loss"]) + 1e-5, (got["state"][0], ref["loss"])
    assert got["state"][2] == ref["n"]


CASES = [(D, V) for D in (8, 20, 50, 64, 128, 256) for V in (2, 17, 3417, 100003)]


@pytest.mark.parametrize("D,V", CASES)
def test_softmax_ce_against_fp64(D, V):
    L, _ = _ops()
    M = 61 if V > 10000 else 203
    h, E_, pos, neg = _case(D, V, M, zlib.crc32(b"ce%d_%d" % (D, V)))
    got = _run(h, E_, pos, neg, L.PREC_BF16X3)
    ref = _ref64(h, E_, pos, neg)
    _check(got, ref)
    assert np.all(got["dh"][pos == 0] == 0.0)
    # the AUC of the sampled negatives (ties are measure-zero here; a near-tie may round either way)
    sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
    auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
    assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6


@pytest.mark.parametrize("D,V", [(20, 17), (50, 3417), (128, 100003)])
def test_plain_bf16_bound(D, V):
    L, _ = _ops()
    M = 61 if V > 10000 else 203
    h, E_, pos, neg = _case(D, V, M, 11 + D)
    _check(_run(h, E_, pos, neg, L.PREC_BF16), _ref64(h, E_, pos, neg, bf16=True))


def test_pitch_and_many_rows():
    """ld > D (an engine's seq_emb column block), more rows than one part of the item sweep, a row count off every tile size."""
    L, _ = _ops()
    h, E_, pos, neg = _case(50, 3417, 1237, 5)
    _check(_run(h, E_, pos, neg, L.PREC_BF16X3, ld=67), _ref64(h, E_, pos, neg))


def test_table_grad_accumulates_and_row_zero_is_untouched():
    L, _ = _ops()
    h, E_, pos, neg = _case(64, 3417, 300, 9)
    rs = np.random.RandomState(1)
    pre = torch.from_numpy(rs.standard_normal(E_.shape).astype(np.float32)).cuda()
    got = _run(h, E_, pos, neg, L.PREC_BF16X3, tg0=pre)
    base = _run(h, E_, pos, neg, L.PREC_BF16X3)
    pre = pre.cpu().numpy()
    assert np.array_equal(got["tg"][0].view(np.int32), pre[0].view(np.int32))
    assert np.array_equal(base["tg"][0], np.zeros(64, np.float32))
    np.testing.assert_allclose(got["tg"][1:], pre[1:] + base["tg"][1:], rtol=0, atol=1e-6)


@pytest.mark.parametrize("D,V,M", [(50, 3417, 1300), (128, 100003, 200), (8, 17, 77)])
def test_two_calls_give_the_same_bits(D, V, M):
    L, _ = _ops()
    h, E_, pos, neg = _case(D, V, M, 3)
    a = _run(h, E_, pos, neg, L.PREC_BF16X3)
    b = _run(h, E_, pos, neg, L.PREC_BF16X3)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_state_block_follows_the_head_contract():
    L, _ = _ops()
    h, E_, pos, neg = _case(50, 500, 400, 4)
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda")
    st[0], st[1], st[2] = 1.5, 2.0, 3.0
    st[4:5].view(torch.int32)[0] = 7
    st[12:13].view(torch.int32)[0] = 0
    got = _run(h, E_, pos, neg, L.PREC_BF16X3, state0=st)
    ref = _run(h, E_, pos, neg, L.PREC_BF16X3)
    s, r = got["state"], ref["state"]
    assert s[0] == np.float32(1.5) + r[0] and s[1] == np.float32(2.0) + r[1] and s[2] == 3.0 + r[2]
    assert np.array_equal(s[8:11], s[0:3])
    assert s[11:12].view(np.int32)[0] == 7 and s[4:5].view(np.int32)[0] == 7
    assert s[12:13].view(np.int32)[0] == 0
    assert r[2] == float((pos != 0).sum())


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _batch(rs, B, T, itemnum, max_bins):
    seq = rs.randint(1, itemnum + 1, (B, T)); pos = rs.randint(1, itemnum + 1, (B, T)); neg = rs.randint(1, itemnum + 1, (B, T))
    for b in range(B):
        n = rs.randint(0, T - 2)
        seq[b, :n] = 0; pos[b, :n] = 0; neg[b, :n] = 0
    pos[1, -1] = itemnum                                         # the table's last row as a target
    time = rs.randint(0, max_bins + 1, (B, T)) * (seq != 0)
    time[:, -1] = 0
    hours = rs.randint(1, 25, (B, T)) * (seq != 0); days = rs.randint(1, 8, (B, T)) * (seq != 0)
    return seq, pos, neg, time, hours, days


def _ce_loss(out, pos):
    """CE over items 1 .. V-1 on the oracle's seq_emb and zero-padded item table, in fp64 (loss / n_target, as Adam sees it)."""
    se, tab = out["seq_emb"], out["item_table"]
    S = se @ tab[1:].t()
    p = torch.as_tensor(np.asarray(pos).reshape(-1), dtype=torch.long)
    ist = p != 0
    lse = torch.logsumexp(S, 1)
    sp = S.gather(1, (p.clamp(min=1) - 1)[:, None])[:, 0]
    return ((lse - sp) * ist).sum() / ist.sum()


@pytest.mark.parametrize("model", ["sasrec", "cast_1", "cast_5", "cast_9"])
def test_engine_ce_step_matches_oracle(E, model):
    from test_model_gpu import engine_relu_gates
    rs = np.random.RandomState(zlib.crc32(model.encode()) % 1000)
    B, T, D, H, itemnum, max_bins = 5, 24, 20, 1, 37, 12
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                 lr=1e-3, seed=7)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                   lr=1e-3)
    eng = E.Engine(model, 9, itemnum, hp, B, training=True, n_slabs=7, loss="ce")
    assert eng.loss == "ce" and not eng.use_index and not eng.bitwise_reproducible
    P = fm.init_params(model, 9, itemnum, ohp, seed=3)
    P = {k: v + 0.1 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
    eng.load_params(P)
    P = {k: v.double().cpu() for k, v in eng.get_params().items()}
    seq, pos, neg, time, hours, days = _batch(rs, B, T, itemnum, max_bins)
    batch = fm.to_batch(seq, pos, neg, time, hours, days)
    eng.set_batch(seq, pos, neg, time, hours, days)
    eng.launch_step(apply=False)
    torch.cuda.synchronize()
    gates, care = engine_relu_gates(eng, B, T, None)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    with fm.handed_over_gates(gates, care, check=True):
        out = fm.forward(model, leaves, ohp, batch, None)
    loss = _ce_loss(out, pos)
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
    # one Adam step on both sides
    eng.Gt.zero_()
    eng.set_step(1)
    eng.launch_step(apply=True)
    torch.cuda.synchronize()
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


def _planted(rs, B, T, itemnum):
    """Sequences of consecutive items (item i is followed by item i + 1), left-padded to T."""
    seq = np.zeros((B, T), np.int64); pos = np.zeros((B, T), np.int64); neg = np.zeros((B, T), np.int64)
    for b in range(B):
        n = rs.randint(T // 2, T + 1)
        s = rs.randint(1, itemnum - n)
        seq[b, T - n:] = np.arange(s, s + n)
        pos[b, T - n:] = np.arange(s + 1, s + n + 1)
        neg[b, T - n:] = rs.randint(1, itemnum + 1, n)
    return seq, pos, neg


def test_fed_multi_step_path_matches_train_step(E):
    B, T, D, itemnum = 16, 20, 32, 300
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=5)
    batches = [_planted(np.random.RandomState(100 + i), B, T, itemnum) for i in range(8)]
    a = E.Engine("sasrec", 10, itemnum, hp, B, training=True, loss="ce")
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
    b = E.Engine("sasrec", 10, itemnum, hp, B, training=True, loss="ce")
    b.capture()
    b.set_step(1)
    for bt in batches:
        b.train_step(*bt)
    torch.cuda.synchronize()
    assert a.step_number() == b.step_number() == 9
    pa, pb = a.get_params(), b.get_params()
    # the embedding backward's float atomics differ in order between runs: rounding, then Adam's divide by sqrt(v).  d loss / d bk
    # == 0 identically, so Adam moves bk by +-lr on rounding noise alone (on any two runs): not compared.
    d = np.concatenate([(pa[k] - pb[k]).abs().reshape(-1).cpu().numpy() for k in pa if not k.endswith(".bk")])
    assert np.quantile(d, 0.999) < 1e-5 and d.max() < 8 * hp.lr, (np.quantile(d, 0.999), d.max())
    assert a.loss_auc()[0] == pytest.approx(b.loss_auc()[0], rel=1e-4)


def test_default_engine_is_unchanged(E):
    hp = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1)
    assert hp.loss == "bce"
    a = E.Engine("cast_1", 10, 500, hp, 64, training=True)
    b = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="bce")
    assert a.loss == "bce" and a.use_index and a.bitwise_reproducible
    names = lambda e: [x[0] for x in e.fwd + e.bwd]
    assert names(a) == names(b) and a.n_kernel_launches() == b.n_kernel_launches()
    assert "cr_softmax_ce" not in names(a) and any(n.startswith("cr_stack_fwd_head") or n.startswith("cr_head") for n in names(a))
    c = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="ce")
    assert "cr_softmax_ce" in names(c) and not any(n.startswith("cr_head") or n == "cr_stack_fwd_head" for n in names(c))
    hp_ce = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1, loss="ce")
    assert E.Engine("cast_1", 10, 500, hp_ce, 8, training=True).loss == "ce"
    assert E.Engine("cast_1", 10, 500, hp_ce, 8, training=False).loss == "bce"      # eval engines ignore it


def test_refusals(E):
    hp = E.Hyper(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=1)
    with pytest.raises(ValueError, match="lazy_adam"):
        E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="ce", lazy_adam=True)
    with pytest.raises(ValueError, match="data parallelism"):
        E.Engine("sasrec", 10, 100, hp, 4, training=True, loss="ce", batch_global=8, row_offset=80)
    with pytest.raises(ValueError, match="hidden_units"):
        E.Engine("sasrec", 10, 100, E.Hyper(maxlen=20, hidden_units=4, num_blocks=1, num_heads=1, seed=1), 8, training=True, loss="ce")
    with pytest.raises(ValueError, match="loss must be one of"):
        E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="softmax")
    from castrec_amd.models import build_model
    import types
    args = types.SimpleNamespace(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3,
                                 max_bins=20, num_context_blocks=1, seed=1, loss="ce")
    m = build_model("sasrec", 10, 100, 0, args)
    with pytest.raises(ValueError, match="data parallelism"):
        m.data_parallel(0, 2)


def test_main_cli_trains_with_ce_and_logs_finite_numbers(tmp_path, monkeypatch, caplog):
    import logging
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "cast_1", "--maxlen", "12", "--batch_size", "4",
                   "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20", "--loss", "ce",
                   "--eval_full_ranking"])
    assert rc == 0
    runs = os.listdir(tmp_path / "saved_models" / "synthetic_tiny")
    d = tmp_path / "saved_models" / "synthetic_tiny" / runs[0]
    import json
    assert json.loads((d / "params.txt").read_text())["loss"] == "ce"
    assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
    import re
    train = [float(x) for x in re.findall(r"TRAIN/loss (\S+)", caplog.text)]
    full = re.findall(r"full ranking: valid \(NDCG@10: (\S+), HR@10: (\S+)\), test \(NDCG@10: (\S+), HR@10: (\S+)\)", caplog.text)
    assert len(train) == 2 and len(full) == 2, caplog.text[-2000:]
    vals = train + [float(x) for row in full for x in row] + [float(x) for x in re.findall(r"\d+\.\d+", (d / "log.txt").read_text())]
    assert all(math.isfinite(v) for v in vals), vals
    assert all(0 < v < 3 * math.log(41) for v in train), train      # (synthetic:tiny: 40 items)


def test_ce_training_learns_a_planted_corpus(E):
    rs = np.random.RandomState(0)
    B, T, D, itemnum = 64, 20, 32, 400
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.1, lr=5e-3, seed=3)
    eng = E.Engine("sasrec", 10, itemnum, hp, B, training=True, loss="ce")
    eng.capture()
    eng.set_step(1)
    for _ in range(250):
        eng.train_step(*_planted(rs, B, T, itemnum))
    torch.cuda.synchronize()
    loss, _ = eng.loss_auc()
    assert loss < 0.3 * math.log(itemnum), loss
    # full-ranking HR@10 of the next item after each test sequence's last one (chance: 10 / 400)
    ev = E.Engine("sasrec", 10, itemnum, hp, B, training=False, share=eng)
    seq, pos, _ = _planted(np.random.RandomState(99), B, T, itemnum)
    ev.forward_eval(seq)
    ids, _, rank = ev.topk(10, targets=pos[:, -1])
    torch.cuda.synchronize()
    hr = float((rank.cpu().numpy() < 10).mean())
    assert hr > 0.5, hr

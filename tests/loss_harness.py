"""GPU side of the candidate-sweep losses' tests: one run() for cr_softmax_ce ("ce"), cr_sampled_ce ("sampled_ce", either proposal) and
cr_gbce ("gbce"), and the bodies of the tests that every loss has, each taking the loss's name and that loss's literals.  castrec_amd is
imported inside the functions: the test modules collect without the native library.

A case is (h, E_, pos, neg, samples) as loss_ref.sampled_case makes it; for "ce" (no samples) the last entry is None."""
import json
import logging
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import fpmodel as fm

import loss_ref
from model_harness import engine_relu_gates

ROW_KEY = {"ce": "lse", "sampled_ce": "lse", "gbce": "l"}       # the per-row output, as each loss's tests name it


def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import lib as L
    from castrec_amd import ops as O
    return L, O


def run(loss, h, E_, pos, neg, samples, prec, beta=1.0, cdf=None, logq=None, N=None, seed=0, step=None, want_tg=True, tg0=None,
        state0=None, ld=None):
    """One call of the loss's kernel on fresh buffers; prec "bf16x3" or "bf16".  What the kernel must write is NaN (-1 for the ids)
    beforehand, and so are the pitch's extra columns, which must never be read into a score."""
    L, O = ops()
    prec = {"bf16x3": L.PREC_BF16X3, "bf16": L.PREC_BF16}[prec]
    M, D = h.shape
    V = E_.shape[0]
    ld = ld or D
    hs = torch.zeros(M, ld, dtype=torch.float32, device="cuda")
    hs[:, :D] = torch.from_numpy(h)
    if ld > D:
        hs[:, D:] = float("nan")
    tab = torch.from_numpy(E_).cuda()
    p = torch.from_numpy(pos).cuda()
    n = torch.from_numpy(neg).cuda()
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda") if state0 is None else state0.clone()
    if step is not None:
        st[4:5].view(torch.int32)[0] = step - 2 ** 32 if step >= 2 ** 31 else step          # (the uint32 word's bits)
    dh = torch.full((M, D), float("nan"), dtype=torch.float32, device="cuda")
    tg = (torch.zeros(V, D, dtype=torch.float32, device="cuda") if tg0 is None else tg0.clone()) if want_tg else None
    row = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    out = dict(dh=dh, tg=tg, state=st)
    out[ROW_KEY[loss]] = row
    if loss == "ce":
        ws = torch.empty(O.softmax_ce_workspace_bytes(M, V, D), dtype=torch.uint8, device="cuda")
        O.softmax_ce(hs, ld, tab, p, st, ws, M, precision=prec, neg=n, d_seq_emb=dh, ldd=D, table_grad=tg, lse_out=row)
    else:
        N = len(samples) if samples is not None else N
        smp = torch.from_numpy(samples).cuda() if samples is not None else None
        out["samples"] = so = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        common = dict(precision=prec, neg=n, samples=smp, seed=seed, step=st[4:5], samples_out=so, d_seq_emb=dh, ldd=D, table_grad=tg)
        if loss == "sampled_ce":
            ws = torch.empty(O.sampled_ce_workspace_bytes(M, N, D), dtype=torch.uint8, device="cuda")
            c = torch.from_numpy(cdf.view(np.int32)).cuda() if cdf is not None else None
            q = torch.from_numpy(logq).cuda() if logq is not None else None
            O.sampled_ce(hs, ld, tab, p, st, ws, M, N, lse_out=row, cdf=c, logq=q, **common)
        else:
            ws = torch.empty(O.gbce_workspace_bytes(M, N, D), dtype=torch.uint8, device="cuda")
            O.gbce(hs, ld, tab, p, st, ws, M, N, beta=beta, loss_out=row, **common)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


# ---- the kernel's contract -----------------------------------------------------------------------------------------------------------
def device_draw_matches(loss, seed, step, V, N, want, **kw):
    """The ids drawn on the device are want(step)'s, and they give the results of the same ids supplied by the caller, bit for bit.
    Returns (h, E_, pos, neg, got) for what one loss checks on top."""
    D, M = 16, 40
    h, E_, pos, neg, _ = loss_ref.sampled_case(D, min(V, 4000), M, 1, 3)
    if V > E_.shape[0]:                                  # (a 10^7-row table: its rows' values do not matter here)
        E_ = np.zeros((V, D), np.float32)
        E_[:4000] = np.random.RandomState(4).standard_normal((4000, D))
    got = run(loss, h, E_, pos, neg, None, "bf16x3", seed=seed, step=step, N=N, want_tg=False, **kw)
    ids = want(step)
    assert np.array_equal(got["samples"], ids)
    assert got["samples"].min() >= 1 and got["samples"].max() <= V - 1
    sup = run(loss, h, E_, pos, neg, ids, "bf16x3", want_tg=False, **{k: v for k, v in kw.items() if k != "cdf"})
    for k in (ROW_KEY[loss], "dh"):
        assert np.array_equal(got[k].view(np.int32), sup[k].view(np.int32)), k
    assert np.array_equal(got["state"][:3].view(np.int32), sup["state"][:3].view(np.int32))     # ([4], [11]: the step words differ)
    if V > 2:
        nxt = run(loss, h, E_, pos, neg, None, "bf16x3", seed=seed, step=step + 1, N=N, want_tg=False, **kw)
        assert not np.array_equal(nxt["samples"], got["samples"])
        assert np.array_equal(nxt["samples"], want(step + 1))
    return h, E_, pos, neg, got


def two_calls_give_the_same_bits(loss, case, rtol=None, atol=None, **kw):
    """rtol, atol: of table_grad's target rows (not "ce": every bit).  Returns the first call's results."""
    h, E_, pos, neg, s = case
    a = run(loss, h, E_, pos, neg, s, "bf16x3", **kw)
    b = run(loss, h, E_, pos, neg, s, "bf16x3", **kw)
    if loss == "ce":                                     # no atomics anywhere: table_grad too
        for k in a:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
        return a
    for k in (ROW_KEY[loss], "dh", "state", "samples"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    keep = np.ones(E_.shape[0], bool)
    keep[pos] = False                                    # target rows take float atomics: rounding order may differ
    assert np.array_equal(a["tg"][keep].view(np.int32), b["tg"][keep].view(np.int32))
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=rtol, atol=atol)
    return a


def table_grad_accumulates_and_untouched_rows_stay(loss, case, atol, **kw):
    """Untouched: the rows that are neither a sample nor a target ("ce": row 0 alone)."""
    h, E_, pos, neg, s = case
    rs = np.random.RandomState(1)
    pre = torch.from_numpy(rs.standard_normal(E_.shape).astype(np.float32)).cuda()
    got = run(loss, h, E_, pos, neg, s, "bf16x3", tg0=pre, **kw)
    base = run(loss, h, E_, pos, neg, s, "bf16x3", **kw)
    pre = pre.cpu().numpy()
    untouched = np.array([0]) if s is None else np.setdiff1d(np.arange(E_.shape[0]), np.concatenate([s, pos[pos != 0]]))
    assert 0 in untouched
    assert np.array_equal(got["tg"][untouched].view(np.int32), pre[untouched].view(np.int32))
    assert np.all(base["tg"][untouched] == 0.0)
    np.testing.assert_allclose(got["tg"], pre + base["tg"], rtol=0, atol=atol)


def state_block_follows_the_head_contract(loss, case, **kw):
    L, _ = ops()
    h, E_, pos, neg, s = case
    st = torch.zeros(L.CR_STATE_FLOATS, dtype=torch.float32, device="cuda")
    st[0], st[1], st[2] = 1.5, 2.0, 3.0
    st[4:5].view(torch.int32)[0] = 7
    got = run(loss, h, E_, pos, neg, s, "bf16x3", state0=st, **kw)
    ref = run(loss, h, E_, pos, neg, s, "bf16x3", **kw)
    g, r = got["state"], ref["state"]
    assert g[0] == np.float32(1.5) + r[0] and g[1] == np.float32(2.0) + r[1] and g[2] == 3.0 + r[2]
    assert np.array_equal(g[8:11], g[0:3])
    assert g[11:12].view(np.int32)[0] == 7 and g[4:5].view(np.int32)[0] == 7
    assert g[12:13].view(np.int32)[0] == 0
    assert r[2] == float((pos != 0).sum())


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def engine_step_matches_oracle(E, model, engine_kw, loss_fn, rel, grad_tol, adam_tol, draw=None, prepare=None):
    """One engine step against the oracle's seq_emb with loss_fn(eng, out, pos, samples) + autograd in fp64, then one Adam step on both
    sides.  draw(seed, step, V, N): the restated draw of a sampled loss (None: "ce", which has no samples and no step word to set);
    prepare(eng, rs) runs on the new engine, before the parameters are drawn.  The loss within rel, every gradient within grad_tol of
    its scale, the large gradients' Adam steps within adam_tol * lr.  Returns the engine."""
    rs = np.random.RandomState(zlib.crc32(model.encode()) % 1000)
    B, T, D, H, itemnum, max_bins = 5, 24, 20, 1, 37, 12
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                 lr=1e-3, seed=7)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.0, max_bins=max_bins, num_context_blocks=1,
                   lr=1e-3)
    eng = E.Engine(model, 9, itemnum, hp, B, training=True, n_slabs=7, **engine_kw)
    if prepare is not None:
        prepare(eng, rs)
    P = fm.init_params(model, 9, itemnum, ohp, seed=3)
    P = {k: v + 0.1 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
    eng.load_params(P)
    P = {k: v.double().cpu() for k, v in eng.get_params().items()}
    seq, pos, neg, time, hours, days = loss_ref.batch(rs, B, T, itemnum, max_bins)
    batch = fm.to_batch(seq, pos, neg, time, hours, days)
    eng.set_batch(seq, pos, neg, time, hours, days)
    if draw is not None:
        eng.set_step(1)
    eng.launch_step(apply=False)
    torch.cuda.synchronize()
    samples = None
    if draw is not None:
        samples = eng.samples.cpu().numpy()
        assert np.array_equal(samples, draw(7, 1, itemnum + 1, engine_kw["ce_negatives"]))
    gates, care = engine_relu_gates(eng, B, T, None)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    with fm.handed_over_gates(gates, care, check=True):
        out = fm.forward(model, leaves, ohp, batch, None)
    loss = loss_fn(eng, out, pos, samples)
    loss.backward()
    G = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    st = eng.state.cpu().numpy()
    n = float((pos != 0).sum())
    assert st[2] == n
    assert st[0] / n == pytest.approx(loss.item(), rel=rel)
    got = eng.grads()
    gmax = max(float(G[k].abs().max()) for k in G)
    for k in G:
        if k.endswith(".bk"):                            # d loss / d bk == 0 identically: rounding noise on both sides
            continue
        ref = G[k].numpy()
        err = float(np.abs(got[k].cpu().double().numpy() - ref).max())
        assert err < grad_tol * max(float(np.abs(ref).max()), 1e-3 * gmax), (k, err, float(np.abs(ref).max()))
    # one Adam step on both sides (the same step word: the same samples)
    eng.Gt.zero_()
    eng.set_step(1)
    eng.launch_step(apply=True)
    torch.cuda.synchronize()
    if draw is not None:
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
            assert float((d_eng - d_orc)[big].abs().max()) <= adam_tol * lr, k
    assert eng.loss_auc()[0] == pytest.approx(loss.item(), rel=rel)
    return eng


def fed_multi_step_path_matches_train_step(E, hyper_kw, engine_kw, make_batch, quantile_bound, max_bound_lr, draw=None,
                                           after_set_step=None):
    """Eight batches of make_batch through enable_feed / train_fed (two graphs of four steps) and through train_step on a second
    engine: the parameters' 0.999 quantile of |difference| below quantile_bound, the largest below max_bound_lr * lr.  draw(seed, step,
    V, N): the restated draw, against every step's samples; after_set_step(eng) runs on both engines once captured.  Returns
    (fed engine, stepped engine, the stepped engine's samples per step, the batches)."""
    B, T, D, itemnum = 16, 20, 32, 300
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=5, **hyper_kw)
    batches = [make_batch(np.random.RandomState(100 + i), B, T, itemnum) for i in range(8)]
    a = E.Engine("sasrec", 10, itemnum, hp, B, training=True, **engine_kw)
    a.capture()
    a.set_step(1)
    if after_set_step is not None:
        after_set_step(a)
    a.enable_feed(n_slots=16, steps_per_graph=4)
    assert a.graph_steps == 4
    ran = 0
    for bt in batches:
        a.feed(*bt)
    while ran < 8:
        ran += a.train_fed()
    torch.cuda.synchronize()
    b = E.Engine("sasrec", 10, itemnum, hp, B, training=True, **engine_kw)
    b.capture()
    b.set_step(1)
    if after_set_step is not None:
        after_set_step(b)
    seen = []
    for bt in batches:
        b.train_step(*bt)
        if draw is not None:
            seen.append(b.samples.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert a.step_number() == b.step_number() == 9
    # each step drew its own samples: those of step k are the draw at step word k
    for k, s in enumerate(seen):
        assert np.array_equal(s, draw(5, k + 1, itemnum + 1, hyper_kw["ce_negatives"])), k
    if draw is not None:
        assert np.array_equal(a.samples.cpu().numpy(), seen[-1])
    pa, pb = a.get_params(), b.get_params()
    # the embedding backward's float atomics differ in order between runs: rounding, then Adam's divide by sqrt(v).  d loss / d bk
    # == 0 identically, so Adam moves bk by +-lr on rounding noise alone (on any two runs): not compared.
    d = np.concatenate([(pa[k] - pb[k]).abs().reshape(-1).cpu().numpy() for k in pa if not k.endswith(".bk")])
    assert np.quantile(d, 0.999) < quantile_bound and d.max() < max_bound_lr * hp.lr, (np.quantile(d, 0.999), d.max())
    assert a.loss_auc()[0] == pytest.approx(b.loss_auc()[0], rel=1e-4)
    return a, b, seen, batches


def main_cli_trains(tmp_path, monkeypatch, caplog, loss_args, params, full_ranking, loss_ceiling):
    """main.py for two epochs on synthetic:tiny with loss_args: params.txt holds params, nothing logged at ERROR, every logged number
    finite, the two training losses in (0, loss_ceiling) (None: positive).  Returns (the log's text, the run's directory)."""
    import main as cli
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    rc = cli.main(["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "cast_1", "--maxlen", "12", "--batch_size", "4",
                   "--hidden_units", "16", "--num_epochs", "2", "--eval_every", "1", "--max_bins", "20"] + loss_args +
                  (["--eval_full_ranking"] if full_ranking else []))
    assert rc == 0
    runs = os.listdir(tmp_path / "saved_models" / "synthetic_tiny")
    d = tmp_path / "saved_models" / "synthetic_tiny" / runs[0]
    got = json.loads((d / "params.txt").read_text())
    assert {k: got[k] for k in params} == params
    assert not [r for r in caplog.records if r.levelno >= logging.ERROR], caplog.text[-2000:]
    train = [float(x) for x in re.findall(r"TRAIN/loss (\S+)", caplog.text)]
    assert len(train) == 2, caplog.text[-2000:]
    vals = train + [float(x) for x in re.findall(r"\d+\.\d+", (d / "log.txt").read_text())]
    if full_ranking:
        full = re.findall(r"full ranking: valid \(NDCG@10: (\S+), HR@10: (\S+)\), test \(NDCG@10: (\S+), HR@10: (\S+)\)", caplog.text)
        assert len(full) == 2, caplog.text[-2000:]
        vals += [float(x) for row in full for x in row]
    assert all(math.isfinite(v) for v in vals), vals
    assert all(0 < v < (loss_ceiling or math.inf) for v in train), train
    return caplog.text, d


def training_learns_a_planted_corpus(E, corpus, steps, make_batch, engine_kw, loss_ceiling, hr_floor, prepare=None):
    """steps steps of sasrec on make_batch's corpus (corpus: B, T, D, itemnum, lr): the loss ends below loss_ceiling (a number, or a
    function of the engine) and the full-ranking HR@10 of the next item after each test sequence's last one (chance: 10 / itemnum)
    above hr_floor.  prepare(eng) runs before the capture.  Returns the engine."""
    rs = np.random.RandomState(0)
    B, T, D, itemnum = corpus["B"], corpus["T"], corpus["D"], corpus["itemnum"]
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.1, lr=corpus["lr"], seed=3)
    eng = E.Engine("sasrec", 10, itemnum, hp, B, training=True, **engine_kw)
    if prepare is not None:
        prepare(eng)
    eng.capture()
    eng.set_step(1)
    for _ in range(steps):
        eng.train_step(*make_batch(rs, B, T, itemnum))
    torch.cuda.synchronize()
    loss, _ = eng.loss_auc()
    ev = E.Engine("sasrec", 10, itemnum, hp, B, training=False, share=eng)
    seq, pos, _ = make_batch(np.random.RandomState(99), B, T, itemnum)
    ev.forward_eval(seq)
    ids, _, rank = ev.topk(10, targets=pos[:, -1])
    torch.cuda.synchronize()
    hr = float((rank.cpu().numpy() < 10).mean())
    print("planted corpus after %d steps: loss %.4f, HR@10 %.3f" % (steps, loss, hr))
    assert loss < (loss_ceiling(eng) if callable(loss_ceiling) else loss_ceiling), loss
    assert hr > hr_floor, hr
    return eng

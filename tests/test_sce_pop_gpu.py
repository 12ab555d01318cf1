"""The popularity proposal of the sampled softmax on the GPU: cr_sampled_ce with logq against fp64 on the corrected logits (supplied
samples, per-element bounds as test_sce_gpu.py), a constant proposal against the uniform path, the device draw through the cdf against
its numpy restatement, determinism, padding and all-hits rows; Engine(ce_proposal="popularity") against the oracle with the corrected
loss + autograd in fp64, its refusals and launch list, graph capture with a change of weights, the fed multi-step path, the CLI and
the skewed planted corpus."""
import math
import zlib

import numpy as np
import pytest
import torch

import loss_harness as H
import loss_ref
import sce_pop_ref as R
from loss_ref import sampled_case as _case
from loss_ref import sampled_softmax_ref64 as _ref64
from model_harness import E  # noqa: F401  (the engine module, a fixture)

pytestmark = pytest.mark.gpu

_PROPOSALS = {}


def _proposal(V):
    """The Zipf proposal of a table size, from the library's builder (built once per size)."""
    if V not in _PROPOSALS:
        from castrec_amd.proposal import build_proposal
        _PROPOSALS[V] = build_proposal(R.zipf_weights(V, 1.0), V)
    return _PROPOSALS[V]


def _run(h, E_, pos, neg, samples, prec, **kw):
    return H.run("sampled_ce", h, E_, pos, neg, samples, prec, **kw)


def _check(got, ref):
    return loss_ref.check(got, ref, 4.0, "lse")


CASES = [(D, N, V) for D in (8, 50, 64, 128, 256) for N in (1, 7, 256, 2048) for V in (17, 3417, 100003)]


@pytest.mark.parametrize("D,N,V", CASES)
def test_corrected_sampled_ce_against_fp64(D, N, V):
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"scepop%d_%d_%d" % (D, N, V)))
    _, logq = _proposal(V)
    got = _run(h, E_, pos, neg, s, "bf16x3", logq=logq)          # (supplied samples: the cdf is not needed)
    ref = _ref64(h, E_, pos, neg, s, logq)
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
    h, E_, pos, neg, s = _case(D, V, 151, N, 11 + D + N)
    _, logq = _proposal(V)
    _check(_run(h, E_, pos, neg, s, "bf16", logq=logq), _ref64(h, E_, pos, neg, s, logq, bf16=True))


@pytest.mark.parametrize("V,D,N", [(17, 50, 40), (4097, 64, 256)])
def test_constant_proposal_agrees_with_the_uniform_path(V, D, N):
    """Equal weights over V - 1 = 2^k items: log Q is one constant exactly, so the corrected softmax is the uniform one -- loss and
    gradients agree within the sum of the two paths' bounds, lse_out differs by log(V - 1) on target rows.  (A bias on the candidates
    but not on the target, or of the wrong sign, shifts the loss by log(V - 1) per row instead.)"""
    from castrec_amd.proposal import build_proposal
    M = 203
    h, E_, pos, neg, s = _case(D, V, M, N, 77 + V)
    cdf, logq = build_proposal(np.ones(V), V)
    assert np.all(logq[1:] == logq[1]) and logq[1] == np.float32(-math.log(V - 1))
    a = _run(h, E_, pos, neg, s, "bf16x3", logq=logq)
    b = _run(h, E_, pos, neg, s, "bf16x3")
    ra, rb = _ref64(h, E_, pos, neg, s, logq), _ref64(h, E_, pos, neg, s)
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
    cdf, logq = _proposal(V)
    h, E_, pos, neg, got = H.device_draw_matches("sampled_ce", seed, step, V, N, lambda step: R.draw(seed, step, cdf, N), cdf=cdf,
                                                 logq=logq)
    again = _run(h, E_, pos, neg, None, "bf16x3", cdf=cdf, logq=logq, seed=seed, step=step, N=N, want_tg=False)
    assert np.array_equal(again["samples"], got["samples"])


@pytest.mark.parametrize("D,V,M,N", [(50, 3417, 1300, 256), (128, 100003, 200, 2048), (8, 17, 77, 300)])
def test_two_calls_give_the_same_bits(D, V, M, N):
    h, E_, pos, neg, _ = _case(D, V, M, N, 3)
    cdf, logq = _proposal(V)
    a = H.two_calls_give_the_same_bits("sampled_ce", (h, E_, pos, neg, None), rtol=1e-5, atol=1e-6, cdf=cdf, logq=logq, seed=9, step=4,
                                       N=N)
    _check(a, _ref64(h, E_, pos, neg, a["samples"], logq))


def test_padding_rows_and_all_hits_rows():
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
    got = _run(h, E_, pos, neg, np.full(8, 7, np.int32), "bf16x3", logq=logq)
    assert got["state"][0] == 0.0 and got["state"][2] == float((pos != 0).sum())
    assert np.all(got["dh"] == 0.0) and np.all(got["tg"] == 0.0)
    # padding rows contribute nothing: the same call with them removed has the same loss and gradients
    s = np.array([3, 9, 9, 7, 20], np.int32)
    pos2 = pos.copy(); pos2[1::5] = 9
    live = pos2 != 0
    a = _run(h, E_, pos2, neg, s, "bf16x3", logq=logq)
    b = _run(h[live], E_, pos2[live], neg[live], s, "bf16x3", logq=logq)
    assert np.all(a["dh"][~live] == 0.0) and np.all(a["tg"][0] == 0.0)
    np.testing.assert_allclose(a["dh"][live], b["dh"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=1e-5, atol=1e-6)
    assert a["state"][0] == pytest.approx(b["state"][0], rel=1e-6) and a["state"][2] == b["state"][2]
    _check(a, _ref64(h, E_, pos2, neg, s, logq))
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
    built = {}

    def set_weights(eng, rs):
        w = np.concatenate([[0.0], (rs.randint(0, 50, eng.itemnum) + 1.0) ** 0.75])
        eng.set_item_weights(w)
        cdf, logq = built["cdf"], built["logq"] = R.build(w)
        assert np.array_equal(eng.item_cdf.cpu().numpy().view(np.uint32), cdf)
        assert np.array_equal(eng.item_logq.cpu().numpy().view(np.int32), logq.view(np.int32))

    eng = H.engine_step_matches_oracle(E, model, dict(loss="sampled_ce", ce_negatives=16, ce_proposal="popularity"),
                                       lambda eng, out, pos, samples: _loss(out, pos, samples, built["logq"]), rel=2e-5, grad_tol=2e-3,
                                       adam_tol=0.02, draw=lambda seed, step, V, N: R.draw(seed, step, built["cdf"], N),
                                       prepare=set_weights)
    assert eng.loss == "sampled_ce" and eng.ce_proposal == "popularity" and not eng.use_index and not eng.bitwise_reproducible


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
    itemnum = 300
    w1 = R.zipf_weights(itemnum + 1, 1.0)
    w2 = w1[::-1].copy()
    cdf1, _ = R.build(w1)
    cdf2, _ = R.build(w2)
    a, b, _, batches = H.fed_multi_step_path_matches_train_step(
        E, dict(loss="sampled_ce", ce_negatives=64, ce_proposal="popularity"), {}, _planted_batch, quantile_bound=1e-5, max_bound_lr=8,
        draw=lambda seed, step, V, N: R.draw(seed, step, cdf1, N), after_set_step=lambda eng: eng.set_item_weights(w1))
    assert a.loss == "sampled_ce" and a.ce_proposal == "popularity"
    # new weights behind a captured graph: the next step draws from the new cdf
    b.set_item_weights(w2)
    b.train_step(*batches[0])
    torch.cuda.synchronize()
    got = b.samples.cpu().numpy()
    assert np.array_equal(got, R.draw(5, 9, cdf2, 64)) and not np.array_equal(got, R.draw(5, 9, cdf1, 64))
    assert math.isfinite(b.loss_auc()[0])


def test_main_cli_trains_with_the_popularity_proposal(tmp_path, monkeypatch, caplog):
    import re
    text, _ = H.main_cli_trains(tmp_path, monkeypatch, caplog, ["--loss", "sampled_ce", "--ce_negatives", "16", "--ce_proposal",
                                                                "popularity", "--ce_pop_power", "0.75"],
                                dict(loss="sampled_ce", ce_proposal="popularity", ce_pop_power=0.75), full_ranking=False,
                                loss_ceiling=None)
    eff = re.findall(r"popularity proposal: power (\S+), effective number of items (\S+) of (\d+)", text)
    assert len(eff) == 1 and float(eff[0][0]) == 0.75 and 1.0 <= float(eff[0][1]) <= float(eff[0][2]), text[-2000:]


def test_popularity_training_learns_the_skewed_planted_corpus(E):
    c = R.PLANTED
    H.training_learns_a_planted_corpus(E, c, c["steps"], R.planted_skewed,
                                       dict(loss="sampled_ce", ce_negatives=c["N"], ce_proposal="popularity"),
                                       loss_ceiling=R.PLANTED_LOSS, hr_floor=R.PLANTED_HR,
                                       prepare=lambda eng: eng.set_item_weights(R.planted_counts() + 1.0))

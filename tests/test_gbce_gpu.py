"""gBCE on the GPU: cr_gbce against fp64 with caller-supplied samples (every element of loss_out, d_seq_emb and table_grad inside 4x the
per-element bound of gbce_ref, which a numpy emulation of the device arithmetic meets at 1x in test_gbce_host.py), rows whose every
sample is a hit, padding, accumulation, the state block, pitch, determinism and the device draw; Engine(loss="gbce") against the
oracle's seq_emb with the gBCE loss + autograd in fp64, the fed multi-step path, the launch list, the refusals, the CLI and the
planted corpus."""
import math
import zlib

import numpy as np
import pytest
import torch

import gbce_ref
import loss_harness as H
import loss_ref
from loss_ref import planted as _planted
from loss_ref import sampled_case as _case
from model_harness import E  # noqa: F401  (the engine module, a fixture)

pytestmark = pytest.mark.gpu


def _run(h, E_, pos, neg, samples, prec, **kw):
    return H.run("gbce", h, E_, pos, neg, samples, prec, **kw)


def _check(got, ref):
    return loss_ref.check(got, ref, 4.0, "l")


CASES = [(D, N, V) for D in (8, 20, 50, 64, 128, 256) for N in (1, 7, 256, 2048) for V in (17, 3417, 100003)]


@pytest.mark.parametrize("D,N,V", CASES)
def test_gbce_against_fp64(D, N, V):
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"gbce%d_%d_%d" % (D, N, V)))
    betas = (1.0, 0.25) + ((1e-3,) if (D, N, V) == (50, 256, 3417) else ())
    for b in betas:
        got = _run(h, E_, pos, neg, s, "bf16x3", beta=b)
        ref = gbce_ref.ref64(h, E_, pos, neg, s, b)
        print("D %d N %d V %d beta %g: worst dE ratio %.3f of 4" % (D, N, V, b, 4 * _check(got, ref)))
        assert np.all(got["dh"][pos == 0] == 0.0) and np.all(got["l"][pos == 0] == 0.0)
        assert np.array_equal(got["samples"], s)
        assert np.all(got["tg"][0] == 0.0)
        sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
        auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
        assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6


@pytest.mark.parametrize("D,N,V", [(20, 256, 17), (50, 256, 3417), (128, 2048, 100003), (256, 7, 3417)])
def test_plain_bf16_bound(D, N, V):
    h, E_, pos, neg, s = _case(D, V, 151, N, 11 + D + N)
    for b in (1.0, 0.25):
        _check(_run(h, E_, pos, neg, s, "bf16", beta=b), gbce_ref.ref64(h, E_, pos, neg, s, b, bf16=True))


def test_pitch_many_rows_and_many_samples():
    """ld > D with NaN in the padding columns, more rows than one part of the sample sweep, N above the part budget's knee."""
    h, E_, pos, neg, s = _case(50, 3417, 1237, 4100, 5)
    _check(_run(h, E_, pos, neg, s, "bf16x3", beta=0.3, ld=67), gbce_ref.ref64(h, E_, pos, neg, s, 0.3))


def test_all_hit_rows_duplicates_and_padding():
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
    got = _run(h, E_, pos, neg, np.full(8, 7, np.int32), "bf16x3", beta=b)
    ref = gbce_ref.ref64(h, E_, pos, neg, np.full(8, 7, np.int32), b)
    _check(got, ref)
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
    a = _run(h, E_, pos2, neg, s, "bf16x3", beta=b)
    c = _run(h[live], E_, pos2[live], neg[live], s, "bf16x3", beta=b)
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
    _check(a, ref2)
    assert np.all(np.abs(a["tg"][9] - (2 * single + tgt9)) <= 4.0 * ref2["e_dE"][9])     # (the row's own bound: its terms cancel)
    untouched = np.setdiff1d(np.arange(V), np.concatenate([s, pos2]))
    assert np.all(a["tg"][untouched] == 0.0) and np.all(a["tg"][0] == 0.0)


@pytest.mark.parametrize("seed,step,V,N", [(42, 1, 3417, 256), (7, 123456, 17, 300), (0, 2 ** 31 + 5, 10 ** 7, 4096),
                                           (0xDEADBEEF, 9, 2, 7)])
def test_device_draw_matches_the_numpy_restatement(seed, step, V, N):
    h, E_, pos, neg, got = H.device_draw_matches("gbce", seed, step, V, N, lambda step: gbce_ref.draw(seed, step, V, N), beta=0.5)
    if V > 2:
        # not the sampled softmax's negatives at the same seed and step
        sce = H.run("sampled_ce", h, E_, pos, neg, None, "bf16x3", seed=seed, step=step, N=N, want_tg=False)
        assert np.array_equal(sce["samples"], loss_ref.draw(seed, step, V, N, loss_ref.SCE_SITE))
        assert not np.array_equal(sce["samples"], got["samples"])


@pytest.mark.parametrize("D,V,M,N", [(50, 3417, 1300, 256), (128, 100003, 200, 2048), (8, 17, 77, 300)])
def test_two_calls_give_the_same_bits(D, V, M, N):
    H.two_calls_give_the_same_bits("gbce", _case(D, V, M, N, 3), rtol=1e-5, atol=1e-6, beta=0.25)


def test_table_grad_accumulates_and_untouched_rows_stay():
    # rows of samples: one += of the same sum, the same bits; target rows: a few atomic adds onto another start, an ulp of ~10 each
    H.table_grad_accumulates_and_untouched_rows_stay("gbce", _case(64, 3417, 300, 256, 9), atol=1e-5, beta=0.25)


def test_state_block_follows_the_head_contract():
    H.state_block_follows_the_head_contract("gbce", _case(50, 500, 400, 64, 4), beta=0.25)


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
    eng = H.engine_step_matches_oracle(E, model, dict(loss="gbce", ce_negatives=16),
                                       lambda eng, out, pos, samples: _gbce_loss(out, pos, samples, eng.gbce_beta), rel=2e-5,
                                       grad_tol=2e-3, adam_tol=0.02, draw=gbce_ref.draw)
    B, itemnum, hp = 5, 37, eng.hp
    assert eng.loss == "gbce" and not eng.use_index and not eng.bitwise_reproducible and eng.ce_negatives == 16
    assert eng.gbce_t == 0.75 and eng.gbce_beta == pytest.approx(gbce_ref.beta(16, itemnum, 0.75), rel=1e-12)
    assert E.Engine(model, 9, itemnum, hp, B, training=True, loss="gbce", ce_negatives=16, gbce_t=0.0).gbce_beta == 1.0
    assert E.Engine(model, 9, itemnum, hp, B, training=True, loss="gbce", ce_negatives=16, gbce_t=1.0).gbce_beta == \
        pytest.approx(16 / 36, rel=1e-12)


def test_fed_multi_step_path_matches_train_step(E):
    a, _, seen, _ = H.fed_multi_step_path_matches_train_step(E, dict(loss="gbce", ce_negatives=64, gbce_t=0.5), {}, _planted,
                                                             quantile_bound=1e-5, max_bound_lr=8, draw=gbce_ref.draw)
    assert a.loss == "gbce" and a.ce_negatives == 64 and a.gbce_beta == pytest.approx(gbce_ref.beta(64, 300, 0.5))
    assert len({s.tobytes() for s in seen}) == 8


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
    H.main_cli_trains(tmp_path, monkeypatch, caplog, ["--loss", "gbce", "--ce_negatives", "16", "--gbce_t", "0.5"],
                      dict(loss="gbce", ce_negatives=16, gbce_t=0.5), full_ranking=True,
                      loss_ceiling=3 * 17 * math.log(2))       # (17 binary terms per row at most, log 2 each at z = 0)


def test_gbce_training_learns_a_planted_corpus(E):
    """The structure and thresholds of test_sampled_ce_training_learns_a_planted_corpus, on gbce_ref.PLANTED_STEPS steps: gBCE first
    settles on the constant-score plateau (loss 2.28 here, ranking at chance) and the fp64 reference of this very objective leaves it
    between steps 450 and 600, so the softmax's 250 steps measure the plateau, not the implementation (250 steps on the GPU: loss
    below the threshold, HR@10 0.078; the reference at 250 steps: loss 2.29, HR@10 0.11).  test_gbce_host.py runs the reference on this
    schedule against the same thresholds."""
    c = gbce_ref.PLANTED
    # half of the loss of an untrained model (every score 0: beta log 2 for the target, log 2 per negative)
    eng = H.training_learns_a_planted_corpus(E, c, gbce_ref.PLANTED_STEPS, _planted, dict(loss="gbce", ce_negatives=c["N"]),
                                             loss_ceiling=lambda eng: 0.5 * (eng.gbce_beta + 64) * math.log(2), hr_floor=0.5)
    assert eng.gbce_t == c["t"]

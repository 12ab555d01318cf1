"""Sampled softmax cross-entropy on the GPU: cr_sampled_ce against fp64 with caller-supplied samples (per-element bounds built from
the fp64 absolute products, as test_ce_gpu.py), accidental hits and duplicates, the device draw against its numpy restatement,
determinism, accumulation and the state block; Engine(loss="sampled_ce") against the oracle's seq_emb with the sampled loss + autograd
in fp64, the fed multi-step path, the unchanged existing engines, the refusals, the CLI and the planted corpus."""
import math
import zlib

import numpy as np
import pytest
import torch

import loss_harness as H
import loss_ref
from loss_ref import SCE_SITE
from loss_ref import planted as _planted
from loss_ref import sampled_case as _case
from loss_ref import sampled_softmax_ref64 as _ref64
from model_harness import E  # noqa: F401  (the engine module, a fixture)

pytestmark = pytest.mark.gpu


def _run(h, E_, pos, neg, samples, prec, **kw):
    return H.run("sampled_ce", h, E_, pos, neg, samples, prec, **kw)


def _check(got, ref):
    return loss_ref.check(got, ref, 4.0, "lse")


def _draw(seed, step, V, N):
    return loss_ref.draw(seed, step, V, N, SCE_SITE)


CASES = [(D, N, V) for D in (8, 20, 50, 64, 128, 256) for N in (1, 7, 256, 2048) for V in (17, 3417, 100003)]


@pytest.mark.parametrize("D,N,V", CASES)
def test_sampled_ce_against_fp64(D, N, V):
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"sce%d_%d_%d" % (D, N, V)))
    got = _run(h, E_, pos, neg, s, "bf16x3")
    ref = _ref64(h, E_, pos, neg, s)
    _check(got, ref)
    assert np.all(got["dh"][pos == 0] == 0.0)
    assert np.array_equal(got["samples"], s)
    assert np.all(got["tg"][0] == 0.0)
    sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
    auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
    assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6


@pytest.mark.parametrize("D,N,V", [(20, 256, 17), (50, 256, 3417), (128, 2048, 100003), (256, 7, 3417)])
def test_plain_bf16_bound(D, N, V):
    h, E_, pos, neg, s = _case(D, V, 151, N, 11 + D + N)
    _check(_run(h, E_, pos, neg, s, "bf16"), _ref64(h, E_, pos, neg, s, bf16=True))


def test_pitch_many_rows_and_many_samples():
    """ld > D, more rows than one part of the sample sweep, N above the part budget's knee."""
    h, E_, pos, neg, s = _case(50, 3417, 1237, 4100, 5)
    _check(_run(h, E_, pos, neg, s, "bf16x3", ld=67), _ref64(h, E_, pos, neg, s))


def test_accidental_hits_duplicates_and_padding():
    D, V, M = 32, 50, 96
    rs = np.random.RandomState(2)
    h = rs.standard_normal((M, D)).astype(np.float32) * 0.3
    E_ = rs.standard_normal((V, D)).astype(np.float32)
    # every sample is the target of every live row: loss 0, zero gradients, nothing touched
    pos = np.full(M, 7, np.int32)
    pos[::3] = 0
    neg = np.zeros(M, np.int32)
    got = _run(h, E_, pos, neg, np.full(8, 7, np.int32), "bf16x3")
    assert got["state"][0] == 0.0 and got["state"][2] == float((pos != 0).sum())
    assert np.all(got["dh"] == 0.0) and np.all(got["tg"] == 0.0)
    # padding rows contribute nothing: the same call with them removed has the same loss and gradients
    s = np.array([3, 9, 9, 7, 20], np.int32)
    pos2 = pos.copy(); pos2[1::5] = 9
    live = pos2 != 0
    a = _run(h, E_, pos2, neg, s, "bf16x3")
    b = _run(h[live], E_, pos2[live], neg[live], s, "bf16x3")
    assert np.all(a["dh"][~live] == 0.0)
    np.testing.assert_allclose(a["dh"][live], b["dh"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["tg"], b["tg"], rtol=1e-5, atol=1e-6)
    assert a["state"][0] == pytest.approx(b["state"][0], rel=1e-6) and a["state"][2] == b["state"][2]
    # a duplicated id: its row of table_grad is twice one copy's contribution (rows that target it excluded: they drop both)
    ref = _ref64(h, E_, pos2, neg, s)
    P1 = np.exp((h.astype(np.float64) @ E_[9].astype(np.float64)) - ref["lse"]) * ((pos2 != 0) & (pos2 != 9))
    single = P1 @ h.astype(np.float64)
    tgt9 = ((pos2 == 9)[:, None] * (np.exp(ref["sp"] - ref["lse"]) - 1.0)[:, None] * h).sum(0)
    np.testing.assert_allclose(a["tg"][9], 2 * single + tgt9, rtol=1e-4, atol=1e-5)
    untouched = np.setdiff1d(np.arange(V), np.concatenate([s, pos2]))
    assert np.all(a["tg"][untouched] == 0.0)


@pytest.mark.parametrize("seed,step,V,N", [(42, 1, 3417, 256), (7, 123456, 17, 300), (0, 2 ** 31 + 5, 10 ** 7, 4096),
                                           (0xDEADBEEF, 9, 2, 7)])
def test_device_draw_matches_the_numpy_restatement(seed, step, V, N):
    H.device_draw_matches("sampled_ce", seed, step, V, N, lambda step: _draw(seed, step, V, N))


@pytest.mark.parametrize("D,V,M,N", [(50, 3417, 1300, 256), (128, 100003, 200, 2048), (8, 17, 77, 300)])
def test_two_calls_give_the_same_bits(D, V, M, N):
    H.two_calls_give_the_same_bits("sampled_ce", _case(D, V, M, N, 3), rtol=1e-5, atol=1e-6)


def test_table_grad_accumulates_and_untouched_rows_stay():
    H.table_grad_accumulates_and_untouched_rows_stay("sampled_ce", _case(64, 3417, 300, 256, 9), atol=1e-6)


def test_state_block_follows_the_head_contract():
    H.state_block_follows_the_head_contract("sampled_ce", _case(50, 500, 400, 64, 4))


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _sce_loss(out, pos, samples):
    """The sampled loss on the oracle's seq_emb and item table, in fp64 (loss / n_target, as Adam sees it)."""
    se, tab = out["seq_emb"], out["item_table"]
    p = torch.as_tensor(np.asarray(pos).reshape(-1), dtype=torch.long)
    s = torch.as_tensor(np.asarray(samples), dtype=torch.long)
    S = se @ tab[s].t()
    st = (se * tab[p]).sum(1)
    S = S.masked_fill(s[None, :] == p[:, None], float("-inf"))
    lse = torch.logsumexp(torch.cat([st[:, None], S], 1), 1)
    ist = p != 0
    return ((lse - st) * ist).sum() / ist.sum()


@pytest.mark.parametrize("model", ["sasrec", "cast_1", "cast_5", "cast_9"])
def test_engine_sampled_ce_step_matches_oracle(E, model):
    eng = H.engine_step_matches_oracle(E, model, dict(loss="sampled_ce", ce_negatives=16),
                                       lambda eng, out, pos, samples: _sce_loss(out, pos, samples), rel=2e-5, grad_tol=2e-3,
                                       adam_tol=0.02, draw=_draw)
    assert eng.loss == "sampled_ce" and not eng.use_index and not eng.bitwise_reproducible and eng.ce_negatives == 16


def test_fed_multi_step_path_matches_train_step(E):
    a, _, seen, _ = H.fed_multi_step_path_matches_train_step(E, dict(loss="sampled_ce", ce_negatives=64), {}, _planted,
                                                             quantile_bound=1e-5, max_bound_lr=8, draw=_draw)
    assert a.loss == "sampled_ce" and a.ce_negatives == 64
    assert len({s.tobytes() for s in seen}) == 8


def test_existing_engines_unchanged_and_refusals(E):
    hp = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1)
    assert hp.loss == "bce" and hp.ce_negatives == 256
    names = lambda e: [x[0] for x in e.fwd + e.bwd]
    a = E.Engine("cast_1", 10, 500, hp, 64, training=True)
    b = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="bce", ce_negatives=17)
    assert a.loss == "bce" and a.use_index and a.bitwise_reproducible
    assert names(a) == names(b) and a.n_kernel_launches() == b.n_kernel_launches()
    assert "cr_sampled_ce" not in names(a)
    c = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="ce")
    c2 = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="ce", ce_negatives=17)
    assert names(c) == names(c2) and "cr_softmax_ce" in names(c) and "cr_sampled_ce" not in names(c)
    s = E.Engine("cast_1", 10, 500, hp, 64, training=True, loss="sampled_ce")
    ns = names(s)
    assert ns.count("cr_sampled_ce") == 1 and "cr_softmax_ce" not in ns
    assert not any(n.startswith("cr_head") or n == "cr_stack_fwd_head" for n in ns)
    assert [n if n != "cr_sampled_ce" else "cr_softmax_ce" for n in ns] == names(c)     # the route of "ce"
    assert s.ce_negatives == 256 and tuple(s.samples.shape) == (256,) and not s.use_index and not s.bitwise_reproducible
    hp_s = E.Hyper(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, seed=1, loss="sampled_ce", ce_negatives=32)
    assert E.Engine("cast_1", 10, 500, hp_s, 8, training=True).ce_negatives == 32
    assert E.Engine("cast_1", 10, 500, hp_s, 8, training=True, ce_negatives=8).ce_negatives == 8
    assert E.Engine("cast_1", 10, 500, hp_s, 8, training=False).loss == "bce"      # eval engines ignore it
    # refusals
    hp = E.Hyper(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, seed=1)
    with pytest.raises(ValueError, match="lazy_adam"):
        E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="sampled_ce", lazy_adam=True)
    with pytest.raises(ValueError, match="data parallelism"):
        E.Engine("sasrec", 10, 100, hp, 4, training=True, loss="sampled_ce", batch_global=8, row_offset=80)
    with pytest.raises(ValueError, match="hidden_units"):
        E.Engine("sasrec", 10, 100, E.Hyper(maxlen=20, hidden_units=4, num_blocks=1, num_heads=1, seed=1), 8, training=True,
                 loss="sampled_ce")
    for n in (0, -1, 16385):
        with pytest.raises(ValueError, match="ce_negatives"):
            E.Engine("sasrec", 10, 100, hp, 8, training=True, loss="sampled_ce", ce_negatives=n)
    from castrec_amd.models import build_model
    import types
    args = types.SimpleNamespace(maxlen=20, hidden_units=16, num_blocks=1, num_heads=1, dropout_rate=0.0, l2_emb=0.0, lr=1e-3,
                                 max_bins=20, num_context_blocks=1, seed=1, loss="sampled_ce", ce_negatives=16)
    m = build_model("sasrec", 10, 100, 0, args)
    with pytest.raises(ValueError, match="data parallelism"):
        m.data_parallel(0, 2)


def test_main_cli_trains_with_sampled_ce_and_logs_finite_numbers(tmp_path, monkeypatch, caplog):
    H.main_cli_trains(tmp_path, monkeypatch, caplog, ["--loss", "sampled_ce", "--ce_negatives", "16"],
                      dict(loss="sampled_ce", ce_negatives=16), full_ranking=True,
                      loss_ceiling=3 * math.log(17))                       # (17 candidates per row at most)


def test_sampled_ce_training_learns_a_planted_corpus(E):
    H.training_learns_a_planted_corpus(E, dict(B=64, T=20, D=32, itemnum=400, lr=5e-3), 250, _planted,
                                       dict(loss="sampled_ce", ce_negatives=64), loss_ceiling=0.5 * math.log(65), hr_floor=0.5)

"""Full-catalogue softmax cross-entropy on the GPU: cr_softmax_ce against fp64 (per-element bounds built from the fp64 absolute
products), accumulation, determinism and the state block; Engine(loss="ce") against the oracle's seq_emb with CE + autograd in fp64,
the fed multi-step path, the unchanged default, the refusals, the CLI and a planted corpus that CE training has to learn."""
import math
import zlib

import numpy as np
import pytest
import torch

import loss_harness as H
import loss_ref
from loss_ref import ce_case as _case
from loss_ref import planted as _planted
from loss_ref import softmax_ref64 as _ref64
from model_harness import E  # noqa: F401  (the engine module, a fixture)

pytestmark = pytest.mark.gpu


def _run(h, E_, pos, neg, prec, **kw):
    return H.run("ce", h, E_, pos, neg, None, prec, **kw)


def _check(got, ref):
    return loss_ref.check(got, ref, 4.0, "lse", full_catalogue=True)
CASES = [(D, V) for D in (8, 20, 50, 64, 128, 256) for V in (2, 17, 3417, 100003)]


@pytest.mark.parametrize("D,V", CASES)
def test_softmax_ce_against_fp64(D, V):
    M = 61 if V > 10000 else 203
    h, E_, pos, neg = _case(D, V, M, zlib.crc32(b"ce%d_%d" % (D, V)))
    got = _run(h, E_, pos, neg, "bf16x3")
    ref = _ref64(h, E_, pos, neg)
    _check(got, ref)
    assert np.all(got["dh"][pos == 0] == 0.0)
    # the AUC of the sampled negatives (ties are measure-zero here; a near-tie may round either way)
    sure = ref["ist"] & (np.abs(ref["sp"] - ref["sn"]) > 1e-3)
    auc_ref = float(((np.sign(ref["sp"] - ref["sn"]) + 1) / 2)[ref["ist"]].sum())
    assert abs(got["state"][1] - auc_ref) <= float((ref["ist"] & ~sure).sum()) + 1e-6


@pytest.mark.parametrize("D,V", [(20, 17), (50, 3417), (128, 100003)])
def test_plain_bf16_bound(D, V):
    M = 61 if V > 10000 else 203
    h, E_, pos, neg = _case(D, V, M, 11 + D)
    _check(_run(h, E_, pos, neg, "bf16"), _ref64(h, E_, pos, neg, bf16=True))


def test_pitch_and_many_rows():
    """ld > D (an engine's seq_emb column block), more rows than one part of the item sweep, a row count off every tile size."""
    h, E_, pos, neg = _case(50, 3417, 1237, 5)
    _check(_run(h, E_, pos, neg, "bf16x3", ld=67), _ref64(h, E_, pos, neg))


def test_table_grad_accumulates_and_row_zero_is_untouched():
    H.table_grad_accumulates_and_untouched_rows_stay("ce", _case(64, 3417, 300, 9) + (None,), atol=1e-6)


@pytest.mark.parametrize("D,V,M", [(50, 3417, 1300), (128, 100003, 200), (8, 17, 77)])
def test_two_calls_give_the_same_bits(D, V, M):
    H.two_calls_give_the_same_bits("ce", _case(D, V, M, 3) + (None,))


def test_state_block_follows_the_head_contract():
    H.state_block_follows_the_head_contract("ce", _case(50, 500, 400, 4) + (None,))


# ---- the engine ----------------------------------------------------------------------------------------------------------------
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
    eng = H.engine_step_matches_oracle(E, model, dict(loss="ce"), lambda eng, out, pos, samples: _ce_loss(out, pos), rel=2e-5,
                                       grad_tol=2e-3, adam_tol=0.02)
    assert eng.loss == "ce" and not eng.use_index and not eng.bitwise_reproducible


def test_fed_multi_step_path_matches_train_step(E):
    H.fed_multi_step_path_matches_train_step(E, {}, dict(loss="ce"), _planted, quantile_bound=1e-5, max_bound_lr=8)


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
    H.main_cli_trains(tmp_path, monkeypatch, caplog, ["--loss", "ce"], dict(loss="ce"), full_ranking=True,
                      loss_ceiling=3 * math.log(41))                       # (synthetic:tiny: 40 items)


def test_ce_training_learns_a_planted_corpus(E):
    H.training_learns_a_planted_corpus(E, dict(B=64, T=20, D=32, itemnum=400, lr=5e-3), 250, _planted, dict(loss="ce"),
                                       loss_ceiling=0.3 * math.log(400), hr_floor=0.5)

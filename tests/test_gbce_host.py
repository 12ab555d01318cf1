"""gBCE, host side (no GPU): cr_gbce's argument checks and workspace query, the ctypes mirror of cr_gbce_desc, the --loss gbce /
--gbce_t options, the numpy restatements of the device draw and of beta, and the error bound of the GPU test itself: a numpy
emulation of the device arithmetic stays within 1x the bounds the GPU gets 4x of (gbce_ref)."""
import functools
import math
import zlib

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

import gbce_ref
import loss_host
import loss_ref


def _check(got, ref):
    return loss_ref.check(got, ref, 1.0, "l")


_valid_desc = functools.partial(loss_host.valid_desc, "gbce")
_rejects = functools.partial(loss_host.rejects, "gbce")


def test_gbce_validates_before_any_hip_call():
    loss_host.refuses_the_common_arguments("gbce")
    for b in (0.0, -0.5, 1.0 + 2.0 ** -20, 2.0, float("nan"), float("inf")):
        d = _valid_desc(); d.beta = b
        _rejects(d, "beta")
    d = _valid_desc(); d.step = None                         # the device draw needs the step word
    _rejects(d, "step")
    d = _valid_desc()                                       # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_gbce_workspace(40, 16, 50) - 1
    _rejects(d, "workspace")
    d = _valid_desc(); d.step, d.samples = None, 16         # caller-supplied samples: no step needed (fails on the workspace only)
    _rejects(d, "workspace")
    for b in (1.0, 1e-3):                                   # both ends of beta's range pass (fail on the workspace only)
        d = _valid_desc(); d.beta = b
        _rejects(d, "workspace")


def test_workspace_query_is_monotone_and_rejects_unsupported_shapes():
    ws = L.lib.cr_gbce_workspace
    loss_host.sampled_workspace_query_is_monotone(ws)
    # no lse2 array, so never above the sampled softmax's
    assert ws(128 * 512, 4096, 256) <= L.lib.cr_sampled_ce_workspace(128 * 512, 4096, 256)


def test_gbce_desc_mirror_matches_c_layout(tmp_path):
    loss_host.desc_mirror_matches_c_layout(tmp_path, "gbce", ("CR_GBCE_SITE",))
    assert L.CR_GBCE_SITE == gbce_ref.CR_GBCE_SITE == 0x6BCE0000 and L.CR_GBCE_SITE != L.CR_SCE_SITE and L.CR_GBCE_SITE >> 24
    assert "cr_gbce" in L.EXPORTS and "cr_gbce_workspace" in L.EXPORTS


def test_cli_takes_gbce_and_gbce_t():
    import main as cli
    from castrec_amd.engine import ALL_LOSSES, LOSSES, Hyper
    base = ["--dataset", "x", "--train_dir", "t", "--model", "cast_1"]
    args = cli.parse_args(base)
    assert args.loss == "bce" and args.ce_negatives == 256 and args.gbce_t == 0.75
    args = cli.parse_args(base + ["--loss", "gbce", "--ce_negatives", "64", "--gbce_t", "0.5"])
    assert args.loss == "gbce" and args.ce_negatives == 64 and args.gbce_t == 0.5
    hp = Hyper(args)
    assert hp.loss == "gbce" and hp.ce_negatives == 64 and hp.gbce_t == 0.5
    assert Hyper().gbce_t == 0.75 and Hyper().loss == "bce"
    assert "gbce" in ALL_LOSSES and LOSSES == ("bce", "ce")
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--gbce_t", "most"])


def test_draw_restatement_matches_a_hand_computed_case():
    seed, step, V, N = 42, 3, 3417, 5
    want = [1 + (x * (V - 1) >> 32) for x in loss_host.hashes_by_hand(seed, step, N, 0x6BCE0000)]
    got = gbce_ref.draw(seed, step, V, N)
    assert got.dtype == np.int32 and got.tolist() == want
    for V in (2, 3, 17, 10 ** 7):
        s = gbce_ref.draw(7, 11, V, 4096)
        assert s.min() >= 1 and s.max() <= V - 1
    assert not np.array_equal(gbce_ref.draw(7, 11, 10 ** 7, 64), gbce_ref.draw(7, 12, 10 ** 7, 64))
    # a site of its own: not the sampled softmax's negatives at the same (seed, step, V)
    assert not np.array_equal(gbce_ref.draw(seed, step, 3417, 64), loss_ref.draw(seed, step, 3417, 64, loss_ref.SCE_SITE))


def test_beta_known_answers():
    b = gbce_ref.beta
    for N, itemnum in ((1, 10), (16, 37), (256, 3416), (4096, 10 ** 7)):
        alpha = N / (itemnum - 1)
        assert b(N, itemnum, 0.0) == 1.0
        assert b(N, itemnum, 1.0) == pytest.approx(alpha, rel=1e-12)
        assert b(N, itemnum, 0.75) == pytest.approx(1.0 - 0.75 * (1.0 - alpha), rel=1e-12)
        assert 0.0 < b(N, itemnum, 1.0) <= b(N, itemnum, 0.5) <= 1.0
    for t in (0.0, 0.3, 1.0):
        assert b(36, 37, t) == 1.0 and b(500, 37, t) == 1.0          # N >= pool: every negative is in the sample
        assert b(5, 1, t) == 1.0 and b(1, 1, t) == 1.0              # itemnum = 1: a pool of (at least) one


BOUND_CASES = [(D, N, V) for D in (8, 50, 256) for N in (1, 7, 256) for V in (17, 3417)]


@pytest.mark.parametrize("D,N,V", BOUND_CASES)
def test_emulated_device_arithmetic_stays_within_the_bounds(D, N, V):
    """The bound the GPU test gives cr_gbce 4x of is met at 1x by bf16 hi / lo operands, fp32 sums and fp32 sigma / softplus."""
    from loss_ref import sampled_case as _case
    M = 203 if D <= 64 else 97
    h, E_, pos, neg, s = _case(D, V, M, N, zlib.crc32(b"gbce%d_%d_%d" % (D, N, V)))
    live = np.flatnonzero(pos)
    assert (N < 2 or s[1] == s[0]) and (N < 3 or (s[2] == pos[live[0]] == pos[live[1]]))       # the planted duplicate and hit
    for b in (1.0, 0.25, 1e-3):
        ref = gbce_ref.ref64(h, E_, pos, neg, s, b)
        _check(gbce_ref.emulate(h, E_, pos, neg, s, b), ref)
        assert np.all(ref["e_l"][pos != 0] > 0) and np.all(ref["e_l"][pos == 0] == 0)


def test_small_e_series_keeps_a_row_of_very_negative_scores():
    """Scores of -18: e = exp(-18) = 2^-26 is below half an ulp of 1, so log(1 + e) as written returns 0 for every negative; the series
    keeps the row's loss inside the bound (and the naive form falls outside it)."""
    D, N, M, V = 8, 2048, 16, 2100
    h = np.zeros((M, D), np.float32); h[:, 0] = 1.0
    E_ = np.zeros((V, D), np.float32); E_[1:, 0] = -18.0
    E_[1:, 1] = np.random.RandomState(0).standard_normal(V - 1)
    pos = np.full(M, 1, np.int32)
    s = np.arange(2, 2 + N).astype(np.int32)
    ref = gbce_ref.ref64(h, E_, pos, np.zeros(M, np.int32), s, 1e-3)
    got = gbce_ref.emulate(h, E_, pos, np.zeros(M, np.int32), s, 1e-3)
    _check(got, ref)
    _sp18 = 18.0 + math.log1p(math.exp(-18.0))
    neg_part = N * math.log1p(math.exp(-18.0))
    assert ref["l"][0] == pytest.approx(1e-3 * _sp18 + neg_part, rel=1e-6)
    naive = np.float32(1e-3 * _sp18)                     # what log(1 + e) -> 0 would leave
    assert abs(float(naive) - ref["l"][0]) > ref["e_l"][0]


def test_fp64_reference_learns_the_planted_corpus_on_the_gpu_tests_schedule():
    """The thresholds of test_gbce_training_learns_a_planted_corpus are reachable: the fp64 reference of the same objective, model and
    schedule passes them -- and not on the sampled softmax's 250 steps, where it still sits on the constant-score plateau (gbce_ref)."""
    c = gbce_ref.PLANTED
    b = gbce_ref.beta(c["N"], c["itemnum"], c["t"])
    losses, hr = gbce_ref.planted_reference(gbce_ref.PLANTED_STEPS, log=(250,))
    plateau = gbce_ref.plateau_loss(c["N"], b)
    assert plateau == pytest.approx(2.28, abs=0.01)
    assert losses[250] == pytest.approx(plateau, rel=0.05)                      # step 250: the plateau, ranking still near chance
    assert losses[gbce_ref.PLANTED_STEPS] < 0.5 * (b + c["N"]) * math.log(2)    # the GPU test's two thresholds
    assert hr > 0.5, hr

"""Sampled softmax cross-entropy, host side (no GPU): cr_sampled_ce's argument checks and workspace query, the ctypes mirror of
cr_sampled_ce_desc, the --loss sampled_ce / --ce_negatives options and the numpy restatement of the device draw."""
import functools

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

import loss_host
import loss_ref
from loss_host import fmix32_by_hand as _fmix32_by_hand
from loss_ref import SCE_SITE

_valid_desc = functools.partial(loss_host.valid_desc, "sampled_ce")
_rejects = functools.partial(loss_host.rejects, "sampled_ce")


def _draw(seed, step, V, N):
    return loss_ref.draw(seed, step, V, N, SCE_SITE)


def test_sampled_ce_validates_before_any_hip_call():
    loss_host.refuses_the_common_arguments("sampled_ce")
    d = _valid_desc(); d.step = None                         # the device draw needs the step word
    _rejects(d, "step")
    d = _valid_desc()                                       # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_sampled_ce_workspace(40, 16, 50) - 1
    _rejects(d, "workspace")
    d = _valid_desc(); d.step, d.samples = None, 16         # caller-supplied samples: no step needed (fails on the workspace only)
    _rejects(d, "workspace")


def test_workspace_query_is_monotone_and_rejects_unsupported_shapes():
    loss_host.sampled_workspace_query_is_monotone(L.lib.cr_sampled_ce_workspace)


def test_sampled_ce_desc_mirror_matches_c_layout(tmp_path):
    loss_host.desc_mirror_matches_c_layout(tmp_path, "sampled_ce", ("CR_SCE_MAX_SAMPLES", "CR_SCE_SITE"))


def test_cli_takes_sampled_ce_and_ce_negatives():
    import main as cli
    from castrec_amd.engine import ALL_LOSSES, Hyper
    base = ["--dataset", "x", "--train_dir", "t", "--model", "cast_1"]
    args = cli.parse_args(base)
    assert args.loss == "bce" and args.ce_negatives == 256
    args = cli.parse_args(base + ["--loss", "sampled_ce", "--ce_negatives", "64"])
    assert args.loss == "sampled_ce" and args.ce_negatives == 64
    hp = Hyper(args)
    assert hp.loss == "sampled_ce" and hp.ce_negatives == 64
    assert Hyper().ce_negatives == 256
    assert "sampled_ce" in ALL_LOSSES
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--ce_negatives", "many"])


def test_draw_restatement_matches_a_hand_computed_case():
    seed, step, V, N = 42, 3, 3417, 5
    want = [1 + (x * (V - 1) >> 32) for x in loss_host.hashes_by_hand(seed, step, N, SCE_SITE)]
    got = _draw(seed, step, V, N)
    assert got.dtype == np.int32 and got.tolist() == want
    assert _fmix32_by_hand(0) == 0 and _fmix32_by_hand(1) == 0x514E28B7      # MurmurHash3 fmix32 reference values
    # every id in [1, V), V = 2 included (the only item is 1)
    for V in (2, 3, 17, 10 ** 7):
        s = _draw(7, 11, V, 4096)
        assert s.min() >= 1 and s.max() <= V - 1
    assert not np.array_equal(_draw(7, 11, 10 ** 7, 64), _draw(7, 12, 10 ** 7, 64))

"""Full-catalogue softmax cross-entropy, host side (no GPU): cr_softmax_ce's argument checks and workspace query, the ctypes mirror of
cr_softmax_ce_desc, and the loss option's defaults (main.py's parser, Hyper)."""
import functools

import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

import loss_host

_valid_desc = functools.partial(loss_host.valid_desc, "softmax_ce")
_rejects = functools.partial(loss_host.rejects, "softmax_ce")


def test_softmax_ce_validates_before_any_hip_call():
    loss_host.refuses_the_common_arguments("softmax_ce")
    d = _valid_desc()                                       # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_softmax_ce_workspace(40, 100, 50) - 1
    _rejects(d, "workspace")


def test_workspace_query_is_monotone_and_rejects_unsupported_shapes():
    ws = L.lib.cr_softmax_ce_workspace
    assert ws(0, 100, 50) == 0 and ws(-1, 100, 50) == 0 and ws(4, 1, 50) == 0 and ws(4, 100, 7) == 0 and ws(4, 100, 257) == 0
    assert ws(4, 100, 4) == 0
    for D in (8, 20, 50, 64, 128, 256):
        prev = 0
        for M in (1, 7, 64, 65, 300, 6400, 25600, 10 ** 6):
            n = ws(M, 3417, D)
            assert n > 0 and n >= prev, (D, M, n, prev)
            prev = n
        prev = 0
        for V in (2, 17, 100, 2048, 2049, 3417, 16384, 16385, 32768, 100003, 368001, 10 ** 7):
            n = ws(25600, V, D)
            assert n > 0 and n >= prev, (D, V, n, prev)
            prev = n
    # O((M + V) D), not [M, V]: the C4 shape's logits alone would be 37.7 GB
    assert ws(25600, 368001, 128) < 64 * 2 ** 20


def test_softmax_ce_desc_mirror_matches_c_layout(tmp_path):
    loss_host.desc_mirror_matches_c_layout(tmp_path, "softmax_ce")


def test_loss_defaults_to_bce():
    import main as cli
    from castrec_amd.engine import Hyper, LOSSES
    args = cli.parse_args(["--dataset", "x", "--train_dir", "t", "--model", "cast_1"])
    assert args.loss == "bce"
    assert cli.parse_args(["--dataset", "x", "--train_dir", "t", "--model", "cast_1", "--loss", "ce"]).loss == "ce"
    with pytest.raises(SystemExit):
        cli.parse_args(["--dataset", "x", "--train_dir", "t", "--model", "cast_1", "--loss", "softmax"])
    assert Hyper().loss == "bce" and Hyper(args).loss == "bce"
    assert Hyper(cli.parse_args(["--dataset", "x", "--train_dir", "t", "--model", "cast_1", "--loss", "ce"])).loss == "ce"
    assert LOSSES == ("bce", "ce")

"""Full-catalogue softmax cross-entropy, host side (no GPU): cr_softmax_ce's argument checks and workspace query, the ctypes mirror of
cr_softmax_ce_desc, and the loss option's defaults (main.py's parser, Hyper)."""
import ctypes
import os
import shutil
import subprocess

import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid_desc(M=40, V=100, D=50):
    """A descriptor that passes every check but the workspace (fake pointers: nothing is launched on a check failure)."""
    d = L.SoftmaxCeDesc()
    d.seq_emb, d.ld, d.table, d.pos, d.neg = 16, D, 16, 16, 16
    d.M, d.D, d.V, d.precision, d.state = M, D, V, L.PREC_BF16X3, 16
    d.d_seq_emb, d.ldd, d.table_grad = 16, D, 16
    return d


def _rejects(d, *words):
    rc = L.lib.cr_softmax_ce(ctypes.byref(d) if d is not None else None, None)
    msg = L.lib.cr_last_error().decode()
    assert rc == -1, (rc, msg)
    assert "cr_softmax_ce" in msg
    for w in words:
        assert w in msg, msg
    return msg


def test_softmax_ce_validates_before_any_hip_call():
    _rejects(None, "NULL descriptor")
    for f in ("seq_emb", "table", "pos", "state"):
        d = _valid_desc()
        setattr(d, f, None)
        _rejects(d, "NULL")
    for D in (4, 7, 257):
        d = _valid_desc(); d.D, d.ld, d.ldd = D, 300, 300
        _rejects(d, "D=%d" % D)
    for V in (1, 0, -3):
        d = _valid_desc(); d.V = V
        _rejects(d, "V=%d" % V)
    for M in (0, -1):
        d = _valid_desc(); d.M = M
        _rejects(d, "M=%d" % M)
    d = _valid_desc(); d.ld = 49
    _rejects(d, "ld=49")
    d = _valid_desc(); d.ldd = 10
    _rejects(d, "ldd=10")
    d = _valid_desc(); d.precision = 7
    _rejects(d, "precision 7")
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
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    probes = [("sizeof(cr_softmax_ce_desc)", ctypes.sizeof(L.SoftmaxCeDesc))]
    probes += [("offsetof(cr_softmax_ce_desc, %s)" % f, getattr(L.SoftmaxCeDesc, f).offset) for f, _ in L.SoftmaxCeDesc._fields_]
    src = tmp_path / "ce.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "castrec.h"\nint main(void){' +
                   "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probes) + 'return 0;}\n')
    exe = tmp_path / "ce"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [n for _, n in probes]


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

"""Sampled softmax cross-entropy, host side (no GPU): cr_sampled_ce's argument checks and workspace query, the ctypes mirror of
cr_sampled_ce_desc, the --loss sampled_ce / --ce_negatives options and the numpy restatement of the device draw."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

import sce_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid_desc(M=40, V=100, D=50, N=16):
    """A descriptor that passes every check but the workspace (fake pointers: nothing is launched on a check failure)."""
    d = L.SampledCeDesc()
    d.seq_emb, d.ld, d.table, d.pos, d.neg = 16, D, 16, 16, 16
    d.M, d.D, d.V, d.N, d.precision, d.state = M, D, V, N, L.PREC_BF16X3, 16
    d.samples, d.seed, d.step = None, 7, 16
    d.d_seq_emb, d.ldd, d.table_grad = 16, D, 16
    return d


def _rejects(d, *words):
    rc = L.lib.cr_sampled_ce(ctypes.byref(d) if d is not None else None, None)
    msg = L.lib.cr_last_error().decode()
    assert rc == -1, (rc, msg)
    assert "cr_sampled_ce" in msg
    for w in words:
        assert w in msg, msg
    return msg


def test_sampled_ce_validates_before_any_hip_call():
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
    for N in (0, -2, L.CR_SCE_MAX_SAMPLES + 1):
        d = _valid_desc(); d.N = N
        _rejects(d, "N=%d" % N)
    d = _valid_desc(); d.ld = 49
    _rejects(d, "ld=49")
    d = _valid_desc(); d.ldd = 10
    _rejects(d, "ldd=10")
    d = _valid_desc(); d.precision = 7
    _rejects(d, "precision 7")
    d = _valid_desc(); d.step = None                         # the device draw needs the step word
    _rejects(d, "step")
    d = _valid_desc()                                       # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_sampled_ce_workspace(40, 16, 50) - 1
    _rejects(d, "workspace")
    d = _valid_desc(); d.step, d.samples = None, 16         # caller-supplied samples: no step needed (fails on the workspace only)
    _rejects(d, "workspace")


def test_workspace_query_is_monotone_and_rejects_unsupported_shapes():
    ws = L.lib.cr_sampled_ce_workspace
    assert ws(0, 16, 50) == 0 and ws(-1, 16, 50) == 0 and ws(4, 0, 50) == 0 and ws(4, -1, 50) == 0
    assert ws(4, L.CR_SCE_MAX_SAMPLES + 1, 50) == 0 and ws(4, 16, 7) == 0 and ws(4, 16, 257) == 0 and ws(4, 16, 4) == 0
    assert ws(1, 1, 8) > 0 and ws(1, L.CR_SCE_MAX_SAMPLES, 256) > 0
    Ns = (1, 7, 31, 64, 256, 1000, 1024, 1025, 2048, 4096, 10000, 16384)
    Ms = (1, 7, 64, 65, 300, 6400, 25600, 65536, 10 ** 6)
    for D in (8, 20, 50, 64, 128, 256):
        for N in Ns:
            prev = 0
            for M in Ms:
                n = ws(M, N, D)
                assert n > 0 and n >= prev, (D, N, M, n, prev)
                prev = n
        for M in Ms:
            prev = 0
            for N in Ns:
                n = ws(M, N, D)
                assert n > 0 and n >= prev, (D, M, N, n, prev)
                prev = n
    # independent of V, O(M + N D): the C5 shape needs well under 100 MB
    assert ws(128 * 512, 4096, 256) < 100 * 2 ** 20


def test_sampled_ce_desc_mirror_matches_c_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    probes = [("sizeof(cr_sampled_ce_desc)", ctypes.sizeof(L.SampledCeDesc)), ("CR_SCE_MAX_SAMPLES", L.CR_SCE_MAX_SAMPLES),
              ("CR_SCE_SITE", L.CR_SCE_SITE)]
    probes += [("offsetof(cr_sampled_ce_desc, %s)" % f, getattr(L.SampledCeDesc, f).offset) for f, _ in L.SampledCeDesc._fields_]
    src = tmp_path / "sce.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "castrec.h"\nint main(void){' +
                   "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probes) + 'return 0;}\n')
    exe = tmp_path / "sce"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [n for _, n in probes]


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


def _fmix32_by_hand(h):
    """MurmurHash3's 32-bit finaliser on plain Python integers (cr_common.hpp cr_fmix32)."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def test_draw_restatement_matches_a_hand_computed_case():
    seed, step, V, N = 42, 3, 3417, 5
    inner = (step * 0x9E3779B9 + sce_ref.CR_SCE_SITE * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
    key = _fmix32_by_hand(seed ^ _fmix32_by_hand(inner))
    want = []
    for j in range(N):
        x = _fmix32_by_hand((key + j * 0x9E3779B1) & 0xFFFFFFFF)
        want.append(1 + (x * (V - 1) >> 32))
    got = sce_ref.draw(seed, step, V, N)
    assert got.dtype == np.int32 and got.tolist() == want
    assert _fmix32_by_hand(0) == 0 and _fmix32_by_hand(1) == 0x514E28B7      # MurmurHash3 fmix32 reference values
    # every id in [1, V), V = 2 included (the only item is 1)
    for V in (2, 3, 17, 10 ** 7):
        s = sce_ref.draw(7, 11, V, 4096)
        assert s.min() >= 1 and s.max() <= V - 1
    assert not np.array_equal(sce_ref.draw(7, 11, 10 ** 7, 64), sce_ref.draw(7, 12, 10 ** 7, 64))

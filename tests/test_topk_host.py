"""Full-catalogue top-K, host side (no GPU): cr_score_topk's argument checks and workspace query, the ctypes mirror of cr_topk_desc,
and the no-draw form of util._eval_inputs that util.evaluate_full builds on."""
import ctypes
import os
import random
import shutil
import subprocess
import types

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd import util as U
from helpers import load_sampler_golden
from topk_harness import rejects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid_desc(B=4, V=100, D=50, K=10):
    """A descriptor that passes every check but the workspace (fake pointers: nothing is launched on a check failure)."""
    d = L.TopkDesc()
    d.query, d.ld, d.table, d.V, d.D, d.B, d.K, d.precision = 16, D, 16, V, D, B, K, L.PREC_BF16X3
    d.top_ids, d.top_scores = 16, 16
    return d


def _rejects(d, *words):
    return rejects(("cr_score_topk", ctypes.byref(d) if d is not None else None, None), *words)


def test_score_topk_validates_before_any_hip_call():
    _rejects(None, "NULL descriptor")
    d = _valid_desc(); d.K = 0
    _rejects(d, "K=0")
    d = _valid_desc(); d.K = L.CR_TOPK_MAX + 1
    _rejects(d, "CR_TOPK_MAX")
    for D in (7, 257):
        d = _valid_desc(); d.D, d.ld = D, 300
        _rejects(d, "D=%d" % D)
    d = _valid_desc(); d.top_ids = None
    _rejects(d, "NULL output")
    d = _valid_desc(); d.top_scores = None
    _rejects(d, "NULL output")
    d = _valid_desc(); d.targets = 16
    _rejects(d, "rank")
    d = _valid_desc(B=3)
    off = np.array([0, 2, 1, 4], np.int64)                  # decreasing at row 1
    d.excl_off, d.excl_ids = off.ctypes.data, 16
    _rejects(d, "excl_off decreases at row 1")
    d = _valid_desc()                                       # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_score_topk_workspace(4, 100, 50, 10) - 1
    _rejects(d, "workspace")


def test_workspace_query_is_monotone_and_rejects_unsupported_shapes():
    ws = L.lib.cr_score_topk_workspace
    assert ws(0, 100, 50, 10) == 0 and ws(4, 0, 50, 10) == 0 and ws(4, 100, 7, 10) == 0 and ws(4, 100, 50, 0) == 0
    assert ws(4, 100, 50, L.CR_TOPK_MAX + 1) == 0 and ws(4, 100, 257, 10) == 0
    for D in (8, 20, 50, 64, 128, 256):
        prev = 0
        for B in (1, 7, 128, 300, 6040, 10000):
            n = ws(B, 368000, D, 10)
            assert n > 0 and n >= prev, (D, B, n, prev)
            prev = n
        prev = 0
        for V in (1, 100, 3416, 100003, 368000, 2000000, 10 ** 7):
            n = ws(128, V, D, 100)
            assert n > 0 and n >= prev, (D, V, n, prev)
            prev = n
        prev = 0
        for K in (1, 10, 100, L.CR_TOPK_MAX):
            n = ws(300, 100003, D, K)
            assert n > 0 and n >= prev, (D, K, n, prev)
            prev = n
    assert ws(10000, 368000, 128, 10) < 2 ** 30               # the chunk lists, not [B, V]


def test_topk_desc_mirror_matches_c_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    probes = [("sizeof(cr_topk_desc)", ctypes.sizeof(L.TopkDesc))]
    probes += [("offsetof(cr_topk_desc, %s)" % f, getattr(L.TopkDesc, f).offset) for f, _ in L.TopkDesc._fields_]
    src = tmp_path / "tk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "castrec.h"\nint main(void){' +
                   "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probes) + 'printf("%d\\n", CR_TOPK_MAX);return 0;}\n')
    exe = tmp_path / "tk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-1] == [n for _, n in probes]
    assert got[-1] == L.CR_TOPK_MAX >= 128


def _cases():
    _, _, corpora = load_sampler_golden()
    for key, c in sorted(corpora.items()):
        for T, seq_len in ((20, None), (50, 3)):
            args = types.SimpleNamespace(maxlen=T, bin_in_hours=24, max_bins=50, log_scale=False,
                                         test_model=("saved_run" if seq_len else None), test_seq_len=seq_len)
            yield key, c, args


def test_no_draw_inputs_match_the_drawing_ones_and_leave_np_random_alone():
    n_users = 0
    for key, c, args in _cases():
        train, valid, test, usernum, itemnum = U.partition(c.to_dict(), c.usernum, c.itemnum)[:5]
        min_td, max_td = U.get_delta_range(train)
        for mode in ("test", "valid"):
            for u in range(1, usernum + 1):
                np.random.seed(u)
                state = np.random.get_state()
                nd = U._eval_inputs(train, valid, test, u, mode, args, itemnum, min_td, max_td, draw=False)
                after = np.random.get_state()
                assert all(np.array_equal(x, y) for x, y in zip(state, after)), "draw=False moved np.random"
                dr = U._eval_inputs(train, valid, test, u, mode, args, itemnum, min_td, max_td)
                if dr is None:
                    assert nd is None
                    continue
                n_users += 1
                for a, b in zip(dr[:4], nd[:4]):
                    np.testing.assert_array_equal(a, b)
                target, rated = nd[4]
                assert dr[4][0] == target
                assert 0 in rated and not (set(dr[4][1:].tolist()) & rated)        # the negatives lie outside `rated`
    assert n_users > 10


def test_eval_users_keep_the_random_state():
    random.seed(3)
    before = random.getstate()
    users = U._eval_users(20000)
    assert random.getstate() == before
    assert list(users) == random.sample(range(1, 20001), 10000)            # the users the sampled evaluator draws next
    assert list(U._eval_users(50)) == list(range(1, 51))

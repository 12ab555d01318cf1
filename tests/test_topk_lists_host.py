"""Top-K over per-query candidate lists, host side (no GPU): candidate_csr on known answers, cr_score_topk_lists' argument checks and
workspace query, the segment rule's known answers, and the header / ctypes agreement of the descriptor and the three prototypes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd.index import candidate_csr
from topk_harness import rejects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cr_score_topk_lists"


# ---- candidate_csr ---------------------------------------------------------------------------------------------------------------------
def test_candidate_csr_makes_rows_unique_and_ascending():
    off, ids = candidate_csr([[5, 3, 5, 9, 3], (7,), np.array([2, 1], np.int32), iter([99, 1])], 4, 100)
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert off.tolist() == [0, 3, 4, 6, 8] and ids.tolist() == [3, 5, 9, 7, 1, 2, 1, 99]


def test_candidate_csr_allows_empty_rows():
    off, ids = candidate_csr([[], [4], []], 3, 10)
    assert off.tolist() == [0, 0, 1, 1] and ids.tolist() == [4]
    off, ids = candidate_csr([[], []], 2, 10)
    assert off.tolist() == [0, 0, 0] and ids.dtype == np.int32 and ids.size == 0


def test_candidate_csr_subtracts_the_exclusions_by_set_difference():
    rows = [[9, 2, 4, 2], [1, 2, 3], [5], [6, 7]]
    excl = [[4, 4, 50, 0, 200], [], [5], [8]]                   # duplicates, ids that are no candidates, 0, ids >= V: ignored
    off, ids = candidate_csr(rows, 4, 100, exclude=excl)
    assert off.tolist() == [0, 2, 5, 5, 7] and ids.tolist() == [2, 9, 1, 2, 3, 6, 7]
    with pytest.raises(ValueError, match="exclude"):
        candidate_csr(rows, 4, 100, exclude=excl[:3])


def test_candidate_csr_refuses_bad_ids_and_a_wrong_row_count():
    for bad in ([[1, 0]], [[100]], [[-1, 5]], [[3, 250]]):
        with pytest.raises(ValueError, match="1 .. 99"):
            candidate_csr(bad, 1, 100)
    assert candidate_csr([[99, 1]], 1, 100)[1].tolist() == [1, 99]
    with pytest.raises(ValueError, match="2 rows for a batch of 3"):
        candidate_csr([[1], [2]], 3, 100)


# ---- cr_score_topk_lists: refusals before any HIP call ---------------------------------------------------------------------------------
def _valid_desc(B=4, V=100, D=50, K=10, lens=(3, 0, 70, 5)):
    """A descriptor that passes every check but the workspace (fake pointers: nothing is launched on a check failure).  Returns it
    with the offsets array it points to (kept alive by the caller)."""
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    d = L.TopkListsDesc()
    d.query, d.ld, d.table, d.V, d.D, d.B, d.K, d.precision = 16, D, 16, V, D, B, K, L.PREC_BF16X3
    d.cand_off, d.cand_ids = off.ctypes.data, 16
    d.top_ids, d.top_scores = 16, 16
    return d, off


def _rejects(d, *words):
    return rejects((NAME, ctypes.byref(d) if d is not None else None, None), *words)


def test_score_topk_lists_validates_before_any_hip_call():
    _rejects(None, "NULL descriptor")
    d, keep = _valid_desc(); d.K = 0
    _rejects(d, "K=0")
    d, keep = _valid_desc(); d.K = L.CR_TOPK_MAX + 1
    _rejects(d, "K=129", "CR_TOPK_MAX")
    for D in (7, 257):
        d, keep = _valid_desc(); d.D, d.ld = D, 300
        _rejects(d, "D=%d" % D)
    d, keep = _valid_desc(); d.ld = 49
    _rejects(d, "ld=49")
    d, keep = _valid_desc(); d.top_ids = None
    _rejects(d, "NULL output")
    d, keep = _valid_desc(); d.top_scores = None
    _rejects(d, "NULL output")
    d, keep = _valid_desc(); d.targets = 16
    _rejects(d, "targets", "rank")
    d, keep = _valid_desc(B=3, lens=(1, 1, 1))
    bad = np.array([0, 2, 1, 4], np.int64)                  # decreasing at row 1
    d.cand_off = bad.ctypes.data
    _rejects(d, "cand_off decreases at row 1")
    bad = np.array([-1, 2, 3, 4], np.int64)
    d.cand_off = bad.ctypes.data
    _rejects(d, "cand_off[0]")
    d, keep = _valid_desc(); d.cand_off = None
    _rejects(d, "cand_off")
    d, keep = _valid_desc(); d.cand_ids = None              # ids named, none given
    _rejects(d, "cand_ids is NULL")
    d, keep = _valid_desc(); d.table = None                 # neither a table nor an index
    _rejects(d, "table")
    d, keep = _valid_desc()
    d.index, d.index_precision, d.index_bytes = 16, L.PREC_BF16, L.lib.cr_topk_index_bytes(100, 50, L.PREC_BF16)
    _rejects(d, "plain bf16 index")
    d.index_precision = 7
    _rejects(d, "index_precision")
    d.index_precision, d.index_bytes = L.PREC_BF16X3, L.lib.cr_topk_index_bytes(100, 50, L.PREC_BF16X3) - 16
    _rejects(d, "index_bytes")
    d, keep = _valid_desc()                                 # everything right but no workspace
    _rejects(d, "workspace")
    d.workspace, d.workspace_bytes = 16, L.lib.cr_score_topk_lists_workspace(4, 70, 50, 10) - 1
    _rejects(d, "workspace")
    d, keep = _valid_desc(B=2, lens=(5000, 70))             # three segments: the lists' workspace is asked for as well
    small = L.lib.cr_score_topk_lists_workspace(2, 70, 50, 10)
    assert L.lib.cr_score_topk_lists_workspace(2, 5000, 50, 10) > small
    d.workspace, d.workspace_bytes = 16, small
    _rejects(d, "workspace")


def test_an_all_empty_call_needs_no_cand_ids_but_still_a_workspace():
    d, keep = _valid_desc(lens=(0, 0, 0, 0)); d.cand_ids = None
    _rejects(d, "workspace")                                # it got past "cand_ids is NULL"


def test_workspace_query_is_zero_outside_the_supported_range():
    ws = L.lib.cr_score_topk_lists_workspace
    assert ws(0, 100, 50, 10) == 0 and ws(4, -1, 50, 10) == 0 and ws(4, 2 ** 31, 50, 10) == 0
    assert ws(4, 100, 7, 10) == 0 and ws(4, 100, 257, 10) == 0
    assert ws(4, 100, 50, 0) == 0 and ws(4, 100, 50, L.CR_TOPK_MAX + 1) == 0
    assert ws(1, 0, 8, 1) > 0 and ws(4, 100, 50, 10) >= 8 * 5
    assert ws(4, 2 ** 31 - 1, 256, L.CR_TOPK_MAX) > 0
    # one segment: the offsets alone, whatever the lists' length; segmented: the segments' lists, not [B, max_len]
    assert ws(10000, 100, 128, 10) == ws(10000, 2000, 128, 10) < 2 ** 20
    assert ws(2, 5000, 50, 10) >= ws(2, 70, 50, 10) + 3 * 2 * (10 * 8 + 8)
    assert ws(1, 10 ** 6, 128, 128) < 2 ** 20


def test_segment_counts_on_the_rules_known_answers():
    seg = L.lib.cr_topk_lists_segments
    assert seg(2, 5000) == 3
    assert seg(2000, 5000) == 1
    assert seg(1, 10 ** 6) == 256
    assert seg(1, 0) == 1
    assert seg(1, 2048) == 1 and seg(1, 2049) == 2          # the 2 048 floor
    assert seg(1024, 10 ** 6) == 1 and seg(512, 10 ** 6) == 2                    # about 1 024 workgroups
    assert seg(0, 10) == 0 and seg(1, -1) == 0


# ---- header <-> ctypes -----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_lists_prototypes():
    hdr = open(os.path.join(ROOT, "include", "castrec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    want = {"cr_score_topk_lists_workspace": ("size_t", ["int B", "int64_t max_len", "int D", "int K"]),
            "cr_topk_lists_segments": ("int", ["int B", "int64_t max_len"]),
            NAME: ("int", ["const cr_topk_lists_desc* d", "void* stream"])}
    so = ctypes.CDLL(L.LIB_PATH)
    for name, (ret, params) in want.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), hdr)
        assert m, "castrec.h does not declare %s %s" % (ret, name)
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
        kinds = [ctypes.POINTER(L.TopkListsDesc) if "cr_topk_lists_desc*" in p else ctypes.c_void_p if "*" in p
                 else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int for p in params]
        f = getattr(L.lib, name)
        assert f.restype is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and list(f.argtypes) == kinds, name
        assert name in L.EXPORTS and hasattr(so, name)


def test_topk_lists_desc_mirror_matches_c_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    probes = [("sizeof(cr_topk_lists_desc)", ctypes.sizeof(L.TopkListsDesc))]
    probes += [("offsetof(cr_topk_lists_desc, %s)" % f, getattr(L.TopkListsDesc, f).offset) for f, _ in L.TopkListsDesc._fields_]
    src = tmp_path / "tl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "castrec.h"\nint main(void){' +
                   "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probes) + "return 0;}\n")
    exe = tmp_path / "tl"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [n for _, n in probes]
    assert len(probes) == 20                                # 19 fields, as cr_topk_desc

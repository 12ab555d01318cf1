"""Shared candidate subsets, host side (no GPU): the global <-> local id translation (castrec_amd.index subset_ids / to_local /
to_global / excl_to_local), the argument checks of cr_topk_index_gather (all before any HIP call: fake pointers, as
test_topk_index_host.py), its prototype in header and ctypes, and the ItemSubset .npz round trip."""
import ctypes
import os
import re

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd.index import excl_csr, excl_to_local, subset_ids, to_global, to_local
import topk_index_ref as R
from topk_harness import rejects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16


def test_subset_ids_normalises_and_refuses():
    m = subset_ids([40, 7, 7, 99, 12, 40], 100)
    assert m.dtype == np.int32 and m.tolist() == [0, 7, 12, 40, 99]
    assert subset_ids(iter([3]), 4).tolist() == [0, 3]                                   # any iterable; V - 1 is an item
    assert subset_ids(np.array([[2, 1], [1, 2]]), 3).tolist() == [0, 1, 2]
    assert subset_ids(range(1, 100), 100).tolist() == list(range(100))
    for bad in ([], [0], [5, 0], [100], [1, 100], [-1], [-3, 4]):
        with pytest.raises(ValueError):
            subset_ids(bad, 100)


def test_to_local_and_back_on_known_answers():
    m = subset_ids([40, 7, 7, 99, 12], 100)                                              # local 1..4 = 7, 12, 40, 99
    loc = to_local(m, [7, 12, 40, 99, 0, 8, 1, 98, 100, 5000, -4])
    assert loc.dtype == np.int32 and loc.tolist() == [1, 2, 3, 4, 0, -1, -1, -1, -1, -1, -1]
    assert to_local(m, np.array([[99, 6], [0, 7]])).tolist() == [[4, -1], [0, 1]]        # shape kept
    # targets: inside -> local id, outside -> -1, which cr_score_topk answers with rank -1 (t outside 1 .. V-1)
    assert to_local(m, np.array([12, 13], np.int32)).tolist() == [2, -1]
    # map-back: local 0, the "fewer than k eligible" filler, stays 0
    back = to_global(m, np.array([[4, 1, 0], [2, 0, 0]], np.int32))
    assert back.tolist() == [[99, 7, 0], [12, 0, 0]]
    assert to_global(m, to_local(m, [7, 12, 40, 99])).tolist() == [7, 12, 40, 99]


def test_exclusion_rows_are_translated_and_absent_ids_dropped():
    m = subset_ids([7, 12, 40, 99], 100)
    rows = [[], [12, 13, 12, 0, 500], [1, 2, 3], [99, 7], []]
    off, ids = excl_to_local(m, *excl_csr(rows, 5))
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert off.tolist() == [0, 0, 2, 2, 4, 4] and ids.tolist() == [2, 2, 4, 1]            # duplicates stay, 0 / absent ids go
    off, ids = excl_to_local(m, *excl_csr([[5], [6]], 2))
    assert off.tolist() == [0, 0, 0] and ids.size == 0
    assert excl_to_local(m, None, None) == (None, None)
    off, ids = excl_to_local(m, np.array([3, 4, 6]), np.array([7, 7, 7, 40, 41, 12, 99], np.int32))       # offsets that start past 0
    assert off.tolist() == [0, 1, 2] and ids.tolist() == [3, 2]


def _gather_rejects(table, index, iprec, V, D, ids, n, prec, out, nbytes, *words):
    rejects(("cr_topk_index_gather", table, index, iprec, V, D, ids, n, prec, out, nbytes, None), *words)


def test_index_gather_validates_before_any_hip_call():
    n = 37
    need = L.lib.cr_topk_index_bytes(n + 1, 50, SPLIT)
    plain_need = L.lib.cr_topk_index_bytes(n + 1, 50, PLAIN)
    T, X = 16, 32                                                                        # fake pointers: never dereferenced
    _gather_rejects(None, None, 0, 100, 50, 16, n, SPLIT, 16, need, "NULL")              # neither source
    _gather_rejects(T, X, SPLIT, 100, 50, 16, n, SPLIT, 16, need, "both")                # both sources
    for src in ((T, None, 0), (None, X, SPLIT)):
        _gather_rejects(*src, 100, 50, None, n, SPLIT, 16, need, "NULL")                 # ids
        _gather_rejects(*src, 100, 50, 16, n, SPLIT, None, need, "NULL")                 # out_index
        for D in (7, 257):
            _gather_rejects(*src, 100, D, 16, n, SPLIT, 16, 1 << 30, "D=%d" % D)
        for bad_n in (0, -3):
            _gather_rejects(*src, 100, 50, 16, bad_n, SPLIT, 16, need, "n=%d" % bad_n)
        _gather_rejects(*src, 100, 50, 16, n, 7, 16, need, "precision")
        _gather_rejects(*src, 100, 50, 16, n, SPLIT, 16, need - 1, "bytes", str(need))
        _gather_rejects(*src, 100, 50, 16, n, SPLIT, 16, plain_need, "bytes")            # a plain-sized buffer for a split sub-index
        _gather_rejects(*src, 100, 50, 16, n, SPLIT, 16, 0, "bytes")
    _gather_rejects(None, X, PLAIN, 100, 50, 16, n, SPLIT, 16, need, "plain")            # a plain index has no lo plane
    _gather_rejects(None, X, PLAIN, 100, 50, 16, n, L.PREC_F32, 16, need, "plain")
    _gather_rejects(None, X, 9, 100, 50, 16, n, SPLIT, 16, need, "index_precision")


def test_header_and_ctypes_agree_on_the_gather_prototype():
    hdr = open(os.path.join(ROOT, "include", "castrec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cr_topk_index_gather\s*\(([^)]*)\)\s*;", hdr)
    assert m, "castrec.h does not declare cr_topk_index_gather"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* table", "const void* index", "int index_precision", "int V", "int D", "const int32_t* ids", "int n",
                      "int precision", "void* out_index", "size_t out_bytes", "void* stream"]
    kinds = [ctypes.c_void_p if "*" in p else ctypes.c_size_t if p.startswith("size_t") else ctypes.c_int for p in params]
    f = L.lib.cr_topk_index_gather
    assert f.restype is ctypes.c_int and list(f.argtypes) == kinds
    assert "cr_topk_index_gather" in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "cr_topk_index_gather")


def test_subset_npz_round_trip_and_refusals(tmp_path):
    import torch
    from castrec_amd.index import ItemIndex, ItemSubset
    rs = np.random.RandomState(2)
    V, D = 61, 20
    T = rs.standard_normal((V, D)).astype(np.float32)
    m = subset_ids([60, 1, 15, 16, 17, 33, 16], V)
    n1 = m.size
    G = np.concatenate([np.zeros((1, D), np.float32), T[m[1:]]])                         # the gathered table
    for name, prec in (("bf16x3", SPLIT), ("bf16", PLAIN)):
        blob = torch.from_numpy(R.build_blob(G, prec).copy())
        sub = ItemSubset(ItemIndex(n1, D, name, blob), torch.from_numpy(m.copy()), V, version=3)
        assert (sub.parent_V, sub.D, sub.precision, sub.version) == (V, D, name, 3)
        assert (sub.index.V, sub.index.D) == (n1, D) and sub.ids.dtype == torch.int32 and sub.ids.tolist() == m.tolist()
        p = str(tmp_path / ("sub_%s.npz" % name))
        assert sub.save(p) == p
        with np.load(p) as z:
            assert sorted(z.files) == ["blob", "ids", "meta"] and z["blob"].dtype == np.uint8 and z["ids"].dtype == np.int32
            assert z["meta"].tolist() == [1, n1, D, prec, V] and z["ids"].tolist() == m.tolist()
        back = ItemSubset.load(p, device="cpu")
        assert (back.parent_V, back.D, back.precision, back.version) == (V, D, name, None)
        assert torch.equal(back.index.blob, blob) and torch.equal(back.ids, sub.ids) and not back.index.blob.is_cuda
        with pytest.raises(RuntimeError, match="CPU"):
            back.search(np.zeros((1, D), np.float32), 3)
        with pytest.raises(ValueError, match="format"):                                  # five meta entries: not an item index file
            ItemIndex.load(p, device="cpu")
        plain_file = str(tmp_path / ("ix_%s.npz" % name))
        ItemIndex(n1, D, name, blob).save(plain_file)
        with pytest.raises(ValueError, match="subset"):
            ItemSubset.load(plain_file, device="cpu")
    good = R.build_blob(G, SPLIT)
    for what, kw in (("short blob", dict(blob=good[:-16], ids=m, meta=[1, n1, D, SPLIT, V])),
                     ("format 2", dict(blob=good, ids=m, meta=[2, n1, D, SPLIT, V])),
                     ("ids of another length", dict(blob=good, ids=m[:-1], meta=[1, n1, D, SPLIT, V])),
                     ("ids past the parent table", dict(blob=good, ids=m, meta=[1, n1, D, SPLIT, 60])),
                     ("ids not ascending", dict(blob=good, ids=m[::-1].copy(), meta=[1, n1, D, SPLIT, V])),
                     ("no ids", dict(blob=good, meta=[1, n1, D, SPLIT, V]))):
        bad = str(tmp_path / "bad.npz")
        kw["meta"] = np.array(kw["meta"], np.int64)
        np.savez(bad, **kw)
        try:
            ItemSubset.load(bad, device="cpu")
        except ValueError:
            continue
        raise AssertionError("ItemSubset.load accepted a file with " + what)
    with pytest.raises(ValueError):                                                      # ids[0] must be the padding row
        ItemSubset(ItemIndex(n1, D, "bf16x3", torch.from_numpy(good.copy())), torch.from_numpy((m + 1).astype(np.int32)), V + 1)

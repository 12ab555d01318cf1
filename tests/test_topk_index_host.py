"""Item index, host side (no GPU): cr_topk_index_bytes, the argument checks of cr_topk_index_build and of cr_score_topk's index fields
(all before any HIP call: fake pointers, as test_topk_host.py), the numpy restatement of the layout, and the .npz round trip."""
import ctypes

import numpy as np
import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
import topk_index_ref as R
from topk_harness import rejects

SPLIT, PLAIN = L.PREC_BF16X3, L.PREC_BF16


def test_index_bytes_is_the_layout_formula():
    nb = L.lib.cr_topk_index_bytes
    for D in (8, 20, 50, 64, 128, 256):
        for V in (1, 16, 17, 3417, 10 ** 7):
            for prec in (SPLIT, PLAIN):
                assert nb(V, D, prec) == R.index_bytes(V, D, prec), (V, D, prec)
            assert nb(V, D, L.PREC_F32) == nb(V, D, SPLIT) == 2 * nb(V, D, PLAIN)
    assert nb(10 ** 7, 256, SPLIT) == 10_240_000_000
    assert nb(3417, 50, SPLIT) == 2 * 214 * 2 * 1024
    for V, D, prec in ((0, 50, SPLIT), (-5, 50, SPLIT), (100, 7, SPLIT), (100, 257, SPLIT), (100, 50, 3), (100, 50, -1)):
        assert nb(V, D, prec) == 0, (V, D, prec)


def _build_rejects(table, V, D, prec, index, nbytes, *words):
    rejects(("cr_topk_index_build", table, V, D, prec, index, nbytes, None), *words)


def test_index_build_validates_before_any_hip_call():
    need = L.lib.cr_topk_index_bytes(100, 50, SPLIT)
    _build_rejects(None, 100, 50, SPLIT, 16, need, "NULL")
    _build_rejects(16, 100, 50, SPLIT, None, need, "NULL")
    for D in (7, 257):
        _build_rejects(16, 100, D, SPLIT, 16, 1 << 30, "D=%d" % D)
    _build_rejects(16, 0, 50, SPLIT, 16, need, "V=0")
    _build_rejects(16, 100, 50, 7, 16, need, "precision")
    _build_rejects(16, 100, 50, SPLIT, 16, need - 1, "bytes", str(need))
    _build_rejects(16, 100, 50, SPLIT, 16, L.lib.cr_topk_index_bytes(100, 50, PLAIN), "bytes")      # a plain-sized buffer for a split index
    _build_rejects(16, 100, 50, SPLIT, 16, 0, "bytes")


def _desc(B=4, V=100, D=50, K=10, precision=SPLIT, index_precision=SPLIT):
    """Passes every check but the workspace; the scores would come from the index: no table."""
    d = L.TopkDesc()
    d.query, d.ld, d.table, d.V, d.D, d.B, d.K, d.precision = 16, D, None, V, D, B, K, precision
    d.top_ids, d.top_scores = 16, 16
    d.index, d.index_bytes, d.index_precision = 16, L.lib.cr_topk_index_bytes(V, D, index_precision), index_precision
    return d


def _rejects(d, *words):
    return rejects(("cr_score_topk", ctypes.byref(d), None), *words)


def test_score_topk_index_fields_validate_before_any_hip_call():
    # an index and no table: everything up to the workspace passes
    for prec, iprec in ((SPLIT, SPLIT), (L.PREC_F32, SPLIT), (PLAIN, SPLIT), (PLAIN, PLAIN), (SPLIT, L.PREC_F32)):
        msg = _rejects(_desc(precision=prec, index_precision=iprec), "workspace")
        assert "index" not in msg and "table" not in msg
    d = _desc(); d.query = None
    _rejects(d, "NULL query")
    d = _desc(); d.index_precision = 5
    _rejects(d, "index_precision")
    for prec in (SPLIT, L.PREC_F32):                              # a plain index has no lo plane
        _rejects(_desc(precision=prec, index_precision=PLAIN), "plain", "index")
    for delta in (-1, 1, -1024):
        d = _desc(); d.index_bytes += delta
        _rejects(d, "index_bytes")
    d = _desc(); d.index_bytes = L.lib.cr_topk_index_bytes(100, 50, PLAIN)       # the size of the other kind
    _rejects(d, "index_bytes")
    d = _desc(); d.index_bytes = 0
    _rejects(d, "index_bytes")
    # without an index nothing changed: the table is required, by the same message
    d = _desc(); d.index, d.index_bytes, d.index_precision = None, 0, 0
    _rejects(d, "NULL query or table")
    d = _desc(); d.index = None; d.table = 16                    # index_bytes / index_precision are ignored without an index
    d.index_bytes, d.index_precision = 12345, 9
    _rejects(d, "workspace")


def test_positional_topk_desc_constructor_still_works():
    d = L.TopkDesc(16, 50, 16, 100, 50, 4, 10, SPLIT, None, None, None, 16, 16, None, None, 0)
    assert d.index is None and d.index_bytes == 0 and d.index_precision == 0
    _rejects(d, "workspace")
    names = [f for f, _ in L.TopkDesc._fields_]
    assert names[-3:] == ["index", "index_bytes", "index_precision"] and names[-4] == "workspace_bytes"


def test_numpy_builder_known_answer():
    T = (np.arange(24, dtype=np.float32).reshape(3, 8) + 1) * np.float32(1.001)       # not bf16-exact: lo is non-zero
    V, D = T.shape
    for prec in (SPLIT, PLAIN):
        blob = R.build_blob(T, prec)
        assert blob.dtype == np.uint8 and blob.size == R.index_bytes(V, D, prec) == L.lib.cr_topk_index_bytes(V, D, prec)
        hi = R._split(T, True)[0]
        np.testing.assert_array_equal(R.group(blob, V, D, 0, 0, 0, 2), hi[2])              # lane 2 = row 2, columns 0 .. 7
        assert R.group_offset(V, D, 0, 0, 0, 2) == 32
        for lane in range(64):
            g = R.group(blob, V, D, 0, 0, 0, lane)
            if lane < 3:
                np.testing.assert_array_equal(g, hi[lane])
            else:                                                                       # rows 3 .. 15, and columns >= 8 (lanes >= 16)
                assert not blob[R.group_offset(V, D, 0, 0, 0, lane):][:16].any(), lane
    blob = R.build_blob(T, SPLIT)
    lo = R._split(T, False)[1]
    assert np.any(lo != 0)
    assert R.group_offset(V, D, 1, 0, 0, 0) == 1024
    np.testing.assert_array_equal(R.group(blob, V, D, 1, 0, 0, 1), lo[1])
    np.testing.assert_array_equal(blob[:1024], R.build_blob(T, PLAIN))                 # plane 0 is the plain index
    # a second tile and a second k-step: row 17, columns 40 .. 47 of a [18, 50] table -> tile 1, k-step 1, lane 16 * 1 + 1
    rs = np.random.RandomState(0)
    T = rs.standard_normal((18, 50)).astype(np.float32)
    blob = R.build_blob(T, SPLIT)
    hi, lo = R._split(T, False)
    np.testing.assert_array_equal(R.group(blob, 18, 50, 0, 1, 1, 17), hi[17, 40:48])
    np.testing.assert_array_equal(R.group(blob, 18, 50, 1, 1, 1, 17), lo[17, 40:48])
    np.testing.assert_array_equal(R.group(blob, 18, 50, 0, 1, 1, 33), np.r_[hi[17, 48:50], np.zeros(6, np.float32)])
    assert not blob[R.group_offset(18, 50, 0, 1, 1, 49):][:16].any()                   # columns 56 .. 63


def test_npz_round_trip_and_refusals(tmp_path):
    import torch
    from castrec_amd.index import ItemIndex
    rs = np.random.RandomState(1)
    T = rs.standard_normal((37, 20)).astype(np.float32)
    for name, prec in (("bf16x3", SPLIT), ("bf16", PLAIN)):
        blob = torch.from_numpy(R.build_blob(T, prec).copy())
        ix = ItemIndex(37, 20, name, blob)
        assert (ix.V, ix.D, ix.precision, ix.version) == (37, 20, name, None)
        p = str(tmp_path / ("ix_%s.npz" % name))
        assert ix.save(p) == p
        with np.load(p) as z:
            assert sorted(z.files) == ["blob", "meta"] and z["blob"].dtype == np.uint8
            assert z["meta"].tolist() == [1, 37, 20, prec]
        back = ItemIndex.load(p, device="cpu")
        assert (back.V, back.D, back.precision, back.version) == (37, 20, name, None)
        assert torch.equal(back.blob, blob) and not back.blob.is_cuda
        with pytest.raises(RuntimeError, match="CPU"):
            back.search(np.zeros((1, 20), np.float32), 3)
    good = R.build_blob(T, SPLIT)
    bad = str(tmp_path / "format2.npz")
    np.savez(bad, blob=good, meta=np.array([2, 37, 20, SPLIT], np.int64))
    with pytest.raises(ValueError, match="format"):
        ItemIndex.load(bad, device="cpu")
    short = str(tmp_path / "short.npz")
    np.savez(short, blob=good[:-16], meta=np.array([1, 37, 20, SPLIT], np.int64))
    with pytest.raises(ValueError, match="blob"):
        ItemIndex.load(short, device="cpu")
    other = str(tmp_path / "other.npz")
    np.savez(other, blob=good, meta=np.array([1, 37, 20, PLAIN], np.int64))           # meta names the other kind
    with pytest.raises(ValueError, match="blob"):
        ItemIndex.load(other, device="cpu")
    with pytest.raises(ValueError):
        ItemIndex(37, 20, "bf16x3", torch.zeros(10, dtype=torch.uint8))

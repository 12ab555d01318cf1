"""The host builder of the occurrence index, as test_index and test_adam_gpu call it."""
import ctypes as C

import numpy as np

import castrec_amd  # noqa: F401
from castrec_amd import lib as L


def build_index(M, V, T_pos, seq, pos, neg, times=1, ng=32, ent=16):
    lay = L.IndexLayout()
    L.check(L.lib.cr_batch_index_layout(M, V, T_pos, ng, ent, C.byref(lay)), "layout")
    b = L.lib.cr_index_builder_create(M, V, T_pos, ng, ent)
    assert b
    out = np.full(lay.total_words, -7, np.int32)
    for _ in range(times):                                # (a builder's work arrays are clean again after every build)
        L.check(L.lib.cr_index_build(b, seq.ctypes.data, pos.ctypes.data, neg.ctypes.data, out.ctypes.data), "build")
    L.lib.cr_index_builder_destroy(b)
    return lay, out

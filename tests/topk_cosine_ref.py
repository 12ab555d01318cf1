"""Numpy restatement of the cosine item index (castrec.h CR_INDEX_COSINE): the rows x / ||x|| exactly as the index writers of
csrc/cr_topk.hip form them, in fp32 with their order of operations, so that topk_index_ref.build_blob(normalise(table), precision) is the
blob the device must produce byte for byte.

A row's lane (li, lg), lg = 0 .. 3, holds columns 32 ks + 8 lg + j of the row, zero past D.  Per lane p = 0, then for ks ascending and
j = 0 .. 7 ascending p = p + v * v (the product rounded, then the sum: no fused multiply-add); across the row's four lanes two xor
exchanges, distance 16 then 32: ss = (p_lg + p_lg^1) + (p_lg^2 + p_lg^3), the same bits in all four because fp32 addition commutes;
inv = ss > 0 ? 1 / sqrt(ss) : 0 with the correctly rounded square root and division numpy has; y = v * inv.  A zero row stays zero."""
import numpy as np

from topk_index_ref import planes, tk_nk


def sum_of_squares(table):
    """table [V, D] float32 -> ss [V] float32, in the writers' order."""
    table = np.ascontiguousarray(table, np.float32)
    V, D = table.shape
    NK = tk_nk(D)
    pad = np.zeros((V, NK * 32), np.float32)
    pad[:, :D] = table
    x = pad.reshape(V, NK, 4, 8)                                           # [row, ks, lg, j]
    p = np.zeros((V, 4), np.float32)
    for ks in range(NK):
        for j in range(8):
            sq = x[:, ks, :, j] * x[:, ks, :, j]
            p = p + sq
    assert sq.dtype == np.float32 and p.dtype == np.float32
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


def normalise(table):
    """table [V, D] float32 -> the float32 table the cosine index is the index of."""
    table = np.ascontiguousarray(table, np.float32)
    ss = sum_of_squares(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ss > 0, np.float32(1.0) / np.sqrt(ss), np.float32(0.0)).astype(np.float32)
    y = table * inv[:, None]
    assert y.dtype == np.float32
    return y


def stored_rows(blob, V, D, precision):
    """The rows a blob holds, as float64 hi + lo (hi alone for a plain index): [V, D].  The inverse of build_blob's layout."""
    NK, n_tiles, P = tk_nk(D), (V + 15) // 16, planes(precision)
    g = np.ascontiguousarray(blob).view(np.uint16).reshape(P, n_tiles, NK, 4, 16, 8)      # [plane, tile, ks, lg, li, j]
    f = (g.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    rows = f.transpose(0, 1, 4, 2, 3, 5).reshape(P, n_tiles * 16, NK * 32)                # [plane, row, column]
    assert not rows[:, V:].any() and not rows[:, :, D:].any(), "the padding of a blob is +0"
    return rows.sum(0)[:V, :D]

"""Numpy restatement of the item index layout (castrec.h "item index"): the blob cr_topk_index_build must produce, byte for byte.

NK = tk_nk(D) k-steps, n_tiles = ceil(V / 16), planes = 2 (split: hi, lo) or 1 (plain: hi).  The blob is an array of 16-byte groups of
eight bf16; group (plane h, tile t, k-step ks, lane l) sits at byte (((h n_tiles + t) NK + ks) 64 + l) 16 and its element j is column
32 ks + 8 (l >> 4) + j of row 16 t + (l & 15): hi = bf16(x), lo = bf16(x - hi); +0 where the row is >= V or the column >= D."""
import numpy as np

from gbce_ref import _split

PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2


def tk_nk(D):
    nk = (D + 31) // 32
    return 1 if nk <= 1 else 2 if nk <= 2 else 4 if nk <= 4 else 8


def planes(precision):
    return {PREC_F32: 2, PREC_BF16X3: 2, PREC_BF16: 1}[precision]


def index_bytes(V, D, precision):
    return planes(precision) * ((V + 15) // 16) * tk_nk(D) * 1024


def group_offset(V, D, h, t, ks, lane):
    """Byte offset of group (plane h, tile t, k-step ks, lane)."""
    return ((((h * ((V + 15) // 16) + t) * tk_nk(D) + ks) * 64) + lane) * 16


def _bits16(x):
    """bf16 values held as fp32 -> their 16 bits."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def build_blob(table, precision=PREC_BF16X3):
    """table [V, D] float32 -> the blob as a uint8 array."""
    table = np.ascontiguousarray(table, np.float32)
    V, D = table.shape
    NK, n_tiles, P = tk_nk(D), (V + 15) // 16, planes(precision)
    hi, lo = _split(table, P == 1)
    out = np.zeros((P, n_tiles, NK, 64, 8), np.uint16)
    for h, src in enumerate([hi, lo][:P]):
        pad = np.zeros((n_tiles * 16, NK * 32), np.uint16)                   # +0 past V and past D
        pad[:V, :D] = _bits16(src)
        # [tile, li, ks, lg, j] -> [tile, ks, lg, li, j]: lane = 16 lg + li
        out[h] = pad.reshape(n_tiles, 16, NK, 4, 8).transpose(0, 2, 3, 1, 4).reshape(n_tiles, NK, 64, 8)
    return out.reshape(-1).view(np.uint8)


def group(blob, V, D, h, t, ks, lane):
    """The eight bf16 of one group, widened to float32."""
    o = group_offset(V, D, h, t, ks, lane)
    return (blob[o:o + 16].view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


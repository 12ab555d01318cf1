"""ItemIndex: an item table pre-split, once, into the operand fragments cr_score_topk's sweep otherwise forms from the fp32 rows in
every workgroup of every call (castrec.h "item index").  Built from a device table, searched with any fp32 queries -- no model and no
engine needed -- and saved / loaded as one file.  A search returns the bits of the same search on the table.

    ix = ItemIndex.build(table)                    # table: float32 CUDA tensor [V, D]; or model.build_item_index()
    ids, scores = ix.search(queries, k=10)         # queries [B, D] float32, numpy or CUDA
    ix.save("items.npz"); ix = ItemIndex.load("items.npz")
"""
import numpy as np
import torch

from . import lib as L
from . import ops as O

FORMAT = 1
PRECISIONS = {"bf16x3": L.PREC_BF16X3, "bf16": L.PREC_BF16, "f32": L.PREC_BF16X3}
_NAMES = {L.PREC_BF16X3: "bf16x3", L.PREC_BF16: "bf16"}


def _prec(p):
    if isinstance(p, str):
        if p not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (sorted(PRECISIONS), p))
        return PRECISIONS[p]
    p = int(p)
    if p == L.PREC_F32:
        p = L.PREC_BF16X3
    if p not in _NAMES:
        raise ValueError("unknown precision %r" % (p,))
    return p


def excl_csr(rows, B):
    """Per-row id iterables -> (host int64 offsets [B + 1], int32 ids) as cr_score_topk takes them; (None, None) for rows None."""
    if rows is None:
        return None, None
    rows = [np.asarray(list(r), np.int64).ravel() for r in rows]
    if len(rows) != B:
        raise ValueError("exclude has %d rows for a batch of %d" % (len(rows), B))
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    ids = np.concatenate(rows).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return off, ids


class ItemIndex(object):
    """V, D: the table's shape; precision: "bf16x3" (hi + lo planes: serves every search precision) or "bf16" (hi only, half the bytes:
    plain-bf16 searches only); blob: the uint8 tensor of castrec.h's layout; version: the parameter version of the model that built it
    (Model.build_item_index), None for an index that was loaded or built from a bare table."""

    def __init__(self, V, D, precision, blob, version=None):
        self.V, self.D, self.precision, self.blob, self.version = int(V), int(D), _NAMES[_prec(precision)], blob, version
        need = L.lib.cr_topk_index_bytes(self.V, self.D, self.prec)
        if need == 0 or blob.numel() != need or blob.dtype != torch.uint8:
            raise ValueError("index blob of %d bytes (%s) does not fit V=%d D=%d precision=%s (%d bytes)"
                             % (blob.numel(), blob.dtype, self.V, self.D, self.precision, need))
        self._ws = None

    @property
    def prec(self):
        return PRECISIONS[self.precision]

    @classmethod
    def build(cls, table, precision="bf16x3", version=None):
        if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.float32 or table.dim() != 2:
            raise TypeError("ItemIndex.build takes a float32 CUDA tensor [V, D]")
        table = table.contiguous()
        p = _prec(precision)
        return cls(table.shape[0], table.shape[1], p, O.topk_index_build(table, p), version)

    def search(self, queries, k, exclude=None, targets=None, precision=None):
        """The k best items for each query row (dot product), as Model.recommend returns them: numpy (ids [B, k], scores [B, k]) and,
        with targets, each target's rank.  exclude: None or one iterable of ids per row.  precision: the search arithmetic, by
        default the index's own."""
        if not self.blob.is_cuda:
            raise RuntimeError("this ItemIndex was loaded on the CPU (inspection only): load it with device='cuda' to search")
        dev = self.blob.device
        q = queries if torch.is_tensor(queries) else torch.from_numpy(np.ascontiguousarray(queries, np.float32))
        q = q.to(dev, torch.float32).contiguous()
        if q.dim() != 2 or q.shape[1] != self.D:
            raise ValueError("queries must be [B, %d], got %s" % (self.D, tuple(q.shape)))
        B, k = q.shape[0], int(k)
        off, ids = excl_csr(exclude, B)
        if ids is not None and ids.size == 0:
            off = ids = None
        if ids is not None:
            ids = torch.from_numpy(ids).to(dev)
        if targets is not None:
            targets = (targets if torch.is_tensor(targets) else torch.from_numpy(np.asarray(targets, np.int32))).to(dev, torch.int32).contiguous()
        need = O.topk_workspace_bytes(B, self.V, self.D, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        top = torch.empty(B, k, dtype=torch.int32, device=dev)
        sc = torch.empty(B, k, dtype=torch.float32, device=dev)
        rk = torch.empty(B, dtype=torch.int32, device=dev) if targets is not None else None
        with torch.cuda.device(dev):
            O.score_topk(q, self.D, (self.V, self.D), B, k, self.prec if precision is None else _prec(precision), off, ids, targets,
                         self._ws, top, sc, rk, index=self.blob, index_precision=self.prec)
        out = (top.cpu().numpy(), sc.cpu().numpy())
        return out + (rk.cpu().numpy(),) if targets is not None else out

    def save(self, path):
        """One uncompressed .npz: blob (uint8) and meta = [format, V, D, precision]."""
        with open(path, "wb") as f:
            np.savez(f, blob=self.blob.cpu().numpy(), meta=np.array([FORMAT, self.V, self.D, self.prec], np.int64))
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """device="cpu" only inspects the file (V, D, precision, blob); such an index does not search.  version is None."""
        with np.load(path) as z:
            meta = [int(x) for x in z["meta"]]
            if len(meta) != 4 or meta[0] != FORMAT:
                raise ValueError("%s: item index format %s, this build reads format %d" % (path, meta[:1], FORMAT))
            _, V, D, p = meta
            need = L.lib.cr_topk_index_bytes(V, D, p) if p in _NAMES else 0
            blob = z["blob"]
            if need == 0 or blob.dtype != np.uint8 or blob.size != need:
                raise ValueError("%s: blob of %d bytes does not fit its meta V=%d D=%d precision=%d (%d bytes)"
                                 % (path, blob.size, V, D, p, need))
        return cls(V, D, p, torch.from_numpy(np.ascontiguousarray(blob)).to(device), None)

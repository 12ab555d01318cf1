"""ItemIndex: an item table pre-split, once, into the operand fragments cr_score_topk's sweep otherwise forms from the fp32 rows in
every workgroup of every call (castrec.h "item index").  Built from a device table, searched with any fp32 queries -- no model and no
engine needed -- and saved / loaded as one file.  A search returns the bits of the same search on the table.

    ix = ItemIndex.build(table)                    # table: float32 CUDA tensor [V, D]; or model.build_item_index()
    ids, scores = ix.search(queries, k=10)         # queries [B, D] float32, numpy or CUDA
    ix.save("items.npz"); ix = ItemIndex.load("items.npz")

ItemSubset: "the best k among these items" for a whole batch -- the allowed rows gathered once into a compact sub-index (castrec.h
cr_topk_index_gather) that the same search runs over; global ids in and out, the score bits of the full search.

    ids, scores = ix.search(queries, k=10, allow=in_stock)      # or: sub = ix.subset(in_stock); sub.search(queries, k=10)

Per-row candidate lists: "the best k among THIS row's candidates" (castrec.h cr_score_topk_lists) -- the rows a list names are gathered
and scored, so the cost follows the lists; global ids, the score bits of the full search.

    ids, scores = ix.search(queries, k=10, candidates=[row_0_ids, row_1_ids, ...])      # combines with exclude=

Keeping an index in step with training (castrec.h cr_topk_index_update / cr_topk_index_sync): rows are rewritten in place, the blob
ends as a fresh build's.

    model.refresh_item_index(ix)                   # "sync" (row-sparse Adam's flags name the moved rows) or "rebuild"
    ids, rows, tok = model.item_delta(tok)         # ... and in a serving process that holds no table: ix.update(ids, rows=rows)
"""
import numpy as np
import torch

from . import lib as L
from . import ops as O

FORMAT = 1                       # a dot-product index: meta = [1, V, D, precision], the file this module has always written
FORMAT_METRIC = 2                # any other metric: one more meta entry, the metric's code
PRECISIONS = {"bf16x3": L.PREC_BF16X3, "bf16": L.PREC_BF16, "f32": L.PREC_BF16X3}
_NAMES = {L.PREC_BF16X3: "bf16x3", L.PREC_BF16: "bf16"}
METRIC_CODES = {"dot": 0, "cosine": 1}
_METRIC_NAMES = {c: m for m, c in METRIC_CODES.items()}


def _metric(m):
    if m not in METRIC_CODES:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRIC_CODES), m))
    return m


def _file_metric(path, code):
    if code not in _METRIC_NAMES:
        raise ValueError("%s: unknown metric code %d (this build knows %s)" % (path, code, _METRIC_NAMES))
    return _METRIC_NAMES[code]


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


# ---- per-row candidate lists (castrec.h cr_score_topk_lists; pure numpy) -----------------------------------------------------------------
def candidate_csr(rows, B, V, exclude=None):
    """One iterable of item ids per row -> (host int64 offsets [B + 1], int32 ids) as cr_score_topk_lists takes them: each row unique
    and ascending, minus the ids of the row's `exclude` (None, or one iterable per row; ids that are no candidates are ignored).
    Empty rows are allowed.  ValueError for a wrong number of rows or a candidate outside 1 .. V-1."""
    rows = [np.unique(np.asarray(r if isinstance(r, np.ndarray) else list(r), np.int64).ravel()) for r in rows]
    if len(rows) != B:
        raise ValueError("candidates has %d rows for a batch of %d" % (len(rows), B))
    for b, r in enumerate(rows):
        if r.size and (r[0] < 1 or r[-1] > V - 1):
            raise ValueError("candidates must be item ids in 1 .. %d, row %d holds %d .. %d" % (V - 1, b, r[0], r[-1]))
    if exclude is not None:
        exclude = [np.asarray(e if isinstance(e, np.ndarray) else list(e), np.int64).ravel() for e in exclude]
        if len(exclude) != B:
            raise ValueError("exclude has %d rows for a batch of %d" % (len(exclude), B))
        rows = [np.setdiff1d(r, e, assume_unique=False) for r, e in zip(rows, exclude)]
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([r.size for r in rows])
    ids = np.concatenate(rows).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return off, ids


def _is_prebuilt(candidates):
    return isinstance(candidates, tuple) and len(candidates) == 2 and torch.is_tensor(candidates[1])


def candidates_for(candidates, B, V, excl_off=None, excl_ids=None):
    """The `candidates` argument of the public searches -> (cand_off, cand_ids) for search(): one iterable of ids per row, from which
    the exclusion CSR (excl_csr) is subtracted row by row, or a prebuilt (off, ids) pair whose ids is an int32 CUDA tensor the caller
    vouches for (distinct within a row; no exclusions can be subtracted from it: ValueError when some are given)."""
    if _is_prebuilt(candidates):
        off, ids = candidates
        if excl_off is not None:
            raise ValueError("a prebuilt (off, ids) candidates pair takes no exclude: subtract the exclusions when building it")
        off = np.ascontiguousarray(_host(off), np.int64)
        if off.shape != (B + 1,) or ids.dtype != torch.int32 or not ids.is_cuda or ids.dim() != 1 or not ids.is_contiguous():
            raise ValueError("prebuilt candidates: off int64 [B + 1 = %d] on the host, ids a contiguous int32 CUDA tensor" % (B + 1))
        if off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] > ids.numel():
            raise ValueError("prebuilt candidates: off must not decrease and must stay inside ids (%d entries)" % ids.numel())
        return off, ids
    exclude = None
    if excl_off is not None:
        o, e = np.asarray(excl_off, np.int64), np.asarray(_host(excl_ids), np.int64)
        exclude = [e[o[b]:o[b + 1]] for b in range(B)]
    return candidate_csr(candidates, B, V, exclude)


# ---- shared candidate subsets: global ids <-> the local ids of a gathered sub-index (pure numpy; ItemSubset and Engine.topk) --------
def subset_ids(ids, V):
    """Any iterable of item ids -> the subset's id map: int32 [n + 1], ascending without duplicates, [0] == 0 (local row 0 is the zero
    padding row, local row 1 + j is item map[1 + j]).  ValueError for an empty set or an id outside 1 .. V-1."""
    a = np.unique(np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), np.int64).ravel())
    if a.size == 0:
        raise ValueError("a subset needs at least one item id")
    if a[0] < 1 or a[-1] > V - 1:
        raise ValueError("subset ids must be item ids in 1 .. %d, got %d .. %d" % (V - 1, a[0], a[-1]))
    return np.concatenate([np.zeros(1, np.int64), a]).astype(np.int32)


def to_local(sorted_ids, ids):
    """Global ids -> local ids of the subset whose id map is sorted_ids (subset_ids): same shape, int32; id 0 stays 0 and an id that
    is not in the subset becomes -1 (as a target that reads "rank -1"; excl_to_local drops it)."""
    sorted_ids = np.asarray(sorted_ids, np.int64)
    ids = np.asarray(ids, np.int64)
    pos = np.minimum(np.searchsorted(sorted_ids, ids), sorted_ids.size - 1)
    return np.where(sorted_ids[pos] == ids, pos, -1).astype(np.int32)


def to_global(sorted_ids, local):
    """Local ids of a search of the subset -> global ids: local 0, the "fewer than k eligible" filler, stays 0."""
    return np.asarray(sorted_ids)[np.asarray(local, np.int64)]


def excl_to_local(sorted_ids, off, ids):
    """An exclusion CSR (excl_csr) on global ids -> the same on local ids; ids outside the subset (and 0) are dropped."""
    if off is None or ids is None:
        return None, None
    off = np.asarray(off, np.int64)
    loc = to_local(sorted_ids, np.asarray(ids, np.int64)[off[0]:off[-1]])
    keep = loc > 0
    kept = np.concatenate([np.zeros(1, np.int64), np.cumsum(keep, dtype=np.int64)])       # kept[i]: survivors among the first i ids
    return kept[off - off[0]], loc[keep].astype(np.int32)


# ---- the one search path (ItemIndex.search, ItemSubset.search, Engine.topk) ---------------------------------------------------------
def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _dev_i32(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.int32))).to(dev, torch.int32).contiguous()


def search(query, ld, B, k, source, precision, owner, excl_off=None, excl_ids=None, targets=None, cand_off=None, cand_ids=None):
    """cr_score_topk, marshalled once: the k best items for the B fp32 query rows query + b * ld (a CUDA tensor's storage) out of
    `source` -- the fp32 item table (a CUDA tensor [V, D]), an ItemIndex of it, or an ItemSubset (the best k among its items).
    precision: the search arithmetic (L.PREC_*).  excl_off / excl_ids: an exclusion CSR (excl_csr) and targets: [B] ids, host or
    device, all on global ids -- a subset's translation to its local ids and back happens here and nowhere else.  owner: the object
    that keeps the workspace between calls (its _topk_ws).  Returns device tensors (ids [B, k] int32, scores [B, k] fp32, rank [B]
    int32 or None for no targets).  cand_off / cand_ids: per-row candidate lists (candidate_csr; candidates_for has subtracted the
    exclusions) -- the best k among row b's own candidates, castrec.h cr_score_topk_lists, from the table or an ItemIndex; without
    them the call is the full search above."""
    dev, k = query.device, int(k)
    if cand_off is not None:
        return _search_lists(query, ld, B, k, source, precision, owner, excl_off, targets, cand_off, cand_ids)
    subset = source if isinstance(source, ItemSubset) else None
    if subset is not None:
        excl_off, excl_ids = excl_to_local(subset._map, excl_off, _host(excl_ids))
        if targets is not None:
            targets = to_local(subset._map, _host(targets))
        source = subset.index
    if excl_ids is not None:
        excl_ids = _dev_i32(excl_ids, dev)
        if excl_ids.numel() == 0:                           # an empty exclusion list is no exclusion list
            excl_off = excl_ids = None
    if targets is not None:
        targets = _dev_i32(targets, dev)
    if torch.is_tensor(source):
        (V, D), table, kw = source.shape, source, {}
    else:
        (V, D), kw = (source.V, source.D), dict(index=source.blob, index_precision=source.prec)
        table = (V, D)
    need = O.topk_workspace_bytes(B, V, D, k)
    ws = getattr(owner, "_topk_ws", None)
    if ws is None or ws.numel() < need:
        ws = owner._topk_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ids = torch.empty(B, k, dtype=torch.int32, device=dev)
    scores = torch.empty(B, k, dtype=torch.float32, device=dev)
    rank = torch.empty(B, dtype=torch.int32, device=dev) if targets is not None else None
    with torch.cuda.device(dev):
        O.score_topk(query, ld, table, B, k, precision, excl_off, excl_ids, targets, ws, ids, scores, rank, **kw)
        if subset is not None:
            ids = subset.ids.to(dev)[ids.long()]            # local -> global; local 0 (fewer than k eligible) stays 0
    return ids, scores, rank


def _search_lists(query, ld, B, k, source, precision, owner, excl_off, targets, cand_off, cand_ids):
    """search() with per-row candidate lists: cr_score_topk_lists, its workspace (sized for the longest row) kept on owner."""
    dev = query.device
    if isinstance(source, ItemSubset):
        raise ValueError("one filter per call: candidates= and an ItemSubset (allow=) exclude each other")
    if excl_off is not None:
        raise ValueError("candidates= takes its exclusions on the host (candidates_for): none may reach the search")
    cand_off = np.ascontiguousarray(cand_off, np.int64)
    if cand_off.shape != (B + 1,):
        raise ValueError("cand_off must have B + 1 = %d entries, got %s" % (B + 1, cand_off.shape))
    cand_ids = _dev_i32(cand_ids, dev) if cand_off[-1] > cand_off[0] else None
    if targets is not None:
        targets = _dev_i32(targets, dev)
    if torch.is_tensor(source):
        (V, D), table, kw = source.shape, source, {}
    else:
        (V, D), kw = (source.V, source.D), dict(index=source.blob, index_precision=source.prec)
        table = (V, D)
    need = O.topk_lists_workspace_bytes(B, int(np.diff(cand_off).max()), D, k)
    ws = getattr(owner, "_topk_lists_ws", None)
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = owner._topk_lists_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ids = torch.empty(B, k, dtype=torch.int32, device=dev)
    scores = torch.empty(B, k, dtype=torch.float32, device=dev)
    rank = torch.empty(B, dtype=torch.int32, device=dev) if targets is not None else None
    with torch.cuda.device(dev):
        O.score_topk_lists(query, ld, table, B, k, precision, cand_off, cand_ids, targets, ws, ids, scores, rank, **kw)
    return ids, scores, rank


def _search_numpy(source, queries, k, exclude, targets, precision, candidates=None):
    """ItemIndex.search and ItemSubset.search: queries (numpy or CUDA) and per-row exclusion lists in, numpy out."""
    index = source.index if isinstance(source, ItemSubset) else source
    if not index.blob.is_cuda:
        raise RuntimeError("this ItemIndex was loaded on the CPU (inspection only): load it with device='cuda' to search")
    q = queries if torch.is_tensor(queries) else torch.from_numpy(np.ascontiguousarray(queries, np.float32))
    q = q.to(index.blob.device, torch.float32).contiguous()
    if q.dim() != 2 or q.shape[1] != index.D:
        raise ValueError("queries must be [B, %d], got %s" % (index.D, tuple(q.shape)))
    B = q.shape[0]
    excl, cand = excl_csr(exclude, B), (None, None)
    if candidates is not None:
        cand, excl = candidates_for(candidates, B, index.V, *excl), (None, None)
    top, sc, rk = search(q, index.D, B, k, source, index.prec if precision is None else _prec(precision), index, *excl,
                         targets=targets, cand_off=cand[0], cand_ids=cand[1])
    out = (top.cpu().numpy(), sc.cpu().numpy())
    return out + (rk.cpu().numpy(),) if rk is not None else out


class ItemIndex(object):
    """V, D: the table's shape; precision: "bf16x3" (hi + lo planes: serves every search precision) or "bf16" (hi only, half the bytes:
    plain-bf16 searches only); blob: the uint8 tensor of castrec.h's layout; version: the parameter version of the model that built it
    (Model.build_item_index), None for an index that was loaded or built from a bare table; token: what the blob is in step with,
    for Model.refresh_item_index / item_delta (models.IndexToken; None: unknown, a refresh rebuilds).  metric: "dot" -- the blob
    holds the table's rows x -- or "cosine" -- it holds x / ||x||, normalised on the device as the blob is written (castrec.h
    CR_INDEX_COSINE: same size, same layout, same search kernels).  update / sync / rebuild and subset carry the index's own metric."""

    def __init__(self, V, D, precision, blob, version=None, metric="dot"):
        self.V, self.D, self.precision, self.blob, self.version = int(V), int(D), _NAMES[_prec(precision)], blob, version
        self.metric = _metric(metric)
        self.token = None
        need = L.lib.cr_topk_index_bytes(self.V, self.D, self.prec)
        if need == 0 or blob.numel() != need or blob.dtype != torch.uint8:
            raise ValueError("index blob of %d bytes (%s) does not fit V=%d D=%d precision=%s (%d bytes)"
                             % (blob.numel(), blob.dtype, self.V, self.D, self.precision, need))

    @property
    def prec(self):
        return PRECISIONS[self.precision]

    @classmethod
    def build(cls, table, precision="bf16x3", version=None, metric="dot"):
        """The index of table (a float32 CUDA tensor [V, D]).  metric="cosine": of its rows normalised, x / ||x|| (a zero row stays
        zero), without a normalised copy of the table: one pass, the same bytes of index."""
        _metric(metric)
        if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.float32 or table.dim() != 2:
            raise TypeError("ItemIndex.build takes a float32 CUDA tensor [V, D]")
        table = table.contiguous()
        p = _prec(precision)
        return cls(table.shape[0], table.shape[1], p, O.topk_index_build(table, p, metric=metric), version, metric)

    def subset(self, ids):
        """An ItemSubset of the items `ids` (any iterable of ids in 1 .. V-1), gathered out of this index: no table needed.  The
        subset inherits precision, version and metric (the rows of a cosine index are normalised already: they are copied)."""
        if not self.blob.is_cuda:
            raise RuntimeError("this ItemIndex was loaded on the CPU (inspection only): load it with device='cuda' to gather a subset")
        m = torch.from_numpy(subset_ids(ids, self.V)).to(self.blob.device)
        with torch.cuda.device(self.blob.device):
            blob = O.topk_index_gather(m[1:], self.prec, index=self.blob, index_precision=self.prec, V=self.V, D=self.D)
        return ItemSubset(ItemIndex(m.numel(), self.D, self.prec, blob, self.version, self.metric), m, self.V, self.version)

    # -- keeping the index in step with its table (castrec.h cr_topk_index_update / cr_topk_index_sync): a row's groups are its own, so
    # the blob is rewritten in place, no allocation, and holds the bytes of a fresh build of the table.  An ItemSubset gathered
    # earlier (subset(), search(allow=)) has its own blob: it stays the snapshot it was.  version: stored in self.version (None for
    # an index that follows no model); Model.refresh_item_index drives sync / rebuild and sets it.  All three write with the index's own
    # metric and take RAW rows: a cosine index normalises them as its build did, so one delta (Model.item_delta) serves either kind.
    def _writable(self, what):
        if not self.blob.is_cuda:
            raise RuntimeError("this ItemIndex was loaded on the CPU (inspection only): load it with device='cuda' to %s it" % what)

    def _table(self, table):
        if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.float32 or tuple(table.shape) != (self.V, self.D):
            raise ValueError("table must be a float32 CUDA tensor [%d, %d], got %s"
                             % (self.V, self.D, tuple(table.shape) if torch.is_tensor(table) else type(table).__name__))
        return table.contiguous()

    def update(self, ids, rows=None, table=None, version=None):
        """Rewrites the rows `ids` in place -- any iterable of item ids or an int32 CUDA tensor, each in 1 .. V-1 (ValueError
        otherwise), duplicates allowed where they carry the same row.  Exactly one source: table, the float32 CUDA tensor [V, D] the
        index follows (row ids[j] is read), or rows, float32 [n, D] (numpy or tensor) with rows[j] the new row of item ids[j] -- a
        delta sent without the table (Model.item_delta), for an index that was load()-ed where no table exists.  An ItemSubset
        gathered from this index earlier stays the snapshot it was."""
        if (rows is None) == (table is None):
            raise ValueError("ItemIndex.update takes exactly one source: rows or table (%s given)" % ("both" if rows is not None else "neither"))
        if torch.is_tensor(ids):
            if ids.dtype != torch.int32 or ids.dim() != 1:
                raise ValueError("ids as a tensor must be int32 [n], got %s %s" % (ids.dtype, tuple(ids.shape)))
            n = ids.numel()
            lo, hi = (int(ids.min()), int(ids.max())) if n else (1, 1)
        else:
            ids = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), np.int64).ravel()
            n = ids.size
            lo, hi = (int(ids.min()), int(ids.max())) if n else (1, 1)
        if n == 0:
            raise ValueError("ItemIndex.update needs at least one id")
        if lo < 1 or hi > self.V - 1:
            raise ValueError("ids must be item ids in 1 .. %d, got %d .. %d" % (self.V - 1, lo, hi))
        if rows is not None:
            src = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows, np.float32))
            if src.dtype != torch.float32 or tuple(src.shape) != (n, self.D):
                raise ValueError("rows must be float32 [%d, %d] (one row per id), got %s %s" % (n, self.D, src.dtype, tuple(src.shape)))
        self._writable("update")
        dev = self.blob.device
        ids = (ids if torch.is_tensor(ids) else torch.from_numpy(ids.astype(np.int32))).to(dev).contiguous()
        src = src.to(dev).contiguous() if rows is not None else self._table(table)
        with torch.cuda.device(dev):
            O.topk_index_update(self.blob, self.V, self.D, self.prec, ids, src, packed=rows is not None, metric=self.metric)
        self.version = version
        return self

    def sync(self, table, flags, since, version=None):
        """Rewrites in place, from table (float32 CUDA [V, D]), every 16-row tile with a row whose flags[r] >= since: flags is the
        int32 CUDA tensor [V] of row-sparse Adam (Engine.lazy_flags: the number of the last step that moved row r), so the rows moved
        by steps since .. are refreshed; the other rows of such a tile are rewritten with the bytes they had.  Tiles without a flagged
        row are neither read nor written.  An ItemSubset gathered earlier stays the snapshot it was."""
        self._writable("sync")
        with torch.cuda.device(self.blob.device):
            O.topk_index_sync(self.blob, self._table(table), self.prec, flags, since, metric=self.metric)
        self.version = version
        return self

    def rebuild(self, table, version=None):
        """The whole blob again from table (float32 CUDA [V, D]), into the tensor it already has: ItemIndex.build without the
        allocation.  An ItemSubset gathered earlier stays the snapshot it was."""
        self._writable("rebuild")
        with torch.cuda.device(self.blob.device):
            O.topk_index_build(self._table(table), self.prec, out=self.blob, metric=self.metric)
        self.version = version
        return self

    def search(self, queries, k, exclude=None, targets=None, precision=None, allow=None, candidates=None):
        """The k best items for each query row (dot product), as Model.recommend returns them: numpy (ids [B, k], scores [B, k]) and,
        with targets, each target's rank.  On a cosine index the dot product is with the normalised rows: a score is q . x / ||x||
        = cos(q, x) ||q||, so the order within a row is the cosine order; the queries are not normalised here (divide a row's scores
        by ||q|| for cosines; Model.similar_items(metric="cosine") does).  exclude: None or one iterable of ids per row.  precision: the search arithmetic, by
        default the index's own.  allow: an iterable of ids -- the best k among those items only, for every row: shorthand for
        self.subset(allow).search(...) (keep the ItemSubset to search the same set again).  candidates: one iterable of ids per
        row -- the best k among THAT row's candidates (minus the row's exclude; a target outside them has rank -1), or a prebuilt
        (off, ids) pair (candidate_csr, ids an int32 CUDA tensor; exclude must then be None).  One filter per call: allow or
        candidates."""
        if allow is not None:
            if candidates is not None:
                raise ValueError("one filter per call: allow= or candidates=")
            return self.subset(allow).search(queries, k, exclude=exclude, targets=targets, precision=precision)
        return _search_numpy(self, queries, k, exclude, targets, precision, candidates)

    def save(self, path):
        """One uncompressed .npz: blob (uint8) and meta = [1, V, D, precision] for a dot-product index (format 1, unchanged), meta =
        [2, V, D, precision, metric code] (format 2; cosine: 1) otherwise."""
        meta = [FORMAT, self.V, self.D, self.prec] if self.metric == "dot" else \
            [FORMAT_METRIC, self.V, self.D, self.prec, METRIC_CODES[self.metric]]
        with open(path, "wb") as f:
            np.savez(f, blob=self.blob.cpu().numpy(), meta=np.array(meta, np.int64))
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """device="cpu" only inspects the file (V, D, precision, metric, blob); such an index does not search.  version is None."""
        with np.load(path) as z:
            meta = [int(x) for x in z["meta"]]
            if not ((len(meta) == 4 and meta[0] == FORMAT) or (len(meta) == 5 and meta[0] == FORMAT_METRIC and "ids" not in z.files)):
                raise ValueError("%s: item index format %s with %d meta entries, this build reads format %d (4 entries) and %d (5; "
                                 "an ItemSubset file loads with ItemSubset.load)" % (path, meta[:1], len(meta), FORMAT, FORMAT_METRIC))
            V, D, p = meta[1:4]
            metric = _file_metric(path, meta[4]) if len(meta) == 5 else "dot"
            need = L.lib.cr_topk_index_bytes(V, D, p) if p in _NAMES else 0
            blob = z["blob"]
            if need == 0 or blob.dtype != np.uint8 or blob.size != need:
                raise ValueError("%s: blob of %d bytes does not fit its meta V=%d D=%d precision=%d (%d bytes)"
                                 % (path, blob.size, V, D, p, need))
        return cls(V, D, p, torch.from_numpy(np.ascontiguousarray(blob)).to(device), None, metric)


SUBSET_FORMAT = 1                # a subset of dot-product rows: meta = [1, n + 1, D, precision, parent_V]
SUBSET_FORMAT_METRIC = 2         # any other metric: a sixth meta entry, the metric's code


class ItemSubset(object):
    """A candidate subset shared by every query of a search: "the best k among these items".  index: an ItemIndex of the gathered
    [n + 1, D] table {0; item ids[1]; ...; item ids[n]} (castrec.h cr_topk_index_gather: the bytes cr_topk_index_build gives on that
    table, so a score has the bits of the full search); ids: int32 [n + 1] on the index's device, ascending, ids[0] == 0 -- local
    row -> global id; parent_V: the rows of the table the ids refer to; version: as ItemIndex.version.  Ascending ids make the local
    order the global order, so ties break as in the full search.  Everything public takes and returns global ids; ranks are ranks
    among the eligible items of the subset.  One subset per call, shared by all rows: a list per row goes through candidates=
    (ItemIndex.search, Model.recommend), not through a subset.

        sub = ix.subset(ids)                           # out of an ItemIndex; or ItemSubset.build(table, ids) from the fp32 table
        top, scores = sub.search(queries, k=10)        # == ix.search(queries, 10, allow=ids)
        sub.save("instock.npz"); sub = ItemSubset.load("instock.npz")
    """

    def __init__(self, index, ids, parent_V, version=None):
        self.index, self.ids, self.parent_V, self.version = index, ids, int(parent_V), version
        self._map = ids.cpu().numpy()
        m = self._map
        if (ids.dtype != torch.int32 or m.ndim != 1 or m.size != index.V or m.size < 2 or m[0] != 0 or np.any(np.diff(m.astype(np.int64)) <= 0)
                or m[-1] > self.parent_V - 1):
            raise ValueError("subset ids must be int32 [%d]: 0, then ascending item ids below %d" % (index.V, self.parent_V))

    D = property(lambda self: self.index.D)
    precision = property(lambda self: self.index.precision)
    prec = property(lambda self: self.index.prec)
    metric = property(lambda self: self.index.metric)

    @classmethod
    def build(cls, table, ids, precision="bf16x3", version=None, metric="dot"):
        """From the fp32 table itself (a float32 CUDA tensor [V, D]): only the subset's rows are read, no full index is needed.
        metric="cosine": the gathered rows are normalised as ItemIndex.build(metric="cosine") normalises them."""
        _metric(metric)
        if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.float32 or table.dim() != 2:
            raise TypeError("ItemSubset.build takes a float32 CUDA tensor [V, D]")
        table = table.contiguous()
        p = _prec(precision)
        V, D = table.shape
        m = torch.from_numpy(subset_ids(ids, V)).to(table.device)
        with torch.cuda.device(table.device):
            blob = O.topk_index_gather(m[1:], p, table=table, metric=metric)
        return cls(ItemIndex(m.numel(), D, p, blob, version, metric), m, V, version)

    def search(self, queries, k, exclude=None, targets=None, precision=None):
        """ItemIndex.search among the subset's items: global ids in, global ids out.  An excluded id outside the subset is ignored; a
        target outside it (or excluded) has rank -1; a row with fewer than k eligible items ends in id 0, score -inf."""
        return _search_numpy(self, queries, k, exclude, targets, precision)

    def save(self, path):
        """One uncompressed .npz: blob (uint8), ids (int32 [n + 1]) and meta = [1, n + 1, D, precision, parent_V] for dot-product rows
        (format 1, unchanged), meta = [2, n + 1, D, precision, parent_V, metric code] (format 2; cosine: 1) otherwise."""
        meta = [SUBSET_FORMAT, self.index.V, self.D, self.prec, self.parent_V]
        if self.metric != "dot":
            meta = [SUBSET_FORMAT_METRIC] + meta[1:] + [METRIC_CODES[self.metric]]
        with open(path, "wb") as f:
            np.savez(f, blob=self.index.blob.cpu().numpy(), ids=self._map, meta=np.array(meta, np.int64))
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """device="cpu" only inspects the file; such a subset does not search.  version is None."""
        with np.load(path) as z:
            meta = [int(x) for x in z["meta"]]
            if "ids" not in z.files or not ((len(meta) == 5 and meta[0] == SUBSET_FORMAT) or
                                            (len(meta) == 6 and meta[0] == SUBSET_FORMAT_METRIC)):
                raise ValueError("%s: not an item subset file of format %d or %d (meta %s; an ItemIndex file loads with ItemIndex.load)"
                                 % (path, SUBSET_FORMAT, SUBSET_FORMAT_METRIC, meta))
            V, D, p, parent_V = meta[1:5]
            metric = _file_metric(path, meta[5]) if len(meta) == 6 else "dot"
            need = L.lib.cr_topk_index_bytes(V, D, p) if p in _NAMES else 0
            blob, ids = z["blob"], z["ids"]
            if need == 0 or blob.dtype != np.uint8 or blob.size != need:
                raise ValueError("%s: blob of %d bytes does not fit its meta n + 1=%d D=%d precision=%d (%d bytes)"
                                 % (path, blob.size, V, D, p, need))
            if ids.dtype != np.int32:
                raise ValueError("%s: ids of type %s, int32 expected" % (path, ids.dtype))
        index = ItemIndex(V, D, p, torch.from_numpy(np.ascontiguousarray(blob)).to(device), None, metric)
        return cls(index, torch.from_numpy(np.ascontiguousarray(ids)).to(device), parent_V, None)

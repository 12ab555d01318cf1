"""Thin op wrappers: torch CUDA tensors in, C-ABI descriptors out.  PyTorch is used only for device
memory and the current HIP stream; every computation is a kernel of libcastrec.so."""
import ctypes as C

import torch

from . import lib as L


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
        raise TypeError("%s must be a float32 CUDA tensor" % name)
    return t


def _i32(t, name):
    if t is not None and (t.dtype != torch.int32 or not t.is_cuda):
        raise TypeError("%s must be an int32 CUDA tensor" % name)
    return t


class Drop:
    """Dropout context of one step: seed, device step counter, data-parallel row offset."""

    def __init__(self, rate, seed, state, row_offset=0):
        self.rate, self.seed, self.state, self.row_offset = float(rate), int(seed) & 0xFFFFFFFF, state, int(row_offset)

    def rng(self, site, enabled=True):
        rate = self.rate if enabled else 0.0
        return L.Rng(rate, site, self.seed, self.state.data_ptr() + 16, self.row_offset)   # &state[4]


NO_DROP = L.Rng(0.0, 0, 0, None, 0)


def step_begin(state):
    L.call("cr_step_begin", _p(state), _stream())


def embed_fwd(ids, table, T, out, ld_out, col_off=0, zero_pad=True, scale=1.0, pos_table=None, addend=None,
              ld_add=0, rng=NO_DROP, mask_ids=None):
    V, D = table.shape
    d = L.EmbedDesc(_p(_i32(ids, "ids")), _p(_f32(table, "table")), ids.numel(), T, D, V, int(zero_pad), float(scale),
                    _p(pos_table), _p(addend), ld_add, rng, _p(mask_ids), _p(_f32(out, "out")), ld_out, col_off)
    L.call("cr_embed_fwd", C.byref(d), _stream())
    return d


def embed_bwd(fdesc, dout, table_grad=None, pos_grad=None, d_addend=None, slab_stride=0, n_slabs=0, out2=None):
    f = L.EmbedDesc.from_buffer_copy(fdesc)
    f.out = _p(dout)
    d = L.EmbedBwdDesc(f, _p(table_grad), _p(pos_grad), _p(d_addend), slab_stride, n_slabs, _p(_f32(out2, "out2")))
    L.call("cr_embed_bwd", C.byref(d), _stream())


def layernorm_fwd(x, ldx, gamma, beta, y, ldy, M, D, x_nonzero=None, y_nonzero=None, eps=1e-8):
    d = L.LnDesc(_p(x), ldx, _p(gamma), _p(beta), _p(y), ldy, M, D, eps, _p(x_nonzero), _p(y_nonzero))
    L.call("cr_layernorm_fwd", C.byref(d), _stream())


def layernorm_bwd(x, ldx, gamma, dy, lddy, dx, lddx, dgamma, dbeta, slab_stride, n_slabs, M, D, accumulate=False, eps=1e-8):
    d = L.LnBwdDesc(_p(x), ldx, _p(gamma), _p(dy), lddy, _p(dx), lddx, int(accumulate), _p(dgamma), _p(dbeta),
                    slab_stride, n_slabs, M, D, eps)
    L.call("cr_layernorm_bwd", C.byref(d), _stream())


def gemm_desc(A, lda, B, ldb, Cm, ldc, M, N, K, bias=None, trans_b=False, relu=False, rng=NO_DROP, residual=None,
              ldr=0, mask_ids=None, accumulate=False, precision=0):
    return L.GemmDesc(_p(A), lda, _p(B), ldb, _p(bias), _p(Cm), ldc, M, N, K, int(trans_b), int(relu), rng,
                      _p(residual), ldr, _p(mask_ids), int(accumulate), int(precision))


def gemm_rows(descs):
    arr = (L.GemmDesc * len(descs))(*descs)
    L.call("cr_gemm_rows", arr, len(descs), _stream())


def wgrad_desc(A, lda, G, ldg, dW, db, M, N, K, ldw=None, precision=0):
    return L.WgradDesc(_p(A), lda, _p(G), ldg, _p(dW), N if ldw is None else ldw, _p(db), M, N, K, int(precision))


def gemm_wgrad(descs, slab_stride, n_slabs):
    arr = (L.WgradDesc * len(descs))(*descs)
    L.call("cr_gemm_wgrad", arr, len(descs), slab_stride, n_slabs, _stream())


def eltwise(op, x, ldx, y, ldy, M, N, aux=None, ldaux=0, rng=NO_DROP, mask_ids=None, accumulate=False):
    d = L.EltDesc(op, _p(x), ldx, _p(aux), ldaux, _p(y), ldy, M, N, rng, _p(mask_ids), int(accumulate))
    L.call("cr_eltwise", C.byref(d), _stream())


def attn_desc(Q, K, V, ld, k_valid, q_valid, residual, ldr, out, ldo, B, T, H, d, rng=NO_DROP, batch_global=None,
              dead_ids=None, attn_weights=None, row_stats=None, precision=0):
    return L.AttnDesc(_p(Q), _p(K), _p(V), ld, _p(k_valid), _p(q_valid), _p(residual), ldr, _p(dead_ids), _p(out), ldo,
                      _p(attn_weights), B, T, H, d, rng, B if batch_global is None else batch_global, _p(row_stats),
                      int(precision))


def attn_fwd(desc):
    L.call("cr_attn_fwd", C.byref(desc), _stream())


def attn_bwd(fdesc, dout, lddo, dQ, dK, dV, ldg, stats, delta=None, dQ_part=None):
    d = L.AttnBwdDesc(L.AttnDesc.from_buffer_copy(fdesc), _p(dout), lddo, _p(dQ), _p(dK), _p(dV), ldg, _p(stats),
                      _p(delta), _p(dQ_part))
    L.call("cr_attn_bwd", C.byref(d), _stream())


def head_fwd_bwd(seq_emb, ld, table, pos, neg, M, D, state, d_seq_emb=None, ldd=0, table_grad=None,
                 pos_logits=None, neg_logits=None, coef_out=None):
    d = L.HeadDesc(_p(seq_emb), ld, _p(table), _p(pos), _p(neg), M, D, table.shape[0], _p(state), _p(d_seq_emb), ldd,
                   _p(table_grad), _p(pos_logits), _p(neg_logits), _p(coef_out))
    L.call("cr_head_fwd_bwd", C.byref(d), _stream())


def head_fwd_bwd_ln(seq_emb, ld, table, pos, neg, M, D, state, x, ldx, gamma, dx, lddx, dgamma, dbeta, slab_stride, n_slabs,
                    d_seq_emb=None, ldd=0, table_grad=None, pos_logits=None, neg_logits=None, coef_out=None, eps=1e-8):
    """cr_head_fwd_bwd with the backward of the LayerNorm that made seq_emb from x (the layernorm_bwd call that would have followed)."""
    d = L.HeadDesc(_p(seq_emb), ld, _p(table), _p(pos), _p(neg), M, D, table.shape[0], _p(state), _p(d_seq_emb), ldd,
                   _p(table_grad), _p(pos_logits), _p(neg_logits), _p(coef_out))
    n = L.LnBwdDesc(_p(x), ldx, _p(gamma), None, 0, _p(dx), lddx, 0, _p(dgamma), _p(dbeta), slab_stride, n_slabs, M, D, eps)
    L.call("cr_head_fwd_bwd_ln", C.byref(d), C.byref(n), _stream())


def test_logits(seq_emb, ld, table, cand, B, T, D, logits):
    L.call("cr_test_logits", _p(seq_emb), ld, _p(table), _p(_i32(cand, "cand")), B, T, D, table.shape[0],
           cand.shape[1], _p(logits), _stream())


def topk_workspace_bytes(B, V, D, K):
    n = L.lib.cr_score_topk_workspace(B, V, D, K)
    if n == 0:
        raise ValueError("cr_score_topk: unsupported shape B=%d V=%d D=%d K=%d (1 <= K <= %d, 8 <= D <= 256)" % (B, V, D, K, L.CR_TOPK_MAX))
    return n


def score_topk(query, ld, table, B, K, precision, excl_off, excl_ids, targets, workspace, top_ids, top_scores, rank=None,
               index=None, index_precision=None):
    """cr_score_topk: query rows query + b * ld (a float32 CUDA tensor's storage), table [V, D]; excl_off a host int64 numpy array
    [B + 1] or None, excl_ids an int32 CUDA tensor; workspace a uint8 CUDA tensor of at least topk_workspace_bytes bytes.
    index: a uint8 CUDA tensor from topk_index_build (index_precision: what it was built with) -- the scores then come from it and
    `table` may be the (V, D) pair instead of the tensor."""
    import numpy as np
    off = None
    if excl_off is not None:
        off = np.ascontiguousarray(excl_off, np.int64)
        if off.shape != (B + 1,):
            raise ValueError("excl_off must have B + 1 = %d entries, got %s" % (B + 1, off.shape))
    if index is not None and not torch.is_tensor(table):
        (V, D), table = table, None
    else:
        V, D = table.shape
    d = L.TopkDesc(_p(_f32(query, "query")), ld, _p(_f32(table, "table")), V, D, B, K, precision,
                   None if off is None else off.ctypes.data, _p(_i32(excl_ids, "excl_ids")), _p(_i32(targets, "targets")),
                   _p(_i32(top_ids, "top_ids")), _p(_f32(top_scores, "top_scores")), _p(_i32(rank, "rank")),
                   _p(workspace), workspace.numel() * workspace.element_size())
    if index is not None:
        if index.dtype != torch.uint8 or not index.is_cuda or not index.is_contiguous():
            raise TypeError("index must be a contiguous uint8 CUDA tensor")
        d.index, d.index_bytes, d.index_precision = index.data_ptr(), index.numel(), int(precision if index_precision is None else index_precision)
    L.call("cr_score_topk", C.byref(d), _stream())


def topk_lists_workspace_bytes(B, max_len, D, K):
    n = L.lib.cr_score_topk_lists_workspace(B, max_len, D, K)
    if n == 0:
        raise ValueError("cr_score_topk_lists: unsupported shape B=%d max_len=%d D=%d K=%d (1 <= K <= %d, 8 <= D <= 256, rows shorter than 2^31)"
                         % (B, max_len, D, K, L.CR_TOPK_MAX))
    return n


def score_topk_lists(query, ld, table, B, K, precision, cand_off, cand_ids, targets, workspace, top_ids, top_scores, rank=None,
                     index=None, index_precision=None):
    """cr_score_topk_lists: the K best of row b's candidates cand_ids[cand_off[b] : cand_off[b + 1]] (cand_off a host int64 numpy array
    [B + 1], cand_ids an int32 CUDA tensor or None when every list is empty); everything else as score_topk, workspace of at least
    topk_lists_workspace_bytes(B, the longest row, D, K) bytes."""
    import numpy as np
    off = np.ascontiguousarray(cand_off, np.int64)
    if off.shape != (B + 1,):
        raise ValueError("cand_off must have B + 1 = %d entries, got %s" % (B + 1, off.shape))
    if index is not None and not torch.is_tensor(table):
        (V, D), table = table, None
    else:
        V, D = table.shape
    d = L.TopkListsDesc(_p(_f32(query, "query")), ld, _p(_f32(table, "table")), V, D, B, K, precision,
                        off.ctypes.data, _p(_i32(cand_ids, "cand_ids")), _p(_i32(targets, "targets")),
                        _p(_i32(top_ids, "top_ids")), _p(_f32(top_scores, "top_scores")), _p(_i32(rank, "rank")),
                        _p(workspace), workspace.numel() * workspace.element_size())
    if index is not None:
        if index.dtype != torch.uint8 or not index.is_cuda or not index.is_contiguous():
            raise TypeError("index must be a contiguous uint8 CUDA tensor")
        d.index, d.index_bytes, d.index_precision = index.data_ptr(), index.numel(), int(precision if index_precision is None else index_precision)
    L.call("cr_score_topk_lists", C.byref(d), _stream())


def topk_index_bytes(V, D, precision=L.PREC_BF16X3):
    n = L.lib.cr_topk_index_bytes(V, D, precision)
    if n == 0:
        raise ValueError("cr_topk_index_bytes: unsupported V=%d D=%d precision=%d (V >= 1, 8 <= D <= 256)" % (V, D, precision))
    return n


METRICS = {"dot": 0, "cosine": L.INDEX_COSINE}     # what an index's rows hold: x, or x / ||x|| (castrec.h CR_INDEX_COSINE)


def _writer_precision(precision, metric):
    """The `precision` argument of the four index writers: the CR_PREC_* value with the metric's flag OR-ed in."""
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    return int(precision) | METRICS[metric]


def topk_index_build(table, precision=L.PREC_BF16X3, out=None, metric="dot"):
    """cr_topk_index_build: the item index of table [V, D] (a contiguous float32 CUDA tensor) as a uint8 CUDA tensor.  metric
    "cosine": the index of the rows x / ||x|| (castrec.h CR_INDEX_COSINE); the same size, searched by the same calls."""
    _f32(table, "table")
    if table.dim() != 2 or not table.is_contiguous():
        raise ValueError("table must be a contiguous [V, D] tensor")
    V, D = table.shape
    n = topk_index_bytes(V, D, precision)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=table.device)
    L.call("cr_topk_index_build", _p(table), V, D, _writer_precision(precision, metric), out.data_ptr(), out.numel(), _stream())
    return out


def topk_index_gather(ids, precision=L.PREC_BF16X3, table=None, index=None, index_precision=None, V=None, D=None, out=None,
                      metric="dot"):
    """cr_topk_index_gather: the index of {0; source row ids[0]; ...} as a uint8 CUDA tensor.  ids: an int32 CUDA tensor [n] of ids in
    1 .. V-1.  The source is `table` (a contiguous float32 CUDA tensor [V, D]) or `index` (a uint8 CUDA tensor from topk_index_build
    of a [V, D] table, built with index_precision) -- exactly one.  metric "cosine": rows read from a table are normalised; the rows
    of an index source are copied as they are (a sub-index of a cosine index is a cosine index whatever is said here)."""
    _i32(ids, "ids")
    wprec = _writer_precision(precision, metric)
    if (table is None) == (index is None):
        raise ValueError("topk_index_gather takes exactly one source: table or index")
    if table is not None:
        _f32(table, "table")
        if table.dim() != 2 or not table.is_contiguous():
            raise ValueError("table must be a contiguous [V, D] tensor")
        V, D = table.shape
        index_precision = 0
    else:
        if index.dtype != torch.uint8 or not index.is_cuda or not index.is_contiguous():
            raise TypeError("index must be a contiguous uint8 CUDA tensor")
        index_precision = int(precision if index_precision is None else index_precision)
        if index.numel() != topk_index_bytes(V, D, index_precision):
            raise ValueError("index of %d bytes is not an index of V=%d D=%d precision=%d" % (index.numel(), V, D, index_precision))
    if ids.dim() != 1 or not ids.is_contiguous() or ids.numel() < 1:
        raise ValueError("ids must be a contiguous [n] tensor, n >= 1")
    n = ids.numel()
    nb = topk_index_bytes(n + 1, D, precision)
    if out is None:
        out = torch.empty(nb, dtype=torch.uint8, device=ids.device)
    L.call("cr_topk_index_gather", _p(table), _p(index), index_precision, V, D, ids.data_ptr(), n, wprec, out.data_ptr(), out.numel(),
           _stream())
    return out


def _index_blob(index, V, D, precision):
    if not torch.is_tensor(index) or index.dtype != torch.uint8 or not index.is_cuda or not index.is_contiguous():
        raise TypeError("index must be a contiguous uint8 CUDA tensor")
    if index.numel() != topk_index_bytes(V, D, precision):
        raise ValueError("index of %d bytes is not an index of V=%d D=%d precision=%d" % (index.numel(), V, D, precision))


def topk_index_update(index, V, D, precision, ids, src, packed, metric="dot"):
    """cr_topk_index_update: rewrites rows ids (an int32 CUDA tensor [n], n >= 1; ids outside 0 .. V-1 are skipped) of `index`, the
    uint8 CUDA blob of a [V, D] table built with `precision`, in place.  src: a contiguous float32 CUDA tensor -- the [V, D] table
    (packed False: the source row of ids[j] is ids[j]) or [n, D] rows in list order (packed True: the source row of ids[j] is j).
    metric: the metric `index` was built with -- "cosine" normalises the raw rows of src as the build did."""
    V, D, precision = int(V), int(D), int(precision)
    wprec = _writer_precision(precision, metric)
    _index_blob(index, V, D, precision)
    if not torch.is_tensor(ids) or not torch.is_tensor(src):
        raise TypeError("ids must be an int32 CUDA tensor and src a float32 CUDA tensor")
    _i32(ids, "ids")
    if ids.dim() != 1 or not ids.is_contiguous() or ids.numel() < 1:
        raise ValueError("ids must be a contiguous [n] tensor, n >= 1")
    n = ids.numel()
    _f32(src, "src")
    want = (n, D) if packed else (V, D)
    if tuple(src.shape) != want or not src.is_contiguous():
        raise ValueError("src must be a contiguous [%d, %d] tensor (%s), got %s"
                         % (want + ("packed rows" if packed else "the table", tuple(src.shape))))
    if ids.device != index.device or src.device != index.device:
        raise ValueError("index, ids and src must be on one device")
    L.call("cr_topk_index_update", _p(src), 1 if packed else 0, V, D, wprec, index.data_ptr(), index.numel(), ids.data_ptr(), n,
           _stream())
    return index


def topk_index_sync(index, table, precision, flags, since, metric="dot"):
    """cr_topk_index_sync: rewrites in place every 16-row tile of `index` (the uint8 CUDA blob of table [V, D], built with `precision`)
    that has a row with (uint32) flags[r] >= since.  table: a contiguous float32 CUDA tensor [V, D]; flags: an int32 CUDA tensor [V]
    (Engine.lazy_flags).  metric: the metric `index` was built with, as in topk_index_update."""
    wprec = _writer_precision(precision, metric)
    if not torch.is_tensor(table) or not torch.is_tensor(flags):
        raise TypeError("table must be a float32 CUDA tensor and flags an int32 CUDA tensor")
    _f32(table, "table")
    if table.dim() != 2 or not table.is_contiguous():
        raise ValueError("table must be a contiguous [V, D] tensor")
    V, D = table.shape
    precision, since = int(precision), int(since)
    _index_blob(index, V, D, precision)
    _i32(flags, "flags")
    if tuple(flags.shape) != (V,) or not flags.is_contiguous():
        raise ValueError("flags must be a contiguous [V = %d] tensor, got %s" % (V, tuple(flags.shape)))
    if not 0 <= since <= 0xffffffff:
        raise ValueError("since=%d must fit an unsigned 32-bit step number" % since)
    if flags.device != index.device or table.device != index.device:
        raise ValueError("index, table and flags must be on one device")
    L.call("cr_topk_index_sync", _p(table), V, D, wprec, index.data_ptr(), index.numel(), flags.data_ptr(), since, _stream())
    return index


def softmax_ce_workspace_bytes(M, V, D):
    n = L.lib.cr_softmax_ce_workspace(M, V, D)
    if n == 0:
        raise ValueError("cr_softmax_ce: unsupported shape M=%d V=%d D=%d (M >= 1, V >= 2, 8 <= D <= 256)" % (M, V, D))
    return n


def softmax_ce(seq_emb, ld, table, pos, state, workspace, M, precision=L.PREC_BF16X3, neg=None, d_seq_emb=None, ldd=0,
               table_grad=None, lse_out=None):
    """cr_softmax_ce: rows seq_emb + m * ld (m < M) of a float32 CUDA tensor's storage against table [V, D]; pos / neg int32 [M];
    state the float32 [CR_STATE_FLOATS] block ([0..2] += the loss / AUC / target sums, snapshot [8..11]); d_seq_emb (rows of pitch
    ldd) written, table_grad accumulated, lse_out [M] written where given; workspace a uint8 CUDA tensor of at least
    softmax_ce_workspace_bytes(M, V, D) bytes."""
    d = L.SoftmaxCeDesc(_p(_f32(seq_emb, "seq_emb")), ld, _p(_f32(table, "table")), _p(_i32(pos, "pos")), _p(_i32(neg, "neg")),
                        M, table.shape[1], table.shape[0], precision, _p(_f32(state, "state")), _p(_f32(d_seq_emb, "d_seq_emb")), ldd,
                        _p(_f32(table_grad, "table_grad")), _p(_f32(lse_out, "lse_out")), _p(workspace),
                        workspace.numel() * workspace.element_size())
    L.call("cr_softmax_ce", C.byref(d), _stream())


def sampled_ce_workspace_bytes(M, N, D):
    n = L.lib.cr_sampled_ce_workspace(M, N, D)
    if n == 0:
        raise ValueError("cr_sampled_ce: unsupported shape M=%d N=%d D=%d (M >= 1, 1 <= N <= %d, 8 <= D <= 256)"
                         % (M, N, D, L.CR_SCE_MAX_SAMPLES))
    return n


def sampled_ce(seq_emb, ld, table, pos, state, workspace, M, N, precision=L.PREC_BF16X3, neg=None, samples=None, seed=0, step=None,
               samples_out=None, d_seq_emb=None, ldd=0, table_grad=None, lse_out=None, cdf=None, logq=None):
    """cr_sampled_ce: the softmax over each row's target and N shared sample ids.  Rows seq_emb + m * ld (m < M) of a float32 CUDA
    tensor's storage against table [V, D]; pos / neg int32 [M]; samples an int32 [N] tensor of ids in [1, V), or None: drawn on the
    device from seed and step (a CUDA tensor whose first 4 bytes are the uint32 step word, e.g. state[4:5]); samples_out int32 [N]
    written where given; state, d_seq_emb, table_grad, lse_out as softmax_ce; workspace a uint8 CUDA tensor of at least
    sampled_ce_workspace_bytes(M, N, D) bytes.  cdf (int32 or uint32 [V], the bits of the uint32 cumulative masses) and logq (float32
    [V]): a popularity proposal and its log-Q correction (castrec_amd.util.build_proposal); both None: the uniform proposal."""
    if cdf is not None and (cdf.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not cdf.is_cuda):
        raise TypeError("cdf must be an int32 / uint32 CUDA tensor")
    d = L.SampledCeDesc(_p(_f32(seq_emb, "seq_emb")), ld, _p(_f32(table, "table")), _p(_i32(pos, "pos")), _p(_i32(neg, "neg")),
                        M, table.shape[1], table.shape[0], N, precision, _p(_i32(samples, "samples")), int(seed) & 0xFFFFFFFF,
                        _p(step), _p(_i32(samples_out, "samples_out")), _p(_f32(state, "state")), _p(_f32(d_seq_emb, "d_seq_emb")),
                        ldd, _p(_f32(table_grad, "table_grad")), _p(_f32(lse_out, "lse_out")), _p(workspace),
                        workspace.numel() * workspace.element_size(), _p(cdf), _p(_f32(logq, "logq")))
    L.call("cr_sampled_ce", C.byref(d), _stream())


def gbce_workspace_bytes(M, N, D):
    n = L.lib.cr_gbce_workspace(M, N, D)
    if n == 0:
        raise ValueError("cr_gbce: unsupported shape M=%d N=%d D=%d (M >= 1, 1 <= N <= %d, 8 <= D <= 256)"
                         % (M, N, D, L.CR_SCE_MAX_SAMPLES))
    return n


def gbce(seq_emb, ld, table, pos, state, workspace, M, N, beta=1.0, precision=L.PREC_BF16X3, neg=None, samples=None, seed=0, step=None,
         samples_out=None, d_seq_emb=None, ldd=0, table_grad=None, loss_out=None):
    """cr_gbce: gSASRec's generalised binary cross-entropy over each row's target (weight beta in (0, 1]) and N shared sample ids.
    Arguments as sampled_ce; loss_out float32 [M] takes each row's loss where given; workspace a uint8 CUDA tensor of at least
    gbce_workspace_bytes(M, N, D) bytes."""
    d = L.GbceDesc(_p(_f32(seq_emb, "seq_emb")), ld, _p(_f32(table, "table")), _p(_i32(pos, "pos")), _p(_i32(neg, "neg")),
                   M, table.shape[1], table.shape[0], N, precision, float(beta), _p(_i32(samples, "samples")), int(seed) & 0xFFFFFFFF,
                   _p(step), _p(_i32(samples_out, "samples_out")), _p(_f32(state, "state")), _p(_f32(d_seq_emb, "d_seq_emb")),
                   ldd, _p(_f32(table_grad, "table_grad")), _p(_f32(loss_out, "loss_out")), _p(workspace),
                   workspace.numel() * workspace.element_size())
    L.call("cr_gbce", C.byref(d), _stream())


def adam_step(p, m, v, table_grad, dense_slabs, n_table, n_dense, n_slabs, lr, state, beta1=0.9, beta2=0.98, eps=1e-8,
              stats=None, step_snapshot=None, lazy_ids=None, lazy_rows=0, lazy_D=0, lazy_flags=None, l2=0.0, n_l2=0,
              slab_counts=None, ids_ring=None, ids_ring_slots=0, ids_slot_elems=0, ids_dst=None, ids_copy_elems=0, tg=None,
              lazy_ids2=None):
    """cr_adam_step (castrec.h cr_adam_desc).  l2 / n_l2: the embedding regulariser on the first n_l2 parameters; slab_counts: int32
    [ceil(n_dense / 256)]; ids_ring .. ids_copy_elems: the id ring whose next slot this launch moves to ids_dst; tg: an L.TgradDesc
    (the table section's gradient from the occurrence index; table_grad may then be None); lazy_ids2: a second int32 device list of
    rows for the row-sparse update (with lazy_ids only)."""
    d = L.AdamDesc(_p(p), _p(m), _p(v), _p(table_grad), _p(dense_slabs), n_table, n_dense, n_slabs, lr, beta1, beta2,
                   eps, _p(state), _p(stats) if stats is not None else None,
                   _p(step_snapshot) if step_snapshot is not None else None, float(l2), int(n_l2),
                   _p(lazy_ids), 0 if lazy_ids is None else lazy_ids.numel(), lazy_rows, lazy_D, _p(lazy_flags),
                   _p(_i32(slab_counts, "slab_counts")), _p(_i32(ids_ring, "ids_ring")), int(ids_ring_slots), int(ids_slot_elems),
                   _p(_i32(ids_dst, "ids_dst")), int(ids_copy_elems))
    if tg is not None:
        d.tg = C.pointer(tg)
    if lazy_ids2 is not None:
        d.lazy_ids2, d.n_lazy_ids2 = _p(_i32(lazy_ids2, "lazy_ids2")), lazy_ids2.numel()
    L.call("cr_adam_step", C.byref(d), _stream())


def reduce_slabs(dense_slabs, n_slabs, n_dense, out, state=None, stats_out=None, slab_counts=None):
    """cr_reduce_slabs: out[i] = sum of the first slab_counts[i // 256] (default n_slabs) slabs of column i; state[0..2] -> stats_out."""
    L.call("cr_reduce_slabs", _p(_f32(dense_slabs, "dense_slabs")), n_slabs, n_dense, _p(_f32(out, "out")), _p(state), _p(stats_out),
           _p(_i32(slab_counts, "slab_counts")), _stream())


def l2_penalty(p, n, scale, state):
    """cr_l2_penalty: state[7] = scale * sum(p[:n] ** 2)."""
    L.call("cr_l2_penalty", _p(_f32(p, "p")), int(n), float(scale), _p(_f32(state, "state")), _stream())


class Graph:
    """HIP graph of one captured step (cr_graph_*)."""

    def __init__(self):
        self.exec = C.c_void_p()

    def begin(self):
        L.call("cr_graph_begin", _stream())

    def end(self):
        L.call("cr_graph_end", _stream(), C.byref(self.exec))

    def launch(self):
        L.call("cr_graph_launch", self.exec, _stream())

    def __del__(self):
        try:
            if self.exec:
                L.lib.cr_graph_destroy(self.exec)
        except Exception:
            pass

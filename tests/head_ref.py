"""fp64 reference of the prediction head (sasrec.py:87-115) behind the stack's final LayerNorm (sasrec.py:85), by torch autograd: what
cr_head_fwd_bwd and cr_head_fwd_bwd_ln (csrc/cr_head.hip) are tested against in tests/test_head_gpu.py.  Pure CPU.

Rows x; s = gamma * (x - mean) / sqrt(var + eps) + beta (eps inside the root); pl = s . E[pos], nl = s . E[neg] on a table whose row 0
reads as zeros; loss_sum = sum over rows with pos != 0 of -log(sigmoid(pl) + 1e-24) - log(1 - sigmoid(nl) + 1e-24).  The gradients are
those of loss_sum (un-normalised: the kernels leave the division by n_target to cr_adam_step)."""
import functools
import types

import numpy as np
import torch

V = 97
EPS = 1e-8


def make_ids(rs, M, distinct):
    """pos / neg ids with every kind of row: padding (pos = 0, with and without neg = 0), pos != 0 with neg = 0, ordinary; distinct: the
    non-zero ids are pairwise distinct (the table scatter is then free of float-atomic ordering), else ids repeat (2 M > V, and rows 3 / 4
    name each other's ids)."""
    if distinct:
        assert 2 * M < V
        ids = (1 + rs.permutation(V - 1))[:2 * M].astype(np.int32)
        pos, neg = ids[:M].copy(), ids[M:].copy()
    else:
        pos = rs.randint(1, V, M).astype(np.int32); neg = rs.randint(1, V, M).astype(np.int32)
        pos[3], neg[3] = neg[4], pos[4]
        pos[7:M - 1:11] = 0                              # padding rows inside every wave's share; the last row stays a real one
        neg[7:M - 1:22] = 0
        neg[5:M - 1:13] = 0
    pos[0] = 0; neg[0] = 0
    pos[1] = 0
    neg[2] = 0
    return pos, neg


@functools.lru_cache(maxsize=None)
def problem(M, D, seed=0):
    """Inputs (fp32-exact float64 arrays, int32 ids) and wanted outputs of one shape; cached: the tests share it and must not write to it."""
    rs = np.random.RandomState(1000 * D + M + seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = f32(2.0 * rs.standard_normal((M, D)) + 0.5)
    gamma = f32(1.0 + 0.1 * rs.standard_normal(D)); beta = f32(0.1 * rs.standard_normal(D))
    table = f32(rs.standard_normal((V, D)) / np.sqrt(D))  # |logit| stays below ~4: at +-20 fp32's 1 - sigmoid(nl) is 0 and no fp32 kernel follows fp64
    pos, neg = make_ids(rs, M, distinct=2 * M < V)
    xt, gt, bt = (torch.tensor(a, requires_grad=True) for a in (x, gamma, beta))
    mean = xt.mean(-1, keepdim=True); var = ((xt - mean) ** 2).mean(-1, keepdim=True)
    s_exact = gt * ((xt - mean) / (var + EPS) ** 0.5) + bt
    ln = _head(s_exact, table, pos, neg)
    ln.loss_t.backward()
    ln.dx, ln.dgamma, ln.dbeta = xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
    # the kernels READ seq_emb: the reference's rows rounded to fp32.  cr_head_fwd_bwd (no LayerNorm part) is judged on exactly those rows
    s = f32(s_exact.detach().numpy())
    plain = _head(torch.tensor(s, requires_grad=True), table, pos, neg)
    plain.loss_t.backward()
    for r in (ln, plain):
        r.d_seq_emb, r.table_grad = r.s_t.grad.numpy(), r.tab_t.grad.numpy()
        r.coef = np.stack([r.pl_t.grad.numpy(), r.nl_t.grad.numpy()])
        r.pl, r.nl, r.loss = r.pl_t.detach().numpy(), r.nl_t.detach().numpy(), float(r.loss_t.detach())
        for a in ("s_t", "tab_t", "pl_t", "nl_t", "loss_t"):
            delattr(r, a)
    return types.SimpleNamespace(M=M, D=D, x=x, gamma=gamma, beta=beta, table=table, pos=pos, neg=neg, s=s, ln=ln, plain=plain,
                                 distinct=2 * M < V)


def _head(s_t, table, pos, neg):
    D = table.shape[1]
    if not s_t.is_leaf:
        s_t.retain_grad()
    tab_t = torch.tensor(table, requires_grad=True)
    tz = torch.cat([torch.zeros(1, D, dtype=torch.float64), tab_t[1:]], 0)
    pl_t = (tz[pos.astype(np.int64)] * s_t).sum(-1); nl_t = (tz[neg.astype(np.int64)] * s_t).sum(-1)
    pl_t.retain_grad(); nl_t.retain_grad()
    ist = torch.tensor((pos != 0).astype(np.float64))
    loss_t = ((-torch.log(torch.sigmoid(pl_t) + 1e-24) - torch.log(1 - torch.sigmoid(nl_t) + 1e-24)) * ist).sum()
    auc = float((((torch.sign(pl_t.detach() - nl_t.detach()) + 1) / 2) * ist).sum())
    return types.SimpleNamespace(s_t=s_t, tab_t=tab_t, pl_t=pl_t, nl_t=nl_t, loss_t=loss_t, auc=auc, n=float(ist.sum()))

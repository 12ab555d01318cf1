"""Plain fp64 numpy references, per-element bounds, case generators and CPU emulations for the four row phases of a transformer
block as include/castrec.h states them (cr_block_desc / cr_block_bwd_desc):
    qkv_fwd   q_in = LN1(x); k_valid = (sum_c x != 0); q_valid = (sum_c q_in != 0); Q = q_in Wq + bq; K = x Wk + bk; V = x Wv + bv
    ffn_fwd   f_in = LN2(o); hid = drop1(relu(f_in W1 + b1)); y = (drop2(hid W2 + b2) + f_in) * (mask_ids != 0)
              tail 1: the next block's qkv_fwd on y; tail 2: out[:, col_out : col_out + D] = LN(y; lnf)
    ffn_bwd   dy (hid, f_in, o, mask_ids) -> d_o, the slabs of dW2 db2 dW1 db1 dgamma2 dbeta2, attn_delta
    qkv_bwd   dqkv, d_o (dq_part) -> dx (written or accumulated, or scattered through the embedding backward) and the slabs of
              dWqkv dbqkv dgamma1 dbeta1
tests/test_block_rows_gpu.py holds all three kernel families to these -- the fp32 tile kernels of csrc/cr_block.hip (form "f32"), the
register-layout backward of csrc/cr_stack_bwd.hip and the wide kernels of csrc/cr_wide.hip (forms "x3" = bf16x3 and "bf16");
tests/test_block_rows_host.py checks the references against torch autograd, shows a CPU emulation of each arithmetic inside every
bound, and shows that named defects are not.

Every input is a float32 value widened (row_ops_ref.draw), so no input rounding enters a bound.  All constants are row_ops_ref's
(U, bound, ln_bound, R_EMBED_FWD, R_EMBED_G, R_EMBED_TABLE) and gemm_ref's (E_SPLIT, E_BF16, BF_ACC); none is added here.

A reference value travels with a per-element error array e: what a kernel that follows the stated arithmetic may be off by at that
point.  Each step pushes e through its absolute Jacobian and adds its own local allowance:
    product       v = a W (+ bias) (+ residual): e_out = e_a |W| (+ e_residual) + prod_local(S, Sp, n, K, r, form), the allowance of the
                  matching gemm_ref form (rows_bound): S the absolute sum, Sp its product part, n = K + bias + residual,
                  r = 1 + dropout
    relu, row mask   1-Lipschitz: e unchanged (zero in a masked row); the gate of the backward is read from the stored hid
    dropout       e times keep / (1 - rate), and one more rounding (r)
    LayerNorm     forward and backward are the same linear map of their argument; with d = the incoming error (times |gamma| in
                  the backward)  e_out = rstd (d + mean d + |xhat| mean(d |xhat|))  (times |gamma| in the forward), plus
                  ln_bound(fp32 restatement, fp64) of the step itself
    weight gradient   dW = A^T G summed over the slabs in fp64: |A|^T e_G + e_A^T |G| + gemm_ref.wgrad_bound(n = M rows)
    column sums   db, dbeta: sum_m e + bound(S, M, 0) (the db rows of gemm_ref.wgrad_bound in the bf16 forms);
                  dgamma = sum_m dy xhat: sum_m e |xhat| + sum_m |dy| ln_bound(row of xhat) (ln_dgamma_bound's envelope of the
                  addends) + bound(S, M, 1) for the products and the sum
A forward stage is also checked on its own: against the fp64 result computed from the kernel's own stored previous stage, with the
local allowance alone (local_*).

k_valid / q_valid are compared as exact 0 / 1 with the flags the STORED rows decide (the fp64 sum of the float32 row the kernel read
or wrote is zero or not).  So every case is drawn with each row's fp64 sum -- of x, of q_in, of y and of the next block's q_in --
either exactly zero (a padding row: all zeros; its q_in is beta1, zero when beta1 is) or at least MARGIN = 100 times its own
summation bound, bound(sum |.|, D, 0), away from zero; a row that is not is drawn again (valid_margin; the host test asserts that
none is left), and a stored row whose sum an fp32 summation could move across zero is reported as a broken premise (decided)."""
import functools
import types

import numpy as np

import dropout_ref as dr
import gemm_ref as G
from row_ops_ref import (F64, LN_EPS, R_EMBED_G, R_EMBED_TABLE, U, _ids, _mask, bound, draw, layernorm_ref, ln_bound, pick_seed,
                         row_factor, wide)

MARGIN = 100.0
SITE1, SITE2, SITE_E, STEP = 3, 4, 9, 5
NS = types.SimpleNamespace


# ------------------------------------------------------------------------------------------------ building blocks
def prod_local(S, Sp, n, K, r, form):
    """gemm_ref.rows_bound on plain arrays"""
    if form == "f32":
        return bound(S, n, r)
    if form == "x3":
        return G.E_SPLIT * Sp + G.BF_ACC * bound((1 + 2.0 ** -7) * S, n + 2 * K, r)
    return (1 + 2.0 ** -8) * G.BF_ACC * bound(S, n, r) + G.E_BF16 * Sp


def wgrad_local(SW, Sb, M, form):
    """gemm_ref.wgrad_bound on plain arrays: (allowance of dW, of db)"""
    return G.wgrad_bound(NS(M=M), (None, SW, None, Sb), form)


def ln64(x, gamma, beta=None, dy=None):
    """row_ops_ref.layernorm_ref's closed form on fp64 arrays as they are (no cast through float32)"""
    x, gamma = np.asarray(x, F64), np.asarray(gamma, F64)
    xc = x - x.mean(1, keepdims=True)
    sd = np.sqrt((xc * xc).mean(1, keepdims=True) + LN_EPS)
    r = NS(xhat=xc / sd, rstd=1.0 / sd)
    r.y = gamma * r.xhat + (0.0 if beta is None else np.asarray(beta, F64))
    if dy is not None:
        dy = np.asarray(dy, F64)
        dg = dy * gamma
        r.dx = (dg - dg.mean(1, keepdims=True) - r.xhat * (dg * r.xhat).mean(1, keepdims=True)) / sd
        r.dgamma_terms = dy * r.xhat
        r.dgamma, r.dbeta = r.dgamma_terms.sum(0), dy.sum(0)
    return r


def ln32(x, gamma, beta=None, dy=None):
    """the same in np.float32, sums left to right: what ln_bound measures E with"""
    return layernorm_ref(x, gamma, np.zeros_like(np.asarray(gamma, np.float32)) if beta is None else beta, dy, fp32=True)


def ln_jac(d, r):
    """|d LN / d argument| applied to a non-negative error d (module docstring), without the gamma factor"""
    return r.rstd * (d + d.mean(1, keepdims=True) + np.abs(r.xhat) * (d * np.abs(r.xhat)).mean(1, keepdims=True))


def ln_fwd(x, e_x, gamma, beta):
    """(y, e_y, local, r64)"""
    r, r32 = ln64(x, gamma, beta), ln32(x, gamma, beta)
    local = np.broadcast_to(ln_bound(r32.y, r.y), r.y.shape)
    return r.y, np.abs(wide(gamma)) * ln_jac(e_x, r) + local, local, r


def ln_bwd(x, gamma, dy, e_dy):
    """LayerNorm backward at the exact input x: NS(dx, e_dx, dgamma, a_dgamma, dbeta, a_dbeta) with a_* the allowances of the column
    sums over all rows"""
    r, r32 = ln64(x, gamma, None, dy), ln32(x, gamma, None, dy)
    g = np.abs(wide(gamma))
    M = x.shape[0]
    e_dx = ln_jac(g * e_dy, r) + ln_bound(r32.dx, r.dx)
    a_dgamma = ((e_dy * np.abs(r.xhat)).sum(0) + (np.abs(dy) * ln_bound(r32.xhat, r.xhat)).sum(0)
                + bound(np.abs(r.dgamma_terms).sum(0), M, 1))
    a_dbeta = e_dy.sum(0) + bound(np.abs(dy).sum(0), M, 0)
    return NS(dx=r.dx, e_dx=e_dx, dgamma=r.dgamma, a_dgamma=a_dgamma, dbeta=r.dbeta, a_dbeta=a_dbeta, xhat=r.xhat)


def dense(a, e_a, W, b, form, f=None, relu=False, res=None, e_res=None, live=None, r=1):
    """(v, e, local): v = ((a W + b) relu) * f + res, zero in the rows that are not live"""
    a, W = np.asarray(a, F64), wide(W)
    K = W.shape[0]
    v, Sp, n = a @ W, np.abs(a) @ np.abs(W), K
    S = Sp.copy()
    if b is not None:
        v, S, n = v + wide(b), S + np.abs(wide(b)), n + 1
    if relu:
        v = np.maximum(v, 0.0)
    e = e_a @ np.abs(W)
    if f is not None:
        v, S, Sp, e = v * f, S * f, Sp * f, e * f
    if res is not None:
        v, S, n, e = v + res, S + np.abs(res), n + 1, e + e_res
    if live is not None:
        v, S, Sp, e = (np.where(live[:, None], t, 0.0) for t in (v, S, Sp, e))
    local = prod_local(S, Sp, n, K, r, form)
    return v, e + local, local


def wgrad(A, e_A, Gm, e_G, form):
    """NS(dW, a_dW, db, a_db): A^T G and colsum(G) over all rows with the allowances of their fp64 slab sums"""
    A, Gm = np.asarray(A, F64), np.asarray(Gm, F64)
    aW, ab = wgrad_local(np.abs(A).T @ np.abs(Gm), np.abs(Gm).sum(0), A.shape[0], form)
    return NS(dW=A.T @ Gm, a_dW=np.abs(A).T @ e_G + e_A.T @ np.abs(Gm) + aW, db=Gm.sum(0), a_db=e_G.sum(0) + ab)


def factors(c):
    """(f1, f2): [M, D] fp64 keep / (1 - rate) of the two feed-forward dropout sites; element index (row_offset + m) * D + col"""
    if c.rate == 0:
        one = np.ones((c.M, c.D), F64)
        return one, one
    s = float(dr.thresh_scale(c.rate)[1])
    return tuple(dr.rows_mask(c.seed, STEP, site, c.rate, c.M, c.D, c.row_offset).astype(F64) * s for site in (SITE1, SITE2))


# ------------------------------------------------------------------------------------------------ cases
def valid_margin(x, slack=1.0):
    """per row: the sum is exactly zero (every element is), or at least MARGIN * slack times its own summation bound away from it"""
    s, S = x.sum(1), np.abs(x).sum(1)
    return (np.abs(x).max(1) == 0) | (np.abs(s) >= MARGIN * slack * bound(S, x.shape[1], 0))


def decided(rows, what):
    """the flags (sum != 0) of stored float32 rows; the premise: no fp32 summation order can move a sum across zero"""
    r = wide(rows)
    assert valid_margin(r, 2.0 / MARGIN).all(), "%s: a stored row's sum is within its summation bound of zero" % what
    return (r.sum(1) != 0).astype(F64)


def _weights(rs, D):
    sc = D ** -0.5
    return NS(ln1_g=draw(rs, D, loc=1.0, scale=0.3), ln1_b=draw(rs, D, loc=0.25, scale=0.3), wqkv=draw(rs, D, 3 * D, scale=sc),
              bqkv=draw(rs, 3 * D, scale=0.3), ln2_g=draw(rs, D, loc=1.0, scale=0.3), ln2_b=draw(rs, D, loc=0.25, scale=0.3),
              w1=draw(rs, D, D, scale=sc), b1=draw(rs, D, scale=0.3), w2=draw(rs, D, D, scale=sc), b2=draw(rs, D, scale=0.3))


@functools.lru_cache(maxsize=None)
def block_case(D, M, rate=0.0, row_offset=0, beta1_zero=False, T=0):
    """One block and everything its four phases read.  Rows with mask_ids == 0 are padding: x is all-zero there.  `next` holds the
    weights of the block behind it (tail 1), lnf_* the final LayerNorm (tail 2).  The backward inputs hid, f_in, q_in, y are the fp64
    forward results rounded to float32; dy, dqkv, d_o_in, dq_part, dx0 are free draws.  T > 0: an embedding recipe `emb` that composes
    x (M % T == 0), with a positional table and an addend."""
    rs = np.random.RandomState((7919 * D + 104729 * M + int(rate * 10) + row_offset + 2 * beta1_zero + 31 * T) % 2 ** 31)
    c = NS(D=D, M=M, rate=rate, row_offset=row_offset, seed=0, T=T, **_weights(rs, D).__dict__)
    c.next = _weights(rs, D)
    c.lnf_g, c.lnf_b = draw(rs, D, loc=1.0, scale=0.3), draw(rs, D, loc=0.25, scale=0.3)
    if beta1_zero:
        c.ln1_b = np.zeros(D, np.float32)
    c.mask_ids = _mask(rs, M) if M > 1 else np.ones(1, np.int32)
    if rate > 0:
        c.seed = pick_seed(rate, M, D, STEP, SITE1, row_offset, 41)
    live = c.mask_ids != 0
    c.x, c.o = draw(rs, M, D), draw(rs, M, D, loc=0.2)
    c.x[~live] = 0
    zero = np.zeros((M, D), F64)
    for _ in range(200):                # draw again the rows whose sums are too close to zero for an exact 0 / 1 flag
        q_in, e_q, _, _ = ln_fwd(wide(c.x), zero, c.ln1_g, c.ln1_b)
        f = ffn_fwd_ref(c, "f32")
        q2, e_q2, _, _ = ln_fwd(f.y, f.e_y, c.next.ln1_g, c.next.ln1_b)
        bad_x = ~(valid_margin(wide(c.x), 2) & valid_margin(q_in, 2)) & live
        bad_o = ~(valid_margin(f.y, 2) & valid_margin(q2, 2)) & live
        dead_ok = (valid_margin(q_in, 2) | live).all() and (valid_margin(q2, 2) | live).all()
        if not (bad_x.any() or bad_o.any()) and dead_ok:
            break
        c.x[bad_x], c.o[bad_o] = draw(rs, int(bad_x.sum()), D), draw(rs, int(bad_o.sum()), D, loc=0.2)
        if not dead_ok:                 # a padding row's q_in is beta1 itself
            c.ln1_b[0] += np.float32(0.25) * (not beta1_zero)
            c.next.ln1_b[0] += np.float32(0.25)
    else:
        raise AssertionError("no draw with decidable row flags")
    q = qkv_fwd_ref(c, "f32")
    c.q_in, c.f_in, c.hid, c.y = (t.astype(np.float32) for t in (q.q_in, f.f_in, f.hid, f.y))
    c.dy, c.dqkv, c.d_o_in, c.dq_part, c.dx0 = draw(rs, M, D), draw(rs, 3, M, D), draw(rs, M, D), draw(rs, M, D), draw(rs, M, D)
    if T:
        assert M % T == 0
        V = 23
        c.emb = NS(M=M, T=T, D=D, V=V, ids=_ids(rs, M, V), table=draw(rs, V, D), zero_pad=1, scale=float(np.float32(D ** 0.5)),
                   pos=draw(rs, T, D), addend=draw(rs, M, D), ld_add=D, rate=rate, step=STEP, site=SITE_E, row_offset=row_offset,
                   seed=c.seed, mask_ids=c.mask_ids, col_off=0, ld_out=D)
    return c


# ------------------------------------------------------------------------------------------------ forward
def qkv_fwd_ref(c, form, x=None, e_x=None, w=None):
    """the pure fp64 chain from x (default: the case's) with propagated errors.  w: the weights (default: the block's own; c.next for
    tail 1).  NS(q_in, e_q_in, k_valid, q_valid, qkv [3, M, D], e_qkv)"""
    w = w or c
    x = wide(c.x) if x is None else x
    e_x = np.zeros_like(x) if e_x is None else e_x
    D = c.D
    q_in, e_q, _, _ = ln_fwd(x, e_x, w.ln1_g, w.ln1_b)
    parts = [dense(q_in if p == 0 else x, e_q if p == 0 else e_x, w.wqkv[:, p * D:(p + 1) * D], w.bqkv[p * D:(p + 1) * D], form) for p in range(3)]
    return NS(q_in=q_in, e_q_in=e_q, k_valid=(x.sum(1) != 0).astype(F64), q_valid=(q_in.sum(1) != 0).astype(F64),
              qkv=np.stack([p[0] for p in parts]), e_qkv=np.stack([p[1] for p in parts]))


def local_qkv_fwd(c, form, x, q_in, w=None):
    """each stored stage against the fp64 step from the stored stage before it: x (what the kernel read or composed) and q_in (what
    it stored), both float32.  [(name, reference, allowance)], and the flags decided by the stored rows"""
    w = w or c
    D = c.D
    ref, _, loc, _ = ln_fwd(wide(x), np.zeros((c.M, D)), w.ln1_g, w.ln1_b)
    out = [("q_in", ref, loc)]
    for p, name in enumerate("QKV"):
        v, _, loc = dense(wide(q_in if p == 0 else x), np.zeros((c.M, D)), w.wqkv[:, p * D:(p + 1) * D], w.bqkv[p * D:(p + 1) * D], form)
        out.append((name, v, loc))
    return out


def ffn_fwd_ref(c, form, o=None):
    """NS(f_in, e_f_in, hid, e_hid, y, e_y): the pure fp64 chain from o"""
    o = wide(c.o) if o is None else o
    f1, f2 = factors(c)
    r = 1 + (c.rate > 0)
    live = c.mask_ids != 0
    f_in, e_f, _, _ = ln_fwd(o, np.zeros_like(o), c.ln2_g, c.ln2_b)
    hid, e_h, _ = dense(f_in, e_f, c.w1, c.b1, form, f=f1, relu=True, r=r)
    y, e_y, _ = dense(hid, e_h, c.w2, c.b2, form, f=f2, res=f_in, e_res=e_f, live=live, r=r)
    return NS(f_in=f_in, e_f_in=e_f, hid=hid, e_hid=e_h, y=y, e_y=e_y)


def local_ffn_fwd(c, form, f_in, hid):
    """[(name, reference, allowance)] of f_in, hid, y from o, the stored f_in and the stored hid"""
    f1, f2 = factors(c)
    r = 1 + (c.rate > 0)
    z = np.zeros((c.M, c.D))
    ref, _, loc, _ = ln_fwd(wide(c.o), z, c.ln2_g, c.ln2_b)
    h, _, hl = dense(wide(f_in), z, c.w1, c.b1, form, f=f1, relu=True, r=r)
    y, _, yl = dense(wide(hid), z, c.w2, c.b2, form, f=f2, res=wide(f_in), e_res=z, live=c.mask_ids != 0, r=r)
    return [("f_in", ref, loc), ("hid", h, hl), ("y", y, yl)]


def final_ln_ref(c, y, e_y):
    """tail 2: (out, e_out, local)"""
    out, e, loc, _ = ln_fwd(y, e_y, c.lnf_g, c.lnf_b)
    return out, e, loc


# ------------------------------------------------------------------------------------------------ backward
def ffn_bwd_ref(c, form, dy, hid, f_in, heads=0, q_in=None, lnf=None):
    """hid, f_in: what the forward stored (fp64 arrays; the gate is hid > 0).  lnf = (y, gamma): the `_ln` form, dy is then the
    gradient of LN(y; lnf) and the final LayerNorm's backward comes first (its dgamma / dbeta are returned as lnf_*).
    heads > 0: attn_delta [heads, M] over each head's columns of d_o * (o - q_in).  NS of values, e_* errors, a_* slab allowances."""
    D, M = c.D, c.M
    f1, f2 = factors(c)
    dr_ = int(c.rate > 0)
    live = (c.mask_ids != 0)[:, None]
    dy, hid, f_in, o = (np.asarray(t, F64) for t in (dy, hid, f_in, wide(c.o)))
    R = NS()
    e_dy = np.zeros_like(dy)
    if lnf is not None:
        n = ln_bwd(np.asarray(lnf[0], F64), lnf[1], dy, e_dy)
        dy, e_dy = n.dx, n.e_dx
        R.lnf_dgamma, R.a_lnf_dgamma, R.lnf_dbeta, R.a_lnf_dbeta = n.dgamma, n.a_dgamma, n.dbeta, n.a_dbeta
    g2 = np.where(live, dy, 0.0) * f2
    e_g2 = np.where(live, e_dy, 0.0) * f2 + bound(np.abs(g2), 0, dr_)
    w2 = wgrad(hid, np.zeros_like(hid), g2, e_g2, form)
    gate = hid > 0
    s1 = float(dr.thresh_scale(c.rate)[1]) if c.rate > 0 else 1.0
    W2t, W1t = wide(c.w2).T, wide(c.w1).T
    dh, S = g2 @ W2t, np.abs(g2) @ np.abs(W2t)
    e_dh = e_g2 @ np.abs(W2t) + prod_local(S, S, D, D, 1, form)
    g1 = np.where(gate, dh * s1, 0.0)
    e_g1 = np.where(gate, e_dh * s1, 0.0) + bound(np.abs(g1), 0, dr_)
    w1 = wgrad(f_in, np.zeros_like(f_in), g1, e_g1, form)
    res = np.where(live, dy, 0.0)
    df, Sp = g1 @ W1t + res, np.abs(g1) @ np.abs(W1t)
    e_df = e_g1 @ np.abs(W1t) + np.where(live, e_dy, 0.0) + prod_local(Sp + np.abs(res), Sp, D + 1, D, 1, form)
    n = ln_bwd(o, c.ln2_g, df, e_df)
    R.__dict__.update(d_o=n.dx, e_d_o=n.e_dx, g_w2=w2.dW, a_g_w2=w2.a_dW, g_b2=w2.db, a_g_b2=w2.a_db, g_w1=w1.dW, a_g_w1=w1.a_dW,
                      g_b1=w1.db, a_g_b1=w1.a_db, g_ln2_g=n.dgamma, a_g_ln2_g=n.a_dgamma, g_ln2_b=n.dbeta, a_g_ln2_b=n.a_dbeta,
                      g2=g2, e_g2=e_g2, g1=g1, e_g1=e_g1)
    if heads:
        diff = o - np.asarray(q_in, F64)
        t, S = n.dx * diff, np.abs(n.dx) * (np.abs(o) + np.abs(np.asarray(q_in, F64)))
        hd = D // heads
        R.attn_delta = t.reshape(M, heads, hd).sum(2).T
        R.e_attn_delta = ((n.e_dx * np.abs(diff)).reshape(M, heads, hd).sum(2) + bound(S.reshape(M, heads, hd).sum(2), hd, 2)).T
    return R


def scatter_ref(e, dx, e_dx, want_pos, want_table, want_addend):
    """row_ops_ref.embed_bwd_ref (large-table mode, tables zero on entry) on an fp64 gradient that carries an error: g = dx * mask *
    keep / (1 - rate); d_addend = g; pos_grad[t] = sum_b g; table_grad[id] = sum scale * g (id 0 skipped).  dict of (value, allowance)"""
    M, D, T = e.M, e.D, e.T
    f = row_factor(e, M, D)
    g, e_g = dx * f, e_dx * f + bound(np.abs(dx * f), 0, R_EMBED_G)
    res = {}
    if want_addend:
        res["d_addend"] = (g, e_g)
    if want_pos:
        B = M // T
        res["pos_grad"] = (g.reshape(B, T, D).sum(0), e_g.reshape(B, T, D).sum(0) + bound(np.abs(g).reshape(B, T, D).sum(0), B, R_EMBED_G))
    if want_table:
        live = e.ids != 0
        tg, tS, tE = np.zeros((e.V, D)), np.zeros((e.V, D)), np.zeros((e.V, D))
        np.add.at(tg, e.ids[live], g[live] * e.scale)
        np.add.at(tS, e.ids[live], np.abs(g[live]) * e.scale)
        np.add.at(tE, e.ids[live], e_g[live] * e.scale)
        cnt = np.bincount(e.ids[live], minlength=e.V).astype(F64)[:, None]
        res["table_grad"] = (tg, tE + bound(tS, cnt, R_EMBED_TABLE))
    return res


def qkv_bwd_ref(c, form, dqkv, d_o, q_in, dq_part=None, dx0=None, e_d_o=None):
    """q_in: what the forward stored.  d_o with its error when it comes from ffn_bwd_ref.  NS(dx, e_dx, dq_in, e_dq_in (what the wide
    form leaves in d_o), g_wqkv [D, 3D], g_bqkv [3D], g_ln1_g, g_ln1_b and their a_*)"""
    D, M = c.D, c.M
    dqkv, d_o, q_in, x = (np.asarray(t, F64) for t in (dqkv, d_o, q_in, c.x))
    z = np.zeros((M, D))
    e_d_o = z if e_d_o is None else e_d_o
    dQ, e_dQ = dqkv[0], z
    if dq_part is not None:
        dQ = dQ + wide(dq_part)
        e_dQ = bound(np.abs(dqkv[0]) + np.abs(wide(dq_part)), 1, 0)
    W = wide(c.wqkv)
    Wq, Wk, Wv = (W[:, p * D:(p + 1) * D] for p in range(3))
    gq, gk, gv = wgrad(q_in, z, dQ, e_dQ, form), wgrad(x, z, dqkv[1], z, form), wgrad(x, z, dqkv[2], z, form)
    Sp = np.abs(dQ) @ np.abs(Wq).T
    dq_in = dQ @ Wq.T + d_o
    e_dq_in = e_dQ @ np.abs(Wq).T + e_d_o + prod_local(Sp + np.abs(d_o), Sp, D + 1, D, 1, form)
    Sp = np.abs(dqkv[1]) @ np.abs(Wk).T + np.abs(dqkv[2]) @ np.abs(Wv).T
    dxp, e_dxp = dqkv[1] @ Wk.T + dqkv[2] @ Wv.T, prod_local(Sp, Sp, 2 * D, 2 * D, 1, form)
    n = ln_bwd(x, c.ln1_g, dq_in, e_dq_in)
    terms = [n.dx, dxp] + ([wide(dx0)] if dx0 is not None else [])
    dx = sum(terms)
    e_dx = n.e_dx + e_dxp + bound(sum(np.abs(t) for t in terms), len(terms), 0)
    return NS(dx=dx, e_dx=e_dx, dq_in=dq_in, e_dq_in=e_dq_in,
              g_wqkv=np.concatenate([gq.dW, gk.dW, gv.dW], 1), a_g_wqkv=np.concatenate([gq.a_dW, gk.a_dW, gv.a_dW], 1),
              g_bqkv=np.concatenate([gq.db, gk.db, gv.db]), a_g_bqkv=np.concatenate([gq.a_db, gk.a_db, gv.a_db]),
              g_ln1_g=n.dgamma, a_g_ln1_g=n.a_dgamma, g_ln1_b=n.dbeta, a_g_ln1_b=n.a_dbeta)


# ------------------------------------------------------------------------------------------------ the arithmetic, emulated
f32 = np.float32
DEFECTS = ("neighbour_column", "bias_row", "drop_index_64", "mean_64", "no_al_bh", "skip_partial_tile")


def _emu_ln(x, gamma, beta, dy=None, defect=None):
    if defect != "mean_64":
        return ln32(x, gamma, beta, dy)
    x, gamma = np.asarray(x, f32), np.asarray(gamma, f32)                 # the mean formed as sum / 64 (the tile's width)
    xc = x - (x.sum(1, keepdims=True) / f32(64)).astype(f32)
    sd = np.sqrt((xc * xc).sum(1, keepdims=True) / f32(64) + f32(LN_EPS)).astype(f32)
    r = NS(xhat=xc / sd)
    r.y = gamma * r.xhat + (f32(0) if beta is None else np.asarray(beta, f32))
    if dy is not None:
        dg = np.asarray(dy, f32) * gamma
        r.dx = (dg - dg.sum(1, keepdims=True) / f32(64) - r.xhat * ((dg * r.xhat).sum(1, keepdims=True) / f32(64))) / sd
        r.dgamma, r.dbeta = (np.asarray(dy, f32) * r.xhat).sum(0), np.asarray(dy, f32).sum(0)
    return r


def _emu_w(W, defect):
    """the weight image a kernel stages: with `neighbour_column` the last column (the one a shifted-back 16-byte chunk holds when
    D % 4 != 0) is read one column to the left"""
    W = np.asarray(W, f32)
    if defect == "neighbour_column":
        W = W.copy()
        W[:, -1] = W[:, -2]
    return W


def _emu_mm(a, b, form, defect=None):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if defect == "no_al_bh" and form == "x3":
        (ah, al), (bh, bl) = G.split(a), G.split(b)
        return (ah @ bl + ah @ bh).astype(f32)
    return G.emu_product(a, b, form)


def _emu_factors(c, defect):
    if defect == "drop_index_64" and c.rate > 0:
        s = f32(dr.thresh_scale(c.rate)[1])
        return tuple(dr.rows_mask(c.seed, STEP, site, c.rate, c.M, 64, c.row_offset)[:, :c.D].astype(f32) * s for site in (SITE1, SITE2))
    return tuple(t.astype(f32) for t in factors(c))


def emu_qkv_fwd(c, form, defect=None, w=None, x=None):
    """NS(q_in, k_valid, q_valid, qkv) float32: LayerNorm in fp32, the projections as the form's product, + bias in fp32"""
    w = w or c
    D = c.D
    x = np.asarray(c.x if x is None else x, f32)
    ln = _emu_ln(x, w.ln1_g, w.ln1_b, defect=defect)
    q_in = ln.y.astype(f32)
    W = w.wqkv
    qkv = np.stack([_emu_mm(q_in if p == 0 else x, _emu_w(W[:, p * D:(p + 1) * D], defect), form, defect) + w.bqkv[p * D:(p + 1) * D] for p in range(3)])
    ssum = lambda a: np.add.accumulate(a, axis=1, dtype=f32)[:, -1]
    return NS(q_in=q_in, qkv=qkv.astype(f32), k_valid=(ssum(x) != 0).astype(f32), q_valid=(ssum(q_in) != 0).astype(f32))


def emu_ffn_fwd(c, form, defect=None):
    """NS(f_in, hid, y) float32, statement by statement as k_block_ln_ffn_fwd"""
    f1, f2 = _emu_factors(c, defect)
    f_in = _emu_ln(c.o, c.ln2_g, c.ln2_b, defect=defect).y.astype(f32)
    hid = np.maximum(_emu_mm(f_in, _emu_w(c.w1, defect), form, defect) + c.b1, f32(0)) * f1
    y = ((_emu_mm(hid, _emu_w(c.w2, defect), form, defect) + c.b2) * f2 + f_in) * (c.mask_ids != 0)[:, None].astype(f32)
    return NS(f_in=f_in, hid=hid.astype(f32), y=y.astype(f32))


def _emu_wgrad(A, Gm, n_slabs, form, defect):
    """(dW slabs, db slabs) float32 over gemm_ref.slab_rows; `skip_partial_tile`: a slab's rows behind its last full 64-row tile are
    left out; `bias_row`: db is row D - 1 of dW (the row in front of the ones row)"""
    M, K = A.shape
    dW, db = np.zeros((n_slabs, K, Gm.shape[1]), f32), np.zeros((n_slabs, Gm.shape[1]), f32)
    for s, (m0, m1) in enumerate(G.slab_rows(M, n_slabs)):
        if defect == "skip_partial_tile":
            m1 = m0 + (m1 - m0) // 64 * 64
        if m0 >= m1:
            continue
        dW[s] = _emu_mm(A[m0:m1].T, Gm[m0:m1], form, defect)
        db[s] = dW[s][K - 1] if defect == "bias_row" else _emu_mm(np.ones((1, m1 - m0), f32), Gm[m0:m1], form, defect)[0]
    return dW, db


def _emu_ln_slabs(x, gamma, dy, n_slabs, defect):
    M, D = x.shape
    dg, db = np.zeros((n_slabs, D), f32), np.zeros((n_slabs, D), f32)
    dx = np.zeros((M, D), f32)
    for s, (m0, m1) in enumerate(G.slab_rows(M, n_slabs)):
        if m0 < m1:
            r = _emu_ln(x[m0:m1], gamma, None, dy[m0:m1], defect)
            dx[m0:m1], dg[s], db[s] = r.dx, r.dgamma, r.dbeta
    return dx, dg, db


def emu_ffn_bwd(c, form, n_slabs, dy, hid, f_in, q_in=None, defect=None, heads=1, lnf=None):
    """the feed-forward backward's steps in float32: NS(d_o, attn_delta [heads, M], and [n_slabs, ...] slabs g_w2 g_b2 g_w1 g_b1
    g_ln2_g g_ln2_b); lnf = (y, gamma): the final LayerNorm's backward first (slabs lnf_dgamma, lnf_dbeta)"""
    _, f2 = _emu_factors(c, defect)
    dy, hid, f_in = (np.asarray(t, f32) for t in (dy, hid, f_in))
    if lnf is not None:
        dy, lnf_dg, lnf_db = _emu_ln_slabs(np.asarray(lnf[0], f32), lnf[1], dy, n_slabs, defect)
    live = (c.mask_ids != 0)[:, None].astype(f32)
    s1 = f32(dr.thresh_scale(c.rate)[1]) if c.rate > 0 else f32(1)
    g2 = dy * live * f2
    g_w2, g_b2 = _emu_wgrad(hid, g2, n_slabs, form, defect)
    g1 = np.where(hid > 0, _emu_mm(g2, _emu_w(c.w2, defect).T, form, defect) * s1, f32(0)).astype(f32)
    g_w1, g_b1 = _emu_wgrad(f_in, g1, n_slabs, form, defect)
    df = (_emu_mm(g1, _emu_w(c.w1, defect).T, form, defect) + dy * live).astype(f32)
    d_o, dg, db = _emu_ln_slabs(c.o, c.ln2_g, df, n_slabs, defect)
    R = NS(d_o=d_o, g_w2=g_w2, g_b2=g_b2, g_w1=g_w1, g_b1=g_b1, g_ln2_g=dg, g_ln2_b=db)
    if lnf is not None:
        R.lnf_dgamma, R.lnf_dbeta = lnf_dg, lnf_db
    if q_in is not None:
        t = (d_o * (c.o - np.asarray(q_in, f32))).reshape(c.M, heads, c.D // heads)
        R.attn_delta = np.add.accumulate(t, axis=2, dtype=f32)[:, :, -1].T
    return R


def emu_qkv_bwd(c, form, n_slabs, dqkv, d_o, q_in, dq_part=None, dx0=None, defect=None):
    D = c.D
    dqkv, d_o, q_in = (np.asarray(t, f32) for t in (dqkv, d_o, q_in))
    dQ = dqkv[0] + dq_part if dq_part is not None else dqkv[0]
    W = [_emu_w(c.wqkv[:, p * D:(p + 1) * D], defect) for p in range(3)]
    gw = [_emu_wgrad(q_in if p == 0 else c.x, dQ if p == 0 else dqkv[p], n_slabs, form, defect) for p in range(3)]
    dq_in = (_emu_mm(dQ, W[0].T, form, defect) + d_o).astype(f32)
    dxp = _emu_mm(np.concatenate([dqkv[1], dqkv[2]], 1), np.concatenate([W[1].T, W[2].T], 0), form, defect)     # one accumulator chain
    ln_dx, dg, db = _emu_ln_slabs(c.x, c.ln1_g, dq_in, n_slabs, defect)
    dx = ln_dx + dxp
    if dx0 is not None:
        dx = dx + dx0
    return NS(dx=dx.astype(f32), g_wqkv=np.concatenate([g[0] for g in gw], 2), g_bqkv=np.concatenate([g[1] for g in gw], 1), g_ln1_g=dg, g_ln1_b=db)


# ------------------------------------------------------------------------------------------------ the cases of the tile family
TILE_D = [4, 5, 6, 7, 8, 20, 33, 50, 63, 64]
TILE_M = [1, 15, 16, 17, 63, 64, 65, 130, 200]
DROPS = [(0.0, 0), (0.3, 0), (0.3, 900), (0.0, 900)]
# (M, n_slabs): one tile group per workgroup (rows per slab <= 64) and two (> 64: 130 = two tiles and 2 rows, 200 = 100 + 100, 65 = a
# tile and a row), slabs without rows ((5, 8): rows per slab 1, three empty; (130, 3): 44 + 44 + 42; (17, 4): 5 + 5 + 5 + 2)
TILE_SLABS = [(130, 1), (130, 3), (200, 2), (5, 8), (64, 1), (65, 1), (1, 1), (15, 2), (16, 1), (17, 4), (63, 2)]


def tile_fwd_cases():
    """[(D, M, rate, row_offset)]: every D against three M, every M against at least three D"""
    out = []
    for i, D in enumerate(TILE_D):
        for j in range(3):
            M = TILE_M[(i + 3 * j + (j == 2)) % len(TILE_M)]
            out.append((D, M) + DROPS[(i + j) % 4])
    return out


def tile_bwd_cases():
    """[(D, M, n_slabs, rate, row_offset, variant)]: every D against four of TILE_SLABS; variant 0..7 = bit 0 dq_part given, bit 1
    dx_accumulate, bit 2 attn_delta given"""
    out = []
    for i, D in enumerate(TILE_D):
        for j in range(4):
            M, ns = TILE_SLABS[(3 * i + 4 * j) % len(TILE_SLABS)]
            out.append((D, M, ns) + DROPS[(i + j) % 4] + ((i + 3 * j) % 8,))
    return out


def ng_of(M, n_slabs):
    """tile groups per workgroup (cr_block.hip, host side): two when a slab has more than 64 rows"""
    return 2 if -(-M // n_slabs) > 64 else 1


def kernel_of(entry, M=0, n_slabs=1, tail=0, scatter=None):
    """the kernel instantiation of csrc/cr_block.hip behind an entry point of the tile family"""
    if entry == "qkv_fwd":
        return "k_block_ln_qkv_fwd<false>"
    if entry == "qkv_fwd_gather":
        return "k_block_ln_qkv_fwd<true>"
    if entry == "ffn_fwd":
        return "k_block_ln_ffn_fwd<%d>" % tail
    if entry == "ffn_bwd":
        return "k_block_ln_ffn_bwd<%d>" % ng_of(M, n_slabs)
    assert entry == "qkv_bwd"
    return "k_block_ln_qkv_bwd<%d, %d>" % (ng_of(M, n_slabs), {None: 0, "table": 1, "pos": 2}[scatter])


@functools.lru_cache(maxsize=None)
def gather_case(D, M, T, rate, row_offset, extras):
    """block_case whose x is composed by the embedding recipe `emb` (row_ops_ref.embed_ref): with a positional table and an addend
    (extras) or the scaled table rows alone (an id 0 then gives an all-zero row).  x_ref, e_x: the composed input and its allowance.
    Rows whose flags would not be decidable get a new addend row (a new table row without extras)."""
    from row_ops_ref import R_EMBED_FWD, embed_ref
    c0 = block_case(D, M, rate, row_offset, False, T)
    c, e = NS(**c0.__dict__), NS(**c0.emb.__dict__)
    c.emb, e.table, e.addend = e, e.table.copy(), e.addend.copy()
    if not extras:
        e.pos, e.addend, e.ld_add = None, None, 0
    rs = np.random.RandomState(D + 64 * M + 3)
    for _ in range(200):
        x, S, n = embed_ref(e)
        e_x = bound(S, n, R_EMBED_FWD)
        q_in, e_q, _, _ = ln_fwd(x, e_x, c.ln1_g, c.ln1_b)
        bad = ~(valid_margin(x, 2) & valid_margin(q_in, 2))
        if not bad.any():
            break
        if extras:
            e.addend[bad] = draw(rs, int(bad.sum()), D)
        else:
            ids = np.unique(e.ids[bad])
            e.table[ids] = draw(rs, len(ids), D)
    else:
        raise AssertionError("no draw with decidable row flags")
    c.x_ref, c.e_x = x, e_x
    return c


# ------------------------------------------------------------------------------------------------ what a result is held to
def items_qkv_fwd(c, form, got, x_got=None, x=None, e_x=None, w=None):
    """[(name, got, reference, allowance)] of one qkv_fwd result got = NS(q_in, qkv, k_valid, q_valid): each stage from the stored
    stage before it (x_got: the float32 input the kernel read or stored), the chain from the exact input (x, e_x) and the flags"""
    x_got = c.x if x_got is None else x_got
    loc = local_qkv_fwd(c, form, x_got, got.q_in, w)
    out = [("q_in from x", got.q_in, loc[0][1], loc[0][2])]
    out += [("%s from the stored rows" % n, got.qkv[p], v, a) for p, (n, v, a) in enumerate(loc[1:])]
    ch = qkv_fwd_ref(c, form, x, e_x, w)
    out += [("q_in, chain", got.q_in, ch.q_in, ch.e_q_in), ("qkv, chain", got.qkv, ch.qkv, ch.e_qkv),
            ("k_valid", got.k_valid, decided(x_got, "x"), np.zeros(c.M)), ("q_valid", got.q_valid, decided(got.q_in, "q_in"), np.zeros(c.M))]
    return out


def items_ffn_fwd(c, form, got):
    """got = NS(f_in, hid, y)"""
    out = [("%s from the stored rows" % n, getattr(got, n), v, a) for n, v, a in local_ffn_fwd(c, form, got.f_in, got.hid)]
    ch = ffn_fwd_ref(c, form)
    return out + [("%s, chain" % n, getattr(got, n), getattr(ch, n), getattr(ch, "e_" + n)) for n in ("f_in", "hid", "y")]


def items_tail1(c, form, got_y, got_next):
    """tail 1: the next block's qkv_fwd on the stored y, and from the exact chain"""
    ch = ffn_fwd_ref(c, form)
    return items_qkv_fwd(c, form, got_next, x_got=got_y, x=ch.y, e_x=ch.e_y, w=c.next)


def items_tail2(c, form, got_y, got_out):
    ch = ffn_fwd_ref(c, form)
    out, e, _ = final_ln_ref(c, ch.y, ch.e_y)
    ref, _, loc = final_ln_ref(c, wide(got_y), np.zeros((c.M, c.D)))
    return [("out from the stored y", got_out, ref, loc), ("out, chain", got_out, out, e)]


FFN_SLABS = ("g_w2", "g_b2", "g_w1", "g_b1", "g_ln2_g", "g_ln2_b")
QKV_SLABS = ("g_wqkv", "g_bqkv", "g_ln1_g", "g_ln1_b")


def items_bwd(R, got, names, rows=()):
    """R: ffn_bwd_ref / qkv_bwd_ref; got: the same names, slabs [n_slabs, ...] float32 (summed here in fp64); rows: the row outputs
    (name, error field)"""
    out = [(n, np.asarray(getattr(got, n), F64).sum(0), getattr(R, n), getattr(R, "a_" + n)) for n in names]
    return out + [(n, getattr(got, n), getattr(R, n), getattr(R, e)) for n, e in rows]


def worst(items):
    """largest error / allowance over items (0 / 0 counts as 0), and the item's name"""
    top, name = 0.0, ""
    for n, got, ref, allow in items:
        err = np.abs(np.asarray(got, F64) - ref)
        w = float(np.nan_to_num(np.where(err == 0, 0.0, err / np.maximum(allow, 1e-300)), nan=np.inf).max()) if err.size else 0.0
        if w > top:
            top, name = w, n
    return top, name


BETA0_CASE = (50, 65, 0.0, 0, True)                # beta1 = 0: an all-zero row gives q_valid == 0 exactly
# (D, M, T, rate, row_offset, extras): x composed by the embedding recipe, with a positional table and an addend or without
GATHER_CASES = [(5, 15, 5, 0.3, 900, True), (50, 130, 10, 0.0, 0, True), (64, 64, 16, 0.3, 0, False), (33, 200, 50, 0.0, 0, False),
                (7, 17, 17, 0.3, 900, True), (20, 1, 1, 0.0, 0, False)]
# (D, M, T, n_slabs, scatter, d_addend): dx scattered into the table alone ("table") or the table and a learned positional table
# ("pos"); block_case(D, M, 0.3, 900, False, T)
SCATTER_CASES = [(5, 15, 5, 2, "table", False), (50, 130, 10, 1, "table", True), (50, 130, 10, 3, "pos", True), (64, 200, 50, 2, "pos", False),
                 (33, 65, 13, 1, "table", True), (63, 64, 16, 1, "pos", True)]
EXTRA_CASES = [BETA0_CASE] + [(D, M, 0.3, 900, False, T) for D, M, T, ns, s, a in SCATTER_CASES]
TILE_KERNELS = (["k_block_ln_qkv_fwd<false>", "k_block_ln_qkv_fwd<true>"] + ["k_block_ln_ffn_fwd<%d>" % t for t in (0, 1, 2)]
                + ["k_block_ln_ffn_bwd<%d>" % g for g in (1, 2)] + ["k_block_ln_qkv_bwd<%d, %d>" % (g, s) for g in (1, 2) for s in (0, 1, 2)])


# ------------------------------------------------------------------------------------------------ the register-layout backward
# csrc/cr_stack_bwd.hip: one workgroup per sequence, 16-row tiles in registers, two rounds of seven tiles; bf16x3 ("x3") / bf16
PREC_OF = {"x3": 1, "bf16": 2}
REG_D = [8, 9, 24, 33, 50, 63, 64]                 # 50 and 64 are constant instantiations, the others the run-time one
REG_T = [1, 15, 16, 17, 112, 113, 224]             # the tile of 16, the round of 7 tiles (112), a second round, the limit
REG_SLABS = ["1", "2", "B", "B+2"]


def reg_cases():
    """[(D, B, T, n_slabs, rate, row_offset, variant)]: every D against three T, every T against three D; variant 0 the plain entry,
    1 `_ln`, 2 `_heads` without the LayerNorm, 3 `_heads` with it (two heads at D = 64); bit 0 of it: dx_accumulate"""
    out = []
    for i, D in enumerate(REG_D):
        for j in range(3):
            T = REG_T[(i + 2 * j + (j == 2)) % len(REG_T)]
            B = (1, 3)[(i // 2 + j) % 2]
            ns = {"1": 1, "2": 2, "B": B, "B+2": B + 2}[REG_SLABS[(i + 3 * j) % 4]]
            out.append((D, B, T, ns) + DROPS[(i + j) % 4] + ((i + j) % 4,))
    return out + [(64, 3, 17, 2, 0.3, 900, 2), (64, 1, 113, 3, 0.0, 0, 3)]


# (D, B, T, n_slabs, scatter, d_addend)
REG_SCATTER = [(50, 3, 17, 2, "table", False), (64, 1, 113, 3, "pos", True), (9, 3, 16, 5, "table", True), (33, 1, 224, 1, "pos", False)]


def reg_rounds(T):
    return 2 if -(-T // 16) > 7 else 1


def reg_empty_slabs(B, T, n_slabs):
    """work items (sequence, round) are dealt to the workgroups in turn: slab s gets items s, s + n_slabs, ..."""
    return list(range(min(n_slabs, reg_rounds(T) * B), n_slabs))


def reg_kernel_of(entry, D, form):
    return "k_stack_%s_bwd<%s, %d>" % (entry, "true" if form == "x3" else "false", D if D in (50, 64) else 0)


# ------------------------------------------------------------------------------------------------ the wide family
# csrc/cr_wide.hip, D = 128 / 192 / 256: 128 rows per workgroup at D = 128 (and in the forward when that still fills the chip), else 64
WIDE_D = [128, 192, 256]
WIDE_M = [1, 63, 64, 65, 127, 128, 129, 300]
WIDE_BIG = (192, 32641)                            # ceil(M / 128) >= 256: the 8-wave forward form at D > 128


def wide_fwd_cases():
    """[(D, M, rate, row_offset)]: every M against two D, every D against five or six M"""
    return [(WIDE_D[(i + j) % 3], M) + DROPS[(i + j) % 4] for i, M in enumerate(WIDE_M) for j in range(2)]


def wide_bwd_cases():
    """[(D, M, n_slabs, rate, row_offset, own, heads, acc)]: own = the kernel forms the weight gradients itself (D = 128 only), else it
    returns g2, g1 and overwrites d_o; heads of attn_delta (0: NULL); dx_accumulate.  n_slabs 1, 2 (row blocks dealt in turn), and
    more than there are row blocks (slabs without rows)"""
    out = []
    for i, M in enumerate(WIDE_M):
        for j in range(2):
            D = WIDE_D[(i + j) % 3]
            h = (0, 1, 2, 4, 8)[(i + 2 * j) % 5]
            h = h // 2 if h and D % (16 * h) else h      # a head's width is a multiple of 16 columns (192 / 8 is not)
            out.append((D, M, (1, 2, 5)[(i + j) % 3]) + DROPS[(i + j) % 4] + (False, h, bool((i + j) % 2)))
    for i, M in enumerate(WIDE_M):                # D = 128 with its own weight gradients
        out.append((128, M, (2, 1, 4)[i % 3]) + DROPS[i % 4] + (True, (8, 4, 0, 2, 1)[i % 5], bool(i % 2)))
    return out


def wide_rows(D, fwd=False, M=0):
    return 128 if D == 128 or (fwd and -(-M // 128) >= 256) else 64


def wide_empty_slabs(D, M, n_slabs):
    return list(range(min(n_slabs, -(-M // wide_rows(D))), n_slabs))


def wide_kernel_of(entry, D, form, M=0, own=False, tail=0):
    sp = "true" if form == "x3" else "false"
    if entry.endswith("fwd"):
        mode = 0 if wide_rows(D, True, M) == 128 else 2
        return "k_wide_%s<%d, %s, %d%s>" % (entry, D // 16, sp, mode, ", %d" % tail if entry == "ffn_fwd" else "")
    return "k_wide_%s<%d, %s, %s>" % (entry, D // 16, sp, "true" if own else "false")


def wide_big():
    """(c, idx): M = 32641 rows at D = 192 (256 row blocks of 128: the 8-wave forward form), the 300 rows of block_case(192, 300)
    repeated -- the forward phases are row-local and the case has no dropout, so a row's reference does not depend on where it
    stands -- and the rows of the first, the last (one row) and three interior row blocks, which is what gets checked"""
    D, M = WIDE_BIG
    base = block_case(D, 300)
    rows = np.arange(M) % 300
    c = NS(**{**base.__dict__, "M": M, "x": base.x[rows], "o": base.o[rows], "mask_ids": base.mask_ids[rows]})
    idx = np.concatenate([np.arange(128 * b, min(M, 128 * (b + 1))) for b in (0, 77, 128, 200, 255)])
    return c, idx


def sub_case(c, idx):
    """the rows idx of a case without dropout as a case of their own"""
    assert c.rate == 0
    return NS(**{**c.__dict__, "M": len(idx), "x": c.x[idx], "o": c.o[idx], "mask_ids": c.mask_ids[idx]})

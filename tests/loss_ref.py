"""CPU side of the candidate-sweep losses' tests (cr_softmax_ce, cr_sampled_ce with either proposal, cr_gbce): the numpy restatement of
the device draw, the makers of the tests' inputs, the fp64 references of the two softmaxes with per-element bounds, and the one
per-element comparison.  numpy, torch (CPU) and dropout_ref only: importable without the native library and without a GPU.

The bounds are built from fp64 quantities only.  A score carries es = u * sum_i |h_mi E_vi| (u = 2^-15 for the three bf16 products,
2^-7 for plain bf16), carried through the p-weighted sums; gbce_ref.ref64 builds its own from the same es."""
import math

import numpy as np

from dropout_ref import M32, fmix32, site_key

SCE_SITE = 0x5CE00000
GBCE_SITE = 0x6BCE0000
PHI = 0x9E3779B1


# ---- the device draw ---------------------------------------------------------------------------------------------------------------
def hashes(seed, step, N, site):
    """key = cr_site_key(seed, step, site); x_j = cr_fmix32(key + j * CR_PHI)."""
    key = site_key(np.uint64(seed & 0xFFFFFFFF), np.uint64(step & 0xFFFFFFFF), np.uint64(site))
    j = np.arange(N, dtype=np.uint64)
    return fmix32((key + j * np.uint64(PHI)) & M32)


def draw(seed, step, V, N, site):
    """The uniform draw of cr_sampled_ce (SCE_SITE) and cr_gbce (GBCE_SITE): s_j = 1 + ((x_j * (V - 1)) >> 32)."""
    x = hashes(seed, step, N, site)
    return (1 + ((x * np.uint64(V - 1)) >> np.uint64(32))).astype(np.int32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def ce_case(D, V, M, seed):
    """h [M, D], table [V, D] (row 0 random too: it must not take part), ~30 % padded rows, repeated targets, one target V-1."""
    rs = np.random.RandomState(seed)
    h = rs.standard_normal((M, D)).astype(np.float32) * (1.5 / math.sqrt(D))
    E_ = rs.standard_normal((V, D)).astype(np.float32) * 1.5
    pos = rs.randint(1, V, M).astype(np.int32)
    pos[rs.rand(M) < 0.3] = 0
    live = np.flatnonzero(pos)
    if len(live) > 3:
        pos[live[1]] = pos[live[0]]                      # a repeated target
        pos[live[2]] = V - 1                             # the table's last row
    neg = rs.randint(1, V, M).astype(np.int32)
    neg[pos == 0] = 0
    return h, E_, pos, neg


def sampled_case(D, V, M, N, seed):
    """h [M, D], table [V, D], ~30 % padded rows, a repeated target, one target V-1; N samples with a duplicate and hits planted."""
    rs = np.random.RandomState(seed)
    h = rs.standard_normal((M, D)).astype(np.float32) * (1.5 / math.sqrt(D))
    E_ = rs.standard_normal((V, D)).astype(np.float32) * 1.5
    pos = rs.randint(1, V, M).astype(np.int32)
    pos[rs.rand(M) < 0.3] = 0
    live = np.flatnonzero(pos)
    if len(live) > 3:
        pos[live[1]] = pos[live[0]]
        pos[live[2]] = V - 1
    neg = rs.randint(1, V, M).astype(np.int32)
    neg[pos == 0] = 0
    s = rs.randint(1, V, N).astype(np.int32)
    if N > 1:
        s[1] = s[0]                                      # a duplicate
    if N > 2 and len(live):
        s[2] = pos[live[0]]                              # an accidental hit of two rows
    return h, E_, pos, neg, s


def batch(rs, B, T, itemnum, max_bins):
    seq = rs.randint(1, itemnum + 1, (B, T)); pos = rs.randint(1, itemnum + 1, (B, T)); neg = rs.randint(1, itemnum + 1, (B, T))
    for b in range(B):
        n = rs.randint(0, T - 2)
        seq[b, :n] = 0; pos[b, :n] = 0; neg[b, :n] = 0
    pos[1, -1] = itemnum                                         # the table's last row as a target
    time = rs.randint(0, max_bins + 1, (B, T)) * (seq != 0)
    time[:, -1] = 0
    hours = rs.randint(1, 25, (B, T)) * (seq != 0); days = rs.randint(1, 8, (B, T)) * (seq != 0)
    return seq, pos, neg, time, hours, days


def planted(rs, B, T, itemnum):
    """Sequences of consecutive items (item i is followed by item i + 1), left-padded to T."""
    seq = np.zeros((B, T), np.int64); pos = np.zeros((B, T), np.int64); neg = np.zeros((B, T), np.int64)
    for b in range(B):
        n = rs.randint(T // 2, T + 1)
        s = rs.randint(1, itemnum - n)
        seq[b, T - n:] = np.arange(s, s + n)
        pos[b, T - n:] = np.arange(s + 1, s + n + 1)
        neg[b, T - n:] = rs.randint(1, itemnum + 1, n)
    return seq, pos, neg


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def softmax_ref64(h, E_, pos, neg, bf16=False):
    """The full-catalogue softmax over items 1 .. V-1: fp64 results and per-element error bounds.  (A sweep of the whole table with no
    hit mask and other sums than sampled_softmax_ref64's: not bit-equal to it on samples = 1 .. V-1, so a function of its own.)"""
    u = 2.0 ** -7 if bf16 else 2.0 ** -15
    acc = 2.0 ** -7 if bf16 else 2.0 ** -14              # relative bound of the fp32 / bf16-operand sums of the gradients
    h = h.astype(np.float64)
    T = E_[1:].astype(np.float64)
    S = h @ T.T                                          # [M, V-1]
    es = u * (np.abs(h) @ np.abs(T).T)
    mx = S.max(1, keepdims=True)
    Z = np.exp(S - mx)
    lse = mx[:, 0] + np.log(Z.sum(1))
    P = Z / Z.sum(1, keepdims=True)
    ist = pos != 0
    rows = np.arange(len(pos))
    e_lse = (P * es).sum(1) + 2.0 ** -20 * (1.0 + np.abs(lse))
    G = P.copy()
    G[rows[ist], pos[ist] - 1] -= 1.0
    G[~ist] = 0.0
    dh = G @ T
    dE = np.zeros_like(E_, dtype=np.float64)
    dE[1:] = G.T @ h
    # |dp_mv| <= p_mv (es_mv + e_lse_m)
    W = P * (es + e_lse[:, None])
    W[~ist] = 0.0
    Pa = np.abs(G)
    e_dh = W @ np.abs(T) + acc * (Pa @ np.abs(T))
    e_dE = np.zeros_like(dE)
    e_dE[1:] = W.T @ np.abs(h) + acc * (Pa.T @ np.abs(h))
    sp = np.where(ist, S[rows, np.maximum(pos, 1) - 1], 0.0)
    loss = float((lse - sp)[ist].sum())
    e_loss = float((e_lse + np.where(ist, es[rows, np.maximum(pos, 1) - 1], 0.0))[ist].sum())
    sn = np.where(neg > 0, S[rows, np.maximum(neg, 1) - 1], 0.0)
    return dict(lse=lse, e_lse=e_lse, dh=dh, e_dh=e_dh, dE=dE, e_dE=e_dE, loss=loss, e_loss=e_loss, n=float(ist.sum()),
                sp=sp, sn=sn, ist=ist)


def sampled_softmax_ref64(h, E_, pos, neg, s, logq=None, bf16=False):
    """The softmax over each row's target and the samples s, hits masked: fp64 results and per-element bounds.  With logq (the
    popularity proposal) on the corrected logits z' = z - log Q, whose one fp32 add costs a score 2^-23 (|z| + |log Q|) more; the
    uniform objective has no such term.  sp / sn (the AUC's scores) are the raw ones either way."""
    u = 2.0 ** -7 if bf16 else 2.0 ** -15
    acc = 2.0 ** -7 if bf16 else 2.0 ** -14
    h = h.astype(np.float64)
    Ed = E_.astype(np.float64)
    Es = Ed[s]                                           # [N, D]
    Et = Ed[pos]                                         # [M, D] (row 0 for padded rows)
    S = S0 = h @ Es.T                                    # [M, N]
    St = St0 = (h * Et).sum(1)
    es = u * (np.abs(h) @ np.abs(Es).T)
    et = u * (np.abs(h) * np.abs(Et)).sum(1)
    if logq is not None:
        lq = np.asarray(logq, np.float64)
        S = S0 - lq[s][None, :]                          # the corrected logits
        St = St0 - lq[pos]
        es = es + 2.0 ** -23 * (np.abs(S0) + np.abs(lq[s])[None, :])
        et = et + 2.0 ** -23 * (np.abs(St0) + np.abs(lq[pos]))
    hit = s[None, :] == pos[:, None]
    mx = np.maximum(np.where(hit, -np.inf, S).max(1), St)
    Z = np.where(hit, 0.0, np.exp(S - mx[:, None]))
    zt = np.exp(St - mx)
    tot = Z.sum(1) + zt
    lse = mx + np.log(tot)
    P = Z / tot[:, None]
    pt = zt / tot
    ist = pos != 0
    e_lse = (P * es).sum(1) + pt * et + 2.0 ** -20 * (1.0 + np.abs(lse))
    Pm = P * ist[:, None]
    gt = np.where(ist, pt - 1.0, 0.0)
    dh = Pm @ Es + gt[:, None] * Et
    dE = np.zeros_like(Ed)
    np.add.at(dE, s, Pm.T @ h)
    np.add.at(dE, pos[ist], gt[ist, None] * h[ist])
    W = P * (es + e_lse[:, None]) * ist[:, None]
    wt = np.where(ist, pt * (et + e_lse), 0.0)
    e_dh = W @ np.abs(Es) + wt[:, None] * np.abs(Et) + acc * (Pm @ np.abs(Es) + np.abs(gt)[:, None] * np.abs(Et))
    e_dE = np.zeros_like(dE)
    np.add.at(e_dE, s, W.T @ np.abs(h) + acc * (Pm.T @ np.abs(h)))
    np.add.at(e_dE, pos[ist], (wt[ist] + acc * np.abs(gt[ist]))[:, None] * np.abs(h[ist]))
    loss = float((lse - St)[ist].sum())
    e_loss = float((e_lse + et)[ist].sum())
    sn = np.where(neg > 0, (h * Ed[neg]).sum(1), 0.0)
    return dict(lse=lse, e_lse=e_lse, dh=dh, e_dh=e_dh, dE=dE, e_dE=e_dE, loss=loss, e_loss=e_loss, n=float(ist.sum()), sp=St0, sn=sn,
                ist=ist)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def check(got, ref, scale, loss_key, full_catalogue=False):
    """Every element of the per-row output (loss_key "lse" or "l", bound "e_" + loss_key), d_seq_emb and table_grad within scale x its
    bound; the state's loss sum and target count.  Returns the worst ratio of table_grad.  full_catalogue (cr_softmax_ce, as its test
    always had it): row 0 of table_grad is not compared here, and the per-row ratio divides by the bare bound, which is never 0."""
    guard, first = (0.0, 1) if full_catalogue else (1e-30, 0)
    r = np.abs(got[loss_key] - ref[loss_key]) / (scale * ref["e_" + loss_key] + guard)
    assert np.all(r <= 1.0), (loss_key, float(r.max()), int(np.argmax(r)))
    r = np.abs(got["dh"] - ref["dh"]) / (scale * ref["e_dh"] + 1e-30)
    assert np.all(r <= 1.0), ("dh", float(r.max()), np.unravel_index(np.argmax(r), r.shape))
    r = np.abs(got["tg"][first:] - ref["dE"][first:]) / (scale * ref["e_dE"][first:] + 1e-30)
    assert np.all(r <= 1.0), ("tg (dE)", float(r.max()), np.unravel_index(np.argmax(r), r.shape))
    assert abs(got["state"][0] - ref["loss"]) <= scale * ref["e_loss"] + 1e-6 * abs(ref["loss"]) + 1e-5, \
        ("state[0]", got["state"][0], ref["loss"])
    assert got["state"][2] == ref["n"], ("state[2]", got["state"][2], ref["n"])
    return float(r.max())

"""Reference side of cr_gbce's tests (castrec.h): the numpy restatement of its device draw and of the engine's beta, the fp64 results with
per-element bounds, and a numpy emulation of the device arithmetic that shows the bounds can be met.

The bounds are built from fp64 quantities only.  A score carries es = u * sum_i |h_mi E_vi| (u = 2^-15 for the three bf16 products,
2^-7 for plain bf16).  |softplus'| = sigma <= 1 and |sigma'| <= 1/4 carry it into the loss and the gradient coefficients:
  loss of a row:  beta et + sum_{live j} sigma_j es_j + 2^-20 (1 + |l|) + n_live 2^-24 l
  coefficient:    es / 4 (a negative), beta et / 4 (the target)
and |E| / |h| carry the coefficients' bounds into dh / dE, plus 2^-14 (2^-7 plain) of sum |g| |E| and sum |g| |h| for the accumulation
and the bf16 split of g, as loss_ref.sampled_softmax_ref64.  The last loss term is the textbook bound of an fp32 sum of n_live + 1 non-negative
terms in any order, (n - 1) 2^-24 sum |x|.  Small-e treatment: softplus(x) = max(x, 0) + log(1 + e) with e = exp(-|x|) loses e whole
once e < 2^-24 if evaluated as written (N such terms lose N e, all of the loss of a row of very negative scores); the device and the
emulation take the series e - e^2 / 2 below e = 2^-12 (truncation < 2^-25 e), so the bound carries no term for it: 2^-20 (1 + |l|)
covers the few-ulp evaluation error of every term (2^-24 absolute from 1 + e above the threshold, against terms >= 2^-12.5)."""
import numpy as np

import loss_ref
from loss_ref import GBCE_SITE as CR_GBCE_SITE


def draw(seed, step, V, N):
    """loss_ref.draw at cr_gbce's site."""
    return loss_ref.draw(seed, step, V, N, CR_GBCE_SITE)


def beta(N, itemnum, t):
    """gSASRec: alpha = the sampling rate over the itemnum - 1 items that are not the target; beta = alpha (t (1 - 1 / alpha) + 1 / alpha)."""
    alpha = min(1.0, N / max(1, itemnum - 1))
    return alpha * (t * (1.0 - 1.0 / alpha) + 1.0 / alpha)


def _softplus64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ref64(h, E_, pos, neg, s, b, bf16=False):
    """fp64 results and per-element bounds (module docstring)."""
    u = 2.0 ** -7 if bf16 else 2.0 ** -15
    acc = 2.0 ** -7 if bf16 else 2.0 ** -14
    h = h.astype(np.float64)
    Ed = E_.astype(np.float64)
    Es = Ed[s]                                           # [N, D]
    Et = Ed[pos]                                         # [M, D] (row 0 for padded rows)
    S = h @ Es.T                                         # [M, N]
    St = (h * Et).sum(1)
    es = u * (np.abs(h) @ np.abs(Es).T)
    et = u * (np.abs(h) * np.abs(Et)).sum(1)
    ist = pos != 0
    live = (s[None, :] != pos[:, None]) & ist[:, None]
    G = _sigmoid64(S) * live
    sneg = (_softplus64(S) * live).sum(1)
    l = np.where(ist, b * _softplus64(-St) + sneg, 0.0)
    e_l = np.where(ist, b * et + (G * es).sum(1) + 2.0 ** -20 * (1.0 + np.abs(l)) + live.sum(1) * 2.0 ** -24 * l, 0.0)
    gt = np.where(ist, b * (_sigmoid64(St) - 1.0), 0.0)
    dh = G @ Es + gt[:, None] * Et
    dE = np.zeros_like(Ed)
    np.add.at(dE, s, G.T @ h)
    np.add.at(dE, pos[ist], gt[ist, None] * h[ist])
    W = 0.25 * es * live
    wt = np.where(ist, 0.25 * b * et, 0.0)
    e_dh = W @ np.abs(Es) + wt[:, None] * np.abs(Et) + acc * (G @ np.abs(Es) + np.abs(gt)[:, None] * np.abs(Et))
    e_dE = np.zeros_like(dE)
    np.add.at(e_dE, s, W.T @ np.abs(h) + acc * (G.T @ np.abs(h)))
    np.add.at(e_dE, pos[ist], (wt[ist] + acc * np.abs(gt[ist]))[:, None] * np.abs(h[ist]))
    sn = np.where(neg > 0, (h * Ed[neg]).sum(1), 0.0)
    return dict(l=l, e_l=e_l, dh=dh, e_dh=e_dh, dE=dE, e_dE=e_dE, loss=float(l.sum()), e_loss=float(e_l.sum()), n=float(ist.sum()),
                sp=St, sn=sn, ist=ist, live=live)


# ---- the device arithmetic in numpy ----------------------------------------------------------------------------------------------
def _bf16(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def _split(x, bf16):
    hi = _bf16(x)
    return hi, (None if bf16 else _bf16(np.float32(x) - hi))


def _prod(A, B, bf16):
    """A @ B from bf16 operands with fp32 accumulation: hi hi only (plain), or lo hi + hi lo + hi hi (small terms first)."""
    ah, al = _split(A, bf16)
    bh, bl = _split(B, bf16)
    if bf16:
        return ah @ bh
    return ((al @ bh) + (ah @ bl)) + (ah @ bh)


def emulate(h, E_, pos, neg, s, b, bf16=False):
    """cr_gbce's arithmetic: scores from the bf16 products summed in fp32, sigma and softplus in fp32 from e = exp(-|z|) (the series
    e - e^2 / 2 below 2^-12), the coefficient matrix split again for the two gradient products, the target terms in fp32."""
    f = np.float32
    h = h.astype(f)
    Es, Et = E_[s].astype(f), E_[pos].astype(f)
    ist = pos != 0
    live = (s[None, :] != pos[:, None]) & ist[:, None]
    S = _prod(h, Es.T, bf16)
    # the target's score is the diagonal of the same product against the gathered rows
    hh, hl = _split(h, bf16)
    th, tl = _split(Et, bf16)
    St = (hh * th).sum(1, dtype=f) if bf16 else ((hl * th).sum(1, dtype=f) + (hh * tl).sum(1, dtype=f)) + (hh * th).sum(1, dtype=f)

    def parts(x):
        e = np.exp(-np.abs(x)).astype(f)
        r = f(1.0) / (f(1.0) + e)
        sig = np.where(x >= 0, r, e * r).astype(f)
        lg = np.where(e < f(2.0 ** -12), e - f(0.5) * e * e, np.log(f(1.0) + e)).astype(f)
        return sig, (np.maximum(x, f(0.0)) + lg).astype(f)

    sg, spl = parts(S)
    G = np.where(live, sg, f(0.0)).astype(f)
    sneg = np.where(live, spl, f(0.0)).sum(1, dtype=f)
    sgt_neg, spl_t = parts(-St)
    l = np.where(ist, f(b) * spl_t + sneg, f(0.0)).astype(f)
    gt = np.where(ist, -f(b) * sgt_neg, f(0.0)).astype(f)
    dh = (_prod(G, Es, bf16) + gt[:, None] * Et).astype(f)
    dh[~ist] = 0.0
    tg = np.zeros(E_.shape, f)
    np.add.at(tg, s, _prod(G.T, h, bf16))
    np.add.at(tg, pos[ist], gt[ist, None] * h[ist])
    state = np.zeros(16, f)
    state[0], state[2] = l.sum(dtype=f), ist.sum()
    return dict(l=l, dh=dh, tg=tg, state=state)


# ---- the planted corpus in fp64 ----------------------------------------------------------------------------------------------------
# The schedule of the planted-corpus training test.  The sampled softmax's test trains 250 steps; gBCE cannot be held to that: with N
# negatives against one positive of weight beta, the first thing the objective teaches is the constant-score solution z = c for every
# pair, sigma(c) = beta / (N + beta), a plateau at loss beta softplus(-c) + N softplus(c) (2.28 at N = 64, beta = 0.37) on which the
# ranking is still chance.  The fp64 reference below (the oracle's sasrec forward, this module's loss, autograd, AdamTF) sits on it
# from step ~100, leaves it between steps 450 and 600 (over initialisation and sample seeds) and then ranks every test sequence's next
# item first (HR@10 = 1.0 from step 600 on).  So the test trains PLANTED_STEPS = 1000 steps, and test_gbce_host.py shows that the
# reference passes the GPU test's thresholds on that schedule and is still on the plateau after the softmax's 250.
PLANTED_STEPS = 1000
PLANTED = dict(B=64, T=20, D=32, itemnum=400, N=64, lr=5e-3, t=0.75)


def plateau_loss(N, b):
    """The loss of the constant-score solution: every z = c with sigma(c) = b / (N + b)."""
    c = np.log(b / N)
    return float(b * _softplus64(-c) + N * _softplus64(c))


def planted_reference(steps, log=(), seed=3):
    """Trains the oracle's sasrec in fp64 on the planted corpus with the gBCE loss over gbce_ref.draw's samples (no dropout); returns
    ({step: loss}, full-ranking HR@10 of the next item after each test sequence's last one), as the GPU test measures them."""
    import torch
    from oracle import fpmodel as fm
    from loss_ref import planted as _planted
    c = PLANTED
    B, T, D, itemnum, N = c["B"], c["T"], c["D"], c["itemnum"], c["N"]
    rs = np.random.RandomState(0)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.0, lr=c["lr"])
    P = {k: v.double() for k, v in fm.init_params("sasrec", 10, itemnum, ohp, seed=seed).items()}
    opt = fm.AdamTF(P, lr=c["lr"])
    b = beta(N, itemnum, c["t"])
    sp = torch.nn.functional.softplus
    losses = {}
    zero = np.zeros((B, T), np.int64)
    for step in range(1, steps + 1):
        seq, pos, neg = _planted(rs, B, T, itemnum)
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
        out = fm.forward("sasrec", leaves, ohp, fm.to_batch(seq, pos, neg, zero, zero, zero), None)
        s = torch.as_tensor(draw(seed, step, itemnum + 1, N).astype(np.int64))
        se, tab = out["seq_emb"], out["item_table"]
        p = torch.as_tensor(pos.reshape(-1))
        ist = p != 0
        live = (s[None, :] != p[:, None]).double()
        loss = ((b * sp(-(se * tab[p]).sum(1)) + (sp(se @ tab[s].t()) * live).sum(1)) * ist).sum() / ist.sum()
        loss.backward()
        P = opt.step(dict(P), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
        if step in log or step == steps:
            losses[step] = float(loss)
    seq, pos, _ = _planted(np.random.RandomState(99), B, T, itemnum)
    with torch.no_grad():
        out = fm.forward("sasrec", P, ohp, fm.to_batch(seq, pos, zero, zero, zero, zero), None)
    sc = out["seq_emb"].reshape(B, T, D)[:, -1] @ out["item_table"].t()
    sc[:, 0] = -float("inf")
    tgt = torch.as_tensor(pos[:, -1])
    rank = (sc > sc.gather(1, tgt[:, None])).sum(1)
    return losses, float((rank < 10).double().mean())

"""Reference side of the popularity proposal of cr_sampled_ce (castrec.h): independent numpy restatements of the host builder and of the
device draw, and the skewed planted corpus in fp64.  (The fp64 results of the corrected objective with their per-element bounds:
loss_ref.sampled_softmax_ref64 with logq.)"""
import math

import numpy as np

import loss_ref
from loss_ref import SCE_SITE as CR_SCE_SITE


def build(w):
    """(cdf uint32 [V], logq float32 [V]) from weights w [V] (w[0] ignored): cdf[v] = min(floor(2^32 W_v / W_{V-1}), 2^32 - 1) over the
    running sums W of w[1:], masses with cdf[V-1] read as 2^32, logq = float32(log(mass / 2^32)), 0 for the padding row."""
    w = np.asarray(w, np.float64)
    V = len(w)
    W = np.cumsum(w[1:])
    top = np.float64(4294967296.0)
    c = np.concatenate([[0.0], np.minimum(np.floor(top * W / W[-1]), top - 1)])
    cdf = c.astype(np.uint32)
    edges = c.copy()
    edges[V - 1] = top
    mass = edges[1:] - edges[:-1]
    assert mass.min() >= 1
    logq = np.concatenate([[0.0], np.log(mass / top)]).astype(np.float32)
    return cdf, logq


def masses(cdf):
    """Q(v) for v = 0 .. V-1 (0 for the padding row) of a built proposal."""
    e = np.asarray(cdf, np.float64).copy()
    e[-1] = 4294967296.0
    return np.concatenate([[0.0], np.diff(e)]) / 4294967296.0


def hashes(seed, step, N):
    return loss_ref.hashes(seed, step, N, CR_SCE_SITE)


def draw(seed, step, cdf, N):
    """s_j = 1 + #{v in [1, V-2] : cdf[v] <= x_j} with the hashes x_j of the uniform draw (the same key, the same site)."""
    V = len(cdf)
    x = hashes(seed, step, N)
    return (np.searchsorted(np.asarray(cdf, np.uint64)[1:V - 1], x, side="right") + 1).astype(np.int32)


def zipf_weights(V, a=1.0):
    """(c + 1)^a with Zipf-like counts c = floor(10^6 / rank^1.1) dealt to the ids by RandomState(V % 1000); [0] is the padding row's."""
    c = np.floor(1e6 / np.arange(1, V + 1, dtype=np.float64) ** 1.1)
    np.random.RandomState(V % 1000).shuffle(c)
    return (c + 1.0) ** a


# ---- the skewed planted corpus -----------------------------------------------------------------------------------------------------
PLANTED = dict(B=64, T=20, D=32, itemnum=400, N=64, lr=5e-3, steps=250, count_batches=200)
PLANTED_LOSS, PLANTED_HR = 0.5 * math.log(65), 0.5


def planted_skewed(rs, B, T, itemnum):
    """loss_ref.planted (item i is followed by item i + 1, left-padded to T) with the start of a sequence drawn as
    1 + int((itemnum - n - 1) u^3): low ids are frequent, high ids rare."""
    seq = np.zeros((B, T), np.int64); pos = np.zeros((B, T), np.int64); neg = np.zeros((B, T), np.int64)
    for b in range(B):
        n = rs.randint(T // 2, T + 1)
        s = 1 + int((itemnum - n - 1) * rs.rand() ** 3)
        seq[b, T - n:] = np.arange(s, s + n)
        pos[b, T - n:] = np.arange(s + 1, s + n + 1)
        neg[b, T - n:] = rs.randint(1, itemnum + 1, n)
    return seq, pos, neg


def planted_counts():
    """Each item's occurrences in count_batches batches of an independent stream of the corpus."""
    c = PLANTED
    rs = np.random.RandomState(12345)
    counts = np.zeros(c["itemnum"] + 1, np.int64)
    for _ in range(c["count_batches"]):
        seq, _, _ = planted_skewed(rs, c["B"], c["T"], c["itemnum"])
        counts += np.bincount(seq.reshape(-1), minlength=c["itemnum"] + 1)
    counts[0] = 0
    return counts


def planted_reference(steps, log=(), seed=3):
    """Trains the oracle's sasrec in fp64 on the skewed planted corpus with the corrected sampled softmax over this module's draw (no
    dropout); returns ({step: loss}, full-ranking HR@10 of the next item after each test sequence's last one), as the GPU test
    measures them."""
    import torch
    from oracle import fpmodel as fm
    c = PLANTED
    B, T, D, itemnum, N = c["B"], c["T"], c["D"], c["itemnum"], c["N"]
    cdf, logq = build(planted_counts() + 1.0)
    lq = torch.as_tensor(logq.astype(np.float64))
    rs = np.random.RandomState(0)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=1, dropout_rate=0.0, lr=c["lr"])
    P = {k: v.double() for k, v in fm.init_params("sasrec", 10, itemnum, ohp, seed=seed).items()}
    opt = fm.AdamTF(P, lr=c["lr"])
    losses = {}
    zero = np.zeros((B, T), np.int64)
    for step in range(1, steps + 1):
        seq, pos, neg = planted_skewed(rs, B, T, itemnum)
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
        out = fm.forward("sasrec", leaves, ohp, fm.to_batch(seq, pos, neg, zero, zero, zero), None)
        s = torch.as_tensor(draw(seed, step, cdf, N).astype(np.int64))
        se, tab = out["seq_emb"], out["item_table"]
        p = torch.as_tensor(pos.reshape(-1))
        ist = p != 0
        S = se @ tab[s].t() - lq[s][None, :]
        st = (se * tab[p]).sum(1) - lq[p]
        S = S.masked_fill(s[None, :] == p[:, None], float("-inf"))
        loss = ((torch.logsumexp(torch.cat([st[:, None], S], 1), 1) - st) * ist).sum() / ist.sum()
        loss.backward()
        P = opt.step(dict(P), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
        if step in log or step == steps:
            losses[step] = float(loss.detach())
    seq, pos, _ = planted_skewed(np.random.RandomState(99), B, T, itemnum)
    with torch.no_grad():
        out = fm.forward("sasrec", P, ohp, fm.to_batch(seq, pos, zero, zero, zero, zero), None)
    sc = out["seq_emb"].reshape(B, T, D)[:, -1] @ out["item_table"].t()
    sc[:, 0] = -float("inf")
    tgt = torch.as_tensor(pos[:, -1])
    rank = (sc > sc.gather(1, tgt[:, None])).sum(1)
    return losses, float((rank < 10).double().mean())

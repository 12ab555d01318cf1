"""The popularity proposal of the sampled softmax (include/castrec.h, cr_sampled_ce): from non-negative item weights to the two
arrays the device reads -- the cumulative masses in units of 2^-32 the draw searches and the log-Q correction of every item, taken
from the same quantised masses so that the correction is that of the draw exactly.  float64, vectorised (10^7 items: under a second)."""
import numpy as np

TWO32 = 2.0 ** 32


def build_proposal(w, V=None):
    """w: non-negative finite weights [V] (w[0], the padding row's, is ignored).  Returns (cdf uint32 [V], logq float32 [V]):
    W_v = sum_{1 <= u <= v} w_u in index order, cdf[0] = 0, cdf[v] = min(floor(2^32 W_v / W_{V-1}), 2^32 - 1); with cdf[V-1] read as
    2^32, mass_v = cdf[v] - cdf[v-1], Q(v) = mass_v / 2^32, logq[0] = 0, logq[v] = float32(log Q(v)).  ValueError, naming the first
    offending id, for a wrong length, a negative or non-finite weight, or an item without mass (every item can be a target, so log Q
    must exist for every item)."""
    w = np.asarray(w, np.float64)
    if w.ndim != 1 or w.shape[0] < 2 or (V is not None and w.shape[0] != V):
        want = "at least 2" if V is None else "%d" % V
        first = w.shape[0] if w.ndim == 1 and (V is None or w.shape[0] < V) else (V or 0)
        raise ValueError("item weights of shape %s: one value per table row, %s in all (first id missing or surplus: %d)"
                         % (w.shape, want, first))
    V = w.shape[0]
    bad = ~(np.isfinite(w[1:]) & (w[1:] >= 0.0))
    if bad.any():
        v = 1 + int(np.argmax(bad))
        raise ValueError("item %d has weight %r: weights must be finite and non-negative" % (v, float(w[v])))
    W = np.cumsum(w[1:])
    if not np.isfinite(W[-1]):
        raise ValueError("item %d: the weights' running sum overflows float64" % (1 + int(np.argmax(~np.isfinite(W)))))
    if not W[-1] > 0.0:
        raise ValueError("item 1 has no mass: every weight is zero")
    c = np.zeros(V, np.float64)
    c[1:] = np.minimum(np.floor(TWO32 * W / W[-1]), TWO32 - 1.0)
    cdf = c.astype(np.uint32)
    c[V - 1] = TWO32                                     # the last entry is read as 2^32: the masses sum to 2^32 exactly
    mass = np.diff(c)
    none = mass < 1.0
    if none.any():
        v = 1 + int(np.argmax(none))
        raise ValueError("item %d has no mass in the quantised proposal (weight %r of a total %r is below 2^-32 of it): every item "
                         "can be a target, so every item needs log Q" % (v, float(w[v]), float(W[-1])))
    logq = np.zeros(V, np.float32)
    logq[1:] = np.log(mass / TWO32).astype(np.float32)
    return cdf, logq


def effective_items(cdf):
    """exp(entropy of Q): the number of equally likely items a uniform proposal of the same entropy would draw from."""
    c = np.asarray(cdf, np.float64).copy()
    c[-1] = TWO32
    q = np.diff(c) / TWO32
    return float(np.exp(-(q * np.log(q)).sum()))

"""One step of cr_adam_step (include/castrec.h cr_adam_desc; csrc/cr_adam.hip) restated in numpy float64, with a per-element error bound
for the fp32 kernel, and the builders of the inputs that tests/test_adam_host.py (CPU: reference, comparator, mutants) and
tests/test_adam_gpu.py (the kernel) share.  No GPU, no native library.

The step.  With n = n_target, inv_n = 1 / n (0 when n = 0), G the un-normalised gradient of an element:
    g = G * inv_n;   i < n_l2:  g += l2 * p0
    m = b1 m0 + (1 - b1) g;   v = b2 v0 + (1 - b2) g^2;   lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);   p = p0 - lr_t m / (sqrt(v) + eps)
G is table_grad[i] on the table section (zeroed afterwards), the sum of the first slab_counts[block] slabs on the dense section, and
under `tg` the scatter of tests/test_index.py::_table_grad_reference (rows without a unit: G = 0, still updated).  Lazy rows: each
listed id in 1 .. lazy_rows - 1 once; every other lazy row keeps p, m, v and its table_grad.  lr, b1, b2, eps and l2 are taken at
their float32 values (the descriptor holds floats); 1 - b1 and 1 - b2 are exact in fp32 for b in [0.5, 1] (Sterbenz).

Exact gradients.  The builders below make every G exact in fp32 (entries are integers in [-32, 32] times 2^-6, `scale` a power of
two, coef * emb products 12-bit, at most a few thousand terms per sum), so that no bound has to cover summation error or order.

Error bounds (u = 2^-24, one fp32 rounding; all magnitudes taken from the fp64 values).
  e_g = K_G u (|G inv_n| + |l2 p0|), K_G = 4: fl(1 / n), the product G * inv_n and the fma's single rounding are three roundings of
        quantities no larger than |G inv_n| + |l2 p0|; the fourth covers second-order terms.  (n a power of two: two of them are
        exact -- the bound is not narrowed for it.)
  b_m = K_M u (|b1 m0| + |(1 - b1) g|) + (1 - b1) e_g, K_M = 3: two products and one sum (or one product and one fma), the sum's
        rounding u |m| <= u (|b1 m0| + |(1 - b1) g|): at most 2 u of that magnitude, the third covers second-order terms.
  b_v = K_V u (b2 v0 + (1 - b2) g^2) + (1 - b2) (2 |g| e_g + e_g^2), K_V = 4: the same with one more product ((1 - b2) * g * g).
        Every term is non-negative, so without l2 this is a purely relative bound of a few u.
  b_p = 2^-23 |p| + R |S| + (lr_t / den) b_m + lr_t (|m| + b_m) d / (den (den - d)),   S = lr_t m / den, den = sqrt(v) + eps,
        d = sqrt(v + b_v) - sqrt(max(v - b_v, 0)) (what b_v can move the root by; no derivative, so v = 0 is covered).
        2^-23 |p| = 2 u |p|: the rounding of the final subtraction.  R = 2e-4 is the relative error granted to the fp32 powf, sqrtf and
        divisions that form lr_t and the step (powf's error is amplified by b1^t / (1 - b1^t) = 9 at t = 1); it is the margin the project
        already uses for this quantity (tests/test_index.py asserts 2e-7 on a step of 1e-3) and is NOT fitted to the kernel.
An element the step does not touch must come back bit-identical (bound 0).  state[5] / state[6] are one fp32 division (and one addition):
relative 2^-22."""
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

U = 2.0 ** -24
R = 2e-4
K_G, K_M, K_V = 4, 3, 4
STATE_RTOL = 2.0 ** -22
PERIOD = 1000003                                          # a prime: no stride of the kernel divides it
COLS = 256                                                # dense parameters per workgroup (ADAM_COLS)

MUTANTS = ("n_l2_off_by_one", "l2_dropped", "inv_n_dropped", "beta2_0.999", "t_off_by_one", "slab_counts_ignored", "one_slab_dropped",
           "unitless_rows_not_moved", "lazy_duplicate_twice", "lazy_id0_applied", "tail_not_updated", "after_table_by_table_rule")


def dyadic(rs, shape):
    """integers in [-32, 32] times 2^-6"""
    return (rs.randint(-32, 33, shape) / 64.0).astype(np.float32)


def make_case(seed, n_table, n_dense, n_slabs=6, l2=0.0, n_l2=0, n_target=16.0, t=3, slab_counts=None, stats_mode="local", lr=1e-2,
              lazy=None, tg=None, ring=None):
    """Inputs of one launch.  p0 normal; m0 in (-1, 1) and v0 in [0, 1) random -- not zero, so that the decay terms count -- with every
    101st element's moments zero (a row no step has touched yet).  lazy = (lazy_rows, lazy_D, ids); tg = dict of make_tg;
    ring = dict(slots, slot_elems, copy_elems, misalign); stats_mode: local | external | self (castrec.h: state, stats, stats + snapshot)."""
    rs = np.random.RandomState(seed)
    c = types.SimpleNamespace()
    n = n_table + n_dense
    c.n_table, c.n_dense, c.n_slabs = int(n_table), int(n_dense), int(n_slabs) if n_dense else 0
    # (a large array repeats a draw of PERIOD values: drawing 20 M normals costs more than the launch and its reference together)
    big = lambda draw, k: np.resize(draw(min(k, PERIOD)), k)
    c.p0 = big(lambda k: rs.standard_normal(k).astype(np.float32), n)
    c.m0 = big(lambda k: rs.uniform(-1, 1, k).astype(np.float32), n)
    c.v0 = big(lambda k: rs.uniform(0, 1, k).astype(np.float32), n)
    c.m0[::101] = 0.0
    c.v0[::101] = 0.0
    c.table_grad = None if tg is not None else big(lambda k: dyadic(rs, k), n_table)
    c.slabs = dyadic(rs, (c.n_slabs, n_dense)) if n_dense else None
    c.slab_counts = None if slab_counts is None else np.asarray(slab_counts, np.int32)
    if c.slab_counts is not None:
        assert len(c.slab_counts) == -(-n_dense // COLS)
        for b, k in enumerate(c.slab_counts):             # what a block does not count must not be read
            c.slabs[k:, b * COLS:(b + 1) * COLS] = np.nan
    c.lr, c.beta1, c.beta2, c.eps, c.l2, c.n_l2 = lr, 0.9, 0.98, 1e-8, float(l2), int(n_l2)
    c.n_target, c.loss_sum, c.auc_sum, c.t, c.state7 = float(n_target), 3.5 * n_target, 0.25 * n_target, int(t), 0.625
    c.stats_mode = stats_mode
    c.lazy, c.tg, c.ring = lazy, tg, ring
    if lazy is not None:
        rows, D, ids = lazy
        assert rows * D <= n_table
        c.lazy = types.SimpleNamespace(rows=rows, D=D, ids=np.asarray(ids, np.int32), flags0=np.zeros(rows, np.uint32))
    if ring is not None:
        c.ring = types.SimpleNamespace(**ring)
        if not hasattr(c.ring, "data"):
            c.ring.data = rs.randint(1, 1 << 20, (c.ring.slots, c.ring.slot_elems)).astype(np.int32)
    return c


def make_tg(seed, D, V, T_pos, B=8, T=25, listed=None, rows2=True):
    """A batch for the occurrence index: about a third of the V rows listed (one of them hot: a row of several lane groups), left
    padding, dyadic gradient rows / head inputs / coefficients, scale a power of two."""
    rs = np.random.RandomState(seed)
    M = B * T
    pool = rs.choice(np.arange(1, V), listed if listed is not None else max(1, V // 3), replace=False)
    draw = lambda: np.where(rs.rand(M) < 0.3, pool[0], pool[rs.randint(0, len(pool), M)]).astype(np.int32)
    seq, pos, neg = draw(), draw(), draw()
    for b in range(B):
        k = rs.randint(0, T // 2)
        seq[b * T:b * T + k] = 0; pos[b * T:b * T + k] = 0; neg[b * T:b * T + k] = 0
    return dict(D=D, V=V, T_pos=T_pos, M=M, seq=seq, pos=pos, neg=neg, scale=8.0, rows=dyadic(rs, (M, D)),
                rows2=dyadic(rs, (M, D)) if rows2 else None, emb=dyadic(rs, (M, D)), coef=dyadic(rs, (2, M)))


def tg_gradient(tg):
    """(fp64 [(V + T_pos) * D] gradient, bool [V + T_pos]: the row has a unit)"""
    if "_grad" in tg:                                     # (computed once per batch: the cases of a batch share it, unchanged)
        return tg["_grad"]
    g = _table_grad_reference(tg["V"], tg["T_pos"], tg["D"], tg["seq"], tg["pos"], tg["neg"], tg["rows"], tg["rows2"], tg["scale"],
                              tg["emb"], tg["coef"])
    listed = np.zeros(tg["V"] + tg["T_pos"], bool)
    listed[np.unique(np.r_[tg["seq"], tg["pos"], tg["neg"]])] = True
    listed[0] = False
    listed[tg["V"]:] = True
    tg["_grad"] = (g.reshape(-1), listed)
    return tg["_grad"]


def _pieces(n, fn, size=1 << 19):
    """fn(lo, hi) over [0, n) in cache-sized pieces, on a few threads where there is more than one piece (numpy releases the lock)"""
    cuts = [(lo, min(lo + size, n)) for lo in range(0, n, size)]
    if len(cuts) <= 1:
        for lo, hi in cuts:
            fn(lo, hi)
        return
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda lh: fn(*lh), cuts))


def _update(c, idx, G, p0, m0, v0, s, f):
    """The kernel's `update` on elements idx (global indices, for n_l2) in arithmetic type f; returns p, m, v and the three bounds."""
    F = lambda x: np.asarray(x, f)
    g = F(G) * s.inv_n if f is np.float32 else G * s.inv_n
    g = F(g)
    reg = idx < s.n_l2
    if s.l2 != 0.0 and reg.any():
        g = np.where(reg, F(np.float64(s.l2) * p0.astype(np.float64) + g.astype(np.float64)), g)      # one rounding: fmaf
    m = F(F(s.b1 * m0) + F(s.c1 * g))
    v = F(F(s.b2 * v0) + F(F(s.c2 * g) * g))
    den = F(np.sqrt(v) + s.eps)
    p = F(p0 - F(F(s.lr_t * m) / den))
    if f is np.float32:
        return p, m, v, None, None, None
    e_g = K_G * U * (np.abs(G * s.inv_n) + np.where(reg, np.abs(s.l2 * p0), 0.0))
    b_m = K_M * U * (np.abs(s.b1 * m0) + np.abs(s.c1 * g)) + s.c1 * e_g
    b_v = K_V * U * (s.b2 * v0 + s.c2 * g * g) + s.c2 * (2 * np.abs(g) * e_g + e_g * e_g)
    d = np.sqrt(v + b_v) - np.sqrt(np.maximum(v - b_v, 0.0))
    b_p = 2.0 ** -23 * np.abs(p) + R * np.abs(s.lr_t * m / den) + s.lr_t / den * b_m + s.lr_t * (np.abs(m) + b_m) * d / (den * (den - d))
    return p, m, v, b_p, b_m, b_v


def reference(c, mutant=None, dtype=np.float64):
    """One step.  dtype float64: the reference and its bounds; float32: the same operations rounded to fp32 one by one (what a correct
    kernel may compute; no bounds).  mutant: one of MUTANTS -- a wrong step the comparator must reject."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = np.float32 if dtype == np.float32 else np.float64
    nt, nd = c.n_table, c.n_dense
    n = nt + nd
    s = types.SimpleNamespace()
    lr, s.b1, s.b2, s.eps, s.l2 = (f(np.float32(x)) for x in (c.lr, c.beta1, 0.999 if mutant == "beta2_0.999" else c.beta2, c.eps, c.l2))
    s.c1, s.c2 = f(1) - s.b1, f(1) - s.b2
    s.n_l2 = c.n_l2 - 1 if mutant == "n_l2_off_by_one" else c.n_l2
    if mutant == "l2_dropped":
        s.l2 = f(0)
    nn = f(np.float32(c.n_target))
    s.inv_n = (f(1) / nn if nn > 0 else f(0)) if mutant != "inv_n_dropped" else f(1 if nn > 0 else 0)
    t = f(c.t + (1 if mutant == "t_off_by_one" else 0))
    with np.errstate(under="ignore"):
        s.lr_t = f(f(lr * np.sqrt(f(1) - np.power(s.b2, t))) / (f(1) - np.power(s.b1, t)))

    # the gradient of every element and who is updated
    G = np.zeros(n, np.float64)
    upd = np.ones(n, bool)
    zeroed = None
    again = np.zeros(n, bool)                             # (mutant: updated a second time, with the zeroed gradient)
    if c.tg is not None:
        g_tab, listed = tg_gradient(c.tg)
        assert len(g_tab) == nt
        G[:nt] = g_tab
        if mutant == "unitless_rows_not_moved":
            upd[:nt] = np.repeat(listed, c.tg["D"])
    else:
        G[:nt] = c.table_grad
        zeroed = np.ones(nt, bool)
        if c.lazy is not None:
            lz = c.lazy
            L = lz.rows * lz.D
            ids = lz.ids[(lz.ids > (-1 if mutant == "lazy_id0_applied" else 0)) & (lz.ids < lz.rows)]
            rows, cnt = np.unique(ids, return_counts=True)
            row_upd = np.zeros(lz.rows, bool)
            row_upd[rows] = True
            upd[:L] = np.repeat(row_upd, lz.D)
            zeroed[:L] = upd[:L]
            if mutant == "lazy_duplicate_twice":
                row_upd[:] = False
                row_upd[rows[cnt > 1]] = True
                again[:L] = np.repeat(row_upd, lz.D)
        if mutant == "tail_not_updated" and nt > 0:
            upd[nt - 1] = False
    if nd:
        counts = np.full(-(-nd // COLS), c.n_slabs) if c.slab_counts is None or mutant == "slab_counts_ignored" else np.minimum(c.slab_counts, c.n_slabs)
        if mutant == "one_slab_dropped":
            counts = np.maximum(counts - 1, 0)
        per = np.repeat(counts, COLS)[:nd]
        use = np.arange(c.n_slabs)[:, None] < per[None, :]
        G[nt:] = np.where(use, c.slabs.astype(np.float64), 0.0).sum(0)
        if mutant == "after_table_by_table_rule":
            G[nt] = 0.0
    else:
        assert mutant not in ("slab_counts_ignored", "one_slab_dropped", "after_table_by_table_rule")

    out = types.SimpleNamespace()
    out.p, out.m, out.v = np.empty(n, f), np.empty(n, f), np.empty(n, f)
    if f is np.float64:
        out.bp, out.bm, out.bv = np.empty(n), np.empty(n), np.empty(n)

    def piece(lo, hi):
        sl = slice(lo, hi)
        p0, m0, v0 = (x[sl].astype(f) for x in (c.p0, c.m0, c.v0))
        idx = np.arange(lo, hi)
        p, m, v, bp, bm, bv = _update(c, idx, G[sl], p0, m0, v0, s, f)
        if again[sl].any():
            p2, m2, v2, _, _, _ = _update(c, idx, np.zeros(hi - lo), p, m, v, s, f)
            p, m, v = np.where(again[sl], p2, p), np.where(again[sl], m2, m), np.where(again[sl], v2, v)
        u = upd[sl]
        out.p[sl], out.m[sl], out.v[sl] = np.where(u, p, p0), np.where(u, m, m0), np.where(u, v, v0)
        if f is np.float64:
            out.bp[sl], out.bm[sl], out.bv[sl] = np.where(u, bp, 0.0), np.where(u, bm, 0.0), np.where(u, bv, 0.0)

    _pieces(n, piece)
    out.updated, out.grad_zeroed, out.G = upd, zeroed, G

    # the scalars the launch leaves in `state`
    nf = float(c.n_target)
    out.state5 = (c.loss_sum / nf if nf > 0 else 0.0) + (c.state7 if c.n_l2 > 0 else 0.0)
    out.state6 = c.auc_sum / nf if nf > 0 else 0.0
    out.state04 = (0.0, 0.0, 0.0, 0.0, c.t + 1) if c.stats_mode == "self" else None      # None: state[0..4] as they were
    out.lazy_flags = None
    if c.lazy is not None:
        out.lazy_flags = c.lazy.flags0.copy()
        ok = c.lazy.ids[(c.lazy.ids > 0) & (c.lazy.ids < c.lazy.rows)]
        out.lazy_flags[ok] = c.t
    out.ring_copy = None
    if c.ring is not None:
        k = c.ring.copy_elems if c.ring.copy_elems else c.ring.slot_elems
        out.ring_copy = c.ring.data[(c.t + 1) % c.ring.slots, :k].copy()
    return out


def worst_ratio(got, ref):
    """max over p, m, v and their elements of |got - ref| / bound (an untouched element: 0 if identical, inf if not; a NaN: inf);
    returns (ratio, which array, element)"""
    found = []
    for name, want, bound in (("p", ref.p, ref.bp), ("m", ref.m, ref.bm), ("v", ref.v, ref.bv)):
        x = np.asarray(got[name])
        assert x.shape == want.shape, (name, x.shape, want.shape)

        def piece(lo, hi, name=name, want=want, bound=bound, x=x):
            xs, b = x[lo:hi].astype(np.float64), bound[lo:hi]
            d = np.abs(xs - want[lo:hi])
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
            r = np.where(np.isfinite(xs), r, np.inf)
            i = int(np.argmax(r))
            found.append((float(r[i]), name, lo + i))

        _pieces(x.size, piece)
    return max(found, key=lambda w: (w[0], -w[2])) if found else (0.0, "", -1)


def accepted(got, ref):
    return worst_ratio(got, ref)[0] <= 1.0


def ring_copy_reference(c, dst0):
    """ids_dst after the launch: the first copied words from slot (t + 1) mod slots, the rest as it was"""
    out = np.array(dst0, copy=True)
    k = c.ring.copy_elems if c.ring.copy_elems else c.ring.slot_elems
    out[:k] = c.ring.data[(c.t + 1) % c.ring.slots, :k]
    return out


def _table_grad_reference(V, T_pos, D, seq, pos, neg, rows, rows2, scale, emb, coef):
    """fp64: what float atomics summed in rounds 1-4"""
    M = len(seq)
    g = np.zeros((V + T_pos, D))
    r = rows.astype(np.float64) + (rows2.astype(np.float64) if rows2 is not None else 0.0)
    np.add.at(g, seq, scale * r)
    np.add.at(g, pos, coef[0][:, None].astype(np.float64) * emb)
    np.add.at(g, neg, coef[1][:, None].astype(np.float64) * emb)
    g[0] = 0.0
    if T_pos:
        g[V:] = r.reshape(M // T_pos, T_pos, D).sum(0)
    return g


# ---- device buffers of the GPU tests -------------------------------------------------------------------------------------------------
GUARD = 64          # elements on either side of a buffer (256 bytes: the buffer itself keeps the allocation's alignment)


class Buf:
    """A device array between two guards; shift: elements the array starts behind the aligned position."""

    def __init__(self, a, fill, shift=0):
        a = np.ascontiguousarray(a)
        self.lo, self.n = GUARD + shift, a.size
        self.host = np.full(a.size + 2 * GUARD + shift, fill, a.dtype)
        self.host[self.lo:self.lo + self.n] = a.reshape(-1)
        self.dev = torch.from_numpy(self.host).cuda()
        self.view = self.dev[self.lo:self.lo + self.n]

    def back(self):
        """the array after the launch; the guards must hold the bits they were given"""
        got = self.dev.cpu().numpy()
        bits = np.int32 if got.itemsize == 4 else np.int64
        assert np.array_equal(got[:self.lo].view(bits), self.host[:self.lo].view(bits)), "guard in front overwritten"
        assert np.array_equal(got[self.lo + self.n:].view(bits), self.host[self.lo + self.n:].view(bits)), "guard behind overwritten"
        return got[self.lo:self.lo + self.n]

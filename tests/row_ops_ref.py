"""Plain fp64 numpy references (no autograd) and case generators for the three row operators: cr_embed_fwd / cr_embed_bwd
(csrc/cr_embed.hip), cr_layernorm_fwd / cr_layernorm_bwd (csrc/cr_layernorm.hip) and cr_eltwise (csrc/cr_eltwise.hip), as
include/castrec.h states them.  tests/test_row_ops_gpu.py holds the kernels to these; tests/test_row_ops_host.py checks the
references against torch autograd and proves, on the generated inputs, the premises the GPU cases rest on.

Every input is drawn as a float32 value (scales and the dropout factor 1/(1 - rate) included) and widened, so the fp64 reference
sees exactly the numbers the kernel sees and no input rounding enters a bound.

Bounds.  u = 2^-24.  An embedding or element-wise output element is a sum of n addends, each of which went through r fp32
roundings before it was added; with S the fp64 sum of the addends' absolute values the kernel may be off by
    bound(S, n, r) = 2 * (r + n) * u * S
(n - 1 roundings of the sum, r per addend, the factor 2 for fused against separate multiply-add).  Every reference here returns
(value, S, n) per output; r, counted from the kernel source, is
    embed forward   R_EMBED_FWD = 4    row * scale, + positional row, + addend, * dropout scale
    d_addend        R_EMBED_G = 2      dout + out2, * dropout scale                      (also pos_grad, a sum over the batch)
    table_grad      R_EMBED_TABLE = 3  the two above, * scale                            (also the slabs of the small-table mode)
    CR_ELT_ADD      R_ELT[ADD] = 0     CR_ELT_DROPOUT, CR_ELT_GRADPREP: 1 (* 1/(1 - rate)); accumulate adds one addend
CR_ELT_COPY, CR_ELT_ROWMASK and CR_ELT_RELU_BWD select and at most add once (a correctly rounded fp32 add): bit for bit.

LayerNorm has no fixed constant: conditioning is mean / spread.  ln_bound() takes, per row (per column for dgamma / dbeta) the
largest deviation E of the same closed form evaluated in np.float32 (layernorm_ref(fp32=True), sums left to right) from fp64 and
allows 4 * E + 16 * u * (the row's largest |reference|); for dbeta the column takes the row's place and the magnitude is the
column's largest absolute addend; for dgamma the rows' envelopes of xhat are carried through the column sum (ln_dgamma_bound)."""
import functools
import types

import numpy as np

import dropout_ref as dr

U = 2.0 ** -24
F64 = np.float64
R_EMBED_FWD, R_EMBED_G, R_EMBED_TABLE = 4, 2, 3
ELT_COPY, ELT_ADD, ELT_DROPOUT, ELT_RELU_BWD, ELT_ROWMASK, ELT_GRADPREP = 0, 1, 2, 3, 4, 5
R_ELT = {ELT_COPY: 0, ELT_ADD: 0, ELT_DROPOUT: 1, ELT_RELU_BWD: 0, ELT_ROWMASK: 0, ELT_GRADPREP: 1}
ELT_EXACT = (ELT_COPY, ELT_ROWMASK, ELT_RELU_BWD)
EMB_SMALL_MAX = 12288          # floats of LDS the small-table kernel keeps (csrc/cr_embed.hip)
LN_EPS = float(np.float32(1e-8))


def bound(S, n, r):
    return 2.0 * (r + np.asarray(n, F64)) * U * S


def draw(rs, *shape, loc=0.0, scale=1.0):
    """float32 draws (the values the device gets)."""
    return (rs.standard_normal(shape) * scale + loc).astype(np.float32)


def wide(a):
    return None if a is None else np.asarray(a, np.float32).astype(F64)


# ------------------------------------------------------------------------------------------------ dropout, row mask
@functools.lru_cache(maxsize=None)
def pick_seed(rate, M, N, step, site, row_offset, base):
    """first seed from `base` whose keep mask keeps between 60 % and 90 % (one element: keeps it) -- chosen from the generator
    alone, so that every dropout case has kept and dropped elements in the expected proportion"""
    for seed in range(base, base + 1000):
        k = dr.rows_mask(seed, step, site, rate, M, N, row_offset).mean()
        if (0.6 < k < 0.9) if M * N > 1 else k == 1.0:
            return seed
    raise AssertionError("no seed")


def row_factor(c, M, N):
    """[M, N] fp64: keep * 1/(1 - rate) (the fp32 factor, widened) * (mask_ids != 0)"""
    f = np.ones((M, N), F64)
    if c.rate > 0:
        _, s = dr.thresh_scale(c.rate)
        f = dr.rows_mask(c.seed, c.step, c.site, c.rate, M, N, c.row_offset).astype(F64) * float(s)
    if c.mask_ids is not None:
        f = f * (c.mask_ids != 0)[:, None]
    return f


def keep_fraction(c, M, N):
    return float(dr.rows_mask(c.seed, c.step, c.site, c.rate, M, N, c.row_offset).mean())


def _ids(rs, M, V, skew=False):
    if skew:        # about 60 % of the rows carry id 1 or id 5 (one owner wave of k_embed_bwd_small: id mod 4 == 1)
        hot = np.where(rs.rand(M) < 0.5, 1, 5 if V > 5 else 1)
        ids = np.where(rs.rand(M) < 0.6, hot, rs.randint(0, V, M))
    else:
        ids = rs.randint(0, V, M)
    ids = ids.astype(np.int32)
    if M >= 2:
        ids[M // 3], ids[M // 2] = 0, V - 1
    return ids


def _mask(rs, M):
    m = (rs.rand(M) > 0.3).astype(np.int32)
    if M >= 2:
        m[0], m[M - 1] = 0, 1
    return m


# ------------------------------------------------------------------------------------------------ embedding
def embed_fwd_case(D, M, full, T=7, V=23):
    """cr_embed_desc.  full: every option on (zero_pad, scale sqrt(D), pos_table, addend at ld_add = D + 3, dropout 0.25 with
    row_offset 700, mask_ids, col_off 2, ld_out = col_off + D + 3); bare: zero_pad 0 and none of them."""
    rs = np.random.RandomState(1000 * D + M + int(full))
    c = types.SimpleNamespace(M=M, T=T, D=D, V=V, ids=_ids(rs, M, V), table=draw(rs, V, D))
    if full:
        c.__dict__.update(zero_pad=1, scale=float(np.float32(D ** 0.5)), pos=draw(rs, T, D), addend=draw(rs, M, D), ld_add=D + 3,
                          rate=0.25, step=3, site=4, row_offset=700, mask_ids=_mask(rs, M), col_off=2, ld_out=D + 5)
        c.seed = pick_seed(c.rate, M, D, c.step, c.site, c.row_offset, 5)
    else:
        c.__dict__.update(zero_pad=0, scale=1.0, pos=None, addend=None, ld_add=0, rate=0.0, step=0, site=0, seed=0, row_offset=0,
                          mask_ids=None, col_off=0, ld_out=D + 5)
    return c


def embed_ref(c):
    """forward of cr_embed_desc: out = (table[id] * scale (0 for id 0 when zero_pad) + pos[m % T] + addend[m]) * keep/(1-rate) * mask.
    Returns (out, S, n), each [M, D]."""
    M, D = c.M, c.D
    row = wide(c.table)[c.ids] * c.scale
    if c.zero_pad:
        row[c.ids == 0] = 0.0
    terms = [row]
    if c.pos is not None:
        terms.append(wide(c.pos)[np.arange(M) % c.T])
    if c.addend is not None:
        terms.append(wide(c.addend)[:, :D])
    f = row_factor(c, M, D)
    return sum(terms) * f, sum(np.abs(t) for t in terms) * f, len(terms)


def embed_bwd_case(D, M, T, V, has2, pos_grad, n_slabs=0, skew=False, tg_start=True, table_grad=True):
    """cr_embed_bwd_desc with dropout, row mask, d_addend, zero_pad and scale sqrt(D) on; dout (+ out2) at col_off 2 of pitch D + 5,
    d_addend at pitch D + 3; table_grad starts non-zero in the large-table forms (it accumulates)."""
    rs = np.random.RandomState(7919 * D + 31 * M + 3 * V + int(has2) + 2 * n_slabs)
    c = types.SimpleNamespace(M=M, T=T, D=D, V=V, ids=_ids(rs, M, V, skew), zero_pad=1, scale=float(np.float32(D ** 0.5)),
                              rate=0.25, step=6, site=9, row_offset=700, mask_ids=_mask(rs, M), col_off=2, ld_out=D + 5,
                              ld_add=D + 3, dout=draw(rs, M, D), out2=draw(rs, M, D) if has2 else None, want_pos=pos_grad,
                              n_slabs=n_slabs, slab_stride=V * D + 11 if n_slabs else 0, want_table=table_grad,
                              tg_start=draw(rs, V, D) if (tg_start and table_grad and not n_slabs) else None)
    c.seed = pick_seed(c.rate, M, D, c.step, c.site, c.row_offset, 11)
    return c


def embed_bwd_ref(c):
    """backward: g = (dout + out2) * mask * keep/(1-rate); d_addend = g; pos_grad[t] = sum_b g[b*T + t]; table_grad[id] += scale * g
    (np.add.at; rows with id 0 skipped when zero_pad).  In the small-table mode table_grad is what the slabs must sum to.
    Returns a dict of (value, S, n)."""
    M, D, T = c.M, c.D, c.T
    terms = [wide(c.dout)] + ([wide(c.out2)] if c.out2 is not None else [])
    f = row_factor(c, M, D)
    g, gS, gn = sum(terms) * f, sum(np.abs(t) for t in terms) * f, len(terms)
    res = dict(d_addend=(g, gS, gn))
    if c.want_pos:
        B = M // T
        res["pos_grad"] = (g.reshape(B, T, D).sum(0), gS.reshape(B, T, D).sum(0), gn * B)
    if c.want_table:
        live = (c.ids != 0) if c.zero_pad else np.ones(M, bool)
        tg = np.zeros((c.V, D), F64) if c.tg_start is None else wide(c.tg_start).copy()
        tS = np.abs(tg)
        np.add.at(tg, c.ids[live], g[live] * c.scale)
        np.add.at(tS, c.ids[live], gS[live] * c.scale)
        cnt = np.bincount(c.ids[live], minlength=c.V).astype(F64)[:, None] * gn + (c.tg_start is not None)
        res["table_grad"] = (tg, tS, np.broadcast_to(cnt, tg.shape))
    return res


def small_table_windows(c):
    """k_embed_bwd_small, D <= 64: per slab the rows [m0, m1), per 64-row window the largest number of rows one wave (id mod 4)
    owns.  More than 16 means a second trip of its `while (todo)` loop.  Returns (rows per slab, windows in the fullest slab,
    largest owned count)."""
    rps = -(-c.M // c.n_slabs)
    most, windows = 0, 0
    for s in range(c.n_slabs):
        m0, m1 = s * rps, min(c.M, (s + 1) * rps)
        windows = max(windows, -(-max(m1 - m0, 0) // 64))
        for h0 in range(m0, m1, 64):
            ids = c.ids[h0:min(h0 + 64, m1)]
            ids = ids[ids != 0] if c.zero_pad else ids
            if len(ids):
                most = max(most, int(np.bincount(ids & 3, minlength=4).max()))
    return rps, windows, most


# the cases of tests/test_row_ops_gpu.py (the host test walks the same lists)
EMBED_FWD_D = [1, 3, 4, 5, 8, 13, 20, 31, 50, 64, 66, 128, 130, 256, 260]
EMBED_FWD_M = [35, 1029]
BWD_POS = [(D, B) for D in (5, 50, 64, 65, 130, 512) for B in (3, 17, 70)]
BWD_ROWS16 = [(D, M, 7) for D in (4, 17, 50, 64) for M in (35, 1029)]
BWD_ROWS16_LOOP = (4, 32768 + 21, 1)                # 2048 workgroups x 16 rows: a second trip of the grid-stride loop
# (D, V, M, T, n_slabs, kind): kind "owner" must meet the >16-owned-rows premise; "atomic" (D > 64: LDS atomics), "fallback"
# (V * D > 12 288: large-table kernels) and "tiny" need not
SMALL = ([(D, V, 1600, 20, ns, "owner") for (D, V) in ((4, 2), (5, 9), (50, 9), (50, 25), (64, 25), (64, 192)) for ns in (1, 12)]
         + [(D, V, 1600, 20, ns, "atomic") for (D, V) in ((65, 9), (128, 9), (128, 96)) for ns in (1, 12)]
         + [(D, V, 1600, 20, ns, "fallback") for (D, V) in ((64, 193), (128, 97)) for ns in (1, 12)]
         + [(50, 9, 5, 5, 8, "tiny")])


@functools.lru_cache(maxsize=4)
def bwd_pos_case(D, B, has2, table_grad=True):
    return embed_bwd_case(D, B * 3, 3, 11, has2, True, table_grad=table_grad)


@functools.lru_cache(maxsize=4)
def bwd_rows16_case(D, M, T, has2):
    return embed_bwd_case(D, M, T, 11, has2, False)


@functools.lru_cache(maxsize=4)
def small_case(D, V, M, T, ns, has2):
    return embed_bwd_case(D, M, T, V, has2, False, n_slabs=ns, skew=True)


# ------------------------------------------------------------------------------------------------ layer normalisation
LN_D = [1, 4, 6, 16, 17, 50, 63, 64, 65, 128, 200, 257, 512]
LN_M = [1, 7, 67]
LN_KINDS = ["ordinary", "zero", "constant", "mean1e3", "spread1e-3", "spike1e4"]


def ln_kinds(M):
    """M = 1: one ordinary row; M = 7: the six kinds and an ordinary row; M = 67: ordinary rows and one zero row (the tensor-level
    bounds of test_ops_gpu.test_layernorm_fwd_bwd hold on these two)."""
    if M == 7:
        return LN_KINDS + ["ordinary"]
    k = ["ordinary"] * M
    if M > 1:
        k[1] = "zero"
    return k


def ln_row(rs, kind, D):
    if kind == "ordinary":
        return draw(rs, D, loc=0.5, scale=2.0)
    if kind == "zero":
        return np.zeros(D, np.float32)
    if kind == "constant":
        return np.full(D, 2.5, np.float32)            # few mantissa bits: every fp32 summation order gives the mean exactly
    if kind == "mean1e3":
        return draw(rs, D, loc=1e3, scale=1.0)        # the one-pass-variance trap: E[x^2] - mean^2 loses ~1e6 * u
    if kind == "spread1e-3":
        return draw(rs, D, loc=1.0, scale=1e-3)
    x = draw(rs, D)
    x[D // 2] = 1e4
    return x


@functools.lru_cache(maxsize=8)
def ln_case(D, M):
    rs = np.random.RandomState(100 * D + M)
    kinds = ln_kinds(M)
    c = types.SimpleNamespace(M=M, D=D, kinds=kinds, x=np.stack([ln_row(rs, k, D) for k in kinds]), gamma=draw(rs, D),
                              beta=draw(rs, D, loc=0.5), dy=draw(rs, M, D), dx0=draw(rs, M, D))
    # the non-zero flags must be decidable in fp32: every row sum of x and of y is exactly 0 or above 2e-3 of the row's absolute
    # sum (the host test asserts 1e-3).  A row of x that is not: its first entry moves by 1; a row of y: beta[0] moves by 1/4.
    undecided = lambda rows: (rows.sum(1) != 0) & (np.abs(rows.sum(1)) < 2e-3 * np.abs(rows).sum(1))
    for _ in range(64):
        bad = undecided(wide(c.x))
        if not bad.any():
            break
        c.x[bad, 0] += np.float32(1.0)
    for _ in range(64):
        if not undecided(layernorm_ref(c.x, c.gamma, c.beta).y).any():
            break
        c.beta[0] += np.float32(0.25)
    return c


def _rsum(a, axis, fp32):
    if not fp32:
        return a.sum(axis, keepdims=True)
    return np.take(np.add.accumulate(a, axis=axis, dtype=np.float32), [-1], axis=axis)      # left to right, every add rounded


def layernorm_ref(x, gamma, beta, dy=None, dx0=None, eps=LN_EPS, fp32=False):
    """modules.py:53-80 in closed form: mean, two-pass variance, eps inside the sqrt; backward
    dx = (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)) / sd (+ dx0), dgamma = sum_m dy * xhat, dbeta = sum_m dy.
    fp32=True evaluates the same formula in np.float32, every sum left to right: the restatement ln_bound() measures E with."""
    t = np.float32 if fp32 else F64
    x, gamma, beta = (np.asarray(a, np.float32).astype(t) for a in (x, gamma, beta))
    D = t(x.shape[1])
    s = _rsum(x, 1, fp32)
    xc = x - s / D
    sd = np.sqrt(_rsum(xc * xc, 1, fp32) / D + t(eps))
    xhat = xc / sd
    y = gamma * xhat + beta
    r = types.SimpleNamespace(y=y, xhat=xhat, x_nonzero=(s[:, 0] != 0).astype(np.float32), y_nonzero=(_rsum(y, 1, fp32)[:, 0] != 0).astype(np.float32))
    if dy is not None:
        dy = np.asarray(dy, np.float32).astype(t)
        dg = dy * gamma
        c1 = _rsum(dg, 1, fp32) / D
        c2 = _rsum(dg * xhat, 1, fp32) / D
        r.dx = (dg - c1 - xhat * c2) / sd
        if dx0 is not None:
            r.dx = np.asarray(dx0, np.float32).astype(t) + r.dx
        r.dgamma_terms = dy * xhat
        r.dgamma, r.dbeta = _rsum(r.dgamma_terms, 0, fp32)[0], _rsum(dy, 0, fp32)[0]
        r.dbeta_terms = dy
    return r


def ln_bound(r32, r64, mag=None):
    """[M, D] tensors: per row; dbeta [D] (a column sum of exact addends): per column, with mag = the column's largest absolute addend"""
    r32 = np.asarray(r32, F64)
    if r64.ndim == 2:
        return 4 * np.abs(r32 - r64).max(1, keepdims=True) + 16 * U * np.abs(r64).max(1, keepdims=True)
    return 4 * np.abs(r32 - r64) + 16 * U * mag


def ln_dgamma_bound(r32, r64, dy):
    """dgamma[c] = sum_m dy[m, c] * xhat[m, c]: a column has one element, and one element of the fp32 restatement can land on the fp64
    value by accident, so its deviation is no measure.  The conditioning lives in the rows of xhat: every addend may be off by |dy|
    times its row's envelope 4 * E_m + 16 * u * max|xhat[m]| (ln_bound on xhat), the errors of the addends add up, and the sum itself
    rounds against the column's largest absolute addend."""
    return (np.abs(wide(dy)) * ln_bound(r32.xhat, r64.xhat)).sum(0) + 16 * U * np.abs(r64.dgamma_terms).max(0)


# ------------------------------------------------------------------------------------------------ element-wise
ELT_SHAPES = [(1, 1), (37, 50), (2100, 251)]
ELT_FORMS = [("copy", ELT_COPY, False), ("add", ELT_ADD, True), ("dropout", ELT_DROPOUT, False), ("relu_bwd", ELT_RELU_BWD, True),
             ("rowmask", ELT_ROWMASK, False), ("gradprep_aux", ELT_GRADPREP, True), ("gradprep_regen", ELT_GRADPREP, False)]


@functools.lru_cache(maxsize=4)
def elt_inputs(M, N):
    rs = np.random.RandomState(M + 7 * N)
    return types.SimpleNamespace(x=draw(rs, M, N), aux=draw(rs, M, N), y0=draw(rs, M, N), mask=_mask(rs, M) if M > 1 else np.zeros(1, np.int32))


def elt_case(form, M, N, masked, accumulate, inplace):
    name, op, has_aux = next(f for f in ELT_FORMS if f[0] == form)
    i = elt_inputs(M, N)
    c = types.SimpleNamespace(M=M, N=N, op=op, form=form, x=i.x, aux=i.aux if has_aux else None, y0=i.x if inplace else i.y0,
                              mask_ids=i.mask if masked else None, accumulate=accumulate, inplace=inplace,
                              rate=0.25 if op in (ELT_DROPOUT, ELT_GRADPREP) else 0.0, step=2, site=3, seed=0, row_offset=0)
    if c.rate > 0:
        c.row_offset = 900
        c.seed = pick_seed(c.rate, M, N, c.step, c.site, c.row_offset, 17)
    return c


def eltwise_ref(c):
    """the six ops as castrec.h defines them, then * (mask_ids != 0), then y0 + value when accumulate.  Returns (y, S, n)."""
    x = wide(c.x)
    aux = wide(c.aux)
    terms = [x]
    if c.op == ELT_ADD:
        terms = [x, aux]
    elif c.op == ELT_RELU_BWD:
        terms = [np.where(aux > 0, x, 0.0)]
    elif c.op == ELT_DROPOUT or (c.op == ELT_GRADPREP and aux is None):
        no_mask = types.SimpleNamespace(**{**c.__dict__, "mask_ids": None})
        terms = [x * row_factor(no_mask, c.M, c.N)]
    elif c.op == ELT_GRADPREP:
        terms = [np.where(aux > 0, x * float(dr.thresh_scale(c.rate)[1]), 0.0)]
    if c.mask_ids is not None:
        terms = [np.where((c.mask_ids != 0)[:, None], t, 0.0) for t in terms]        # (+0, as the kernel writes it)
    if c.accumulate:
        terms = [wide(c.y0)] + terms
    return sum(terms), sum(np.abs(t) for t in terms), len(terms)

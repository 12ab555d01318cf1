"""A rounding model of the fp64 oracle for plain bf16 (attn_precision="bf16", CR_PREC_BF16): the same graphs (oracle/fpmodel.py)
with the operands of every matrix product rounded to bf16 (round to nearest even) in front of an fp64 product, forward and
backward.  What separates the model from the exact oracle is what plain bf16 may cost -- per parameter and per shape, computed from
the oracle alone, on the CPU -- and the kernels are held to a small multiple of it (grad_report; tests/test_bf16_envelope_gpu.py,
tests/test_model_gpu.py).  tests/test_bf16_ref_host.py checks the helper itself, and that the bound has room for a correct kernel
and none for a 20 % defect of one weight-gradient tile.

The model leaves the kernels' fp32 accumulation, their LayerNorm / softmax / dropout arithmetic and the order of their sums to the
additive term of the bound (GRAD_ABS etc.: what the split form bf16x3, which has no operand rounding to speak of, is held to)."""
import numpy as np
import torch

from oracle import fpmodel as fm

GRAD_FACTOR, GRAD_ABS = 3.0, 2e-3       # |got - exact| <= (3 E_k + 2e-3) * max(own largest entry, 1e-3 of the global one)
ACT_ABS = LOSS_ABS = 2e-4               # forward rows: 3 E_act + 2e-4 of the largest entry; loss: 3 E_loss + 2e-4, relative
FLOOR = 1e-3                            # (the denominator floor test_model_gpu.worst_grad_error has always used)

# (model, D, H, T, B, L, draw): the smallest shapes that reach each plain-bf16 code path (tests/test_bf16_envelope_gpu.py says which).
# draw: which draw of parameters and batch (draw_case).  Two shapes do not use draw 0: at cast_1 128 2 37 it gives ctx_time.1.wk a bound
# of 0.165 of its largest entry, above the cap of test_bf16_ref_host (the cap is a condition on the draw); at sasrec 256 4 50 the
# three model runs' errors of the loss -- one signed scalar -- all but cancel (6.6e-5) and the stand-ins sit at 2.5 times the
# loss bound.
SHAPES = [("sasrec", 50, 1, 224, 2, 2, 0), ("sasrec", 64, 1, 256, 2, 2, 0), ("cast_1", 20, 1, 241, 2, 2, 0),
          ("sasrec", 36, 1, 104, 3, 2, 0), ("sasrec", 50, 1, 96, 3, 2, 0), ("sasrec", 64, 2, 50, 3, 2, 0),
          ("sasrec", 128, 4, 40, 3, 2, 0), ("sasrec", 192, 3, 40, 3, 1, 0), ("sasrec", 256, 4, 50, 5, 1, 1), ("cast_1", 128, 2, 37, 3, 2, 2),
          ("cast_4", 128, 4, 24, 3, 1, 0), ("sasrec", 256, 4, 300, 2, 1, 0), ("sasrec", 66, 1, 18, 2, 1, 0), ("sasrec", 96, 3, 40, 3, 1, 0),
          ("cast_1", 50, 1, 200, 4, 2, 0)]


def make_batch(rs, B, T, itemnum, max_bins, all_zero_time_rows=True):
    seq = rs.randint(1, itemnum + 1, (B, T)); pos = rs.randint(1, itemnum + 1, (B, T)); neg = rs.randint(1, itemnum + 1, (B, T))
    for b in range(B):
        n = rs.randint(0, T - 2)
        seq[b, :n] = 0; pos[b, :n] = 0; neg[b, :n] = 0
    seq[0, :] = 0; pos[0, :] = 0; neg[0, :] = 0                  # an all-padding sequence
    seq[0, -1] = 3; pos[0, -1] = 4; neg[0, -1] = 5               # ... with a single real position
    time = rs.randint(0, max_bins + 1, (B, T)) * (seq != 0)
    time[:, -1] = 0                                              # most recent item is always bin 0 (sampler.py:61-64)
    if all_zero_time_rows and B > 2:
        time[2, :] = 0                                           # all interactions in one bin: no valid context key
    hours = rs.randint(1, 25, (B, T)) * (seq != 0); days = rs.randint(1, 8, (B, T)) * (seq != 0)
    return seq, pos, neg, time, hours, days


def draw_case(model, D, H, T, B, L, draw=0, dropout=0.0, itemnum=41, max_bins=9):
    """(P, hp, batch arrays): the draw of test_model_gpu._other_shapes (parameters as the fp32 values an engine would hold)."""
    rs = np.random.RandomState(D + T + draw)
    hp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=L, num_heads=H, dropout_rate=dropout, max_bins=max_bins, num_context_blocks=1, lr=1e-3)
    P = fm.init_params(model, 9, itemnum, hp, seed=8)
    P = {k: (v + 0.05 * torch.tensor(rs.standard_normal(tuple(v.shape)))).float().double() for k, v in P.items()}
    return P, hp, make_batch(rs, B, T, itemnum, max_bins)


# ---------------------------------------------------------------------------------------------------------------------------
# roundings
# ---------------------------------------------------------------------------------------------------------------------------
def _jittered(x, jitter):
    if jitter is None:
        return x
    gen, amplitude = jitter
    u = torch.rand(x.shape, generator=gen, dtype=torch.float64) * 2 - 1
    return x * (1 + u * amplitude)


def bf16_rne(x, jitter=None):
    """fp64 -> fp32 -> bf16 (both round to nearest even) -> fp64.  jitter = (generator, amplitude): the value is multiplied by
    1 + u * amplitude, u uniform in +-1, first -- an in-kernel intermediate is only known to the fp32 arithmetic that made it."""
    return _jittered(x, jitter).to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_stochastic(gen):
    """A rounding of the same grid with another realisation of the noise: fp32, then up or down in magnitude with the probability
    of the distance (16 random bits added below the bf16 mantissa, then truncated).  The stand-in for a correct kernel."""
    def rnd(x, jitter=None):
        bits = x.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        r = torch.randint(0, 1 << 16, bits.shape, generator=gen, dtype=torch.int64)
        finite = (bits & 0x7F800000) != 0x7F800000
        bits = torch.where(finite, (bits + r) & 0xFFFF0000, bits)
        bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
        return bits.view(torch.float32).to(torch.float64).reshape(x.shape)
    return rnd


class Rounding(object):
    """The switches of one RoundedMM product.  fwd / bwd: round the operands of the forward product / of the two backward products
    (bwd without fwd is not a thing).  a_inter, b_inter, g_inter: the operand (g: the incoming gradient) is an in-kernel
    intermediate, `jitter` applies to it; else it is an input, rounded as it stands.  rnd: the rounding.
    a_scale: callable(a) -> positive tensor f; the FORWARD product rounds a / f and multiplies f back in fp64 (a kernel that rounds
    un-normalised softmax numerators and divides by the row sum afterwards), the backward products take a rounded as it stands."""

    def __init__(self, fwd=True, bwd=True, a_inter=False, b_inter=False, g_inter=False, jitter=None, rnd=bf16_rne, a_scale=None):
        assert fwd or not bwd
        self.fwd, self.bwd, self.a_inter, self.b_inter, self.g_inter, self.jitter, self.rnd = fwd, bwd, a_inter, b_inter, g_inter, jitter, rnd
        self.a_scale = a_scale

    def __call__(self, x, inter):
        return self.rnd(x, self.jitter if inter else None)

    def a_forward(self, a):
        if self.a_scale is None:
            return None
        f = self.a_scale(a)
        return self(a / f, self.a_inter) * f


EXACT = Rounding(fwd=False, bwd=False)


def _sum_to(x, shape):
    """x summed over its broadcast dimensions down to `shape`"""
    while x.dim() > len(shape):
        x = x.sum(0)
    for i, n in enumerate(shape):
        if n == 1 and x.shape[i] != 1:
            x = x.sum(i, keepdim=True)
    return x


class RoundedMM(torch.autograd.Function):
    """a @ b with bf16 operands and an fp64 product: forward bf(a) @ bf(b); backward bf(g) @ bf(b)^T and bf(a)^T @ bf(g)  (the
    operands a kernel stages for its data- and weight-gradient products are the rounded ones again).  With the rounding off: the
    products torch.matmul's own autograd forms, bit for bit (a [.., M, K] @ b [K, N] folds the leading dimensions into the rows,
    so the weight gradient is ONE product over all rows)."""

    @staticmethod
    def forward(ctx, a, b, r):
        ar, br = (r(a, r.a_inter), r(b, r.b_inter)) if r.fwd else (a, b)
        ctx.r = r
        ctx.save_for_backward(*((ar, br) if r.bwd else (a, b)))
        af = r.a_forward(a) if r.fwd else None
        return torch.matmul(ar if af is None else af, br)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        r = ctx.r
        if r.bwd:
            g = r(g, r.g_inter)
        ga = gb = None
        if b.dim() == 2 and a.dim() > 2:
            a2, g2 = a.reshape(-1, a.shape[-1]), g.reshape(-1, g.shape[-1])
            if ctx.needs_input_grad[0]:
                ga = g2.mm(b.t()).reshape(a.shape)
            if ctx.needs_input_grad[1]:
                gb = a2.t().mm(g2)
        else:
            if ctx.needs_input_grad[0]:
                ga = _sum_to(torch.matmul(g, b.transpose(-1, -2)), a.shape)
            if ctx.needs_input_grad[1]:
                gb = _sum_to(torch.matmul(a.transpose(-1, -2), g), b.shape)
        return ga, gb, None


ATTENTION_SITES = (".scores", ".pv")


def product(fwd=True, bwd=True, rnd=bf16_rne, sites=None):
    """the product fm.rounded_products installs: every site rounded alike (the model-level runs use no jitter); sites: only the
    products whose site name ends with one of these are rounded, the others are exact"""
    r = Rounding(fwd=fwd, bwd=bwd, rnd=rnd)
    if sites is None:
        return lambda a, b, site: RoundedMM.apply(a, b, r)
    return lambda a, b, site: RoundedMM.apply(a, b, r) if site.endswith(sites) else a @ b


# ---------------------------------------------------------------------------------------------------------------------------
# the envelope
# ---------------------------------------------------------------------------------------------------------------------------
def own_gates(model, P, hp, batch, drop):
    """the ReLU gates of the exact oracle's own run, by site (what an engine hands over on the GPU)"""
    rec, plain = {}, fm._relu

    def spy(x, site):
        rec[site] = (x.detach() > 0)
        return plain(x, site)
    fm._relu = spy
    try:
        fm.forward(model, P, hp, batch, drop)
    finally:
        fm._relu = plain
    return rec


BIASES = (".b1", ".b2", ".bq", ".bk", ".bv")


def run(model, P, hp, batch, drop, gates, care, prod=None, round_biases=False):
    """one oracle run on handed-over gates (not audited: a rounded run's pre-activations differ at the 8-bit level)"""
    if round_biases:
        P = {k: (bf16_rne(v) if k.endswith(BIASES) else v) for k, v in P.items()}
    with fm.handed_over_gates(gates, care, check=False):
        if prod is None:
            return fm.loss_and_grads(model, P, hp, batch, drop)
        with fm.rounded_products(prod):
            return fm.loss_and_grads(model, P, hp, batch, drop)


def denominators(G):
    """per parameter: its own largest gradient entry, floored at 1e-3 of the global one"""
    gmax = max(float(G[k].abs().max()) for k in G)
    return {k: max(float(G[k].abs().max()), FLOOR * gmax) for k in G}


def deviation(out, G, out0, G0, den):
    """(per-parameter, forward rows, loss) deviation of one run from the exact one, each relative as the bounds are"""
    e = {k: float((G[k] - G0[k]).abs().max()) / den[k] for k in G0}
    a, a0 = out["seq_emb"].detach(), out0["seq_emb"].detach()
    act = float((a - a0).abs().max() / (a0.abs().max() + 1e-12))
    loss = abs(float(out["loss"].detach()) - float(out0["loss"].detach())) / abs(float(out0["loss"].detach()))
    return e, act, loss


def envelope(model, P, hp, batch, drop, gates, care, fp32_row_phases=False):
    """(out_exact, G_exact, E, E_act, E_loss): E[k] = the largest deviation of parameter k's gradient over the model's variants
    from the exact oracle's, relative to max(own largest entry, 1e-3 of the global one); E_act the same for seq_emb (relative to its
    largest entry), E_loss for the loss (relative).  All runs share the handed-over gates and the dropout masks.  Variants:
      (a) every product rounded, forward and backward;
      (b) the forward products only (a backward on fp32 products of stored activations);
      (c) as (a), with the bias vectors b1 b2 bq bk bv rounded too: the register-layout kernels carry the biases in a ones column
          of the bf16 operand;
      (d) with fp32_row_phases only -- an engine whose plan holds the tile kernels cr_block_ln_*, which take no precision and form
          the projections, the feed-forward and their gradients on fp32 products under every attn_precision (read in engine.py
          op_block / _block_bwd_three_launches): the scores and probabilities x V products only, forward and backward."""
    out0, G0 = run(model, P, hp, batch, drop, gates, care)
    den = denominators(G0)
    E, E_act, E_loss = {k: 0.0 for k in G0}, 0.0, 0.0
    variants = [(product(), False), (product(bwd=False), False), (product(), True)]
    if fp32_row_phases:
        variants.append((product(sites=ATTENTION_SITES), False))
    for prod, rb in variants:
        e, act, loss = deviation(*run(model, P, hp, batch, drop, gates, care, prod, rb), out0, G0, den)
        E = {k: max(E[k], e[k]) for k in E}
        E_act, E_loss = max(E_act, act), max(E_loss, loss)
    return out0, G0, E, E_act, E_loss


def grad_bound(E):
    return {k: GRAD_FACTOR * E[k] + GRAD_ABS for k in E}


def grad_report(got, G, E):
    """[(error / bound, name, error, E_k, bound)], worst first; error relative to max(own largest entry, 1e-3 of the global one).
    d loss / d bk == 0 identically (rounding noise on both sides): not listed."""
    den, bound = denominators(G), grad_bound(E)
    rows = []
    for k in G:
        if k.endswith(".bk"):
            continue
        g = got[k].detach().cpu().double() if isinstance(got[k], torch.Tensor) else torch.as_tensor(got[k], dtype=torch.float64)
        err = float((g - G[k]).abs().max()) / den[k]
        rows.append((err / bound[k], k, err, E[k], bound[k]))
    return sorted(rows, reverse=True)

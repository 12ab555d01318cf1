"""Parity of the bf16-MFMA attention kernels (csrc/cr_attn_bf.hip, through the C ABI) against the float64 torch
restatement of modules.py:208-269 (test_ops_gpu.attn_core_ref).

Tolerances (max abs error relative to the tensor's max abs value):
  CR_PREC_BF16X3 (hi + lo split, three products): 2e-4 -- the form whose end-to-end logits must stay within the
                 north star's 1e-3 fp32 bound (checked at model level in test_model_gpu.py); observed ~1e-5
  CR_PREC_BF16   (plain bf16 operands, fp32 accumulation): 3e-2 of the exact reference -- bf16 has 8 significand bits (2^-9 = 2e-3
                 per operand rounding); BASELINE.json configs[1] names bf16, the reference itself is fp32 -- AND, since rounding itself
                 accounts for 2e-3 to 5e-3 of that, so that a 1-2 % defect would pass: the split form's 2e-4 (+ 2 J) of the MATCHED
                 model, the same reference with the operands of its products rounded where the kernels round them (rounded_model)
"""
import numpy as np
import pytest
import torch

import bf16_ref as br
import dropout_ref as dr
from ops_harness import attn_core_ref, dev, new_state, relerr

pytestmark = pytest.mark.gpu

TOL = {1: 2e-4, 2: 3e-2}

CASES = [  # B, T, H, d, rate
    (3, 8, 1, 8, 0.0), (2, 50, 1, 50, 0.0), (2, 200, 1, 50, 0.2), (3, 37, 2, 32, 0.0), (2, 50, 4, 32, 0.5),
    (1, 256, 1, 64, 0.0), (2, 100, 2, 25, 0.3), (5, 16, 1, 50, 0.0), (5, 24, 1, 20, 0.0), (4, 20, 1, 50, 0.2),
    (130, 50, 1, 50, 0.2),          # more (sample, head) pairs than CUs: one workgroup per sample, two rounds of tiles
    (2, 200, 4, 32, 0.2),           # config C4's head geometry (D = 128, 4 heads)
    # T > 256: K / V (Q / dOut) stream through LDS in 256-row chunks, online softmax in the forward
    (3, 257, 1, 50, 0.0), (2, 300, 1, 50, 0.2), (2, 512, 2, 64, 0.0), (2, 512, 4, 64, 0.2), (1, 1024, 1, 16, 0.1),
]


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


def make_case(B, T, H, d, rate, seed_off=0):
    rs = np.random.RandomState(B * 1000 + T + d + seed_off)
    Cc = H * d
    Q = rs.standard_normal((B, T, Cc)); K = rs.standard_normal((B, T, Cc)); V = rs.standard_normal((B, T, Cc))
    resid = rs.standard_normal((B, T, Cc)); dout = rs.standard_normal((B, T, Cc))
    kvalid = (rs.rand(B, T) > 0.2).astype(np.float64); qvalid = (rs.rand(B, T) > 0.1).astype(np.float64)
    kvalid[0, :max(2, T // 4)] = 0                       # left padding: first queries see no valid key -> uniform rows
    if B > 1:
        kvalid[1, :] = 0                                 # a sample with NO valid key at all (CAST context, all bins 0)
    dout[0, 0] = 0
    return Q, K, V, resid, dout, kvalid, qvalid


class SoftmaxRowTerm(torch.autograd.Function):
    """softmax over the last axis; the backward takes its row term from outside: dS = P (dP - delta), delta = cell["delta"] [rows],
    where autograd would form sum_k P dP itself.  cell["P"]: the probabilities of the forward."""

    @staticmethod
    def forward(ctx, s, cell):
        p = torch.softmax(s, -1)
        ctx.save_for_backward(p)
        ctx.cell = cell
        cell["P"] = p.detach()
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return p * (g - ctx.cell["delta"][..., None]), None


JITTER = 2.0 ** -20             # the relative error of an fp32 exp of an argument up to 16: what an in-kernel intermediate carries into its rounding


def rounded_model(Q, K, V, resid, dout, kvalid, qvalid, H, keep, rate, jitter=None):
    """attn_core_ref through bf16_ref.RoundedMM: the matched model of the plain-bf16 kernels (cr_attn_bf.hip).  Q, K, V, dOut are inputs,
    rounded as they stand; the probabilities (after query mask and dropout scale: as multiplied) and dS / sqrt(d) are in-kernel
    intermediates (`jitter` = a generator: +-2^-20 relative before rounding).  Two places where the kernels differ from the plain
    autograd of that model, both read in cr_attn_bf.hip and restated here on the REFERENCE side:
      - delta, the row term of the softmax backward, is sum_c dOut (out - residual) over the head's columns, from the forward's OWN
        (rounded-product) output and the unrounded dOut (bf_bwd_q_pass), where autograd forms sum_k P dP from the exact
        probabilities and the rounded product dP: the two differ at the rounding level, not at fp32's;
      - T > 256 (k_bf_fwd_long, online softmax): the forward rounds the UN-normalised numerators exp(s - m), m the running row
        maximum through the key's 256-key chunk, and divides by the row sum in fp32 afterwards; rows without a valid key take 1/T as
        they are.  The backward passes recompute normalised probabilities and round those (bf_bwd_k_pass)."""
    N, T, C = Q.shape
    d = C // H
    jit = None if jitter is None else (jitter, JITTER)
    cell = {}

    def numerators_scale(a):                             # f with P = exp(s - m_chunk) * f: the largest probability through the key's chunk
        P = cell["P"]
        f = torch.ones_like(P)
        run = torch.zeros(P.shape[:-1], dtype=P.dtype)
        for c0 in range(0, T, 256):
            run = torch.maximum(run, P[..., c0:c0 + 256].max(-1).values)
            f[..., c0:c0 + 256] = run[..., None]
        has_key = (torch.cumsum(torch.tensor(kvalid), 1) > 0).repeat(H, 1)[:, :, None]      # else: a uniform row
        return torch.where((f > 0) & has_key, f, torch.ones_like(f))
    r_scores = br.Rounding(g_inter=True, jitter=jit)
    r_pv = br.Rounding(a_inter=True, jitter=jit, a_scale=numerators_scale if T > 256 else None)
    Qt, Kt, Vt = (torch.tensor(a, requires_grad=True) for a in (Q, K, V))
    out, w = attn_core_ref(Qt, Kt, Vt, torch.tensor(kvalid), torch.tensor(qvalid), torch.tensor(resid), H, keep, rate,
                           mm=lambda a, b, site: br.RoundedMM.apply(a, b, r_scores if site == "scores" else r_pv),
                           softmax=lambda s_: SoftmaxRowTerm.apply(s_, cell))
    dO = torch.tensor(dout)
    cell["delta"] = torch.cat(torch.split(dO * (out.detach() - torch.tensor(resid)), d, dim=2), 0).sum(-1)
    out.backward(dO)
    M = N * T
    return dict(w=w.detach().numpy(), out=out.detach().numpy().reshape(M, C), dV=Vt.grad.numpy().reshape(M, C),
                dQ=Qt.grad.numpy().reshape(M, C), dK=Kt.grad.numpy().reshape(M, C))


def matched_model_and_bounds(Q, K, V, resid, dout, kvalid, qvalid, H, keep, rate):
    """(model, bound per tensor): the unjittered model and TOL[1] + 2 J, J the largest deviation of four jittered runs from it
    (relative to the tensor's largest entry, as relerr)"""
    args = (Q, K, V, resid, dout, kvalid, qvalid, H, keep, rate)
    base = rounded_model(*args)
    J = {k: 0.0 for k in base}
    for seed in range(4):
        run = rounded_model(*args, jitter=torch.Generator().manual_seed(100 + seed))
        J = {k: max(J[k], relerr(run[k], base[k])) for k in base}
    return base, {k: TOL[1] + 2 * J[k] for k in base}, J


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("B,T,H,d,rate", CASES)
def test_attention_bf16_mfma_fwd_bwd(ops, B, T, H, d, rate, prec):
    Q, K, V, resid, dout, kvalid, qvalid = make_case(B, T, H, d, rate)
    Cc, M = H * d, B * T
    ld = Cc + 5
    st = new_state(step=3)
    drop = ops.Drop(rate, seed=11, state=st)
    keep = dr.attn_mask(11, 3, 21, rate, H, B, T) if rate > 0 else None
    Qt, Kt, Vt = (torch.tensor(a, requires_grad=True) for a in (Q, K, V))
    ref, w = attn_core_ref(Qt, Kt, Vt, torch.tensor(kvalid), torch.tensor(qvalid), torch.tensor(resid), H, keep, rate)
    ref.backward(torch.tensor(dout))

    def padded(a):
        buf = torch.full((M, ld), float("nan"), device="cuda")
        buf[:, :Cc] = dev(a.reshape(M, Cc))
        return buf
    Qd, Kd, Vd, Rd, dOd = padded(Q), padded(K), padded(V), padded(resid), padded(dout)
    out = torch.full((M, ld), float("nan"), device="cuda")
    wts = torch.full((H * B, T, T), float("nan"), device="cuda")
    rst = torch.full((H * B * T * 4,), float("nan"), device="cuda")
    kvd, qvd = dev(kvalid.reshape(-1)), dev(qvalid.reshape(-1))
    long_t = T > 256                                     # the chunked forward does not materialise attention_weights
    desc = ops.attn_desc(Qd, Kd, Vd, ld, kvd, qvd, Rd, ld, out, ld, B, T, H, d, rng=drop.rng(21),
                         attn_weights=None if long_t else wts, row_stats=rst, precision=prec)
    ops.attn_fwd(desc)
    dQ, dK, dV = (torch.full((M, ld), float("nan"), device="cuda") for _ in range(3))
    stats = torch.full((H * B * T * 4,), float("nan"), device="cuda")
    ops.attn_bwd(desc, dOd, ld, dQ, dK, dV, ld, stats)           # delta formed inside (from out and residual)
    torch.cuda.synchronize()
    errs = dict(w=0.0 if long_t else relerr(wts, w.detach().numpy()), out=relerr(out[:, :Cc], ref.detach().numpy().reshape(M, Cc)),
                dV=relerr(dV[:, :Cc], Vt.grad.numpy().reshape(M, Cc)), dQ=relerr(dQ[:, :Cc], Qt.grad.numpy().reshape(M, Cc)),
                dK=relerr(dK[:, :Cc], Kt.grad.numpy().reshape(M, Cc)))
    print("bf16-mfma attn errs prec=%d" % prec, errs)
    tol = TOL[prec]
    if prec == 2:
        # the matched model first: plain bf16 held to the split form's bound (+ 2 J); the bound must stay a tenth of 3e-2
        model, bound, J = matched_model_and_bounds(Q, K, V, resid, dout, kvalid, qvalid, H, keep, rate)
        assert max(bound.values()) <= 3e-3, (bound, J)
        got = dict(w=wts, out=out[:, :Cc], dV=dV[:, :Cc], dQ=dQ[:, :Cc], dK=dK[:, :Cc])
        merr = {k: (0.0 if (k == "w" and long_t) else relerr(got[k], model[k])) for k in model}
        print("   against the matched model:", merr, " J:", J)
        for k, e in merr.items():
            assert e < bound[k], (k, merr, bound)
    for k, e in errs.items():
        assert e < tol, (k, errs)
    assert torch.isnan(out[:, Cc:]).all() and torch.isnan(dQ[:, Cc:]).all()      # nothing written outside the head blocks
    if H == 1:
        # delta supplied by the caller (the fused FFN backward emits it): same result
        delta = (dOd[:, :Cc] * (out[:, :Cc] - Rd[:, :Cc])).sum(1).contiguous()
        dQ2, dK2, dV2 = (torch.full((M, ld), float("nan"), device="cuda") for _ in range(3))
        part = torch.full((M, ld), float("nan"), device="cuda")
        ops.attn_bwd(desc, dOd, ld, dQ2, dK2, dV2, ld, stats, delta=delta, dQ_part=part)
        torch.cuda.synchronize()
        assert relerr(dQ2[:, :Cc] + part[:, :Cc], Qt.grad.numpy().reshape(M, Cc)) < tol
        assert relerr(dK2[:, :Cc], Kt.grad.numpy().reshape(M, Cc)) < tol
        assert relerr(dV2[:, :Cc], Vt.grad.numpy().reshape(M, Cc)) < tol
        if prec == 2:
            assert relerr(dQ2[:, :Cc] + part[:, :Cc], model["dQ"]) < bound["dQ"]
            assert relerr(dK2[:, :Cc], model["dK"]) < bound["dK"] and relerr(dV2[:, :Cc], model["dV"]) < bound["dV"]


def test_attention_bf16_mfma_is_reproducible(ops):
    """No atomics anywhere: two launches on the same inputs are bitwise equal."""
    B, T, H, d, rate = 3, 200, 1, 50, 0.2
    Q, K, V, resid, dout, kvalid, qvalid = make_case(B, T, H, d, rate)
    M = B * T
    st = new_state(step=5)
    drop = ops.Drop(rate, seed=3, state=st)
    Qd, Kd, Vd, Rd, dOd = (dev(a.reshape(M, d)) for a in (Q, K, V, resid, dout))
    kvd, qvd = dev(kvalid.reshape(-1)), dev(qvalid.reshape(-1))
    res = []
    for _ in range(2):
        out = torch.empty(M, d, device="cuda"); rst = torch.empty(B * T * 4, device="cuda")
        desc = ops.attn_desc(Qd, Kd, Vd, d, kvd, qvd, Rd, d, out, d, B, T, H, d, rng=drop.rng(7), row_stats=rst, precision=1)
        ops.attn_fwd(desc)
        dQ, dK, dV = (torch.empty(M, d, device="cuda") for _ in range(3))
        ops.attn_bwd(desc, dOd, d, dQ, dK, dV, d, torch.empty(B * T * 4, device="cuda"))
        torch.cuda.synchronize()
        res.append((out, dQ, dK, dV))
    for a, b in zip(*res):
        assert torch.equal(a, b)

"""What the whole-model GPU tests share (test_model_gpu, test_full_size_gpu, test_bf16_envelope_gpu and the loss tests): the engine
fixture, the oracle's dropout masks and ReLU gates taken from an engine, the tolerances per precision and the one-step parity run
_other_shapes."""
import numpy as np
import pytest
import torch

import bf16_ref as br
import dropout_ref as dr
from bf16_ref import make_batch
from oracle import fpmodel as fm


@pytest.fixture(scope="module")
def E():
    import castrec_amd  # noqa: F401
    from castrec_amd import engine
    return engine


def oracle_drop(eng_mod, seed, step, rate, B, T, H):
    def drop(site, shape):
        sid = eng_mod.site_id(site)
        if site.endswith(".attn"):
            return torch.tensor(dr.attn_mask(seed, step, sid, rate, H, B, T))
        ncol = shape[-1]
        return torch.tensor(dr.rows_mask(seed, step, sid, rate, B * T, ncol).reshape(shape))
    return drop


def rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


# ("bf16": what stays of the bounds from before the rounding model, beside the envelope's -- act and loss as they were; grad only sizes
#  the check that d loss / d bk vanishes)
TOL = {"f32": dict(grad=2e-4, act=2e-5, loss=2e-5, auc=1e-6), "bf16x3": dict(grad=2e-3, act=2e-4, loss=2e-4, auc=1e-6),
       "bf16": dict(grad=2e-1, act=3e-2, loss=2e-2, auc=None)}
assert br.GRAD_ABS == TOL["bf16x3"]["grad"] and br.ACT_ABS == TOL["bf16x3"]["act"] and br.LOSS_ABS == TOL["bf16x3"]["loss"]


def engine_relu_gates(eng, B, T, drop):
    """(gates, care): the ReLU gates of an engine's last forward, by the oracle's site names (fpmodel.RELU_GATES): read from
    the stored post-ReLU activations (FFN hidden: post-dropout, so a dropped unit's gate is unknown -- and irrelevant, its
    mask is 0: `care` is False there, and fpmodel.handed_over_gates audits the rest against the oracle's own pre > 0)."""
    gates, care = {}, {}
    live = (eng.ids["seq"] != 0).reshape(B * T, 1)              # every block ends with `*= mask` (sasrec.py:83): a padded row has no gradient
    for name, buf in eng._bufs.items():
        if name.endswith(".hid"):
            site = name[:-4]                                    # "trunk.0"
            g = buf > 0
            c = live.expand(B * T, buf.shape[1])
            if drop is not None:
                kept = drop(site + ".ffn1", (B * T, buf.shape[1])).reshape(B * T, -1).to(g.device)
                g = g | ~kept
                c = c & kept
            care[site + ".relu"] = c.reshape(B, T, -1).cpu()
            gates[site + ".relu"] = g.reshape(B, T, -1).cpu()
    if "mlp.h" in eng._bufs:
        gates["mlp.relu1"] = (eng._bufs["mlp.h"] > 0).reshape(B, T, -1).cpu()
        outb = eng._bufs["seq_emb"] if eng.model in ("cast_5", "cast_6") else eng._bufs["x0"]
        rowlive = (eng.ids["seq"] != 0).reshape(B * T, 1) if eng.model == "cast_9" else torch.ones(B * T, 1, dtype=torch.bool, device=outb.device)
        gates["mlp.relu2"] = ((outb > 0) | ~rowlive).reshape(B, T, -1).cpu()     # cast_9 masks the rows after the ReLU (their gradient is 0)
        care["mlp.relu2"] = rowlive.expand(B * T, outb.shape[1]).reshape(B, T, -1).cpu()
    return gates, care


def oracle_with_engine_gates(eng, B, T, drop, prec, fn):
    """fn() = the oracle run.  f32: the oracle's own gates.  Split precision: the engine's gates, audited (differences only
    at the kink, on < 1e-3 of the units: fpmodel.handed_over_gates).  Plain bf16 (activations differ by 1e-2; the
    throughput option, not a parity claim): handed over without the audit."""
    if prec == "f32":
        return fn()
    gates, care = engine_relu_gates(eng, B, T, drop)
    with fm.handed_over_gates(gates, care, check=(prec == "bf16x3")):
        return fn()


def oracle_or_envelope(eng, model, P, ohp, batch, B, T, drop, prec):
    """(out, G, env): the oracle's run on the engine's masks (and, off f32, gates: oracle_with_engine_gates); plain bf16: with the
    rounding model's envelope of that run env = (E, E_act, E_loss) (bf16_ref.envelope: three model runs on the same gates and masks,
    a fourth where the plan holds the tile kernels cr_block_ln_*, whose row phases are fp32 products whatever the precision)."""
    if prec != "bf16":
        return oracle_with_engine_gates(eng, B, T, drop, prec, lambda: fm.loss_and_grads(model, P, ohp, batch, drop)) + (None,)
    gates, care = engine_relu_gates(eng, B, T, drop)
    tile_kernels = any(n.startswith("cr_block_ln_") for n, _, _ in eng.fwd + eng.bwd)
    out, G, Eg, E_act, E_loss = br.envelope(model, P, ohp, batch, drop, gates, care, fp32_row_phases=tile_kernels)
    return out, G, (Eg, E_act, E_loss)


def act_loss_tol(prec, env):
    """plain bf16: 3 E + the bf16x3 bound, and never looser than the bound from before the model"""
    tol = TOL[prec]
    if prec != "bf16":
        return tol["act"], tol["loss"]
    return min(tol["act"], br.GRAD_FACTOR * env[1] + br.ACT_ABS), min(tol["loss"], br.GRAD_FACTOR * env[2] + br.LOSS_ABS)


def worst_grad_error(got, G, prec, env=None):
    """(error, parameter name, threshold): largest element error of a parameter against that parameter's largest
    gradient (floored at 1e-3 of the global scale).  Plain bf16: the error as a share of the parameter's own bound
    (3 E_k + 2e-3) of that scale (bf16_ref.grad_report), threshold 1.  d loss / d bk == 0 identically (rounding noise on both
    sides): not compared."""
    if prec == "bf16":
        rep = br.grad_report(got, G, env[0])
        share, k, err, Ek, bound = rep[0]
        return share, "%s: error %.3g of its own scale, E %.3g, bound %.3g" % (k, err, Ek, bound), 1.0
    gmax = max(float(G[k].abs().max()) for k in G)
    names = [k for k in G if not k.endswith(".bk")]
    def emax(k):
        a = got[k].cpu().double().numpy(); b = G[k].numpy()
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * gmax))
    w = max((emax(k), k) for k in names)
    return w[0], w[1], TOL[prec]["grad"]


def _other_shapes(E, model, D, H, T, L, B=3, prec="f32", itemnum=41, max_bins=9, zipf=None, kink_free=False, n_slabs=5, dropout=0.1, grad_tol=None,
                  draw=0, report=None):
    """kink_free: the feed-forward pre-activations are pushed away from the ReLU kink (small W1, biases of +-1 alternating by
    unit), the oracle runs with ITS OWN gates (no hand-over), and the test first proves that the engine's gates are the
    same everywhere: gradient parity of the split-precision kernels with nothing taken from the engine but the dropout masks."""
    rs = np.random.RandomState(D + T + draw)
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=L, num_heads=H, dropout_rate=dropout, max_bins=max_bins,
                 num_context_blocks=1, lr=1e-3, seed=11)
    ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=L, num_heads=H, dropout_rate=dropout, max_bins=max_bins,
                   num_context_blocks=1, lr=1e-3)
    eng = E.Engine(model, 9, itemnum, hp, B, training=True, n_slabs=n_slabs, attn_precision=prec)      # n_slabs None: the engine's own choice
    assert eng.fused == (D <= 64)
    P = fm.init_params(model, 9, itemnum, ohp, seed=8)
    P = {k: v + 0.05 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
    if kink_free:
        assert not any(k.startswith("mlp.") for k in P)
        for k in P:
            if k.endswith(".w1"):
                P[k] = 0.1 * P[k]
            elif k.endswith(".b1"):
                P[k] = torch.where(torch.arange(P[k].numel()) % 2 == 0, 1.0, -1.0).to(P[k].dtype).reshape(P[k].shape)
    eng.load_params(P)
    P = {k: v.double().cpu() for k, v in eng.get_params().items()}
    seq, pos, neg, time, hours, days = make_batch(rs, B, T, itemnum, max_bins)
    if zipf:                                             # long-tail ids: a few hot rows take most of the scatter / head atomics
        w = 1.0 / np.arange(1, itemnum + 1, dtype=np.float64) ** zipf
        cdf = np.cumsum(w / w.sum())
        draw = lambda: (np.searchsorted(cdf, rs.random_sample((B, T))).clip(0, itemnum - 1) + 1)
        live = seq != 0
        seq, pos, neg = draw() * live, draw() * live, draw() * live
    eng.set_batch(seq, pos, neg, time, hours, days)
    eng.launch_step(apply=False)
    torch.cuda.synchronize()
    drop = oracle_drop(E, 11, 1, dropout, B, T, H)
    # split-precision attention perturbs activations by ~1e-5: the oracle takes the engine's ReLU gates like it takes its
    # dropout masks, so that units within 1e-5 of the kink do not flip on one side only (see fpmodel.RELU_GATES)
    batch = fm.to_batch(seq, pos, neg, time, hours, days)
    run = lambda: fm.loss_and_grads(model, P, ohp, batch, drop)
    env = None
    if kink_free:
        gates, care = engine_relu_gates(eng, B, T, drop)
        with fm.handed_over_gates(gates, care, max_share=0.0, min_units=0) as audit:      # premise: not ONE gate differs ...
            run()
        assert audit and all(a[0] > 0 for a in audit.values())
        assert all(float(g.float().mean()) > 0.2 and float(g.float().mean()) < 0.8 for g in gates.values())   # ... on a real on / off mix
        out, G = run()                                                                    # the oracle on its own gates
    else:
        out, G, env = oracle_or_envelope(eng, model, P, ohp, batch, B, T, drop, prec)
    act_tol, loss_tol = act_loss_tol(prec, env)
    st = eng.state.cpu().numpy()
    loss_ref = float(out["loss"].detach())
    loss_err = abs(float(st[0] / st[2]) - loss_ref) / abs(loss_ref)
    got = eng.grads()
    worst = worst_grad_error(got, G, prec, env)
    act_err = rel(eng.seq_emb, out["seq_emb"].reshape(B * T, -1))
    if prec == "bf16":
        print("plain bf16 %s D %d H %d T %d B %d: loss %.3g (bound %.3g), rows %.3g (bound %.3g), worst gradient at %.2f of its bound (%s)"
              % (model, D, H, T, B, loss_err, loss_tol, act_err, act_tol, worst[0], worst[1]))
    if report is not None:                               # (tools/probes/bf16_vs_oracle.py: the figures, taken before anything is asserted)
        report.append(dict(eng=eng, loss=(loss_err, loss_tol), act=(act_err, act_tol), worst=worst,
                           grads=br.grad_report(got, G, env[0]) if env is not None else None, env=env))
    assert loss_err <= loss_tol, (loss_err, loss_tol)
    # (f32 / bf16x3: twice the bound of the small-shape cases; plain bf16: the parameter's own bound, nothing on top)
    assert worst[0] < ((1 if prec == "bf16" else 2) * worst[2] if grad_tol is None else grad_tol), worst
    assert act_err < act_tol, (act_err, act_tol)                                # forward parity (north-star bound 1e-3)
    return eng

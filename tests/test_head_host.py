"""tests/head_ref.py on the CPU: a plain fp32 torch evaluation of the same graph must stay below HALF of every bound tests/test_head_gpu.py
holds the kernels to (the reference and the number format together leave the kernels at least the other half), and a head that forgets
the padding mask must not pass."""
import numpy as np
import pytest
import torch

import head_ref as R

BOUNDS = {"pl": 2e-6, "nl": 2e-6, "loss": 2e-6, "d_seq_emb": 3e-6, "table_grad": 3e-6, "coef": 3e-6, "dx": 2e-5, "dgamma": 5e-6, "dbeta": 5e-6}


def fp32_head(P, masked=True):
    f = lambda a: torch.tensor(a, dtype=torch.float32, requires_grad=True)
    x, g, b, tab = f(P.x), f(P.gamma), f(P.beta), f(P.table)
    mean = x.mean(-1, keepdim=True); var = ((x - mean) ** 2).mean(-1, keepdim=True)
    s = g * ((x - mean) / (var + R.EPS) ** 0.5) + b
    s.retain_grad()
    tz = torch.cat([torch.zeros(1, P.D), tab[1:]], 0)
    pl = (tz[P.pos.astype(np.int64)] * s).sum(-1); nl = (tz[P.neg.astype(np.int64)] * s).sum(-1)
    pl.retain_grad(); nl.retain_grad()
    ist = torch.tensor((P.pos != 0).astype(np.float32)) if masked else torch.ones(P.M)
    loss = ((-torch.log(torch.sigmoid(pl) + 1e-24) - torch.log(1 - torch.sigmoid(nl) + 1e-24)) * ist).sum()
    loss.backward()
    return dict(pl=pl.detach(), nl=nl.detach(), loss=loss.detach(), d_seq_emb=s.grad, table_grad=tab.grad, coef=torch.stack([pl.grad, nl.grad]),
                dx=x.grad, dgamma=g.grad, dbeta=b.grad)


def errors(P, got):
    rel = lambda a, w: float(np.abs(a.double().numpy() - w).max() / (np.abs(w).max() + 1e-30))
    return {k: rel(v, np.asarray(getattr(P.ln, k), np.float64)) for k, v in got.items()}


@pytest.mark.parametrize("M,D", [(261, 50), (133, 72), (69, 260), (5, 24)])
def test_fp32_evaluation_stays_under_half_of_every_bound(M, D):
    err = errors(R.problem(M, D), fp32_head(R.problem(M, D)))
    print({k: "%.1e" % v for k, v in err.items()})
    assert all(v < 0.5 * BOUNDS[k] for k, v in err.items()), err


def test_a_head_without_the_padding_mask_is_rejected():
    P = R.problem(261, 50)
    err = errors(P, fp32_head(P, masked=False))
    assert all(err[k] > BOUNDS[k] for k in ("loss", "d_seq_emb", "table_grad", "coef", "dx", "dgamma", "dbeta")), err
    assert (P.pos == 0).sum() > 3 and ((P.pos != 0) & (P.neg == 0)).sum() > 3 and len(set(P.pos[P.pos != 0])) < (P.pos != 0).sum()

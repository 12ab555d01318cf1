"""Times cr_softmax_ce (full-catalogue softmax cross-entropy, csrc/cr_ce.hip) with HIP events at the shapes of DESIGN.md section 11,
against the MFMA roof, beside a torch fp32 composition of the same computation (matmul -> logsumexp -> the two gradient matmuls,
chunked over rows where the [M, V] matrix does not fit), and the CAST1 training step at the headline shape with loss "bce" and "ce".

    python tools/ce_bench.py [--shapes a,b] [--reps 5] [--out DIR/ce_bench.json] [--no-torch] [--no-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import castrec_amd  # noqa: E402,F401
from castrec_amd import engine as E  # noqa: E402
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402

SHAPES = {"a": ("headline, ml-1m", 25600, 3417, 50), "b": ("C4 vocabulary", 25600, 368001, 128)}
BF16_PEAK = 2.5e15                # dense bf16 MFMA FLOP / s (spec)


def _time(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    out.sort()
    return out[len(out) // 2], out


def torch_ce(h, table, pos, chunk):
    """fp32 torch: loss sum, dh, dE of the same objective, `chunk` rows at a time."""
    T = table[1:]
    dE = torch.zeros_like(table)
    dh = torch.empty_like(h)
    loss = torch.zeros((), device=h.device)
    for r0 in range(0, h.shape[0], chunk):
        hs, ps = h[r0:r0 + chunk], pos[r0:r0 + chunk].long()
        s = hs @ T.t()
        lse = torch.logsumexp(s, 1)
        ist = (ps != 0).float()
        g = torch.exp(s - lse[:, None])
        idx = (ps.clamp(min=1) - 1)[:, None]
        loss = loss + ((lse - s.gather(1, idx)[:, 0]) * ist).sum()
        g.scatter_add_(1, idx, -torch.ones_like(idx, dtype=g.dtype))
        g *= ist[:, None]
        dh[r0:r0 + chunk] = g @ T
        dE[1:] += g.t() @ hs
    return loss, dh, dE


def run(key, reps, with_torch):
    name, M, V, D = SHAPES[key]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g) * 0.5
    h = torch.randn(M, D, device="cuda", generator=g) * (1.0 / D ** 0.5)
    pos = torch.randint(1, V, (M,), device="cuda", generator=g, dtype=torch.int32)
    pos[torch.rand(M, device="cuda", generator=g) < 0.2] = 0
    neg = torch.randint(1, V, (M,), device="cuda", generator=g, dtype=torch.int32)
    st = torch.zeros(L.CR_STATE_FLOATS, device="cuda")
    dh = torch.empty(M, D, device="cuda")
    tg = torch.zeros(V, D, device="cuda")
    ws = torch.empty(O.softmax_ce_workspace_bytes(M, V, D), dtype=torch.uint8, device="cuda")
    dpad = (D + 31) // 32 * 32
    dpad = 32 if dpad <= 32 else 64 if dpad <= 64 else 128 if dpad <= 128 else 256
    res = []
    for prec, pname, nprod in ((L.PREC_BF16X3, "bf16x3", 3), (L.PREC_BF16, "bf16", 1)):
        fn = lambda: O.softmax_ce(h, D, table, pos, st, ws, M, precision=prec, neg=neg, d_seq_emb=dh, ldd=D, table_grad=tg)
        t, all_t = _time(fn, reps)
        flop = 3 * nprod * 2.0 * M * (V - 1) * dpad                 # three passes, each a [M, V] x D product (padded k)
        r = dict(shape=key, name=name, M=M, V=V, D=D, D_padded=dpad, precision=pname, time_s=t, times_s=all_t, mfma_flop=flop,
                 mfma_roof_s=flop / BF16_PEAK, mfma_fraction=flop / BF16_PEAK / t, workspace_bytes=ws.numel())
        res.append(r)
    if with_torch:
        chunk = M if M * V * 4 <= 2 * 2 ** 30 else max(256, (2 * 2 ** 30) // (V * 4) // 256 * 256)
        try:
            tb, tall = _time(lambda: torch_ce(h, table, pos, chunk), max(3, reps // 2), warm=1)
            loss_t, dh_t, dE_t = torch_ce(h, table, pos, chunk)
            st.zero_(); tg.zero_()
            O.softmax_ce(h, D, table, pos, st, ws, M, precision=L.PREC_BF16X3, neg=neg, d_seq_emb=dh, ldd=D, table_grad=tg)
            torch.cuda.synchronize()
            agree = dict(loss_rel=float(abs(st[0] - loss_t) / abs(loss_t)),
                         dh_rel=float((dh - dh_t).abs().max() / dh_t.abs().max()),
                         dE_rel=float((tg - dE_t).abs().max() / dE_t.abs().max()))
            for r in res:
                r.update(torch_fp32_s=tb, torch_fp32_times_s=tall, torch_chunk_rows=chunk, speedup_vs_torch=tb / r["time_s"])
            res[0]["agree_with_torch_fp32"] = agree
        except RuntimeError as e:                         # (out of memory: reported, not fatal)
            res[0]["torch_error"] = str(e)[:200]
        torch.cuda.empty_cache()
    for r in res:
        print(json.dumps(r), flush=True)
    return res


def train_step_ms(loss, reps, prepare=None, **engine_kw):
    """CAST1 at the headline shape (bench.py HEADLINE: B 128, maxlen 200, D 50, 2 blocks), one captured step per launch.
    engine_kw: further Engine options; prepare(eng): what the engine needs before its first step."""
    B, T, itemnum = 128, 200, 3416
    hp = E.Hyper(maxlen=T, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, max_bins=200, lr=1e-3, seed=42)
    eng = E.Engine("cast_1", 6040, itemnum, hp, B, training=True, loss=loss, **engine_kw)
    if prepare is not None:
        prepare(eng)
    rs = np.random.RandomState(0)
    seq = rs.randint(1, itemnum + 1, (B, T)); seq[:, :20] = 0
    pos = rs.randint(1, itemnum + 1, (B, T)) * (seq != 0); neg = rs.randint(1, itemnum + 1, (B, T)) * (seq != 0)
    time_ = rs.randint(0, 201, (B, T)) * (seq != 0)
    eng.set_batch(seq, pos, neg, time_, np.zeros_like(seq), np.zeros_like(seq))
    eng.capture()
    eng.set_step(1)
    n = 20

    def steps():
        for _ in range(n):
            eng.graph.launch()
    t, _ = _time(steps, reps)
    r = dict(model="cast_1", B=B, T=T, D=50, loss=loss, ms_per_step=1e3 * t / n, launches=eng.n_kernel_launches(),
             loss_after=eng.loss_auc()[0], **engine_kw)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    res = [r for k in a.shapes.split(",") for r in run(k, a.reps, not a.no_torch)]
    steps = [] if a.no_step else [train_step_ms(l, a.reps) for l in ("bce", "ce")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res, train_step=steps), f, indent=1)


if __name__ == "__main__":
    main()

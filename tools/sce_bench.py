"""Times cr_sampled_ce (sampled softmax cross-entropy with shared uniform negatives, csrc/cr_ce.hip) with HIP events at the shapes of
DESIGN.md section 12, against the MFMA roof, beside cr_softmax_ce at the same shape (where it is affordable) and a torch fp32
composition of the same loss (gather -> matmul -> mask -> logsumexp -> the two gradient matmuls), and the CAST1 training step at the
headline shape with loss "bce", "ce" and "sampled_ce" (N = 256).

    python tools/sce_bench.py [--shapes a,b,c] [--reps 7] [--out DIR/sce_bench.json] [--no-torch] [--no-ce] [--no-step]

--proposal popularity draws the negatives from Zipf item weights (seeded) and applies the log-Q correction.
--ab times that proposal (B) against the uniform one (A) in this process, interleaved A B A B, and reports the ratio of the medians;
with --proposal uniform both sides are the uniform path: the A/A spread such a ratio has to be read against.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import castrec_amd  # noqa: E402,F401
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402
from ce_bench import _time, train_step_ms  # noqa: E402

# key: (name, M, V, D, sample counts)
SHAPES = {"a": ("headline, ml-1m", 25600, 3417, 50, (256, 1024)),
          "b": ("C4 vocabulary", 25600, 368001, 128, (1024, 4096)),
          "c": ("C5 table", 128 * 512, 10 ** 7, 256, (4096,))}
BF16_PEAK = 2.5e15                # dense bf16 MFMA FLOP / s (spec)


def torch_sce(h, table, pos, s):
    """fp32 torch: loss sum, dh, dE of the same objective with the ids s [N]."""
    pl = pos.long()
    sl = s.long()
    Es = table[sl]
    Et = table[pl]
    S = h @ Es.t()
    st = (h * Et).sum(1)
    S.masked_fill_(sl[None, :] == pl[:, None], float("-inf"))
    lse = torch.logsumexp(torch.cat([st[:, None], S], 1), 1)
    ist = (pl != 0).float()
    P = torch.exp(S - lse[:, None]) * ist[:, None]
    gt = (torch.exp(st - lse) - 1.0) * ist
    dh = P @ Es + gt[:, None] * Et
    dE = torch.zeros_like(table)
    dE.index_add_(0, sl, P.t() @ h)
    dE.index_add_(0, pl, gt[:, None] * h)
    return ((lse - st) * ist).sum(), dh, dE


def zipf_proposal(V, seed=0):
    """Device (cdf, logq) of the weights floor(10^6 / rank^1.1) + 1 dealt to the ids by RandomState(seed)."""
    from castrec_amd.proposal import build_proposal
    w = np.floor(1e6 / np.arange(1, V + 1, dtype=np.float64) ** 1.1) + 1.0
    np.random.RandomState(seed).shuffle(w)
    cdf, logq = build_proposal(w, V)
    return torch.from_numpy(cdf.view(np.int32)).cuda(), torch.from_numpy(logq).cuda()


def _time_ab(fa, fb, reps, warm=2):
    """Medians and sorted times of fa and fb timed in turn (A B A B ...), HIP events."""
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e-3)
    for o in out:
        o.sort()
    return out[0][reps // 2], out[0], out[1][reps // 2], out[1]


def _dpad(D):
    d = (D + 31) // 32 * 32
    return 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 256


def run(key, reps, with_torch, with_ce, proposal="uniform", ab=False):
    name, M, V, D, Ns = SHAPES[key]
    cdf, logq = zipf_proposal(V) if proposal == "popularity" else (None, None)
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g) * 0.5
    h = torch.randn(M, D, device="cuda", generator=g) * (1.0 / D ** 0.5)
    pos = torch.randint(1, V, (M,), device="cuda", generator=g, dtype=torch.int32)
    pos[torch.rand(M, device="cuda", generator=g) < 0.2] = 0
    neg = torch.randint(1, V, (M,), device="cuda", generator=g, dtype=torch.int32)
    st = torch.zeros(L.CR_STATE_FLOATS, device="cuda")
    st[4:5].view(torch.int32)[0] = 1
    dh = torch.empty(M, D, device="cuda")
    tg = torch.zeros(V, D, device="cuda")
    dpad = _dpad(D)
    ce_t = None
    if with_ce and key != "c":
        ws = torch.empty(O.softmax_ce_workspace_bytes(M, V, D), dtype=torch.uint8, device="cuda")
        ce_t, _ = _time(lambda: O.softmax_ce(h, D, table, pos, st, ws, M, neg=neg, d_seq_emb=dh, ldd=D, table_grad=tg), reps)
        del ws
    res = []
    for N in Ns:
        ws = torch.empty(O.sampled_ce_workspace_bytes(M, N, D), dtype=torch.uint8, device="cuda")
        so = torch.empty(N, dtype=torch.int32, device="cuda")
        for prec, pname, nprod in ((L.PREC_BF16X3, "bf16x3", 3), (L.PREC_BF16, "bf16", 1)):
            fn = lambda: O.sampled_ce(h, D, table, pos, st, ws, M, N, precision=prec, neg=neg, seed=42, step=st[4:5], samples_out=so,
                                      d_seq_emb=dh, ldd=D, table_grad=tg, cdf=cdf, logq=logq)
            if ab:
                fu = lambda: O.sampled_ce(h, D, table, pos, st, ws, M, N, precision=prec, neg=neg, seed=42, step=st[4:5],
                                          samples_out=so, d_seq_emb=dh, ldd=D, table_grad=tg)
                tu, all_u, t, all_t = _time_ab(fu, fn, reps)
            else:
                t, all_t = _time(fn, reps)
            flop = 3 * nprod * 2.0 * M * N * dpad                     # three passes, each a [M, N] x D product (padded k)
            r = dict(shape=key, name=name, M=M, V=V, D=D, N=N, D_padded=dpad, precision=pname, time_s=t, times_s=all_t, mfma_flop=flop,
                     mfma_roof_s=flop / BF16_PEAK, mfma_fraction=flop / BF16_PEAK / t, workspace_bytes=ws.numel(), proposal=proposal)
            if ab:
                r.update(uniform_time_s=tu, uniform_times_s=all_u, ratio_to_uniform=t / tu)
            if ce_t is not None:
                r.update(softmax_ce_bf16x3_s=ce_t, speedup_vs_softmax_ce=ce_t / t)
            res.append(r)
        if with_torch:
            try:
                s = so.clone()
                tb, tall = _time(lambda: torch_sce(h, table, pos, s), reps, warm=1)
                loss_t, dh_t, dE_t = torch_sce(h, table, pos, s)
                st[:4].zero_(); tg.zero_()
                O.sampled_ce(h, D, table, pos, st, ws, M, N, precision=L.PREC_BF16X3, neg=neg, samples=s, d_seq_emb=dh, ldd=D,
                             table_grad=tg)                             # (the uniform objective: what torch_sce states)
                torch.cuda.synchronize()
                agree = dict(loss_rel=float(abs(st[0] - loss_t) / abs(loss_t)),
                             dh_rel=float((dh - dh_t).abs().max() / dh_t.abs().max()),
                             dE_rel=float((tg - dE_t).abs().max() / dE_t.abs().max()))
                del dE_t
                for r in res[-2:]:
                    r.update(torch_fp32_s=tb, torch_fp32_times_s=tall, speedup_vs_torch=tb / r["time_s"])
                res[-2]["agree_with_torch_fp32"] = agree
            except RuntimeError as e:                     # (out of memory: reported, not fatal)
                res[-2]["torch_error"] = str(e)[:200]
            torch.cuda.empty_cache()
        for r in res[-2:]:
            print(json.dumps(r), flush=True)
        del ws
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-ce", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--proposal", choices=["uniform", "popularity"], default="uniform")
    ap.add_argument("--ab", action="store_true", help="time --proposal against the uniform path, interleaved (uniform: the A/A spread)")
    a = ap.parse_args()
    res = []
    for k in a.shapes.split(","):
        res += run(k, a.reps, not a.no_torch, not a.no_ce, a.proposal, a.ab)
        torch.cuda.empty_cache()
    steps = [] if a.no_step else [train_step_ms(l, a.reps) for l in ("bce", "ce", "sampled_ce")]
    if not a.no_step and a.proposal == "popularity":
        w = np.floor(1e6 / np.arange(1, 3418, dtype=np.float64) ** 1.1) + 1.0
        np.random.RandomState(0).shuffle(w)
        steps.append(train_step_ms("sampled_ce", a.reps, prepare=lambda eng: eng.set_item_weights(w), ce_proposal="popularity"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res, train_step=steps), f, indent=1)


if __name__ == "__main__":
    main()

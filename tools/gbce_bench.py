"""Times cr_gbce (gSASRec's generalised binary cross-entropy over shared uniform negatives, csrc/cr_ce.hip) with HIP events at the
shapes of DESIGN.md sections 12 / 13, with the device draw, d_seq_emb and table_grad, in both precisions; in the same process
cr_sampled_ce at the same shape (the yardstick: one candidate sweep more per row) and a torch fp32 composition of the same loss
(gather -> matmul -> mask -> softplus / sigmoid -> the two gradient matmuls + index_add); and the CAST1 training step at the headline
shape with loss "bce", "ce", "sampled_ce" and "gbce" (N = 256).

    python tools/gbce_bench.py [--shapes a,b,c] [--reps 7] [--out DIR/gbce_bench.json] [--no-torch] [--no-step]

--dump DIR writes what cr_softmax_ce, cr_sampled_ce (uniform and popularity proposal, device draw) and cr_gbce compute at the cases of
DUMP_CASES per precision, and at one of them with each optional pointer NULL (state, lse_out, d_seq_emb, samples and the table_grad
rows that are no row's target: the outputs that have the same bits on every call) as .npy files, and exits;
--lib PATH runs that through another build of libcastrec.so (loaded beside this one: lib.py binds every symbol of this header on
import, so an older build cannot stand in through CASTREC_LIB); --compare DIR_A DIR_B says whether two dumps hold the same bits.
"""
import argparse
import ctypes as C
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
from sce_bench import BF16_PEAK, SHAPES, _dpad, zipf_proposal  # noqa: E402


def torch_gbce(h, table, pos, s, beta):
    """fp32 torch: loss sum, dh, dE of the same objective with the ids s [N]."""
    pl = pos.long()
    sl = s.long()
    Es = table[sl]
    Et = table[pl]
    S = h @ Es.t()
    st = (h * Et).sum(1)
    ist = (pl != 0).float()
    live = (sl[None, :] != pl[:, None]).float() * ist[:, None]
    sp = torch.nn.functional.softplus
    loss = ((beta * sp(-st) + (sp(S) * live).sum(1)) * ist).sum()
    G = torch.sigmoid(S) * live
    gt = beta * (torch.sigmoid(st) - 1.0) * ist
    dh = G @ Es + gt[:, None] * Et
    dE = torch.zeros_like(table)
    dE.index_add_(0, sl, G.t() @ h)
    dE.index_add_(0, pl, gt[:, None] * h)
    return loss, dh, dE


def run(key, reps, with_torch, beta=0.5):
    name, M, V, D, Ns = SHAPES[key]
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
    res = []
    for N in Ns:
        ws = torch.empty(max(O.gbce_workspace_bytes(M, N, D), O.sampled_ce_workspace_bytes(M, N, D)), dtype=torch.uint8, device="cuda")
        so = torch.empty(N, dtype=torch.int32, device="cuda")
        for prec, pname, nprod in ((L.PREC_BF16X3, "bf16x3", 3), (L.PREC_BF16, "bf16", 1)):
            fg = lambda: O.gbce(h, D, table, pos, st, ws, M, N, beta=beta, precision=prec, neg=neg, seed=42, step=st[4:5],
                                samples_out=so, d_seq_emb=dh, ldd=D, table_grad=tg)
            fs = lambda: O.sampled_ce(h, D, table, pos, st, ws, M, N, precision=prec, neg=neg, seed=42, step=st[4:5], samples_out=so,
                                      d_seq_emb=dh, ldd=D, table_grad=tg)
            # the pair interleaved (A B A B): a drift of the box moves both medians
            _time(fg, 1); _time(fs, 1)
            tgs, tss = [], []
            for _ in range(reps):
                tgs.append(_time(fg, 1, warm=0)[0])
                tss.append(_time(fs, 1, warm=0)[0])
            tgs.sort(); tss.sort()
            t, t_sce = tgs[len(tgs) // 2], tss[len(tss) // 2]
            flop = 4 * nprod * 2.0 * M * N * dpad                     # two sweeps (row, item), each a score and a gradient product
            r = dict(shape=key, name=name, M=M, V=V, D=D, N=N, D_padded=dpad, precision=pname, beta=beta, time_s=t, times_s=tgs,
                     sampled_ce_s=t_sce, sampled_ce_times_s=tss, ratio_vs_sampled_ce=t / t_sce, mfma_flop=flop,
                     mfma_roof_s=flop / BF16_PEAK, mfma_fraction=flop / BF16_PEAK / t, workspace_bytes=O.gbce_workspace_bytes(M, N, D))
            res.append(r)
        if with_torch:
            try:
                O.gbce(h, D, table, pos, st, ws, M, N, beta=beta, neg=neg, seed=42, step=st[4:5], samples_out=so)
                s = so.clone()
                tb, tall = _time(lambda: torch_gbce(h, table, pos, s, beta), reps, warm=1)
                loss_t, dh_t, dE_t = torch_gbce(h, table, pos, s, beta)
                st[:4].zero_(); tg.zero_()
                O.gbce(h, D, table, pos, st, ws, M, N, beta=beta, precision=L.PREC_BF16X3, neg=neg, samples=s, d_seq_emb=dh, ldd=D,
                       table_grad=tg)
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


# ---- the candidate-sweep losses, bit for bit -------------------------------------------------------------------------------------
# (M, V, D, N): the smallest shapes that reach each path of csrc/cr_ce.hip
DUMP_CASES = (("nk1", 77, 17, 8, 7),              # one k-step, a ragged row tile, fewer candidates than one block
              ("base", 1300, 3417, 50, 256),      # two k-steps, catalogue parts > 1, more than 64 blocks in the catalogue sweep
              ("nk4", 200, 3417, 100, 300),       # four k-steps, N no multiple of the block
              ("nk8", 130, 1031, 200, 70),        # eight k-steps
              ("long", 100, 3417, 50, 2100))      # sampled kinds only: more than 64 blocks, more than one dedup chunk
DUMP_OPS = ("cr_softmax_ce", "cr_sampled_ce", "cr_sampled_ce_pop", "cr_gbce")      # _pop: popularity proposal, device draw
DUMP_VARIANTS = ("all", "no_neg", "no_dh", "no_tg")                                # the optional pointers NULL: at "base" only


def dump(out_dir, lib_path):
    """Every op of csrc/cr_ce.hip at DUMP_CASES x both precisions, and at "base" with neg, d_seq_emb or table_grad NULL, through
    `lib_path` (None: this build; a build from before an op: without it)."""
    lib = L.lib
    if lib_path:
        lib = C.CDLL(os.path.abspath(lib_path))
        for n, desc in (("cr_softmax_ce", L.SoftmaxCeDesc), ("cr_sampled_ce", L.SampledCeDesc), ("cr_gbce", L.GbceDesc)):
            if not hasattr(lib, n):
                continue
            getattr(lib, n).restype, getattr(lib, n).argtypes = C.c_int, [C.POINTER(desc), C.c_void_p]
            getattr(lib, n + "_workspace").restype, getattr(lib, n + "_workspace").argtypes = C.c_size_t, [C.c_int] * 3
        lib.cr_last_error.restype = C.c_char_p
    os.makedirs(out_dir, exist_ok=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    n_files = 0
    for case, M, V, D, N in DUMP_CASES:
        rs = np.random.RandomState(7)
        h = torch.from_numpy(rs.standard_normal((M, D)).astype(np.float32) * (1.5 / D ** 0.5)).cuda()
        table = torch.from_numpy(rs.standard_normal((V, D)).astype(np.float32) * 1.5).cuda()
        pos_h = rs.randint(1, V, M).astype(np.int32)
        pos_h[rs.rand(M) < 0.3] = 0
        pos = torch.from_numpy(pos_h).cuda()
        neg_all = torch.from_numpy((rs.randint(1, V, M) * (pos_h != 0)).astype(np.int32)).cuda()
        cdf, logq = zipf_proposal(V)
        keep = np.ones(V, bool)
        keep[pos_h] = False                               # the sampled ops' target rows take float atomics
        for variant in (DUMP_VARIANTS if case == "base" else DUMP_VARIANTS[:1]):
            for prec, pname in ((L.PREC_BF16X3, "bf16x3"), (L.PREC_BF16, "bf16")):
                for op in DUMP_OPS:
                    fn = op[:-4] if op.endswith("_pop") else op
                    if not hasattr(lib, fn) or (case == "long" and op == "cr_softmax_ce"):
                        continue
                    st = torch.zeros(L.CR_STATE_FLOATS, device="cuda")
                    st[4:5].view(torch.int32)[0] = 3
                    neg = None if variant == "no_neg" else neg_all
                    dh = None if variant == "no_dh" else torch.zeros(M, D, device="cuda")
                    tg = None if variant == "no_tg" else torch.zeros(V, D, device="cuda")
                    lse = torch.zeros(M, device="cuda")
                    so = torch.zeros(N, dtype=torch.int32, device="cuda")
                    if op == "cr_softmax_ce":
                        ws = torch.empty(lib.cr_softmax_ce_workspace(M, V, D), dtype=torch.uint8, device="cuda")
                        d = L.SoftmaxCeDesc(p(h), D, p(table), p(pos), p(neg), M, D, V, prec, p(st), p(dh), D, p(tg), p(lse), p(ws),
                                            ws.numel())
                    elif op == "cr_gbce":
                        ws = torch.empty(lib.cr_gbce_workspace(M, N, D), dtype=torch.uint8, device="cuda")
                        d = L.GbceDesc(p(h), D, p(table), p(pos), p(neg), M, D, V, N, prec, 0.4, None, 42, p(st) + 16, p(so), p(st), p(dh),
                                       D, p(tg), p(lse), p(ws), ws.numel())
                    else:
                        ws = torch.empty(lib.cr_sampled_ce_workspace(M, N, D), dtype=torch.uint8, device="cuda")
                        pop = op.endswith("_pop")
                        d = L.SampledCeDesc(p(h), D, p(table), p(pos), p(neg), M, D, V, N, prec, None, 42, p(st) + 16, p(so), p(st), p(dh),
                                            D, p(tg), p(lse), p(ws), ws.numel(), p(cdf) if pop else None, p(logq) if pop else None)
                    rc = getattr(lib, fn)(C.byref(d), stream)
                    if rc != 0:
                        raise RuntimeError("%s failed: %s" % (op, lib.cr_last_error().decode()))
                    torch.cuda.synchronize()
                    outs = dict(state=st, lse_out=lse, samples=so)
                    if dh is not None:
                        outs["d_seq_emb"] = dh
                    if tg is not None:
                        outs["table_grad"] = tg if op == "cr_softmax_ce" else tg.cpu()[torch.from_numpy(keep)]
                    for k, v in outs.items():
                        np.save(os.path.join(out_dir, "%s_%s_%s_%s_%s.npy" % (case, variant, op, pname, k)), v.cpu().numpy())
                        n_files += 1
    print("dumped %d arrays to" % n_files, out_dir, "through", lib_path or L.LIB_PATH)


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    same = names == sorted(f for f in os.listdir(b) if f.endswith(".npy")) and bool(names)
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        ok = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print("%-50s %s" % (f, "identical" if ok else "DIFFERENT"))
        same = same and ok
    print("all identical" if same else "NOT identical")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--dump", default=None, metavar="DIR")
    ap.add_argument("--lib", default=None, metavar="PATH")
    ap.add_argument("--compare", nargs=2, default=None, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.dump:
        dump(a.dump, a.lib)
        return 0
    res = []
    for k in [k for k in a.shapes.split(",") if k]:
        res += run(k, a.reps, not a.no_torch)
        torch.cuda.empty_cache()
    steps = [] if a.no_step else [train_step_ms(l, a.reps) for l in ("bce", "ce", "sampled_ce", "gbce")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res, train_step=steps), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

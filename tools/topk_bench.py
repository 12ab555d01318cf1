"""Times cr_score_topk (full-catalogue top-K, csrc/cr_topk.hip) with HIP events at the shapes of DESIGN.md "Full-catalogue top-K",
against the HBM and MFMA roofs, beside torch.matmul (fp32) + torch.topk where the [B, V] score matrix fits.

    python tools/topk_bench.py [--shapes a,b,c,d] [--reps 5] [--out DIR/topk_bench.json] [--no-torch]

--index compares the search of an item index (castrec.h cr_topk_index_build, cr_topk_desc.index) with the search of the table it was built
from, in one process: per sample table, index, table again (the second table series is the A/A spread the ratio is judged against), median of
--reps 7 samples of HIP-event time, every sample long enough to time (--min-sample seconds of back-to-back calls), both precisions; the build
timed on its own; at (c) and (d) also a plain-bf16 index (half the bytes).  Default --out: profiles/topk/topk_index_bench.json.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import castrec_amd  # noqa: E402,F401
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402

SHAPES = {"a": ("ml-1m", 3416, 50, 6040, 10), "b": ("C4 vocabulary", 368000, 128, 10000, 10),
          "c": ("C5 table, 128 users", 10 ** 7, 256, 128, 100), "d": ("C5 table, 1024 users", 10 ** 7, 256, 1024, 100)}
HBM = 8.0e12                      # bytes / s (spec)
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


def run(key, reps, with_torch):
    name, V, D, B, K = SHAPES[key]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g) * 0.05
    q = torch.randn(B, D, device="cuda", generator=g)
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    ids = torch.empty(B, K, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    fn = lambda: O.score_topk(q, D, table, B, K, L.PREC_BF16X3, None, None, None, ws, ids, sc)
    t, all_t = _time(fn, reps)
    nbytes = V * D * 4 + B * D * 4 + B * K * 8
    flop = 2.0 * B * V * D * 3
    t_hbm, t_mfma = nbytes / HBM, flop / BF16_PEAK
    bound = "hbm" if t_hbm >= t_mfma else "mfma"
    r = dict(shape=key, name=name, V=V, D=D, B=B, K=K, time_s=t, times_s=all_t, hbm_bytes=nbytes, hbm_roof_s=t_hbm,
             hbm_fraction=t_hbm / t, mfma_flop_bf16x3=flop, mfma_roof_s=t_mfma, mfma_fraction=t_mfma / t, binding=bound,
             binding_fraction=max(t_hbm, t_mfma) / t, workspace_bytes=ws.numel())
    if with_torch and B * V * 4 <= 48 * 2 ** 30:
        def base():
            s = q @ table.t()
            s[:, 0] = -float("inf")
            return torch.topk(s, K, dim=1)
        try:
            tb, _ = _time(base, max(2, reps // 2), warm=1)
            r.update(torch_matmul_topk_s=tb, speedup_vs_torch=tb / t)
            bs = base()
            ref = bs.indices.to(torch.int32)
            r["agree_with_torch_ids"] = float((ref == ids).float().mean())
        except RuntimeError as e:                         # (out of memory: reported, not fatal)
            r["torch_error"] = str(e)[:200]
        torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    return r


def _sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def _median(x):
    return sorted(x)[len(x) // 2]


def run_index(key, reps, min_sample):
    name, V, D, B, K = SHAPES[key]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
    q = torch.randn(B, D, device="cuda", generator=g)
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    out = []
    for pname, prec in (("bf16x3", L.PREC_BF16X3), ("bf16", L.PREC_BF16)):
        kinds = [("split", L.PREC_BF16X3)] + ([("plain", L.PREC_BF16)] if prec == L.PREC_BF16 and key in ("c", "d") else [])
        blobs, t_build = {}, {}
        for kind, ip in kinds:
            blob = torch.empty(O.topk_index_bytes(V, D, ip), dtype=torch.uint8, device="cuda")
            build = lambda: O.topk_index_build(table, ip, out=blob)
            build(); torch.cuda.synchronize()
            t1 = _sample(build, 1)
            n = max(1, int(min_sample / max(t1, 1e-6)) + 1)
            t_build[kind] = _median([_sample(build, n) for _ in range(reps)])
            blobs[kind] = (blob, ip)
        res = {k: (torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, K, dtype=torch.float32, device="cuda"))
               for k in ["table"] + [k for k, _ in kinds]}
        fns = {"table": lambda: O.score_topk(q, D, table, B, K, prec, None, None, None, ws, *res["table"])}
        for kind, _ in kinds:
            fns[kind] = (lambda kind: lambda: O.score_topk(q, D, (V, D), B, K, prec, None, None, None, ws, *res[kind],
                                                           index=blobs[kind][0], index_precision=blobs[kind][1]))(kind)
        for f in fns.values():                                  # warm every form, and check the results agree bit for bit
            f(); f()
        torch.cuda.synchronize()
        same = {kind: bool(torch.equal(res[kind][0], res["table"][0]) and
                           torch.equal(res[kind][1].view(torch.int32), res["table"][1].view(torch.int32))) for kind, _ in kinds}
        n = max(1, int(min_sample / max(_sample(fns["table"], 1), 1e-6)) + 1)
        series = {k: [] for k in ["table", "table_again"] + [k for k, _ in kinds]}
        for _ in range(reps):                                   # A B (P) A: interleaved, so that drift hits every series alike
            series["table"].append(_sample(fns["table"], n))
            for kind, _ in kinds:
                series[kind].append(_sample(fns[kind], n))
            series["table_again"].append(_sample(fns["table"], n))
        t_table, t_again = _median(series["table"]), _median(series["table_again"])
        r = dict(shape=key, name=name, V=V, D=D, B=B, K=K, precision=pname, calls_per_sample=n, samples=reps, t_table_s=t_table,
                 t_table_again_s=t_again, aa_ratio=t_again / t_table, table_bytes=V * D * 4, series_s=series)
        for kind, _ in kinds:
            t_ix = _median(series[kind])
            gain = t_table - t_ix
            r[kind] = dict(index_bytes=blobs[kind][0].numel(), t_index_s=t_ix, t_build_s=t_build[kind], index_over_table=t_ix / t_table,
                           bit_identical=same[kind], break_even_searches=(t_build[kind] / gain if gain > 0 else None))
        print(json.dumps({k: v for k, v in r.items() if k != "series_s"}), flush=True)
        out.append(r)
        del blobs, fns, res
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--index", action="store_true", help="table search against item-index search (see the module docstring)")
    ap.add_argument("--min-sample", type=float, default=0.05, help="--index: seconds of back-to-back calls per timed sample")
    a = ap.parse_args()
    if a.index:
        reps = a.reps if "--reps" in sys.argv else 7
        res = [r for k in a.shapes.split(",") for r in run_index(k, reps, a.min_sample)]
        out = a.out or os.path.join(ROOT, "profiles", "topk", "topk_index_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res), f, indent=1)
        return
    res = [run(k, a.reps, not a.no_torch) for k in a.shapes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res), f, indent=1)


if __name__ == "__main__":
    main()

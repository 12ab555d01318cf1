"""Times the cosine item index (castrec.h CR_INDEX_COSINE) with HIP events, tools/topk_bench.py's method (median of --reps 3 samples,
every sample --min-sample seconds of back-to-back calls), bf16x3, at (V, D) = (368 000, 128) and (10^7, 256):

  * build: the cosine build, the dot build, and what a user had before -- torch `table / table.norm(dim=1, keepdim=True)` into a second
    fp32 table, then the dot build of that copy (timed together, and the torch part alone);
  * sync of a cosine index with every tile flagged and with 1 % of the rows flagged (beside the dot sync);
  * one search at shape (b) of DESIGN.md section 10 (V 368 000, D 128, B 10 000, K 10) on a cosine and on a dot index, interleaved.

    python tools/topk_cosine_bench.py [--shapes b,c] [--out profiles/topk_cosine/bench.json]
    python tools/topk_cosine_bench.py --baseline      # a tree without the cosine metric: the dot build and the torch composition only
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import castrec_amd  # noqa: E402,F401
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402
from topk_bench import SHAPES, _median, _sample  # noqa: E402

PREC = L.PREC_BF16X3


def _timed(fn, reps, min_sample):
    fn(); fn()
    torch.cuda.synchronize()
    n = max(1, int(min_sample / max(_sample(fn, 1), 1e-6)) + 1)
    s = [_sample(fn, n) for _ in range(reps)]
    return dict(t_s=_median(s), samples_s=s, calls_per_sample=n)


def run(key, reps, min_sample, baseline):
    name, V, D, B, K = SHAPES[key]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
    blob = torch.empty(O.topk_index_bytes(V, D, PREC), dtype=torch.uint8, device="cuda")
    r = dict(shape=key, name=name, V=V, D=D, precision="bf16x3", table_bytes=V * D * 4, index_bytes=blob.numel(), baseline=bool(baseline))
    r["build_dot"] = _timed(lambda: O.topk_index_build(table, PREC, out=blob), reps, min_sample)

    def torch_normalise():
        return table / table.norm(dim=1, keepdim=True)

    def torch_then_build():
        O.topk_index_build(torch_normalise(), PREC, out=blob)

    r["torch_normalise"] = _timed(torch_normalise, reps, min_sample)
    r["torch_normalise_then_build_dot"] = _timed(torch_then_build, reps, min_sample)
    torch.cuda.empty_cache()
    if not baseline:
        r["build_cosine"] = _timed(lambda: O.topk_index_build(table, PREC, out=blob, metric="cosine"), reps, min_sample)
        r["cosine_over_torch_composition"] = r["build_cosine"]["t_s"] / r["torch_normalise_then_build_dot"]["t_s"]
        r["cosine_over_dot_build"] = r["build_cosine"]["t_s"] / r["build_dot"]["t_s"]
        every = torch.ones(V, dtype=torch.int32, device="cuda")
        some = (torch.rand(V, device="cuda", generator=g) < 0.01).to(torch.int32)
        r["flagged_tile_fraction_at_1pct_rows"] = float(torch.nn.functional.pad(some, (0, -V % 16)).view(-1, 16).max(1).values.float().mean())
        for what, flags in (("all", every), ("1pct_rows", some)):
            for metric in ("cosine", "dot"):
                r["sync_%s_%s" % (metric, what)] = _timed(lambda: O.topk_index_sync(blob, table, PREC, flags, 1, metric=metric), reps, min_sample)
    print(json.dumps({k: (v["t_s"] if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
    return r


def run_search(reps, min_sample):
    name, V, D, B, K = SHAPES["b"]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
    q = torch.randn(B, D, device="cuda", generator=g)
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    ids = torch.empty(B, K, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    blobs = {m: O.topk_index_build(table, PREC, metric=m) for m in ("dot", "cosine")}
    fns = {m: (lambda m: lambda: O.score_topk(q, D, (V, D), B, K, PREC, None, None, None, ws, ids, sc, index=blobs[m], index_precision=PREC))(m)
           for m in blobs}
    for f in fns.values():
        f(); f()
    torch.cuda.synchronize()
    n = max(1, int(min_sample / max(_sample(fns["dot"], 1), 1e-6)) + 1)
    series = {"dot": [], "cosine": [], "dot_again": []}
    for _ in range(reps):                                       # A B A: interleaved, so that drift hits every series alike
        series["dot"].append(_sample(fns["dot"], n))
        series["cosine"].append(_sample(fns["cosine"], n))
        series["dot_again"].append(_sample(fns["dot"], n))
    r = dict(shape="b", name=name, V=V, D=D, B=B, K=K, precision="bf16x3", calls_per_sample=n, samples=reps, series_s=series,
             t_search_dot_s=_median(series["dot"]), t_search_cosine_s=_median(series["cosine"]), t_search_dot_again_s=_median(series["dot_again"]))
    r["cosine_over_dot"] = r["t_search_cosine_s"] / r["t_search_dot_s"]
    r["aa_ratio"] = r["t_search_dot_again_s"] / r["t_search_dot_s"]
    print(json.dumps({k: v for k, v in r.items() if k != "series_s"}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="b,c")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-sample", type=float, default=0.05)
    ap.add_argument("--baseline", action="store_true", help="a tree without metric=: the dot build and the torch composition only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), builds=[run(k, a.reps, a.min_sample, a.baseline) for k in a.shapes.split(",")])
    if not a.baseline:
        res["search"] = run_search(a.reps, a.min_sample)
    out = a.out or os.path.join(ROOT, "profiles", "topk_cosine", "bench_baseline.json" if a.baseline else "bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

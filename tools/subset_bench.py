"""Times a search of a shared candidate subset (castrec.h cr_topk_index_gather; castrec_amd.index.ItemSubset) against the full indexed
search, with HIP events: V = 368 000, D = 128, B = 10 000, K = 10, a bf16x3 index.

    python tools/subset_bench.py [--reps 3] [--fractions 0.01,0.1,0.5] [--out profiles/topk/subset_bench.json]

Per subset of random ids: the gather out of the index alone, the gather from the fp32 table alone, the search of the gathered sub-index
alone (cr_score_topk with V = n + 1) and gather + search; the median of --reps single calls each, after two warm calls.  The full
search (existing code) is timed in the same run, before and after the subsets.  The one gate: gather + search of the 10 % subset takes
less time than the full search (exit status 1 otherwise).  The id translation and the map-back of ItemSubset.search are host numpy and
one device gather over [B, K]; they are not part of these device times."""
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

V, D, B, K = 368000, 128, 10000, 10
PREC = L.PREC_BF16X3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fractions", default="0.01,0.1,0.5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "subset_bench.json"))
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
    table[0] = 0
    q = torch.randn(B, D, device="cuda", generator=g)
    full = O.topk_index_build(table, PREC)
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    ids_out = torch.empty(B, K, dtype=torch.int32, device="cuda")
    sc_out = torch.empty(B, K, dtype=torch.float32, device="cuda")
    search_full = lambda: O.score_topk(q, D, (V, D), B, K, PREC, None, None, None, ws, ids_out, sc_out, index=full, index_precision=PREC)
    t_full, full_all = _time(search_full, a.reps)
    rows = []
    for frac in [float(x) for x in a.fractions.split(",")]:
        n = max(1, int(round(frac * (V - 1))))
        ids = (torch.randperm(V - 1, device="cuda", generator=g)[:n] + 1).sort().values.to(torch.int32)
        blob = torch.empty(O.topk_index_bytes(n + 1, D, PREC), dtype=torch.uint8, device="cuda")
        gather = lambda: O.topk_index_gather(ids, PREC, index=full, index_precision=PREC, V=V, D=D, out=blob)
        gather_table = lambda: O.topk_index_gather(ids, PREC, table=table, out=blob)
        search = lambda: O.score_topk(q, D, (n + 1, D), B, K, PREC, None, None, None, ws, ids_out, sc_out, index=blob, index_precision=PREC)
        both = lambda: (gather(), search())
        t_gt, _ = _time(gather_table, a.reps)
        t_g, g_all = _time(gather, a.reps)
        t_s, s_all = _time(search, a.reps)
        t_b, b_all = _time(both, a.reps)
        r = dict(fraction=frac, n=n, sub_index_bytes=blob.numel(), t_gather_s=t_g, t_gather_from_table_s=t_gt, t_search_s=t_s,
                 t_gather_plus_search_s=t_b, sum_s=t_g + t_s, over_full=t_b / t_full, search_over_full=t_s / t_full,
                 times_s=dict(gather=g_all, search=s_all, gather_plus_search=b_all))
        print(json.dumps({k: v for k, v in r.items() if k != "times_s"}), flush=True)
        rows.append(r)
    t_full2, full_all2 = _time(search_full, a.reps)
    ten = [r for r in rows if abs(r["fraction"] - 0.1) < 1e-9]
    gate = bool(ten and ten[0]["t_gather_plus_search_s"] < min(t_full, t_full2)) if ten else None
    res = dict(device=torch.cuda.get_device_name(0), V=V, D=D, B=B, K=K, precision="bf16x3", reps=a.reps, t_full_s=t_full,
               t_full_again_s=t_full2, full_times_s=full_all + full_all2, subsets=rows, gate_10pct_faster_than_full=gate)
    print(json.dumps(dict(t_full_s=t_full, t_full_again_s=t_full2, gate_10pct_faster_than_full=gate)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if gate in (True, None) else 1


if __name__ == "__main__":
    sys.exit(main())

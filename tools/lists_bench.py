"""Times top-K over per-query candidate lists (castrec.h cr_score_topk_lists) against the full indexed search, with HIP events:
V = 368 000, D = 128, B = 10 000, K = 10, bf16x3 (the setup of section 18).

    python tools/lists_bench.py [--reps 3] [--lengths 100,1000,10000] [--out profiles/topk/lists_bench.json]

Per list length n: B rows of n random distinct ids each, searched from the fp32 table and from a bf16x3 index; the median of --reps
single calls each, after two warm calls.  Reported beside the time: the gathered bytes (B n rows x the row bytes of that source: D
floats from the table, two planes of NK 32 bf16 from the index) over the time as a fraction of 8 TB/s, and the ratio to the full
indexed search (existing code), which is timed in the same run, before and after the lists.  The one gate: at n = 1 000 the faster
of the two sources takes less time than the full search (exit status 1 otherwise)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import castrec_amd  # noqa: E402,F401
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402

V, D, B, K = 368000, 128, 10000, 10
PREC = L.PREC_BF16X3
HBM = 8e12


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


def _rows(g, n):
    """[B, n] int32 on the device: n distinct ids of 1 .. V-1 per row, in random order (a random start and a random odd stride modulo
    V - 1 would repeat a pattern across rows; an argsort of uniform keys over a window does not)."""
    out = torch.empty(B, n, dtype=torch.int32, device="cuda")
    step = max(1, (1 << 24) // max(n, 1024))
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        w = min(V - 1, max(4 * n, 4096))                                   # n of a window of w ids at a random offset
        keys = torch.rand(b1 - b0, w, device="cuda", generator=g)
        pick = keys.argsort(dim=1)[:, :n]
        start = torch.randint(0, V - 1, (b1 - b0, 1), device="cuda", generator=g)
        out[b0:b1] = ((start + pick * ((V - 1) // w)) % (V - 1) + 1).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lengths", default="100,1000,10000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "lists_bench.json"))
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
    row_bytes = dict(table=4 * D, index=2 * 2 * 32 * ((D + 31) // 32))
    rows = []
    for n in [int(x) for x in a.lengths.split(",")]:
        cand = _rows(g, n)
        srt = cand.sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()) and int(srt.min()) >= 1 and int(srt.max()) <= V - 1
        del srt
        off = np.arange(B + 1, dtype=np.int64) * n
        flat = cand.reshape(-1)
        lws = torch.empty(O.topk_lists_workspace_bytes(B, n, D, K), dtype=torch.uint8, device="cuda")
        li, ls = torch.empty_like(ids_out), torch.empty_like(sc_out)
        from_table = lambda: O.score_topk_lists(q, D, table, B, K, PREC, off, flat, None, lws, li, ls)
        from_index = lambda: O.score_topk_lists(q, D, (V, D), B, K, PREC, off, flat, None, lws, li, ls, index=full, index_precision=PREC)
        r = dict(n=n, segments=int(L.lib.cr_topk_lists_segments(B, n)))
        keep = {}
        for name, fn in (("table", from_table), ("index", from_index)):
            t, t_all = _time(fn, a.reps)
            keep[name] = (li.clone(), ls.clone())
            nbytes = B * n * row_bytes[name]
            r[name] = dict(t_s=t, times_s=t_all, gathered_bytes=nbytes, of_8tbs=nbytes / t / HBM, over_full=t / t_full)
        r["same_bits_from_both_sources"] = bool(torch.equal(keep["table"][0], keep["index"][0])
                                                and torch.equal(keep["table"][1].view(torch.int32), keep["index"][1].view(torch.int32)))
        print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "times_s"} if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
        rows.append(r)
        del cand, flat, lws
    t_full2, full_all2 = _time(search_full, a.reps)
    thousand = [r for r in rows if r["n"] == 1000]
    gate = bool(min(thousand[0]["table"]["t_s"], thousand[0]["index"]["t_s"]) < min(t_full, t_full2)) if thousand else None
    res = dict(device=torch.cuda.get_device_name(0), V=V, D=D, B=B, K=K, precision="bf16x3", reps=a.reps, t_full_s=t_full,
               t_full_again_s=t_full2, full_times_s=full_all + full_all2, lists=rows, gate_n1000_faster_than_full=gate)
    print(json.dumps(dict(t_full_s=t_full, t_full_again_s=t_full2, gate_n1000_faster_than_full=gate)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if gate in (True, None) else 1


if __name__ == "__main__":
    sys.exit(main())

"""Times the ways of bringing an item index in step with its table (castrec.h cr_topk_index_build / cr_topk_index_sync /
cr_topk_index_update), with HIP events, on a bf16x3 index:

    timeout -k 10 900 python tools/index_refresh_bench.py [--reps 3] [--shapes 368000x128,10000000x256] [--touched 1000,50000,1000000]
                                                         [--out profiles/index_refresh/index_refresh_bench.json]

Per shape and per uniformly random set of touched rows, four device times: the full build (existing code: the yardstick), sync from
a flag array that names the set, update from the id list with the table as the source, update from packed rows.  A time is the median
of --reps windows after two warm windows; a window is one event pair around as many back-to-back calls as fill about 50 ms (at least
one, at most 200), divided by their number -- a single call of a few microseconds would measure the event pair.  Every form is
idempotent, so repeated calls do the same work.  Before anything is timed each form is run once on an index of the OLD table and
its blob compared, byte for byte, with a build from the new table.  Beside each time: the bytes the form must move, from the shapes
(build: the table read, the blob written; sync: the flags read, 16 table rows read and a tile written per touched tile; update: the
ids, one row read and one row's groups written per id)."""
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

PREC = L.PREC_BF16X3
SINCE = 7


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def _time(fn, reps, warm=2, fill=0.05):
    fn()
    torch.cuda.synchronize()
    inner = max(1, min(200, int(fill / max(_window(fn, 1), 1e-7))))
    for _ in range(warm):
        _window(fn, inner)
    out = sorted(_window(fn, inner) for _ in range(reps))
    return out[len(out) // 2], out, inner


def _nk(D):
    nk = (D + 31) // 32
    return 1 if nk <= 1 else 2 if nk <= 2 else 4 if nk <= 4 else 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="368000x128,10000000x256")
    ap.add_argument("--touched", default="1000,50000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_refresh", "index_refresh_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("index_refresh_bench needs the GPU: nothing here is a time without one")
    g = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for shape in a.shapes.split(","):
        V, D = (int(x) for x in shape.split("x"))
        nb = O.topk_index_bytes(V, D, PREC)
        row_bytes = 2 * _nk(D) * 64                                      # one row's groups in both planes
        old = torch.randn(V, D, device="cuda", generator=g).mul_(0.05)
        blob = torch.empty(nb, dtype=torch.uint8, device="cuda")
        t_build, build_all, inner = _time(lambda: O.topk_index_build(old, PREC, out=blob), a.reps)
        build_bytes = V * D * 4 + nb
        print(json.dumps(dict(V=V, D=D, form="build", t_s=t_build, bytes=build_bytes, GBps=build_bytes / t_build * 1e-9, calls=inner)), flush=True)
        rows = []
        for n in (int(x) for x in a.touched.split(",")):
            if n >= V:
                continue
            ids = (torch.randperm(V - 1, device="cuda", generator=g)[:n] + 1).to(torch.int32)
            new = old.clone()
            new[ids.long()] += 1.0
            packed = new[ids.long()].contiguous()
            flags = torch.zeros(V, dtype=torch.int32, device="cuda")
            flags[ids.long()] = SINCE
            tiles = int(torch.unique(ids >> 4).numel())
            forms = {"sync": (lambda: O.topk_index_sync(blob, new, PREC, flags, SINCE), V * 4 + tiles * (16 * D * 4 + 16 * row_bytes)),
                     "update_table": (lambda: O.topk_index_update(blob, V, D, PREC, ids, new, False), n * (4 + D * 4 + row_bytes)),
                     "update_packed": (lambda: O.topk_index_update(blob, V, D, PREC, ids, packed, True), n * (4 + D * 4 + row_bytes))}
            want = O.topk_index_build(new, PREC)
            r = dict(touched=n, touched_fraction=n / V, tiles=tiles, tile_fraction=tiles / ((V + 15) // 16))
            for name, (fn, nbytes) in forms.items():
                O.topk_index_build(old, PREC, out=blob)
                fn()
                torch.cuda.synchronize()
                if not torch.equal(blob, want):
                    sys.exit("%s at V=%d D=%d n=%d: the blob is not the rebuild's" % (name, V, D, n))
                t, every, inner = _time(fn, a.reps)
                r[name] = dict(t_s=t, times_s=every, calls_per_window=inner, bytes=nbytes, GBps=nbytes / t * 1e-9, over_build=t / t_build)
                print(json.dumps(dict(V=V, D=D, touched=n, form=name, t_s=t, bytes=nbytes, over_build=t / t_build, calls=inner)), flush=True)
            del want, new, packed, flags
            rows.append(r)
        t_build2, build_all2, _ = _time(lambda: O.topk_index_build(old, PREC, out=blob), a.reps)
        results.append(dict(V=V, D=D, index_bytes=nb, build=dict(t_s=t_build, t_again_s=t_build2, times_s=build_all + build_all2, bytes=build_bytes),
                            sets=rows))
        del old, blob
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), precision="bf16x3", reps=a.reps, shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| V | D | touched rows | tiles hit | build | sync | update (table) | update (packed) |")
    print("|---|---|---|---|---|---|---|---|")
    ms = lambda d: "%.3f ms (%.1f MB)" % (d["t_s"] * 1e3, d["bytes"] * 1e-6)
    for s in results:
        for r in s["sets"]:
            print("| %d | %d | %d | %.1f %% | %s | %s | %s | %s |" % (s["V"], s["D"], r["touched"], 100 * r["tile_fraction"], ms(s["build"]),
                                                                   ms(r["sync"]), ms(r["update_table"]), ms(r["update_packed"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times whole training steps of sasrec with dense against row-sparse Adam (Engine(row_sparse_adam=True)) under
the sampled losses, in bf16x3, at the three shapes of DESIGN.md section 12:

    (a) headline: B 128, T 200, D 50, V 3 417, N 256          (b) B 128, T 200, D 128, 4 heads, V 368 001, N 1 024
    (c) B 128, T 512, D 256, 4 heads, 2 blocks, V 10 000 000, N 4 096

    python tools/sparse_step_bench.py [--shapes a,b,c] [--losses sampled_ce,gbce] [--reps 7] [--out profiles/row_sparse/step_bench.json]

Each shape is measured in ONE process -- the dense and the row-sparse engine of a loss share the parameter vector and are timed in
turn (dense, sparse, dense, sparse, ...: HIP events over `n` launches of the captured step's graph, median of --reps) -- and that
process is a child of this one, run under its own `timeout`: a shape that fails or hangs ends the run there, and nothing is started on
the GPU behind it.  The ids of a batch are uniform over the catalogue (every row of seq | pos distinct at (c): the most rows a
batch can touch).  --child SHAPE is that child; with --modes dense (or sparse) it builds and runs one kind of engine only -- the form to
put behind `rocprofv3 --kernel-trace --stats --`, a run of its own.

The gate (shape c): the row-sparse step's median is below the dense step's by more than the dense runs' own spread (max - min)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key: (name, B, T, D, heads, blocks, itemnum, N, launches per timed interval, seconds the child may take)
SHAPES = {"a": ("headline, ml-1m", 128, 200, 50, 1, 2, 3416, 256, 20, 300),
          "b": ("C4 vocabulary", 128, 200, 128, 4, 2, 368000, 1024, 20, 300),
          "c": ("C5 table", 128, 512, 256, 4, 2, 10 ** 7 - 1, 4096, 5, 900)}


def child(key, losses, modes, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import castrec_amd  # noqa: F401
    from castrec_amd import engine as E
    name, B, T, D, H, NB, itemnum, N, n, _ = SHAPES[key]
    rs = np.random.RandomState(0)
    seq = rs.randint(1, itemnum + 1, (B, T)); seq[:, :T // 10] = 0
    pos = rs.randint(1, itemnum + 1, (B, T)) * (seq != 0)
    neg = rs.randint(1, itemnum + 1, (B, T)) * (seq != 0)
    owner = None
    out = []
    for loss in losses:
        hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=NB, num_heads=H, dropout_rate=0.2, lr=1e-3, seed=42, loss=loss, ce_negatives=N)
        eng = {}
        for mode in modes:
            e = E.Engine("sasrec", 10, itemnum, hp, B, training=True, attn_precision="bf16x3", share=owner, row_sparse_adam=(mode == "sparse"))
            owner = owner or e                            # one parameter vector for every engine of the shape (10 GB at (c))
            e.set_batch(seq, pos, neg)
            e.capture()
            e.set_step(1)
            eng[mode] = e

        def run(e):
            for _ in range(n):
                e.graph.launch()
        for e in eng.values():                            # warm-up: two intervals each
            run(e); run(e)
        torch.cuda.synchronize()
        times = {m: [] for m in eng}
        for _ in range(reps):
            for m, e in eng.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); run(e); b.record()
                torch.cuda.synchronize()
                times[m].append(a.elapsed_time(b) / n)
        r = dict(shape=key, name=name, model="sasrec", B=B, T=T, D=D, heads=H, blocks=NB, V=itemnum + 1, N=N, loss=loss, precision="bf16x3",
                 launches_per_interval=n, reps=reps)
        for m, e in eng.items():
            ts = sorted(times[m])
            touched = int(torch.unique(torch.cat([e.ids_all[:2].reshape(-1), e.samples])).numel())
            r[m] = dict(ms_per_step=ts[len(ts) // 2], all_ms=ts, spread_ms=ts[-1] - ts[0], kernel_launches=e.n_kernel_launches(),
                        loss_after=e.loss_auc()[0], rows_listed=touched)
        if len(eng) == 2:
            d, s = r["dense"], r["sparse"]
            r["sparse_over_dense"] = s["ms_per_step"] / d["ms_per_step"]
            r["faster_by_more_than_dense_spread"] = bool(d["ms_per_step"] - s["ms_per_step"] > d["spread_ms"])
        print("RESULT " + json.dumps(r), flush=True)
        out.append(r)
        del eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--losses", default="sampled_ce,gbce")
    ap.add_argument("--modes", default="dense,sparse")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_sparse", "step_bench.json"))
    ap.add_argument("--child", default=None, help="measure this shape in this process (what the parent runs under `timeout`)")
    a = ap.parse_args()
    losses, modes = a.losses.split(","), a.modes.split(",")
    if a.child:
        child(a.child, losses, modes, a.reps)
        return 0
    results, failed = [], None
    for key in a.shapes.split(","):
        limit = SHAPES[key][-1]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", key, "--losses", a.losses,
               "--modes", a.modes, "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        results += [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0:
            # a fault, an abort or the time limit: nothing more is started on the GPU
            failed = dict(shape=key, returncode=p.returncode)
            print("shape %s: exit status %d -- stopping" % (key, p.returncode), flush=True)
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(results=results, failed=failed), f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

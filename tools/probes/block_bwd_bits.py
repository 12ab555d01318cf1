#!/usr/bin/env python
"""Bits of the block backward, one-launch (cr_stack_bwd1.hip) and three-launch (cr_stack_bwd.hip): one SHA-256 per case and array, for
comparing two builds of the library (CASTREC_LIB=<other .so> selects the build; the default is the tree's).  Same use as head_bits.py:

    python tools/probes/block_bwd_bits.py --save DIR_B > branch.txt
    CASTREC_LIB=/elsewhere/libcastrec_parent.so python tools/probes/block_bwd_bits.py --save DIR_P > parent.txt
    python tools/probes/block_bwd_bits.py --compare parent.txt branch.txt DIR_P DIR_B > bits_compare.txt     (exit status 1 on a difference)

A case: cast_1, two blocks, dropout 0.2, seed and batch of tests/test_model_gpu.py::test_register_layout_kernels_equal_the_tile_kernels,
one launch_step(apply=False); hashed: seq_emb, every entry of Engine.grads() and the do / dqkv / dx2 buffers of each block.  Shapes
(T, D, H, B) below, each with bf16x3 and bf16, with the default plan and with CASTREC_NO_BLOCK_BWD=1, with n_slabs below and above B;
(40, 50, 1, 6) once more with CASTREC_NO_INDEX=1 (the float-atomic scatter).  Every case runs twice on fresh engines: an array whose two
runs differ (float atomics) is listed as `name~` -- not hashed for the comparison; --save keeps it, and --compare holds the two builds'
copies together at the tolerance of test_index_and_atomics_paths_agree (1e-4 of the array's largest entry)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(40, 50, 1, 6), (200, 50, 1, 3), (33, 24, 1, 5), (224, 50, 1, 2), (100, 63, 1, 9), (50, 64, 2, 5), (100, 64, 1, 3)]


def compare(a, b, dir_a=None, dir_b=None):
    """One row per case: the number of hashed arrays and, per build, one SHA-256 over the case's (array, hash) lines in order -- equal
    when every array's bits are.  An array that differs gets a row of its own under its case, and so does every `name~` array."""
    import numpy as np
    rows = [[l.split() for l in open(f) if l.strip()] for f in (a, b)]
    assert [r[:2] for r in rows[0]] == [r[:2] for r in rows[1]], "the two listings hold different cases or arrays"
    differ, cases = 0, {}
    for (case, arr, ha), (_, _, hb) in zip(*rows):
        cases.setdefault(case, []).append((arr, ha, hb))
    print("# %-52s %6s %-16s %-16s" % ("case", "arrays", os.path.basename(a), os.path.basename(b)))
    for case, arrs in cases.items():
        hashed = [t for t in arrs if not t[0].endswith("~")]
        da, db = (hashlib.sha256("".join("%s %s\n" % (t[0], t[i]) for t in hashed).encode()).hexdigest()[:16] for i in (1, 2))
        print("%-54s %6d %s %s %s" % (case, len(hashed), da, db, "equal" if da == db else "DIFFERENT"))
        for arr, ha, hb in arrs:
            if arr.endswith("~"):                          # not reproducible within one build: compared by value
                x, y = (np.load(os.path.join(d, "%s.%s.npy" % (case, arr))) for d in (dir_a, dir_b))
                err = float(np.abs(x - y).max()) / max(1e-6, float(np.abs(x).max()))
                differ += err > 1e-4
                print("    %-50s relative difference %.3g %s" % (arr, err, "within 1e-4 (atomic order)" if err <= 1e-4 else "DIFFERENT"))
            elif ha != hb:
                differ += 1
                print("    %-50s %s %s DIFFERENT" % (arr, ha[:16], hb[:16]))
    print("# %d cases, %d arrays, %d different" % (len(cases), len(rows[0]), differ))
    return 1 if differ else 0


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import castrec_amd  # noqa: F401
    from castrec_amd import engine as E, lib as L
    from bf16_ref import make_batch
    print("# library %s" % os.path.basename(L.LIB_PATH), file=sys.stderr)
    save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
    if save:
        os.makedirs(save, exist_ok=True)

    def run(T, D, H, B, prec, n_slabs):
        hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.2, max_bins=9, seed=13)
        eng = E.Engine("cast_1", 9, 45, hp, B, training=True, n_slabs=n_slabs, attn_precision=prec)
        eng.P.add_(0.05 * torch.randn(eng.P.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)))
        eng.set_batch(*make_batch(np.random.RandomState(5), B, T, 45, 9))
        eng.launch_step(apply=False)
        torch.cuda.synchronize()
        got = {"seq_emb": eng.seq_emb}
        got.update({"grad." + k: v for k, v in eng.grads().items()})
        got.update({k: v for k, v in eng._bufs.items() if k.endswith(("do", "dqkv", "dx2"))})
        return [n for n, _, _ in eng.bwd], {k: v.detach().cpu().numpy().copy() for k, v in got.items()}

    cases = [(s, prec, env, lo) for s in SHAPES for prec in ("bf16x3", "bf16") for env in ("", "CASTREC_NO_BLOCK_BWD") for lo in (True, False)]
    cases.append((SHAPES[0], "bf16x3", "CASTREC_NO_INDEX", False))
    for (T, D, H, B), prec, env, lo in cases:
        n_slabs = max(1, B // 2) if lo else B + 2
        label = "T%d.D%d.H%d.B%d.%s.%s.slabs%d" % (T, D, H, B, prec, env[8:].lower() or "default", n_slabs)
        if env:
            os.environ[env] = "1"
        try:
            names, one = run(T, D, H, B, prec, n_slabs)
            _, two = run(T, D, H, B, prec, n_slabs)
        finally:
            os.environ.pop(env, None)
        one_launch = "cr_stack_block_bwd" in names
        assert one_launch == (env != "CASTREC_NO_BLOCK_BWD" and not (D == 64 and H == 1)), (label, names)
        print("%s plan %s" % (label, "one-launch" if one_launch else "three-launch"), file=sys.stderr)
        for k in sorted(one):
            same = np.array_equal(one[k], two[k], equal_nan=True)
            name = k if same else k + "~"
            print("%s %s %s" % (label, name, hashlib.sha256(np.ascontiguousarray(one[k]).tobytes()).hexdigest()))
            if save and not same:
                np.save(os.path.join(save, "%s.%s.npy" % (label, name)), one[k])
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:6]) if len(sys.argv) > 1 and sys.argv[1] == "--compare" else main())

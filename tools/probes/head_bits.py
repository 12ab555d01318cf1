#!/usr/bin/env python
"""Bits of the prediction head over the cases of the test suite: one SHA-256 per case and array, for comparing two builds of the library
(CASTREC_LIB=<other .so> selects the build; the default is the tree's).  Same use as adam_bits.py:

    python tools/probes/head_bits.py > branch.txt
    CASTREC_LIB=/elsewhere/libcastrec_parent.so python tools/probes/head_bits.py > parent.txt
    python tools/probes/head_bits.py --compare parent.txt branch.txt > bits_compare.txt      (exit status 1 when a line differs)
    python tools/probes/head_bits.py --save DIR        besides: every hashed array as DIR/<case>.<array>.npy
    python tools/probes/head_bits.py --ulps DIR_A DIR_B   the largest distance in units of the last place, per case and array that differs

cr_head_fwd_bwd / cr_head_fwd_bwd_ln: every case of tests/test_head_gpu.py through that module's run(), which is wrapped to hash what it
returns -- the per-row outputs and the slabs of both launches.  What float atomics order is left out: the three state sums except where
one workgroup makes them (cr_head_fwd_bwd at M = 5 and D <= 128; for cr_head_fwd_bwd_ln every M = 5 case is run once more on ONE slab,
for this listing only), the table gradient except where the non-zero ids are pairwise distinct (M = 5).  The tests' own assertions stay
in force.
cr_stack_fwd_head: the cases of tests/test_model_gpu.py::test_prediction_head_as_the_tail_of_the_last_forward_launch; after the test's
own step the forward launches run once more and coef_out, dx and the final LayerNorm's slabs are hashed, with the AUC sum and n_target
(small integers: exact in any order).  The loss sum is listed as `loss~`: its workgroups add to it with float atomics, so the line
may differ between two runs of ONE build; --compare shows such lines and does not count them."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_bits import cases, ulps  # noqa: E402


def compare(a, b):
    rows = [[l.split() for l in open(f) if l.strip()] for f in (a, b)]
    assert [r[:2] for r in rows[0]] == [r[:2] for r in rows[1]], "the two listings hold different cases"
    differ = 0
    print("# %-88s %-16s %-64s %-64s" % ("case", "array", os.path.basename(a), os.path.basename(b)))
    for (case, arr, ha), (_, _, hb) in zip(*rows):
        counted = not arr.endswith("~")
        differ += ha != hb and counted
        print("%-90s %-16s %s %s %s" % (case, arr, ha, hb, "equal" if ha == hb else "DIFFERENT" if counted else "differs (atomic order)"))
    print("# %d lines, %d different" % (len(rows[0]), differ))
    return 1 if differ else 0


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import ctypes as C
    import numpy as np
    import torch
    import castrec_amd  # noqa: F401
    from castrec_amd import engine as E, lib as L, ops
    import test_head_gpu as TH
    import test_model_gpu as TM
    print("# library %s" % os.path.basename(L.LIB_PATH), file=sys.stderr)
    save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
    if save:
        os.makedirs(save, exist_ok=True)
    listing, sys.stdout = sys.stdout, sys.stderr          # (the tests print their error figures: those go to stderr)

    def emit(label, name, a):
        a = np.ascontiguousarray(a)
        print("%s %s %s" % (label, name, hashlib.sha256(a.tobytes()).hexdigest()), file=listing)
        if save:
            np.save(os.path.join(save, "%s.%s.npy" % (label, name)), a)

    def emit_case(label, c, got, one_workgroup):
        for k in sorted(got):
            if k == "tg0" or (k.endswith(".state") and not one_workgroup) or (k.endswith(".table_grad") and c.M != 5):
                continue
            emit(label, k, got[k])

    for name in ("test_head", "test_head_ln"):
        fn = getattr(TH, name)
        for cid, kw in cases(fn):
            label = "%s[%s]" % (name, cid)
            real_run, seen = TH.run, []
            TH.run = lambda o, c: seen.append((c, real_run(o, c))) or seen[-1][1]
            try:
                fn(ops=ops, **kw)
            finally:
                TH.run = real_run
            (c, got), = seen
            emit_case(label, c, got, one_workgroup=not c.ln and c.M == 5 and c.D <= 128)
            if c.ln and c.M == 5:
                c1 = TH.case(True, c.D, c.pitch, 5, 1, c.tg)
                emit_case(label + "+one_slab", c1, {k: v for k, v in real_run(ops, c1).items() if k.endswith(".state")}, True)
            listing.flush()

    def floats_at(eng, ptr, n):
        """n floats at device address ptr, out of whichever tensor of the engine holds them"""
        pool = [t for t in list(vars(eng).values()) + list(eng._bufs.values()) if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32]
        for t in pool:
            base = t.untyped_storage().data_ptr()
            if base <= ptr and ptr + 4 * n <= base + t.untyped_storage().nbytes():
                flat = torch.empty(0, dtype=torch.float32, device=t.device).set_(t.untyped_storage())
                return flat[(ptr - base) // 4:(ptr - base) // 4 + n].cpu().numpy()
        raise LookupError("no tensor of the engine holds %#x" % ptr)

    fn = TM.test_prediction_head_as_the_tail_of_the_last_forward_launch
    for cid, kw in cases(fn):
        label = "%s[%s]" % (fn.__name__, cid)
        real, kept = TM._other_shapes, []
        TM._other_shapes = lambda *a, **k: kept.append(real(*a, **k)) or kept[-1]
        try:
            fn(E=E, **kw)
        finally:
            TM._other_shapes = real
        eng, = kept
        assert eng.fwd[-1][0] == "cr_stack_fwd_head"
        d, n = eng.fwd[-1][2][1]._obj, eng.fwd[-1][2][2]._obj
        eng.set_step(1)
        eng._run(eng.fwd, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = eng.state.cpu().numpy()
        emit(label, "coef", floats_at(eng, d.coef_out, 2 * d.M))
        emit(label, "dx", floats_at(eng, n.dx, (d.M - 1) * n.lddx + d.D).reshape(-1))
        written = 2 * eng.B                                # workgroup (sequence, half) writes slab half * B + sequence; the others are not written
        emit(label, "dgamma", np.stack([floats_at(eng, n.dgamma + 4 * s * n.slab_stride, d.D) for s in range(written)]))
        emit(label, "dbeta", np.stack([floats_at(eng, n.dbeta + 4 * s * n.slab_stride, d.D) for s in range(written)]))
        emit(label, "auc_n", st[1:3])
        emit(label, "loss~", st[0:1])
        listing.flush()
        del eng, kept
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    sys.exit(compare(*sys.argv[2:4]) if mode == "--compare" else ulps(*sys.argv[2:4]) if mode == "--ulps" else main())

#!/usr/bin/env python
"""Bits of cr_adam_step and cr_table_grad over the cases of the test suite: one SHA-256 per case and array, for comparing two builds
of the library (CASTREC_LIB=<other .so> selects the build; the default is the tree's).

    python tools/probes/adam_bits.py > branch.txt
    CASTREC_LIB=/elsewhere/libcastrec_parent.so python tools/probes/adam_bits.py > parent.txt
    python tools/probes/adam_bits.py --compare parent.txt branch.txt > bits_compare.txt      (exit status 1 when a line differs)
    python tools/probes/adam_bits.py --save DIR        besides: every hashed array as DIR/<case>.<array>.npy
    python tools/probes/adam_bits.py --ulps DIR_A DIR_B   the largest distance in units of the last place, per case and array that differs

The cases are not restated here: every test of tests/test_adam_gpu.py that goes through that module's run() is called with its own
parametrisation (CASTREC_ADAM_STREAM where the test forces it) and run() is wrapped to hash the p, m, v it returns; the same for the
table gradient that tests/test_index.py::test_table_grad_gather_equals_the_scatter has cr_table_grad write.  The tests' own
assertions stay in force: a build that fails one ends the listing there."""
import hashlib
import inspect
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    rows = [[l.split() for l in open(f) if l.strip()] for f in (a, b)]
    assert [r[:2] for r in rows[0]] == [r[:2] for r in rows[1]], "the two listings hold different cases"
    differ = 0
    print("# %-78s %-6s %-64s %-64s" % ("case", "array", os.path.basename(a), os.path.basename(b)))
    for (case, arr, ha), (_, _, hb) in zip(*rows):
        differ += ha != hb
        print("%-80s %-6s %s %s %s" % (case, arr, ha, hb, "equal" if ha == hb else "DIFFERENT"))
    print("# %d lines, %d different" % (len(rows[0]), differ))
    return 1 if differ else 0


def ulps(a, b):
    import numpy as np
    order = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    worst = {}
    for f in sorted(os.listdir(a)):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        d = np.abs(order(x) - order(y))
        if d.max() > 0:
            print("%-90s max %d ulps, %d of %d elements differ" % (f[:-4], d.max(), int((d > 0).sum()), d.size))
            t = f.split("[")[0]
            worst[t] = max(worst.get(t, 0), int(d.max()))
    print("# largest difference per test: %s" % worst)
    return 0


class Env:
    """what the tests use of pytest's monkeypatch"""

    def __init__(self):
        self.saved = {}

    def setenv(self, k, v):
        self.saved.setdefault(k, os.environ.get(k))
        os.environ[k] = v

    def undo(self):
        for k, v in self.saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def cases(fn):
    """(id, kwargs) of a test function under its parametrize marks, in pytest's order of ids (the last mark varies slowest)"""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    axes = []
    for m in marks:
        names = [n.strip() for n in m.args[0].split(",")]
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    for combo in itertools.product(*axes):
        kw = {}
        for c in combo:
            kw.update(c)
        yield "-".join(str(v) for c in combo for v in c.values()), kw


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import castrec_amd  # noqa: F401
    from castrec_amd import lib as L, ops
    import test_adam_gpu as TA
    import test_index as TI
    print("# library %s" % os.path.basename(L.LIB_PATH), file=sys.stderr)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    label, count = [""], [0]
    save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
    if save:
        os.makedirs(save, exist_ok=True)
    listing, sys.stdout = sys.stdout, sys.stderr          # (the tests print their error figures: those go to stderr)

    real_run = TA.run

    def run(*a, **kw):
        got, flags = real_run(*a, **kw)
        count[0] += 1
        for k in ("p", "m", "v"):
            print("%s#%d %s %s" % (label[0], count[0], k, sha(got[k])), file=listing)
            if save:
                np.save(os.path.join(save, "%s#%d.%s.npy" % (label[0], count[0], k)), got[k])
        return got, flags
    TA.run = run

    real_call = L.call

    def call(name, *a):
        real_call(name, *a)
        if name == "cr_table_grad":                       # a[1]: the address of the array the kernel writes: the caller's tensor there
            out, = [x for x in sys._getframe(1).f_locals.values() if isinstance(x, torch.Tensor) and x.data_ptr() == a[1]]
            torch.cuda.synchronize()
            count[0] += 1
            print("%s#%d grad %s" % (label[0], count[0], sha(out.cpu().numpy())), file=listing)
    L.call = call

    tests = [(TA, n) for n, f in vars(TA).items() if n.startswith("test_") and "run(ops" in inspect.getsource(f)]
    tests.append((TI, "test_table_grad_gather_equals_the_scatter"))
    for mod, name in tests:
        fn = getattr(mod, name)
        for cid, kw in cases(fn):
            label[0], count[0] = "%s[%s]" % (name, cid), 0
            env = Env()
            if "ops" in inspect.signature(fn).parameters:
                kw["ops"] = ops
            if "monkeypatch" in inspect.signature(fn).parameters:
                kw["monkeypatch"] = env
            try:
                fn(**kw)
            finally:
                env.undo()
            listing.flush()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    sys.exit(compare(*sys.argv[2:4]) if mode == "--compare" else ulps(*sys.argv[2:4]) if mode == "--ulps" else main())

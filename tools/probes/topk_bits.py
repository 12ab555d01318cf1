#!/usr/bin/env python
"""Bits of the catalogue search over the cases of the test suite: one SHA-256 per case and kind of array, for comparing two builds of
the library (CASTREC_LIB=<other .so> selects the build; the default is the tree's).  Same use as adam_bits.py:

    python tools/probes/topk_bits.py > branch.txt
    CASTREC_LIB=/elsewhere/libcastrec_parent.so python tools/probes/topk_bits.py > parent.txt
    python tools/probes/topk_bits.py --compare parent.txt branch.txt > bits_compare.txt      (exit status 1 when a line differs)

The cases are not restated here: the tests named in TESTS are called with their own parametrisation, and the three functions of
castrec_amd.ops that every search and every index goes through are wrapped -- score_topk (ids, scores, rank as the kernels left them),
topk_index_build and topk_index_gather (blob).  A case's line for one kind of array is the hash of every such array the case produced,
in order, each with its shape.  The search has no float atomics and a fixed chunk partition: two builds that compute the same thing
give the same listing, and --compare has no tolerance.  The tests' own assertions stay in force."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_bits import cases, compare  # noqa: E402

TESTS = [("test_topk_index_gpu", "test_indexed_search_is_bit_identical"),
         ("test_topk_index_gpu", "test_indexed_search_is_bit_identical_on_ties"),
         ("test_topk_index_gpu", "test_indexed_search_is_bit_identical_on_many_chunks"),
         ("test_topk_index_gpu", "test_built_blob_equals_the_numpy_layout"),
         ("test_topk_subset_gpu", "test_gathered_sub_index_has_the_bytes_of_a_build_on_the_gathered_table"),
         ("test_topk_subset_gpu", "test_subset_search_is_the_full_search_restricted")]
KINDS = ("ids", "scores", "rank", "blob")


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import importlib
    import torch
    import castrec_amd  # noqa: F401
    from castrec_amd import lib as L, ops as O
    print("# library %s" % os.path.basename(L.LIB_PATH), file=sys.stderr)
    listing, sys.stdout = sys.stdout, sys.stderr
    sums = {}

    def add(kind, t):
        torch.cuda.synchronize()
        a = t.cpu().numpy()
        sums[kind][0].update(("%s%s;" % (a.dtype, a.shape)).encode() + a.tobytes())
        sums[kind][1] += 1

    real = O.score_topk, O.topk_index_build, O.topk_index_gather

    def score_topk(query, ld, table, B, K, precision, excl_off, excl_ids, targets, workspace, top_ids, top_scores, rank=None, **kw):
        real[0](query, ld, table, B, K, precision, excl_off, excl_ids, targets, workspace, top_ids, top_scores, rank, **kw)
        add("ids", top_ids)
        add("scores", top_scores)
        if rank is not None:
            add("rank", rank)

    def blob_of(fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            add("blob", out)
            return out
        return wrapped

    O.score_topk, O.topk_index_build, O.topk_index_gather = score_topk, blob_of(real[1]), blob_of(real[2])
    for mod, name in TESTS:
        fn = getattr(importlib.import_module(mod), name)
        for cid, kw in cases(fn):
            sums.clear()
            sums.update((k, [hashlib.sha256(), 0]) for k in KINDS)
            fn(**kw)
            for k in KINDS:
                if sums[k][1]:
                    print("%s[%s](%d) %s %s" % (name, cid, sums[k][1], k, sums[k][0].hexdigest()), file=listing)
            listing.flush()
    return 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else main())

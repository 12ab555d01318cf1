#!/usr/bin/env python
"""HIP-event times of the prediction head's three entries, for comparing two builds of the library (CASTREC_LIB=<other .so>; run the two
alternating, several rounds each): cr_head_fwd_bwd_ln in its vector form (coef_out, no table_grad), cr_head_fwd_bwd_ln with table_grad
(the strided form and its float-atomic scatter) and cr_head_fwd_bwd (d_seq_emb + table_grad), at M = 25 600 rows and
  D = 50, the headline's table (3 417 rows: cache-resident), and
  D = 256, a 4 M-row table (4 GB: far beyond the 256 MiB Infinity Cache), a fresh set of ids per launch (bench.py gather_block).
One JSON line: us per launch, the median of 5 windows of 24 launches each."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    M, n_sl, NW, reps, windows = 25600, 256, 3, 24, 5
    res = {}
    for D, V in ((50, 3417), (256, 4_000_000)):
        rs = np.random.RandomState(D)
        table = torch.empty(V, D, device="cuda").uniform_(-0.05, 0.05)
        tg = torch.zeros(V, D, device="cuda")
        pn = torch.from_numpy(rs.randint(1, V, (NW + reps, 2, M)).astype(np.int32)).cuda()
        s, x, dx, ds = (torch.randn(M, D, device="cuda") for _ in range(4))
        gam = torch.ones(D, device="cuda")
        slabs = torch.zeros(n_sl, 2 * D, device="cuda")
        coef = torch.empty(2, M, device="cuda")
        st = torch.zeros(16, device="cuda")
        ln = lambda k, **kw: O.head_fwd_bwd_ln(s, D, table, pn[k, 0], pn[k, 1], M, D, st, x, D, gam, dx, D, slabs, slabs[0, D:], 2 * D, n_sl, **kw)
        forms = {"head_ln vector form": lambda k: ln(k, coef_out=coef),
                 "head_ln with table_grad": lambda k: ln(k, table_grad=tg),
                 "head": lambda k: O.head_fwd_bwd(s, D, table, pn[k, 0], pn[k, 1], M, D, st, d_seq_emb=ds, ldd=D, table_grad=tg)}
        for name, f in forms.items():
            us = []
            for _ in range(windows):
                for k in range(NW):
                    f(k)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(reps):
                    f(NW + k)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / reps)
            res["%s, D = %d" % (name, D)] = round(float(np.median(us)), 2)
        del table, tg
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""cr_adam_step alone at the headline shape: HIP-event time per launch as built, with one slab, and the sizes behind it.

    --big    instead: cr_adam_step alone on a synthetic table of 64 Mi floats per array (256 MB: the size at which the sweep switches
             to its streaming forms), once from a gradient array (k_adam<., 0, 1>) and once from an occurrence index at D = 128
             (k_adam<., 32, 4>); CASTREC_ADAM_STREAM=0 / 1 forces the plain / the streaming form.  5 warm-up launches, 20 timed (HIP
             events); one JSON line per case."""
import ctypes as C, json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import castrec_amd
from castrec_amd import engine as E, lib as L, ops, synth
from castrec_amd.sampler import WarpSampler


def big(n_table=64 << 20, D=128, M=128 * 200, warmup=5, reps=20):
    rs = np.random.RandomState(0)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    V = n_table // D
    p = torch.randn(n_table + 256, device=dev) * 0.05
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    slabs = torch.randn(1, 256, device=dev)
    state = torch.zeros(16, device=dev)
    state[2] = 1000.0
    state[4:5].view(torch.int32).fill_(3)
    # the index of one headline-sized batch (Zipf ids, as tests/test_index.py draws them) over a table of V rows of D columns
    w = np.r_[0.0, 1.0 / np.arange(1, V) ** 1.2]
    seq, pos, neg = (rs.choice(V, M, p=w / w.sum()).astype(np.int32) for _ in range(3))
    ng, ent, lay = C.c_int(), C.c_int(), L.IndexLayout()
    assert L.lib.cr_tgrad_geometry(D, C.byref(ng), C.byref(ent)) == 1
    L.check(L.lib.cr_batch_index_layout(M, V, 0, ng.value, ent.value, C.byref(lay)), "layout")
    b = L.lib.cr_index_builder_create(M, V, 0, ng.value, ent.value)
    ix = np.zeros(lay.total_words, np.int32)
    L.check(L.lib.cr_index_build(b, seq.ctypes.data, pos.ctypes.data, neg.ctypes.data, ix.ctypes.data), "build")
    L.lib.cr_index_builder_destroy(b)
    d_ix, rows, emb, coef = t(ix), t(rs.standard_normal((M, D)).astype(np.float32)), t(rs.standard_normal((M, D)).astype(np.float32)), \
        t(rs.standard_normal((2, M)).astype(np.float32))
    part = torch.zeros(lay.cap_blocks, (D + 3) // 4 * 4, device=dev)
    tickets = torch.zeros(lay.cap_blocks, dtype=torch.int32, device=dev)
    tg = L.TgradDesc(d_ix.data_ptr(), None, 0, 0, 0, state.data_ptr() + 16, lay, rows.data_ptr(), None, D, float(np.sqrt(D)),
                     emb.data_ptr(), D, coef.data_ptr(), D, part.data_ptr(), tickets.data_ptr())
    for label in ("table_grad", "index_D128"):
        grad = torch.randn(n_table, device=dev) if label == "table_grad" else None
        ts = []
        for r in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.adam_step(p, m, v, grad, slabs, n_table, 256, 1, 1e-3, state, tg=None if grad is not None else tg)
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append(e0.elapsed_time(e1) * 1e3)
        assert bool(torch.isfinite(p).all())
        print(json.dumps(dict(case=label, n_table=n_table, stream_env=os.environ.get("CASTREC_ADAM_STREAM"), lib=os.path.basename(L.LIB_PATH),
                              us_median=float(np.median(ts)), us_min=float(np.min(ts)), us_max=float(np.max(ts)))))
        del grad


if "--big" in sys.argv[1:]:
    big()
    sys.exit(0)

B, T = 128, 200
corpus = synth.preset("ml-1m")
sargs = types.SimpleNamespace(seed=42, bin_in_hours=48, max_bins=200, log_scale=False)
smp = WarpSampler(sargs, corpus, corpus.usernum, corpus.itemnum, batch_size=B, maxlen=T)
u, seq, pos, neg, ts_, rat, hrs, dys, _ = smp.next_batch()
smp.close()
hp = E.Hyper(maxlen=T, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.2, max_bins=200, lr=1e-3)
eng = E.Engine("cast_1", corpus.usernum, corpus.itemnum, hp, B, training=True)
eng.set_batch(seq, pos, neg, ts_, hrs, dys)
for _ in range(3):
    eng.launch_step()
torch.cuda.synchronize()
ad = eng._adam[2][0]._obj
lay = eng.layout
print("n_table", lay.n_table, "n_dense", lay.n_dense, "n_slabs", ad.n_slabs, "slab counts", None if eng.slab_counts is None else eng.slab_counts.cpu().numpy().tolist())
s = torch.cuda.current_stream().cuda_stream
big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")


def timed(label, reps=40, dirty=False):
    ts = []
    for _ in range(reps):
        if dirty:
            big.add_(1.0)                                  # 512 MB through the caches: the slabs come from HBM
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng._run([eng._adam], s)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    print("%-40s median %.1f us  min %.1f" % (label, np.median(ts), np.min(ts)))


timed("as built (slabs warm in the caches)")
timed("as built, caches flushed before", dirty=True)
ns, cnt = ad.n_slabs, ad.slab_counts
ad.n_slabs = 1
timed("one slab")
timed("one slab, caches flushed", dirty=True)
ad.n_slabs = ns
nd = ad.n_dense
ad.n_dense = 256
timed("256 dense parameters (table section + launch)")
ad.n_dense = nd

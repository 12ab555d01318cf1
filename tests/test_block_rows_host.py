"""tests/block_rows_ref.py on the CPU: the fp64 references of the four row phases agree with torch autograd in float64 (1e-12 relative,
every variant: tails, the `_ln` form, heads, dq_part, dx_accumulate, scatter), a numpy emulation of each arithmetic (the fp32 k-ordered
fmaf chain, split bf16x3, plain bf16: gemm_ref.emu_product, and layernorm_ref(fp32=True)) stays inside every bound on every case of the
GPU sweep -- the proof that a correct kernel can pass -- named defects applied to that emulation do not, and the premises the cases of
tests/test_block_rows_gpu.py rest on hold on the generated inputs themselves."""
import numpy as np
import pytest
import torch

import block_rows_ref as B
import gemm_ref as G
from row_ops_ref import LN_EPS, bound, embed_ref, wide

F64 = np.float64
FORMS = ["f32", "x3", "bf16"]


def close(got, want, tol=1e-12):
    want = np.asarray(want, F64)
    assert np.abs(np.asarray(got, F64) - want).max() <= tol * max(np.abs(want).max(), 1e-300)


def T(a, grad=False):
    return torch.tensor(np.asarray(a, F64), requires_grad=grad)


def t_ln(x, g, b):
    xc = x - x.mean(-1, keepdim=True)
    return g * (xc / ((xc * xc).mean(-1, keepdim=True) + LN_EPS) ** 0.5) + b


# ------------------------------------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("D,M,rate,lnf,heads", [(5, 17, 0.0, False, 1), (33, 65, 0.3, False, 1), (64, 48, 0.3, True, 2), (50, 130, 0.0, True, 1)])
def test_ffn_refs_against_autograd(D, M, rate, lnf, heads):
    """forward (with tail 2) and backward (plain and `_ln`, attn_delta per head) of the feed-forward phase"""
    c = B.block_case(D, M, rate, 900)
    f1, f2 = (T(f) for f in B.factors(c))
    live = T((c.mask_ids != 0).astype(F64))[:, None]
    P = {k: T(wide(getattr(c, k)), True) for k in ("ln2_g", "ln2_b", "w1", "b1", "w2", "b2", "lnf_g", "lnf_b")}
    o = T(wide(c.o), True)
    f_in = t_ln(o, P["ln2_g"], P["ln2_b"])
    hid = torch.relu(f_in @ P["w1"] + P["b1"]) * f1
    y = ((hid @ P["w2"] + P["b2"]) * f2 + f_in) * live
    out = t_ln(y, P["lnf_g"], P["lnf_b"])
    ref = B.ffn_fwd_ref(c, "f32")
    close(ref.f_in, f_in.detach()); close(ref.hid, hid.detach()); close(ref.y, y.detach())
    close(B.final_ln_ref(c, ref.y, ref.e_y)[0], out.detach())
    (out if lnf else y).backward(T(wide(c.dy)))
    q_in = wide(c.q_in)
    R = B.ffn_bwd_ref(c, "f32", wide(c.dy), hid.detach().numpy(), f_in.detach().numpy(), heads=heads, q_in=q_in,
                      lnf=(y.detach().numpy(), c.lnf_g) if lnf else None)
    for m in range(M):
        close(R.d_o[m], o.grad.numpy()[m])
    for name, key in (("g_w2", "w2"), ("g_b2", "b2"), ("g_w1", "w1"), ("g_b1", "b1"), ("g_ln2_g", "ln2_g"), ("g_ln2_b", "ln2_b")):
        close(getattr(R, name), P[key].grad.numpy())
    if lnf:
        close(R.lnf_dgamma, P["lnf_g"].grad.numpy()); close(R.lnf_dbeta, P["lnf_b"].grad.numpy())
    delta = (o.grad.numpy() * (wide(c.o) - q_in)).reshape(M, heads, D // heads).sum(2).T
    close(R.attn_delta, delta)
    assert R.attn_delta.shape == (heads, M)


@pytest.mark.parametrize("D,M,dq_part,acc,scatter", [(6, 16, False, False, None), (33, 65, True, True, None), (64, 130, True, False, None),
                                                     (20, 60, False, False, "extras"), (7, 15, True, False, "table")])
def test_qkv_refs_against_autograd(D, M, dq_part, acc, scatter):
    """forward (from x, and from a gathered x) and backward (dq_part, dx_accumulate, scattered through the embedding recipe); the
    gradient of o reaches q_in through the residual of the attention output"""
    c = B.gather_case(D, M, 5, 0.3, 900, scatter == "extras") if scatter else B.block_case(D, M, 0.3, 900)
    P = {k: T(wide(getattr(c, k)), True) for k in ("ln1_g", "ln1_b", "wqkv", "bqkv")}
    if scatter:
        e = c.emb
        table, pos, add = T(wide(e.table), True), T(np.zeros((e.T, D)) if e.pos is None else wide(e.pos), True), T(np.zeros((M, D)) if e.addend is None else wide(e.addend), True)
        tz = torch.cat([torch.zeros(1, D, dtype=torch.float64), table[1:]], 0)
        from row_ops_ref import row_factor
        x = (tz[torch.tensor(e.ids, dtype=torch.int64)] * e.scale + pos.repeat(M // e.T, 1) + add) * T(row_factor(e, M, D))
        close(embed_ref(e)[0], x.detach())
        x_np, kw = x.detach().numpy(), dict(x=x.detach().numpy(), e_x=c.e_x)
    else:
        x = T(wide(c.x), True)
        x_np, kw = wide(c.x), {}
    q_in = t_ln(x, P["ln1_g"], P["ln1_b"])
    qkv = torch.stack([(q_in if p == 0 else x) @ P["wqkv"][:, p * D:(p + 1) * D] + P["bqkv"][p * D:(p + 1) * D] for p in range(3)])
    ref = B.qkv_fwd_ref(c, "f32", **kw)
    close(ref.q_in, q_in.detach()); close(ref.qkv, qkv.detach())
    assert np.array_equal(ref.k_valid, (x_np.sum(1) != 0)) and np.array_equal(ref.q_valid, q_in.detach().numpy().sum(1) != 0)
    dqkv = wide(c.dqkv).copy()
    dQ = dqkv[0] + (wide(c.dq_part) if dq_part else 0.0)
    ((qkv * T(np.stack([dQ, dqkv[1], dqkv[2]]))).sum() + (q_in * T(wide(c.d_o_in))).sum()).backward()
    cc = B.NS(**{**c.__dict__, "x": x_np})              # the backward reads x as stored: exact here
    R = B.qkv_bwd_ref(cc, "f32", dqkv, wide(c.d_o_in), q_in.detach().numpy(), c.dq_part if dq_part else None, c.dx0 if acc else None)
    for name, key in (("g_wqkv", "wqkv"), ("g_bqkv", "bqkv"), ("g_ln1_g", "ln1_g"), ("g_ln1_b", "ln1_b")):
        close(getattr(R, name), P[key].grad.numpy())
    if not scatter:
        want = x.grad.numpy() + (wide(c.dx0) if acc else 0.0)
        for m in range(M):
            close(R.dx[m], want[m])
        return
    sc = B.scatter_ref(c.emb, R.dx, R.e_dx, True, True, True)
    close(sc["table_grad"][0], table.grad.numpy()); close(sc["pos_grad"][0], pos.grad.numpy()); close(sc["d_addend"][0], add.grad.numpy())
    assert (sc["table_grad"][0][0] == 0).all()


# ------------------------------------------------------------------------------------------------ the emulation inside the bounds
def bwd_ratio(c, form, ns, variant, defect=None):
    """(largest error / allowance of the feed-forward backward, of the projection backward, names) of the emulation"""
    R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=1, q_in=wide(c.q_in))
    g = B.emu_ffn_bwd(c, form, ns, c.dy, c.hid, c.f_in, c.q_in, defect=defect)
    a = B.worst(B.items_bwd(R, g, B.FFN_SLABS, [("d_o", "e_d_o"), ("attn_delta", "e_attn_delta")]))
    dqp, dx0 = c.dq_part if variant & 1 else None, c.dx0 if variant & 2 else None
    R = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), dqp, dx0)
    g = B.emu_qkv_bwd(c, form, ns, c.dqkv, c.d_o_in, c.q_in, dqp, dx0, defect=defect)
    b = B.worst(B.items_bwd(R, g, B.QKV_SLABS, [("dx", "e_dx")]))
    return a, b


@pytest.mark.parametrize("form", FORMS)
def test_emulation_inside_bounds(form):
    """every case of the GPU sweep, forward (both tails) and backward; the largest ratio per operation is printed"""
    top = {}

    def note(op, w):
        top[op] = max(top.get(op, (0.0, "")), w)
    for D, M, rate, ro in B.tile_fwd_cases():
        c = B.block_case(D, M, rate, ro)
        note("qkv_fwd", B.worst(B.items_qkv_fwd(c, form, B.emu_qkv_fwd(c, form))))
        f = B.emu_ffn_fwd(c, form)
        note("ffn_fwd", B.worst(B.items_ffn_fwd(c, form, f)))
        note("tail 1", B.worst(B.items_tail1(c, form, f.y, B.emu_qkv_fwd(c, form, w=c.next, x=f.y))))
        note("tail 2", B.worst(B.items_tail2(c, form, f.y, B.ln32(f.y, c.lnf_g, c.lnf_b).y)))
    for D, M, ns, rate, ro, v in B.tile_bwd_cases():
        a, b = bwd_ratio(B.block_case(D, M, rate, ro), form, ns, v)
        note("ffn_bwd", a); note("qkv_bwd", b)
    print("largest emulated error / bound, %s: %s" % (form, ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in top.items())))
    assert all(v[0] <= 1.0 for v in top.values()), top


@pytest.mark.parametrize("form", ["x3", "bf16"])
def test_emulation_inside_bounds_register_layout(form):
    """the cases of the register-layout backward: `_ln`, two heads at D = 64, dx_accumulate"""
    top = {}
    for D, Bn, T, ns, rate, ro, v in B.reg_cases():
        c = B.block_case(D, Bn * T, rate, ro)
        heads = 2 if (D == 64 and v >= 2) else 1
        ln = v in (1, 3)
        R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=heads, q_in=wide(c.q_in), lnf=(wide(c.y), c.lnf_g) if ln else None)
        g = B.emu_ffn_bwd(c, form, ns, c.dy, c.hid, c.f_in, c.q_in, heads=heads, lnf=(c.y, c.lnf_g) if ln else None)
        names = B.FFN_SLABS + (("lnf_dgamma", "lnf_dbeta") if ln else ())
        top["ffn_bwd"] = max(top.get("ffn_bwd", (0.0, "")), B.worst(B.items_bwd(R, g, names, [("d_o", "e_d_o"), ("attn_delta", "e_attn_delta")])))
        dx0 = c.dx0 if v & 1 else None
        R = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), None, dx0)
        g = B.emu_qkv_bwd(c, form, ns, c.dqkv, c.d_o_in, c.q_in, None, dx0)
        top["qkv_bwd"] = max(top.get("qkv_bwd", (0.0, "")), B.worst(B.items_bwd(R, g, B.QKV_SLABS, [("dx", "e_dx")])))
    print("largest emulated error / bound, register layout, %s: %s" % (form, top))
    assert all(v[0] <= 1.0 for v in top.values()), top


@pytest.mark.parametrize("form", ["x3", "bf16"])
def test_emulation_inside_bounds_wide(form):
    """the cases of the wide family, forward and backward (g2, g1 and the overwritten d_o included)"""
    top = {}

    def note(op, w):
        top[op] = max(top.get(op, (0.0, "")), w)
    for D, M, rate, ro in B.wide_fwd_cases():
        c = B.block_case(D, M, rate, ro)
        note("qkv_fwd", B.worst(B.items_qkv_fwd(c, form, B.emu_qkv_fwd(c, form))))
        note("ffn_fwd", B.worst(B.items_ffn_fwd(c, form, B.emu_ffn_fwd(c, form))))
    for D, M, ns, rate, ro, own, heads, acc in B.wide_bwd_cases():
        c = B.block_case(D, M, rate, ro)
        R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=max(heads, 1), q_in=wide(c.q_in))
        g = B.emu_ffn_bwd(c, form, ns, c.dy, c.hid, c.f_in, c.q_in, heads=max(heads, 1))
        note("ffn_bwd", B.worst(B.items_bwd(R, g, B.FFN_SLABS, [("d_o", "e_d_o"), ("attn_delta", "e_attn_delta")])))
        dx0 = c.dx0 if acc else None
        R = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), None, dx0)
        g = B.emu_qkv_bwd(c, form, ns, c.dqkv, c.d_o_in, c.q_in, None, dx0)
        note("qkv_bwd", B.worst(B.items_bwd(R, g, B.QKV_SLABS, [("dx", "e_dx")])))
    print("largest emulated error / bound, wide, %s: %s" % (form, top))
    assert all(v[0] <= 1.0 for v in top.values()), top


def test_bounds_have_no_room_for_the_named_defects():
    """what the GPU tests must notice, on the CPU: each defect applied to the emulation leaves a bound at the shapes named"""
    # one weight column read from the neighbouring column at D % 4 != 0
    for D, M in ((5, 17), (33, 65), (63, 16)):
        c = B.block_case(D, M)
        assert B.worst(B.items_qkv_fwd(c, "f32", B.emu_qkv_fwd(c, "f32", "neighbour_column")))[0] > 100
        assert B.worst(B.items_ffn_fwd(c, "f32", B.emu_ffn_fwd(c, "f32", "neighbour_column")))[0] > 100
        a, b = bwd_ratio(c, "f32", 1, 0, "neighbour_column")
        assert a[0] > 100 and b[0] > 100
    # the bias gradient taken from row D - 1 instead of the ones row
    for D, M, ns in ((5, 17, 1), (50, 130, 3), (63, 65, 1)):
        a, b = bwd_ratio(B.block_case(D, M), "f32", ns, 0, "bias_row")
        assert a[0] > 100 and a[1] in ("g_b1", "g_b2") and b[0] > 100 and b[1] == "g_bqkv"
    # the dropout index using 64 in place of D: another mask (at D = 64 the same one)
    for D, M in ((5, 17), (50, 65), (63, 130)):
        c = B.block_case(D, M, 0.3, 900)
        assert B.worst(B.items_ffn_fwd(c, "f32", B.emu_ffn_fwd(c, "f32", "drop_index_64")))[0] > 100
        assert bwd_ratio(c, "f32", 2, 0, "drop_index_64")[0][0] > 100
    # the mean formed as sum / 64
    for D, M in ((5, 17), (50, 65), (63, 130)):
        c = B.block_case(D, M)
        assert B.worst(B.items_qkv_fwd(c, "f32", B.emu_qkv_fwd(c, "f32", "mean_64")))[0] > 100
        assert B.worst(B.items_ffn_fwd(c, "f32", B.emu_ffn_fwd(c, "f32", "mean_64")))[0] > 100
        a, b = bwd_ratio(c, "f32", 1, 0, "mean_64")
        assert a[0] > 100 and b[0] > 100
    # al * bh dropped from the split product
    for D, M in ((8, 17), (50, 65), (64, 130)):
        c = B.block_case(D, M)
        assert B.worst(B.items_qkv_fwd(c, "x3", B.emu_qkv_fwd(c, "x3", "no_al_bh")))[0] > 10
        assert B.worst(B.items_ffn_fwd(c, "x3", B.emu_ffn_fwd(c, "x3", "no_al_bh")))[0] > 10
        a, b = bwd_ratio(c, "x3", 1, 0, "no_al_bh")
        assert a[0] > 10 and b[0] > 10
    # a slab's last partial tile skipped
    for D, M, ns in ((5, 130, 1), (50, 65, 1), (64, 200, 2), (33, 17, 4)):
        a, b = bwd_ratio(B.block_case(D, M), "f32", ns, 0, "skip_partial_tile")
        assert a[0] > 100 and b[0] > 100


# ------------------------------------------------------------------------------------------------ premises
def all_cases():
    seen = {}
    for D, M, rate, ro in B.tile_fwd_cases():
        seen[(D, M, rate, ro, False)] = None
    for D, M, ns, rate, ro, v in B.tile_bwd_cases():
        seen[(D, M, rate, ro, False)] = None
    for key in B.EXTRA_CASES:
        seen[key] = None
    for D, Bn, T, ns, rate, ro, v in B.reg_cases():
        seen[(D, Bn * T, rate, ro, False)] = None
    for D, Bn, T, ns, s, a in B.REG_SCATTER:
        seen[(D, Bn * T, 0.3, 900, False, T)] = None
    for D, M, rate, ro in B.wide_fwd_cases():
        seen[(D, M, rate, ro, False)] = None
    for c in B.wide_bwd_cases():
        seen[(c[0], c[1], c[3], c[4], False)] = None
    return [B.block_case(*k) for k in seen] + [B.sub_case(*B.wide_big())]


def test_every_row_flag_is_decidable():
    """the valid-mask condition on every drawn case, no row excluded: a row's fp64 sum is exactly zero or MARGIN summation bounds away
    from it -- for x and q_in, for y and the next block's q_in (tail 1), and for every gathered input"""
    n = 0
    for c in all_cases():
        z = np.zeros((c.M, c.D))
        q_in, e_q, _, _ = B.ln_fwd(wide(c.x), z, c.ln1_g, c.ln1_b)
        f = B.ffn_fwd_ref(c, "f32")
        q2, e_q2, _, _ = B.ln_fwd(f.y, f.e_y, c.next.ln1_g, c.next.ln1_b)
        for v in (wide(c.x), q_in, f.y, q2):
            assert B.valid_margin(v).all(), (c.D, c.M)
        live = c.mask_ids != 0
        assert (wide(c.x)[~live] == 0).all() and (f.y[~live] == 0).all()
        n += 1
    for key in B.GATHER_CASES:
        c = B.gather_case(*key)
        q_in, e_q, _, _ = B.ln_fwd(c.x_ref, c.e_x, c.ln1_g, c.ln1_b)
        assert B.valid_margin(c.x_ref).all() and B.valid_margin(q_in).all(), key
    c = B.block_case(*B.BETA0_CASE)
    q = B.qkv_fwd_ref(c, "f32")
    dead = c.mask_ids == 0
    assert dead.any() and (c.ln1_b == 0).all() and (q.q_valid[dead] == 0).all() and (q.k_valid[dead] == 0).all() and (q.q_valid[~dead] == 1).all()
    assert n > 40


def test_premises_shapes():
    fwd, bwd = B.tile_fwd_cases(), B.tile_bwd_cases()
    assert {c[0] for c in fwd} == {c[0] for c in bwd} == set(B.TILE_D) == {4, 5, 6, 7, 8, 20, 33, 50, 63, 64}
    assert {c[1] for c in fwd} == set(B.TILE_M) == {1, 15, 16, 17, 63, 64, 65, 130, 200}
    for D in B.TILE_D:
        assert len({c[1] for c in fwd if c[0] == D}) >= 2 and len({c[1:3] for c in bwd if c[0] == D}) >= 2
    for M in B.TILE_M:
        assert len({c[0] for c in fwd if c[1] == M}) >= 2
    assert {(0.0, 0), (0.3, 0), (0.3, 900)} <= {c[2:4] for c in fwd} and {(0.0, 0), (0.3, 0), (0.3, 900)} <= {c[3:5] for c in bwd}
    pairs = {c[1:3] for c in bwd}
    assert {(130, 1), (130, 3), (200, 2), (5, 8), (64, 1), (65, 1)} <= pairs
    for ms in pairs:
        assert len({c[0] for c in bwd if c[1:3] == ms}) >= 2, ms
    assert {B.ng_of(*p) for p in pairs} == {1, 2}
    assert B.ng_of(64, 1) == 1 and B.ng_of(65, 1) == 2 and B.ng_of(130, 3) == 1 and B.ng_of(200, 2) == 2
    assert sum(a == b for a, b in G.slab_rows(5, 8)) == 3 and sum(a == b for a, b in G.slab_rows(17, 4)) == 0
    assert [b - a for a, b in G.slab_rows(130, 1)] == [130]                    # two tile groups, then a third trip of 2 rows: odd tile count
    assert {c[5] for c in bwd} == set(range(8))                                # dq_part x dx_accumulate x attn_delta
    for D in (5, 50, 64):                                                      # the ones column (D < 64) and the colsum route (D = 64), both NG
        assert {B.ng_of(c[1], c[2]) for c in bwd if c[0] == D} == {1, 2} or D == 5
    assert {B.ng_of(c[1], c[2]) for c in bwd if c[0] == 64} == {1, 2} and {B.ng_of(c[1], c[2]) for c in bwd if c[0] < 64 and c[0] % 4} == {1, 2}
    assert B.kernel_of("qkv_bwd", 130, 1, scatter="pos") == "k_block_ln_qkv_bwd<2, 2>" and B.kernel_of("ffn_bwd", 130, 3) == "k_block_ln_ffn_bwd<1>"
    kernels = {B.kernel_of("qkv_fwd"), B.kernel_of("qkv_fwd_gather")} | {B.kernel_of("ffn_fwd", tail=t) for t in (0, 1, 2)}
    kernels |= {B.kernel_of("ffn_bwd", c[1], c[2]) for c in bwd} | {B.kernel_of("qkv_bwd", c[1], c[2]) for c in bwd}
    kernels |= {B.kernel_of("qkv_bwd", M, ns, scatter=s) for D, M, T_, ns, s, add in B.SCATTER_CASES}
    assert kernels == set(B.TILE_KERNELS), sorted(set(B.TILE_KERNELS) - kernels)
    for c in all_cases():
        if c.rate > 0:
            f1, f2 = B.factors(c)
            assert c.M * c.D < 16 or (0.4 < (f1 != 0).mean() < 0.95 and 0.4 < (f2 != 0).mean() < 0.95 and (f1 != f2).any())
        if c.M * c.D >= 64:
            pre = B.ffn_fwd_ref(c, "f32")
            assert 0.2 < (pre.hid > 0).mean() < 0.8
        if c.M > 1:
            assert 0 < (c.mask_ids != 0).sum() < c.M


def test_split_images():
    """the operand constants the bf16 bounds rest on, on drawn data"""
    x = wide(B.block_case(50, 65).x)
    hi, lo = G.split(B.block_case(50, 65).x)
    assert (np.abs(x - hi) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(x - hi - lo) <= 2.0 ** -16 * np.abs(x)).all()
    assert bound(1.0, 3, 1) == 8 * B.U


def test_premises_register_layout_and_wide():
    reg = B.reg_cases()
    assert {c[0] for c in reg} == set(B.REG_D) == {8, 9, 24, 33, 50, 63, 64} and {c[2] for c in reg} == set(B.REG_T) == {1, 15, 16, 17, 112, 113, 224}
    assert {c[1] for c in reg} == {1, 3}
    for D in B.REG_D:
        assert len({c[1:3] for c in reg if c[0] == D}) >= 2
    for T_ in B.REG_T:
        assert len({c[0] for c in reg if c[2] == T_}) >= 2
    kinds = {("1" if ns == 1 else "2" if ns == 2 and Bn != 2 else "B" if ns == Bn else "B+2" if ns == Bn + 2 else "?") for D, Bn, T_, ns, *_ in reg}
    assert {"1", "2", "B+2"} <= kinds and any(ns == Bn == 3 for D, Bn, T_, ns, *_ in reg)
    assert B.reg_rounds(112) == 1 and B.reg_rounds(113) == 2 and B.reg_rounds(224) == 2
    assert any(B.reg_empty_slabs(c[1], c[2], c[3]) for c in reg) and B.reg_empty_slabs(1, 113, 3) == [2] and B.reg_empty_slabs(3, 16, 5) == [3, 4]
    assert {c[6] for c in reg} == {0, 1, 2, 3} and {c[6] for c in reg if c[0] == 64} >= {2, 3}            # `_ln`, `_heads` with and without it; two heads
    assert {B.reg_kernel_of("ffn", c[0], f) for c in reg for f in ("x3", "bf16")} == {
        "k_stack_ffn_bwd<%s, %d>" % (sp, ds) for sp in ("true", "false") for ds in (0, 50, 64)}
    assert {s for *_, s, a in B.REG_SCATTER} == {"table", "pos"} and {a for *_, a in B.REG_SCATTER} == {False, True}
    fwd, bwd = B.wide_fwd_cases(), B.wide_bwd_cases()
    assert {c[0] for c in fwd} == {c[0] for c in bwd} == {128, 192, 256} and {c[1] for c in fwd} == {c[1] for c in bwd} == {1, 63, 64, 65, 127, 128, 129, 300}
    for M in B.WIDE_M:
        assert len({c[0] for c in fwd if c[1] == M}) >= 2 and len({c[0] for c in bwd if c[1] == M}) >= 2
    assert all(c[0] == 128 for c in bwd if c[5]) and {c[1] for c in bwd if c[5]} == set(B.WIDE_M) and any(c[0] == 128 and not c[5] for c in bwd)
    assert {c[6] for c in bwd} == {0, 1, 2, 4, 8} and all(not c[6] or (c[0] // c[6]) % 16 == 0 for c in bwd) and {c[7] for c in bwd} == {False, True}
    assert any(B.wide_empty_slabs(c[0], c[1], c[2]) for c in bwd if c[5]) and any(B.wide_empty_slabs(c[0], c[1], c[2]) for c in bwd if not c[5])
    assert B.wide_rows(128) == 128 and B.wide_rows(192) == 64 and B.wide_rows(192, True, 300) == 64 and B.wide_rows(*B.WIDE_BIG[:1], True, B.WIDE_BIG[1]) == 128
    c, idx = B.wide_big()
    assert c.M == 32641 and -(-c.M // 128) == 256 and idx[0] == 0 and idx[-1] == c.M - 1 and len(idx) == 4 * 128 + 1

"""The fused row phases of a transformer block in all three kernel families, called through the C ABI and held element by element to
the fp64 numpy references and bounds of tests/block_rows_ref.py (tests/test_block_rows_host.py checks those references against torch
autograd, shows a CPU emulation of each arithmetic inside every bound and named defects outside):
    tile kernels, fp32, D 4..64                 csrc/cr_block.hip                  cr_block_ln_*
    register-layout backward, bf16x3 / bf16, D 8..64    csrc/cr_stack_bwd.hip, cr_rbwd.hpp    cr_stack_ffn_bwd*, cr_stack_qkv_bwd*
    wide, bf16x3 / bf16, D 128 / 192 / 256      csrc/cr_wide.hip                   cr_wide_ln_*
The attention core is not called (no cr_attn_*, cr_stack_fwd, cr_stack_block_bwd).

Every operand and every output sits in an allocation of its own, one float past a 16-byte boundary (the kernels take dword alignment;
no entry point asks for more), between guard words of ops_harness.SENTINEL -- a NaN with a payload -- that must come back bit for
bit.  Outputs start as that NaN: an element the contract says is written must be finite afterwards, every slab of n_slabs included,
and a slab that owns no row must be exact zeros (cr_adam_step / cr_reduce_slabs read them all).  Each backward form runs twice and
must give the same bits (the float atomics of the scatter forms exempt the table / positional gradient).  A refusal comes from the
host checks in front of the launch, is pinned by its cr_last_error text and leaves every output word as it was.  A test walks its
cases itself and reports every failing one.

What reaches what (block_rows_ref.kernel_of / reg_kernel_of / wide_kernel_of name the instantiation of a case; it is printed with
every failure):
  k_block_ln_qkv_fwd<false>       test_qkv_fwd: D x M of tile_fwd_cases (D % 4 != 0: the shifted-back chunk of fetch_w / stream_fetch;
                                  M = 1 .. 200: waves without rows, partial strips, four workgroups), beta1 = 0 with all-zero rows
  k_block_ln_qkv_fwd<true>        test_qkv_fwd_gather: x composed in the kernel, with and without positional table / addend, dropout with
                                  row_offset 900
  k_block_ln_ffn_fwd<0|1|2>       test_ffn_fwd[0|1|2]: dropout 0 / 0.3, row_offset 0 / 900; tail 2 at col_out = 3 of ld_out = D + 5
  k_block_ln_ffn_bwd<1|2>         test_ffn_bwd: (M, n_slabs) of TILE_SLABS: one and two tile groups, an odd tile count, a partial last
                                  tile, slabs without rows; the ones column (D < 64) and the column-sum route (D = 64); attn_delta or NULL
  k_block_ln_qkv_bwd<1|2, 0>      test_qkv_bwd: the same, dq_part given or NULL, dx written or accumulated
  k_block_ln_qkv_bwd<1|2, 1|2>    test_qkv_bwd_scatter: table only, with pos_grad, with d_addend
  k_stack_ffn_bwd<true|false, 0|50|64>   test_reg_ffn_bwd[x3|bf16]: cr_stack_ffn_bwd, _ln (dy at a pitch of D + 3), _heads with and without the
                                  LayerNorm, two heads at D = 64; T = 1 .. 224 (one tile, seven, a second round), B = 1, 3,
                                  n_slabs 1, 2, B, B + 2 (work items dealt in turn; slabs without any)
  k_stack_qkv_bwd<true|false, 0|50|64>   test_reg_qkv_bwd[x3|bf16] (dx written or accumulated), test_reg_qkv_bwd_scatter[x3|bf16]
  k_wide_qkv_fwd / k_wide_ffn_fwd<8|12|16, true|false, 0|2(, 0)>   test_wide_fwd[x3|bf16]: 128 rows per workgroup at D = 128, 64 above;
                                  <12, *, 0>: test_wide_fwd_8_waves_above_128 (M = 32641: 256 row blocks)
  k_wide_ffn_fwd<8, true|false, 0, 1|2>   test_wide_fwd_tail[1|2-x3|bf16]
  k_wide_ffn_bwd / k_wide_qkv_bwd<8, *, true>    test_wide_bwd[x3|bf16], D = 128 with its own weight gradients
  k_wide_ffn_bwd / k_wide_qkv_bwd<8|12|16, *, false>   test_wide_bwd[x3|bf16], NULL weight-gradient pointers: g2, g1 and the overwritten d_o
  host checks                     test_refusals, test_refusals_leave_outputs, test_reg_refusals, test_wide_refusals
  one reference, every form       test_forms_share_one_reference"""
import ctypes as C

import numpy as np
import pytest
import torch

import block_rows_ref as B
import gemm_ref as G
from ops_harness import SENTINEL, Pad, dev, new_state
from row_ops_ref import wide

pytestmark = pytest.mark.gpu

F64 = np.float64
FORM = "f32"


@pytest.fixture(scope="module")
def ops():
    import castrec_amd  # noqa: F401
    from castrec_amd import ops as O
    assert torch.cuda.is_available()
    return O


class Fails(list):
    """the failing cases of one test, and the largest error / bound it saw (printed in front of the assertion)"""
    top = 0.0

    def report(self, what):
        print("%s: largest error / bound %.3f" % (what, self.top))
        assert not self, "%d failed:\n%s" % (len(self), "\n".join(self[:40]))


def hold(items, what, fails):
    """every (name, got, reference, allowance): an element outside its allowance (a NaN -- never written -- is) is a failure"""
    for name, got, ref, allow in items:
        err = np.abs(np.asarray(got, F64) - ref)
        ratio = np.nan_to_num(np.where(err == 0, 0.0, err / np.maximum(allow, 1e-300)), nan=np.inf)
        fails.top = max(fails.top, float(ratio.max()) if ratio.size else 0.0)
        bad = ~(err <= allow)
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, ratio, 0)), err.shape)
            fails.append("%s, %s: %d of %d outside; worst at %s got %r, reference %r, error / bound %.3g" % (
                what, name, int(bad.sum()), bad.size, i, float(np.asarray(got)[i]), float(ref[i]), float(ratio[i])))


class Dev:
    """the device side of one call: named Pads (inputs with data, outputs all SENTINEL), each its own allocation at lead = 1"""

    def __init__(self, ops, c):
        self.ops, self.c, self.pads, self.outs = ops, c, {}, []
        self.state = new_state(step=B.STEP)
        self.mask = dev(c.mask_ids, torch.int32)

    def put(self, name, data, rows=None, cols=None):
        data = np.asarray(data, np.float32)
        rows, cols = (1, data.size) if data.ndim == 1 else (int(np.prod(data.shape[:-1])), data.shape[-1])
        self.pads[name] = Pad(rows, cols, [(0, cols)], data, lead=1)
        return self.pads[name].t.data_ptr()

    def out(self, name, rows, cols, ld=None, col=0, data=None):
        self.pads[name] = Pad(rows, ld or cols, [(col, cols)], data, lead=1)
        self.outs.append(name)
        return self.pads[name].t.data_ptr()

    def get(self, name, shape=None):
        a = self.pads[name].read()
        return a.reshape(shape) if shape else a

    def rng(self, site, rate=None):
        c = self.c
        rate = c.rate if rate is None else rate
        return self.ops.Drop(rate, c.seed, self.state, c.row_offset).rng(site) if rate > 0 else self.ops.NO_DROP

    def weights(self, w, names):
        """the parameter vectors of w, uploaded once per Dev"""
        pre = "next." if w is not self.c else ""
        return {n: self.pads[pre + n].t.data_ptr() if pre + n in self.pads else self.put(pre + n, getattr(w, n)) for n in names}

    def intact(self, what, fails):
        """guards of every Pad intact, every output element finite"""
        for n, p in self.pads.items():
            if not p.untouched():
                fails.append("%s: words outside %s were written" % (what, n))
        for n in self.outs:
            if not np.isfinite(self.get(n)).all():
                fails.append("%s: %s has elements that were not written" % (what, n))

    def all_sentinel(self, names=None):
        return all(bool((self.pads[n].whole.view(torch.int32) == SENTINEL).all()) for n in (names or self.outs))


GAP = 3


class Slabs:
    """n_slabs slabs of one odd stride, one float past the boundary, all SENTINEL: per gradient (name, size) a region, GAP words apart"""

    def __init__(self, n_slabs, regions):
        self.ns, self.off, o = n_slabs, {}, 2
        for name, size in regions:
            self.off[name] = (o, size)
            o += size + GAP
        self.stride = (o + 4) | 1
        self.whole = torch.full((1 + n_slabs * self.stride + 9,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.body = self.whole[1:1 + n_slabs * self.stride].view(n_slabs, self.stride)

    def ptr(self, name):
        return self.whole.data_ptr() + 4 * (1 + self.off[name][0])

    def read(self, name):
        o, n = self.off[name]
        return self.body[:, o:o + n].cpu().numpy()

    def guards_intact(self):
        keep = torch.ones_like(self.whole, dtype=torch.bool)
        inner = keep[1:1 + self.ns * self.stride].view(self.ns, self.stride)
        for o, n in self.off.values():
            inner[:, o:o + n] = False
        return bool((self.whole.view(torch.int32)[keep] == SENTINEL).all())

    def all_sentinel(self):
        return bool((self.whole.view(torch.int32) == SENTINEL).all())


def slabs_of(sl, c, n_slabs, shapes, what, fails, empty=None):
    """NS of [n_slabs, ...] arrays; every slab written, the slabs without rows (default: by gemm_ref.slab_rows) exact zeros, nothing
    written between the regions"""
    got = B.NS()
    if empty is None:
        empty = [s for s, (m0, m1) in enumerate(G.slab_rows(c.M, n_slabs)) if m0 == m1]
    for name, shape in shapes.items():
        a = sl.read(name)
        if not np.isfinite(a).all():
            fails.append("%s: %s: a slab element was not written" % (what, name))
        if empty and (a[empty] != 0).any():
            fails.append("%s: %s: a slab without rows is not zero" % (what, name))
        setattr(got, name, a.reshape((n_slabs,) + shape))
    if not sl.guards_intact():
        fails.append("%s: words outside the slab regions were written" % what)
    return got


def call(ops, name, *args):
    from castrec_amd import lib as L
    L.call(name, *args, torch.cuda.current_stream().cuda_stream)


def lib():
    from castrec_amd import lib as L
    return L


def block_desc(d, c, w=None, **ptrs):
    """cr_block_desc over the Pads of d: the weights of w (default the case's own) and the row buffers given by name"""
    L = lib()
    w = w or c
    W = d.weights(w, ("ln1_g", "ln1_b", "wqkv", "bqkv", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2"))
    g = lambda n: ptrs.get(n)
    return L.BlockDesc(c.M, c.D, W["ln1_g"], W["ln1_b"], W["wqkv"], W["bqkv"], W["ln2_g"], W["ln2_b"], W["w1"], W["b1"], W["w2"], W["b2"],
                       g("x"), g("q_in"), g("qkv"), g("k_valid"), g("q_valid"), g("o"), g("f_in"), g("hid"), g("y"), d.mask.data_ptr(),
                       d.rng(B.SITE1), d.rng(B.SITE2))


def qkv_outs(d, c, pre=""):
    M, D = c.M, c.D
    return dict(q_in=d.out(pre + "q_in", M, D), qkv=d.out(pre + "qkv", 3 * M, D), k_valid=d.out(pre + "k_valid", 1, M), q_valid=d.out(pre + "q_valid", 1, M))


def qkv_got(d, c, pre=""):
    M, D = c.M, c.D
    return B.NS(q_in=d.get(pre + "q_in"), qkv=d.get(pre + "qkv", (3, M, D)), k_valid=d.get(pre + "k_valid", (M,)), q_valid=d.get(pre + "q_valid", (M,)))


# ------------------------------------------------------------------------------------------------ forward
def test_qkv_fwd(ops):
    fails = Fails()
    for key in [k + (False,) for k in B.tile_fwd_cases()] + [B.BETA0_CASE]:
        c = B.block_case(*key)
        what = "%s D %d M %d%s" % (B.kernel_of("qkv_fwd"), c.D, c.M, " beta1 = 0" if key[4] else "")
        d = Dev(ops, c)
        desc = block_desc(d, c, x=d.put("x", c.x), **qkv_outs(d, c))
        call(ops, "cr_block_ln_qkv_fwd", C.byref(desc))
        d.intact(what, fails)
        hold(B.items_qkv_fwd(c, FORM, qkv_got(d, c)), what, fails)
    fails.report("qkv_fwd")


def embed_desc(d, c, e, out):
    L = lib()
    ids = dev(e.ids, torch.int32)
    d.keep = getattr(d, "keep", []) + [ids]
    rng = d.ops.Drop(e.rate, e.seed, d.state, e.row_offset).rng(e.site) if e.rate > 0 else d.ops.NO_DROP
    return L.EmbedDesc(ids.data_ptr(), d.put("table", e.table), e.M, e.T, e.D, e.V, e.zero_pad, e.scale,
                       d.put("pos", e.pos) if e.pos is not None else None, d.put("addend", e.addend) if e.addend is not None else None,
                       e.ld_add, rng, d.mask.data_ptr(), out, e.D, 0)


def test_qkv_fwd_gather(ops):
    fails = Fails()
    for key in B.GATHER_CASES:
        c = B.gather_case(*key)
        what = "%s D %d M %d T %d rate %.1f extras %d" % ((B.kernel_of("qkv_fwd_gather"),) + key[:4] + key[5:])
        d = Dev(ops, c)
        x = d.out("x", c.M, c.D)
        desc = block_desc(d, c, x=x, **qkv_outs(d, c))
        e = embed_desc(d, c, c.emb, x)
        call(ops, "cr_block_ln_qkv_fwd_gather", C.byref(desc), C.byref(e))
        d.intact(what, fails)
        got = qkv_got(d, c)
        hold([("x composed", d.get("x"), c.x_ref, c.e_x)], what, fails)
        hold(B.items_qkv_fwd(c, FORM, got, x_got=d.get("x"), x=c.x_ref, e_x=c.e_x), what, fails)
    fails.report("qkv_fwd_gather")


@pytest.mark.parametrize("tail", [0, 1, 2])
def test_ffn_fwd(ops, tail):
    L = lib()
    fails = Fails()
    for key in B.tile_fwd_cases():
        c = B.block_case(*key)
        M, D = c.M, c.D
        what = "%s D %d M %d rate %.1f row_offset %d" % ((B.kernel_of("ffn_fwd", tail=tail),) + key)
        d = Dev(ops, c)
        y = d.out("y", M, D)
        desc = block_desc(d, c, o=d.put("o", c.o), f_in=d.out("f_in", M, D), hid=d.out("hid", M, D), y=y)
        if tail == 0:
            call(ops, "cr_block_ln_ffn_fwd", C.byref(desc))
        elif tail == 1:
            nxt = block_desc(d, c, w=c.next, x=y, **qkv_outs(d, c, "next."))
            t = L.BlockTailDesc(1, C.pointer(nxt), None, None, None, 0, 0)
            call(ops, "cr_block_ln_ffn_fwd_tail", C.byref(desc), C.byref(t))
        else:
            t = L.BlockTailDesc(2, None, d.put("lnf_g", c.lnf_g), d.put("lnf_b", c.lnf_b), d.out("out", M, D, ld=D + 5, col=3), D + 5, 3)
            call(ops, "cr_block_ln_ffn_fwd_tail", C.byref(desc), C.byref(t))
        d.intact(what, fails)
        got = B.NS(f_in=d.get("f_in"), hid=d.get("hid"), y=d.get("y"))
        hold(B.items_ffn_fwd(c, FORM, got), what, fails)
        if tail == 1:
            hold(B.items_tail1(c, FORM, got.y, qkv_got(d, c, "next.")), what + " next block", fails)
        if tail == 2:
            hold(B.items_tail2(c, FORM, got.y, d.get("out")), what, fails)
    fails.report("ffn_fwd, tail %d" % tail)


# ------------------------------------------------------------------------------------------------ backward
def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def bwd_desc(d, c, sl, n_slabs, **ptrs):
    """cr_block_bwd_desc: forward buffers f.* and backward pointers by name; the gradient slabs of sl"""
    L = lib()
    f = block_desc(d, c, **{k: v for k, v in ptrs.items() if k in ("x", "q_in", "o", "f_in", "hid", "y")})
    g = lambda n: sl.ptr(n) if n in sl.off else None
    p = lambda n: ptrs.get(n)
    return L.BlockBwdDesc(f, p("dy"), p("d_o"), p("dqkv"), p("dx"), int(ptrs.get("dx_accumulate", 0)), g("g_ln1_g"), g("g_ln1_b"), g("g_wqkv"),
                          g("g_bqkv"), g("g_ln2_g"), g("g_ln2_b"), g("g_w1"), g("g_b1"), g("g_w2"), g("g_b2"), sl.stride, n_slabs,
                          p("attn_delta"), p("dq_part"))


def ffn_shapes(D):
    return dict(g_w2=(D, D), g_b2=(D,), g_w1=(D, D), g_b1=(D,), g_ln2_g=(D,), g_ln2_b=(D,))


def qkv_shapes(D):
    return dict(g_wqkv=(D, 3 * D), g_bqkv=(3 * D,), g_ln1_g=(D,), g_ln1_b=(D,))


def run_ffn_bwd(ops, c, n_slabs, delta, over=None, entry="cr_block_ln_ffn_bwd"):
    M, D = c.M, c.D
    d = Dev(ops, c)
    sl = Slabs(n_slabs, [(n, int(np.prod(s))) for n, s in ffn_shapes(D).items()])
    desc = bwd_desc(d, c, sl, n_slabs, dy=d.put("dy", c.dy), hid=d.put("hid", c.hid), f_in=d.put("f_in", c.f_in), o=d.put("o", c.o),
                    q_in=d.put("q_in", c.q_in), d_o=d.out("d_o", M, D), attn_delta=d.out("attn_delta", 1, M) if delta else None)
    for k, v in (over or {}).items():
        setattr(desc.f if k in ("D", "M") else desc, k, v)
    call(ops, entry, C.byref(desc))
    return d, sl


def test_ffn_bwd(ops):
    fails = Fails()
    for D, M, ns, rate, ro, variant in B.tile_bwd_cases():
        c = B.block_case(D, M, rate, ro)
        delta = bool(variant & 4)
        what = "%s D %d M %d slabs %d rate %.1f row_offset %d attn_delta %d" % (B.kernel_of("ffn_bwd", M, ns), D, M, ns, rate, ro, delta)
        (d, sl), (d2, sl2) = run_ffn_bwd(ops, c, ns, delta), run_ffn_bwd(ops, c, ns, delta)
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, ffn_shapes(D), what, fails)
        got.d_o = d.get("d_o")
        R = B.ffn_bwd_ref(c, FORM, wide(c.dy), wide(c.hid), wide(c.f_in), heads=1, q_in=wide(c.q_in))
        rows = [("d_o", "e_d_o")]
        if delta:
            got.attn_delta = d.get("attn_delta")
            rows.append(("attn_delta", "e_attn_delta"))
        hold(B.items_bwd(R, got, B.FFN_SLABS, rows), what, fails)
        if not (same_bits(sl.whole, sl2.whole) and all(same_bits(d.pads[n].whole, d2.pads[n].whole) for n in d.outs)):
            fails.append(what + ": two launches differ")
    fails.report("ffn_bwd")


def run_qkv_bwd(ops, c, n_slabs, dq_part, acc, sc=None, over=None):
    """sc = (scatter, d_addend) of SCATTER_CASES: dx is NULL and the embedding backward takes the rows"""
    L = lib()
    M, D = c.M, c.D
    d = Dev(ops, c)
    sl = Slabs(n_slabs, [(n, int(np.prod(s))) for n, s in qkv_shapes(D).items()])
    dx = None if sc else d.out("dx", M, D, data=c.dx0 if acc else None)
    desc = bwd_desc(d, c, sl, n_slabs, dqkv=d.put("dqkv", c.dqkv), d_o=d.put("d_o", c.d_o_in), q_in=d.put("q_in", c.q_in), x=d.put("x", c.x),
                    dq_part=d.put("dq_part", c.dq_part) if dq_part else None, dx=dx, dx_accumulate=acc)
    for k, v in (over or {}).items():
        setattr(desc.f if k in ("D", "M") else desc, k, v)
    if sc is None:
        call(ops, "cr_block_ln_qkv_bwd", C.byref(desc))
        return d, sl
    e = c.emb
    f = embed_desc(d, c, e, None)
    zeros = lambda n, r: d.out(n, r, D, data=np.zeros((r, D), np.float32))
    s = L.EmbedBwdDesc(f, zeros("table_grad", e.V), zeros("pos_grad", e.T) if sc[0] == "pos" else None,
                       d.out("d_addend", M, D) if sc[1] else None, 0, sc[2] if len(sc) > 2 else 0, None)
    call(ops, "cr_block_ln_qkv_bwd_scatter", C.byref(desc), C.byref(s))
    return d, sl


def test_qkv_bwd(ops):
    fails = Fails()
    for D, M, ns, rate, ro, variant in B.tile_bwd_cases():
        c = B.block_case(D, M, rate, ro)
        dq_part, acc = bool(variant & 1), bool(variant & 2)
        what = "%s D %d M %d slabs %d dq_part %d dx_accumulate %d" % (B.kernel_of("qkv_bwd", M, ns), D, M, ns, dq_part, acc)
        (d, sl), (d2, sl2) = run_qkv_bwd(ops, c, ns, dq_part, acc), run_qkv_bwd(ops, c, ns, dq_part, acc)
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, qkv_shapes(D), what, fails)
        got.dx = d.get("dx")
        R = B.qkv_bwd_ref(c, FORM, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), c.dq_part if dq_part else None, c.dx0 if acc else None)
        hold(B.items_bwd(R, got, B.QKV_SLABS, [("dx", "e_dx")]), what, fails)
        if not (same_bits(sl.whole, sl2.whole) and same_bits(d.pads["dx"].whole, d2.pads["dx"].whole)):
            fails.append(what + ": two launches differ")
    fails.report("qkv_bwd")


def test_qkv_bwd_scatter(ops):
    fails = Fails()
    for D, M, T, ns, scatter, addend in B.SCATTER_CASES:
        c = B.block_case(D, M, 0.3, 900, False, T)
        what = "%s D %d M %d T %d slabs %d d_addend %d" % (B.kernel_of("qkv_bwd", M, ns, scatter=scatter), D, M, T, ns, addend)
        (d, sl), (d2, sl2) = (run_qkv_bwd(ops, c, ns, False, False, (scatter, addend)) for _ in range(2))
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, qkv_shapes(D), what, fails)
        R = B.qkv_bwd_ref(c, FORM, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in))
        hold(B.items_bwd(R, got, B.QKV_SLABS), what, fails)
        sc = B.scatter_ref(c.emb, R.dx, R.e_dx, scatter == "pos", True, addend)
        hold([(n, d.get(n), v, a) for n, (v, a) in sc.items()], what, fails)
        if not (same_bits(sl.whole, sl2.whole) and (not addend or same_bits(d.pads["d_addend"].whole, d2.pads["d_addend"].whole))):
            fails.append(what + ": two launches differ")
    fails.report("qkv_bwd_scatter")


# ------------------------------------------------------------------------------------------------ what the host refuses
def test_refusals(ops):
    """every refusal comes from the host checks in front of the launch; the message names the entry point and the reason"""
    L = lib()
    c = B.block_case(5, 15, 0.3, 900, False, 5)

    def fwd(entry, D):
        d = Dev(ops, c)
        desc = block_desc(d, c, x=d.put("x", c.x), o=d.put("o", c.o), f_in=d.out("f_in", c.M, c.D), hid=d.out("hid", c.M, c.D),
                          y=d.out("y", c.M, c.D), **qkv_outs(d, c))
        desc.D = D
        if entry.endswith("tail"):
            t = L.BlockTailDesc(2, None, d.put("lnf_g", c.lnf_g), d.put("lnf_b", c.lnf_b), d.out("out", c.M, c.D), c.D, 0)
            return call(ops, entry, C.byref(desc), C.byref(t))
        if entry.endswith("gather"):
            return call(ops, entry, C.byref(desc), C.byref(embed_desc(d, c, c.emb, desc.x)))
        call(ops, entry, C.byref(desc))

    for D in (3, 65):
        for entry in ("cr_block_ln_qkv_fwd", "cr_block_ln_qkv_fwd_gather", "cr_block_ln_ffn_fwd", "cr_block_ln_ffn_fwd_tail"):
            with pytest.raises(RuntimeError, match=r"%s: D=%d outside \[4, 64\]" % (entry, D)):
                fwd(entry, D)
        with pytest.raises(RuntimeError, match=r"cr_block_ln_ffn_bwd: D=%d outside \[4, 64\]" % D):
            run_ffn_bwd(ops, c, 2, True, over=dict(D=D))
        with pytest.raises(RuntimeError, match=r"cr_block_ln_qkv_bwd: D=%d outside \[4, 64\]" % D):
            run_qkv_bwd(ops, c, 2, True, False, over=dict(D=D))
        with pytest.raises(RuntimeError, match=r"cr_block_ln_qkv_bwd_scatter: D=%d outside \[4, 64\]" % D):
            run_qkv_bwd(ops, c, 2, False, False, ("pos", True), over=dict(D=D))
    with pytest.raises(RuntimeError, match=r"cr_block_ln_qkv_bwd_scatter: dx_accumulate is not supported"):
        run_qkv_bwd(ops, c, 2, False, False, ("pos", True), over=dict(dx_accumulate=1))
    with pytest.raises(RuntimeError, match=r"cr_block_ln_qkv_bwd_scatter: small-table mode is not fused"):
        run_qkv_bwd(ops, c, 2, False, False, ("pos", True, 2))
    with pytest.raises(RuntimeError, match=r"cr_block_ln_ffn_bwd: NULL gradient pointer"):
        run_ffn_bwd(ops, c, 2, True, over=dict(n_slabs=0))
    torch.cuda.synchronize()


def test_refusals_leave_outputs(ops):
    """the same refusals with the buffers kept: every output word still holds its sentinel, the zeroed scatter targets their zeros"""
    L = lib()
    c = B.block_case(5, 15, 0.3, 900, False, 5)
    M, D = c.M, c.D
    for bad in (3, 65):
        d = Dev(ops, c)
        sl = Slabs(2, [(n, int(np.prod(s))) for n, s in {**ffn_shapes(D), **qkv_shapes(D)}.items()])
        desc = bwd_desc(d, c, sl, 2, dy=d.put("dy", c.dy), hid=d.put("hid", c.hid), f_in=d.put("f_in", c.f_in), o=d.put("o", c.o),
                        q_in=d.put("q_in", c.q_in), x=d.put("x", c.x), dqkv=d.put("dqkv", c.dqkv), d_o=d.out("d_o", M, D),
                        attn_delta=d.out("attn_delta", 1, M), dx=d.out("dx", M, D))
        desc.f.D = bad
        fdesc = block_desc(d, c, x=d.put("x2", c.x), o=d.put("o2", c.o), f_in=d.out("f_in2", M, D), hid=d.out("hid2", M, D), y=d.out("y", M, D),
                           **qkv_outs(d, c))
        fdesc.D = bad
        stream = torch.cuda.current_stream().cuda_stream
        assert L.lib.cr_block_ln_ffn_bwd(C.byref(desc), stream) != 0 and b"outside [4, 64]" in L.lib.cr_last_error()
        assert L.lib.cr_block_ln_qkv_bwd(C.byref(desc), stream) != 0 and b"cr_block_ln_qkv_bwd: D=" in L.lib.cr_last_error()
        assert L.lib.cr_block_ln_qkv_fwd(C.byref(fdesc), stream) != 0 and b"cr_block_ln_qkv_fwd: D=" in L.lib.cr_last_error()
        assert L.lib.cr_block_ln_ffn_fwd(C.byref(fdesc), stream) != 0 and b"cr_block_ln_ffn_fwd: D=" in L.lib.cr_last_error()
        torch.cuda.synchronize()
        assert d.all_sentinel() and sl.all_sentinel()
    # the scatter form: dx_accumulate = 1 and the small-table mode
    for over, n_slabs_sc, msg in ((dict(dx_accumulate=1), 0, b"dx_accumulate is not supported"), ({}, 2, b"small-table mode is not fused")):
        d = Dev(ops, c)
        sl = Slabs(2, [(n, int(np.prod(s))) for n, s in qkv_shapes(D).items()])
        desc = bwd_desc(d, c, sl, 2, dqkv=d.put("dqkv", c.dqkv), d_o=d.put("d_o", c.d_o_in), q_in=d.put("q_in", c.q_in), x=d.put("x", c.x), **over)
        f = embed_desc(d, c, c.emb, None)
        zeros = lambda n, r: d.out(n, r, D, data=np.zeros((r, D), np.float32))
        s = L.EmbedBwdDesc(f, zeros("table_grad", c.emb.V), zeros("pos_grad", c.emb.T), d.out("d_addend", M, D), 0, n_slabs_sc, None)
        assert L.lib.cr_block_ln_qkv_bwd_scatter(C.byref(desc), C.byref(s), torch.cuda.current_stream().cuda_stream) != 0
        assert msg in L.lib.cr_last_error()
        torch.cuda.synchronize()
        assert sl.all_sentinel() and d.all_sentinel(["d_addend"]) and (d.get("table_grad") == 0).all() and (d.get("pos_grad") == 0).all()
        assert d.pads["table_grad"].untouched() and d.pads["pos_grad"].untouched()


# ================================================================================================ register-layout backward
# csrc/cr_stack_bwd.hip (cr_rbwd.hpp): k_stack_ffn_bwd / k_stack_qkv_bwd<SPLIT, DS>, DS = 50, 64 or 0 (any other D); one workgroup per
# (sequence, round of seven 16-row tiles), dealt to the n_slabs workgroups in turn.  [x3 | bf16] = CR_PREC_BF16X3 | CR_PREC_BF16.
FORMS = pytest.mark.parametrize("form", ["x3", "bf16"])


def ln_bwd_desc(d, c, sl, n_slabs, y):
    """the cr_layernorm_bwd call of the stack's final LayerNorm: x = this block's y, dy at a pitch of D + 3, slabs of the block"""
    L = lib()
    M, D = c.M, c.D
    d.pads["lnf_dy"] = Pad(M, D + 3, [(0, D)], c.dy, lead=1)
    return L.LnBwdDesc(y, D, d.put("lnf_g", c.lnf_g), d.pads["lnf_dy"].t.data_ptr(), D + 3, None, 0, 0, sl.ptr("lnf_dgamma"), sl.ptr("lnf_dbeta"),
                       sl.stride, n_slabs, M, D, 1e-8)


def run_reg_ffn(ops, c, Bn, T, n_slabs, form, variant, heads, delta, over=None, prec=None):
    L = lib()
    M, D = c.M, c.D
    d = Dev(ops, c)
    shapes = dict(ffn_shapes(D), lnf_dgamma=(D,), lnf_dbeta=(D,)) if variant in (1, 3) else ffn_shapes(D)
    sl = Slabs(n_slabs, [(n, int(np.prod(s))) for n, s in shapes.items()])
    ln = variant in (1, 3)
    y = d.put("y", c.y) if ln else None
    desc = bwd_desc(d, c, sl, n_slabs, dy=None if ln else d.put("dy", c.dy), hid=d.put("hid", c.hid), f_in=d.put("f_in", c.f_in),
                    o=d.put("o", c.o), q_in=d.put("q_in", c.q_in), y=y, d_o=d.out("d_o", M, D),
                    attn_delta=d.out("attn_delta", heads, M) if delta else None)
    n = ln_bwd_desc(d, c, sl, n_slabs, y) if ln else None
    for k, v in (over or {}).items():
        setattr(desc.f if k in ("D", "M") else desc, k, v)
    prec = B.PREC_OF[form] if prec is None else prec
    if variant == 0:
        call(ops, "cr_stack_ffn_bwd", C.byref(desc), Bn, T, prec)
    elif variant == 1:
        call(ops, "cr_stack_ffn_bwd_ln", C.byref(desc), C.byref(n), Bn, T, prec)
    else:
        call(ops, "cr_stack_ffn_bwd_heads", C.byref(desc), C.byref(n) if ln else None, Bn, T, heads, prec)
    return d, sl, shapes


@FORMS
def test_reg_ffn_bwd(ops, form):
    """cr_stack_ffn_bwd, _ln, _heads (two heads at D = 64): D x T x B x n_slabs of reg_cases"""
    fails = Fails()
    for D, Bn, T, ns, rate, ro, variant in B.reg_cases():
        c = B.block_case(D, Bn * T, rate, ro)
        heads = 2 if (D == 64 and variant >= 2) else 1
        delta = variant > 0 or ns % 2 == 0
        what = "%s variant %d D %d B %d T %d slabs %d rate %.1f heads %d" % (B.reg_kernel_of("ffn", D, form), variant, D, Bn, T, ns, rate, heads)
        (d, sl, shapes), (d2, sl2, _) = (run_reg_ffn(ops, c, Bn, T, ns, form, variant, heads, delta) for _ in range(2))
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, shapes, what, fails, empty=B.reg_empty_slabs(Bn, T, ns))
        got.d_o = d.get("d_o")
        lnf = (wide(c.y), c.lnf_g) if variant in (1, 3) else None
        R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=heads, q_in=wide(c.q_in), lnf=lnf)
        rows = [("d_o", "e_d_o")]
        if delta:
            got.attn_delta = d.get("attn_delta")
            rows.append(("attn_delta", "e_attn_delta"))
        hold(B.items_bwd(R, got, tuple(shapes), rows), what, fails)
        if not (same_bits(sl.whole, sl2.whole) and all(same_bits(d.pads[n].whole, d2.pads[n].whole) for n in d.outs)):
            fails.append(what + ": two launches differ")
    fails.report("register-layout ffn_bwd, %s" % form)


def run_reg_qkv(ops, c, Bn, T, n_slabs, form, acc, sc=None, over=None, prec=None, dq_part=False):
    L = lib()
    M, D = c.M, c.D
    d = Dev(ops, c)
    sl = Slabs(n_slabs, [(n, int(np.prod(s))) for n, s in qkv_shapes(D).items()])
    dx = None if sc else d.out("dx", M, D, data=c.dx0 if acc else None)
    desc = bwd_desc(d, c, sl, n_slabs, dqkv=d.put("dqkv", c.dqkv), d_o=d.put("d_o", c.d_o_in), q_in=d.put("q_in", c.q_in), x=d.put("x", c.x),
                    dx=dx, dx_accumulate=acc, dq_part=d.put("dq_part", c.dq_part) if dq_part else None)
    for k, v in (over or {}).items():
        setattr(desc.f if k in ("D", "M") else desc, k, v)
    prec = B.PREC_OF[form] if prec is None else prec
    if sc is None:
        call(ops, "cr_stack_qkv_bwd", C.byref(desc), Bn, T, prec)
        return d, sl
    e = c.emb
    f = embed_desc(d, c, e, None)
    zeros = lambda n, r: d.out(n, r, D, data=np.zeros((r, D), np.float32))
    s = L.EmbedBwdDesc(f, zeros("table_grad", e.V), zeros("pos_grad", e.T) if sc[0] == "pos" else None,
                       d.out("d_addend", M, D) if sc[1] else None, 0, 0, None)
    call(ops, "cr_stack_qkv_bwd_scatter", C.byref(desc), C.byref(s), Bn, T, prec)
    return d, sl


@FORMS
def test_reg_qkv_bwd(ops, form):
    fails = Fails()
    for D, Bn, T, ns, rate, ro, variant in B.reg_cases():
        c = B.block_case(D, Bn * T, rate, ro)
        acc = bool(variant & 1)
        what = "%s D %d B %d T %d slabs %d dx_accumulate %d" % (B.reg_kernel_of("qkv", D, form), D, Bn, T, ns, acc)
        (d, sl), (d2, sl2) = (run_reg_qkv(ops, c, Bn, T, ns, form, acc) for _ in range(2))
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, qkv_shapes(D), what, fails, empty=B.reg_empty_slabs(Bn, T, ns))
        got.dx = d.get("dx")
        R = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), None, c.dx0 if acc else None)
        hold(B.items_bwd(R, got, B.QKV_SLABS, [("dx", "e_dx")]), what, fails)
        if not (same_bits(sl.whole, sl2.whole) and same_bits(d.pads["dx"].whole, d2.pads["dx"].whole)):
            fails.append(what + ": two launches differ")
    fails.report("register-layout qkv_bwd, %s" % form)


@FORMS
def test_reg_qkv_bwd_scatter(ops, form):
    fails = Fails()
    for D, Bn, T, ns, scatter, addend in B.REG_SCATTER:
        c = B.block_case(D, Bn * T, 0.3, 900, False, T)
        what = "%s scatter %s D %d B %d T %d slabs %d d_addend %d" % (B.reg_kernel_of("qkv", D, form), scatter, D, Bn, T, ns, addend)
        (d, sl), (d2, sl2) = (run_reg_qkv(ops, c, Bn, T, ns, form, False, (scatter, addend)) for _ in range(2))
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, qkv_shapes(D), what, fails, empty=B.reg_empty_slabs(Bn, T, ns))
        R = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in))
        hold(B.items_bwd(R, got, B.QKV_SLABS), what, fails)
        sc = B.scatter_ref(c.emb, R.dx, R.e_dx, scatter == "pos", True, addend)
        hold([(n, d.get(n), v, a) for n, (v, a) in sc.items()], what, fails)
        if not (same_bits(sl.whole, sl2.whole) and (not addend or same_bits(d.pads["d_addend"].whole, d2.pads["d_addend"].whole))):
            fails.append(what + ": two launches differ")
    fails.report("register-layout qkv_bwd_scatter, %s" % form)


def test_reg_refusals(ops):
    """cr_stack_bwd_supported's reasons, the heads rule, dq_part and a scatter with dx_accumulate: refused in front of the launch, the
    outputs still all sentinel"""
    c = B.block_case(64, 48, 0.3, 900, False, 16)
    c8 = B.block_case(8, 48, 0.3, 900, False, 16)

    def ffn(cc=c, Bn=3, T=16, heads=1, variant=2, prec=None, **over):
        run_reg_ffn(ops, cc, Bn, T, 2, "x3", variant, heads, True, over=over, prec=prec)

    def qkv(cc=c, Bn=3, T=16, prec=None, sc=None, acc=False, dq_part=False, **over):
        run_reg_qkv(ops, cc, Bn, T, 2, "x3", acc, sc, over=over, prec=prec, dq_part=dq_part)

    for fn, kw, msg in [(ffn, dict(D=7), r"cr_stack_ffn_bwd_heads: unsupported \(hidden size 8\.\.64\)"),
                        (ffn, dict(D=65), r"cr_stack_ffn_bwd_heads: unsupported \(hidden size 8\.\.64\)"),
                        (qkv, dict(D=7), r"cr_stack_qkv_bwd: unsupported \(hidden size 8\.\.64\)"),
                        (qkv, dict(D=65), r"cr_stack_qkv_bwd: unsupported \(hidden size 8\.\.64\)"),
                        (ffn, dict(variant=0, Bn=1, T=225, M=225), r"cr_stack_ffn_bwd: unsupported \(T <= 224"),
                        (qkv, dict(Bn=1, T=225, M=225), r"cr_stack_qkv_bwd: unsupported \(T <= 224"),
                        (ffn, dict(variant=1, Bn=2, T=16), r"cr_stack_ffn_bwd_ln: unsupported \(M = B T\)"),
                        (qkv, dict(Bn=3, T=17), r"cr_stack_qkv_bwd: unsupported \(M = B T\)"),
                        (ffn, dict(prec=0), r"cr_stack_ffn_bwd_heads: unsupported \(bf16 arithmetic"),
                        (qkv, dict(prec=0), r"cr_stack_qkv_bwd: unsupported \(bf16 arithmetic"),
                        (ffn, dict(cc=c8, heads=2), r"cr_stack_ffn_bwd_heads: attn_delta per head is formed for one head, or two heads at D = 64"),
                        (ffn, dict(heads=4), r"cr_stack_ffn_bwd_heads: attn_delta per head"),
                        (qkv, dict(dq_part=True), r"cr_stack_qkv_bwd: dq_part .* is not taken"),
                        (qkv, dict(sc=("pos", True), dx_accumulate=1), r"cr_stack_qkv_bwd_scatter: dx_accumulate with a scatter")]:
        with pytest.raises(RuntimeError, match=msg):
            fn(**kw)
    torch.cuda.synchronize()
    # the same with the buffers kept
    L = lib()
    M, D = c.M, c.D
    d = Dev(ops, c)
    sl = Slabs(2, [(n, int(np.prod(s))) for n, s in {**ffn_shapes(D), **qkv_shapes(D)}.items()])
    desc = bwd_desc(d, c, sl, 2, dy=d.put("dy", c.dy), hid=d.put("hid", c.hid), f_in=d.put("f_in", c.f_in), o=d.put("o", c.o),
                    q_in=d.put("q_in", c.q_in), x=d.put("x", c.x), dqkv=d.put("dqkv", c.dqkv), d_o=d.out("d_o", M, D),
                    attn_delta=d.out("attn_delta", 2, M), dx=d.out("dx", M, D))
    stream = torch.cuda.current_stream().cuda_stream
    for Bn, T, prec, heads in ((3, 16, 0, 1), (1, 225, 1, 1), (2, 16, 2, 1), (3, 16, 1, 4)):
        assert L.lib.cr_stack_ffn_bwd_heads(C.byref(desc), None, Bn, T, heads, prec, stream) != 0
        if heads == 1:
            assert L.lib.cr_stack_qkv_bwd(C.byref(desc), Bn, T, prec, stream) != 0
            assert L.lib.cr_stack_bwd_supported(C.byref(desc), Bn, T, prec) == 0
    assert L.lib.cr_stack_bwd_supported(C.byref(desc), 3, 16, 1) == 1
    torch.cuda.synchronize()
    assert d.all_sentinel() and sl.all_sentinel()


# ================================================================================================ the wide family
# csrc/cr_wide.hip: D = 128 / 192 / 256, bf16x3 / bf16; k_wide_qkv_fwd, k_wide_ffn_fwd<NCT, SPLIT, MODE(, TAIL)>, k_wide_ffn_bwd,
# k_wide_qkv_bwd<NCT, SPLIT, WG> (block_rows_ref.wide_kernel_of)
def run_wide_fwd(ops, c, form, tail=0, col_out=4, what=None):
    L = lib()
    M, D = c.M, c.D
    prec = B.PREC_OF[form]
    d = Dev(ops, c)
    y = d.out("y", M, D)
    desc = block_desc(d, c, x=d.put("x", c.x), o=d.put("o", c.o), f_in=d.out("f_in", M, D), hid=d.out("hid", M, D), y=y, **qkv_outs(d, c))
    if tail == 0:
        call(ops, "cr_wide_ln_qkv_fwd", C.byref(desc), prec)
        call(ops, "cr_wide_ln_ffn_fwd", C.byref(desc), prec)
    elif tail == 1:
        nxt = block_desc(d, c, w=c.next, x=y, **qkv_outs(d, c, "next."))
        d.keep = [nxt]
        call(ops, "cr_wide_ln_ffn_fwd_tail", C.byref(desc), C.byref(L.BlockTailDesc(1, C.pointer(nxt), None, None, None, 0, 0)), prec)
    else:
        t = L.BlockTailDesc(2, None, d.put("lnf_g", c.lnf_g), d.put("lnf_b", c.lnf_b), d.out("out", M, D, ld=D + 8, col=col_out), D + 8, col_out)
        call(ops, "cr_wide_ln_ffn_fwd_tail", C.byref(desc), C.byref(t), prec)
    return d


@FORMS
def test_wide_fwd(ops, form):
    """cr_wide_ln_qkv_fwd and cr_wide_ln_ffn_fwd: D x M of wide_fwd_cases; 64 and 128 rows per workgroup"""
    fails = Fails()
    for key in B.wide_fwd_cases():
        c = B.block_case(*key)
        what = "%s / %s D %d M %d rate %.1f row_offset %d" % ((B.wide_kernel_of("qkv_fwd", c.D, form, c.M), B.wide_kernel_of("ffn_fwd", c.D, form, c.M)) + key)
        d = run_wide_fwd(ops, c, form)
        d.intact(what, fails)
        hold(B.items_qkv_fwd(c, form, qkv_got(d, c)), what, fails)
        hold(B.items_ffn_fwd(c, form, B.NS(f_in=d.get("f_in"), hid=d.get("hid"), y=d.get("y"))), what, fails)
    fails.report("wide forward, %s" % form)


@FORMS
@pytest.mark.parametrize("tail", [1, 2])
def test_wide_fwd_tail(ops, form, tail):
    fails = Fails()
    for M, rate, ro in ((1, 0.0, 0), (65, 0.3, 900), (129, 0.3, 0), (300, 0.0, 0)):
        c = B.block_case(128, M, rate, ro)
        what = "%s M %d rate %.1f" % (B.wide_kernel_of("ffn_fwd", 128, form, M, tail=tail), M, rate)
        d = run_wide_fwd(ops, c, form, tail)
        d.outs = [n for n in d.outs if n not in ("q_in", "qkv", "k_valid", "q_valid")]         # this block's own projections are not run here
        d.intact(what, fails)
        got = B.NS(f_in=d.get("f_in"), hid=d.get("hid"), y=d.get("y"))
        hold(B.items_ffn_fwd(c, form, got), what, fails)
        if tail == 1:
            hold(B.items_tail1(c, form, got.y, qkv_got(d, c, "next.")), what + " next block", fails)
        else:
            hold(B.items_tail2(c, form, got.y, d.get("out")), what, fails)
    fails.report("wide ffn_fwd tail %d, %s" % (tail, form))


@FORMS
def test_wide_fwd_8_waves_above_128(ops, form):
    """M = 32641 at D = 192: ceil(M / 128) = 256 row blocks, the 8-wave forward form of both entries; the first, the last and three
    interior row blocks are held to the reference, every row must be written"""
    fails = Fails()
    c, idx = B.wide_big()
    assert B.wide_kernel_of("qkv_fwd", c.D, form, c.M).endswith(", 0>") and B.wide_kernel_of("qkv_fwd", c.D, form, 300).endswith(", 2>")
    what = "%s M %d" % (B.wide_kernel_of("qkv_fwd", c.D, form, c.M), c.M)
    d = run_wide_fwd(ops, c, form)
    d.intact(what, fails)
    s = B.sub_case(c, idx)
    q = qkv_got(d, c)
    hold(B.items_qkv_fwd(s, form, B.NS(q_in=q.q_in[idx], qkv=q.qkv[:, idx], k_valid=q.k_valid[idx], q_valid=q.q_valid[idx])), what, fails)
    hold(B.items_ffn_fwd(s, form, B.NS(f_in=d.get("f_in")[idx], hid=d.get("hid")[idx], y=d.get("y")[idx])), what, fails)
    fails.report("wide forward, 8 waves at D = 192, %s" % form)


def run_wide_bwd(ops, c, n_slabs, form, own, heads, acc, over=None, prec=None, dq_part=False):
    """both backward entries on one Dev: NS(d, sl, shapes)"""
    M, D = c.M, c.D
    d = Dev(ops, c)
    shapes = {**ffn_shapes(D), **qkv_shapes(D)} if own else dict(g_ln2_g=(D,), g_ln2_b=(D,), g_ln1_g=(D,), g_ln1_b=(D,))
    sl = Slabs(n_slabs, [(n, int(np.prod(s))) for n, s in shapes.items()])
    desc = bwd_desc(d, c, sl, n_slabs, dy=d.put("dy", c.dy), hid=d.put("hid", c.hid), f_in=d.put("f_in", c.f_in), o=d.put("o", c.o),
                    q_in=d.put("q_in", c.q_in), x=d.put("x", c.x), d_o=d.out("d_o", M, D),
                    attn_delta=d.out("attn_delta", heads, M) if heads else None)
    g2, g1 = d.out("g2", M, D), d.out("g1", M, D)
    for k, v in (over or {}).items():
        setattr(desc.f if k in ("D", "M") else desc, k, v)
    prec = B.PREC_OF[form] if prec is None else prec
    call(ops, "cr_wide_ln_ffn_bwd", C.byref(desc), g2, g1, heads, prec)
    # the projection backward on buffers of its own: d_o is an input here (and, without own weight gradients, overwritten)
    desc.d_o, desc.dqkv, desc.dx, desc.dx_accumulate = d.put("d_o_in", c.d_o_in), d.put("dqkv", c.dqkv), d.out("dx", M, D, data=c.dx0 if acc else None), int(acc)
    if dq_part:
        desc.dq_part = d.put("dq_part", c.dq_part)
    call(ops, "cr_wide_ln_qkv_bwd", C.byref(desc), prec)
    return d, sl, shapes


@FORMS
def test_wide_bwd(ops, form):
    """cr_wide_ln_ffn_bwd and cr_wide_ln_qkv_bwd: with their own weight gradients (D = 128) and with NULL weight-gradient pointers
    (g2, g1 returned, d_o overwritten with dQ Wq^T + d_o); heads 0 / 1 / 2 / 4 / 8; dx written or accumulated"""
    fails = Fails()
    for D, M, ns, rate, ro, own, heads, acc in B.wide_bwd_cases():
        c = B.block_case(D, M, rate, ro)
        what = "%s / %s D %d M %d slabs %d rate %.1f heads %d dx_accumulate %d" % (
            B.wide_kernel_of("ffn_bwd", D, form, own=own), B.wide_kernel_of("qkv_bwd", D, form, own=own), D, M, ns, rate, heads, acc)
        (d, sl, shapes), (d2, sl2, _) = (run_wide_bwd(ops, c, ns, form, own, heads, acc) for _ in range(2))
        if own:
            d.outs = [n for n in d.outs if n not in ("g2", "g1")]          # not written when the kernel forms the weight gradients itself
        d.intact(what, fails)
        got = slabs_of(sl, c, ns, shapes, what, fails, empty=B.wide_empty_slabs(D, M, ns))
        got.d_o, got.dx = d.get("d_o"), d.get("dx")
        R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=heads, q_in=wide(c.q_in))
        rows = [("d_o", "e_d_o")]
        if heads:
            got.attn_delta = d.get("attn_delta")
            rows.append(("attn_delta", "e_attn_delta"))
        if not own:
            got.g2, got.g1 = d.get("g2"), d.get("g1")
            rows += [("g2", "e_g2"), ("g1", "e_g1")]
        hold(B.items_bwd(R, got, tuple(n for n in B.FFN_SLABS if n in shapes), rows), what, fails)
        Q = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in), None, c.dx0 if acc else None)
        rows = [("dx", "e_dx")]
        if not own:
            got.dq_in = d.get("d_o_in")
            rows.append(("dq_in", "e_dq_in"))
        elif not np.array_equal(d.get("d_o_in"), c.d_o_in):
            fails.append(what + ": d_o was written although the kernel formed the weight gradients itself")
        hold(B.items_bwd(Q, got, tuple(n for n in B.QKV_SLABS if n in shapes), rows), what, fails)
        if own and not (d.all_sentinel(["g2", "g1"])):
            fails.append(what + ": g2 / g1 were written")
        if not (same_bits(sl.whole, sl2.whole) and all(same_bits(d.pads[n].whole, d2.pads[n].whole) for n in d.outs)):
            fails.append(what + ": two launches differ")
    fails.report("wide backward, %s" % form)


def test_wide_refusals(ops):
    L = lib()
    c = B.block_case(128, 65, 0.3, 900)
    M, D = c.M, c.D
    stream = torch.cuda.current_stream().cuda_stream

    def fwd(entry, tail=None, **over):
        d = Dev(ops, c)
        desc = block_desc(d, c, x=d.put("x", c.x), o=d.put("o", c.o), f_in=d.out("f_in", M, D), hid=d.out("hid", M, D), y=d.out("y", M, D), **qkv_outs(d, c))
        for k, v in over.items():
            setattr(desc, k, v)
        if tail is None:
            rc = getattr(L.lib, entry)(C.byref(desc), 1, stream)
        else:
            t = L.BlockTailDesc(2, None, d.put("lnf_g", c.lnf_g), d.put("lnf_b", c.lnf_b), d.out("out", M, D, ld=D + 8, col=tail), D + 8, tail)
            rc = L.lib.cr_wide_ln_ffn_fwd_tail(C.byref(desc), C.byref(t), 1, stream)
        msg = L.lib.cr_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and d.all_sentinel(), (entry, over, msg)
        return msg

    for D_bad in (64, 160):
        for entry in ("cr_wide_ln_qkv_fwd", "cr_wide_ln_ffn_fwd"):
            assert fwd(entry, D=D_bad) == entry + ": D must be 128, 192 or 256"
        assert fwd(None, tail=4, D=D_bad) == "cr_wide_ln_ffn_fwd_tail: D must be 128, 192 or 256"
    assert fwd(None, tail=4, D=192) == "cr_wide_ln_ffn_fwd_tail: the tails are taken at D = 128 only"
    assert fwd(None, tail=3) == "cr_wide_ln_ffn_fwd_tail: bad final-LayerNorm tail"

    def bwd(match, own=True, heads=2, dq_part=False, **over):
        with pytest.raises(RuntimeError, match=match):
            run_wide_bwd(ops, c, 2, "x3", own, heads, False, over=over, dq_part=dq_part)

    bwd(r"cr_wide_ln_ffn_bwd: D must be 128, 192 or 256", D=64)
    bwd(r"cr_wide_ln_ffn_bwd: D must be 128, 192 or 256", D=160)
    bwd(r"cr_wide_ln_ffn_bwd: weight gradients are formed at D = 128 only", D=192)
    bwd(r"cr_wide_ln_ffn_bwd: attn_delta needs heads whose width is a multiple of 16 columns", heads=16)
    bwd(r"cr_wide_ln_ffn_bwd: attn_delta needs heads whose width is a multiple of 16 columns", heads=3)
    bwd(r"cr_wide_ln_qkv_bwd: dq_part .* is not taken", dq_part=True)
    # the projection backward alone: D = 64, 160, and weight-gradient pointers at D = 192; outputs kept
    d = Dev(ops, c)
    sl = Slabs(2, [(n, int(np.prod(s))) for n, s in qkv_shapes(D).items()])
    desc = bwd_desc(d, c, sl, 2, q_in=d.put("q_in", c.q_in), x=d.put("x", c.x), d_o=d.out("d_o", M, D), dqkv=d.put("dqkv", c.dqkv), dx=d.out("dx", M, D))
    for D_bad, msg in ((64, b"D must be 128, 192 or 256"), (160, b"D must be 128, 192 or 256"), (192, b"weight gradients are formed at D = 128 only")):
        desc.f.D = D_bad
        assert L.lib.cr_wide_ln_qkv_bwd(C.byref(desc), 1, stream) != 0 and msg in L.lib.cr_last_error()
    torch.cuda.synchronize()
    assert d.all_sentinel() and sl.all_sentinel()


# ================================================================================================ one reference for every form
def test_forms_share_one_reference(ops):
    """castrec.h: the register-layout backward "equals" the tile kernels, the fused forms equal their separate calls.  Where two forms
    compute the same thing from the same inputs, each is held to its own bound of the SAME fp64 reference (never kernel against kernel):
    the tile backward and the register-layout backward in both precisions; the gathering forward and cr_embed_fwd + cr_block_ln_qkv_fwd;
    tail 1 and cr_block_ln_ffn_fwd + the next block's cr_block_ln_qkv_fwd"""
    fails = Fails()
    for D, Bn, T in ((50, 3, 17), (64, 1, 113), (9, 3, 16)):
        c = B.block_case(D, Bn * T, 0.3, 900)
        refs = {}
        for form in ("f32", "x3", "bf16"):
            what = "D %d B %d T %d, %s" % (D, Bn, T, form)
            if form == "f32":
                d, sl = run_ffn_bwd(ops, c, 2, True)
                q, ql = run_qkv_bwd(ops, c, 2, False, False)
                empty = None
            else:
                d, sl, _ = run_reg_ffn(ops, c, Bn, T, 2, form, 0, 1, True)
                q, ql = run_reg_qkv(ops, c, Bn, T, 2, form, False)
                empty = B.reg_empty_slabs(Bn, T, 2)
            got = slabs_of(sl, c, 2, ffn_shapes(D), what, fails, empty=empty)
            got.d_o, got.attn_delta = d.get("d_o"), d.get("attn_delta")
            R = B.ffn_bwd_ref(c, form, wide(c.dy), wide(c.hid), wide(c.f_in), heads=1, q_in=wide(c.q_in))
            hold(B.items_bwd(R, got, B.FFN_SLABS, [("d_o", "e_d_o"), ("attn_delta", "e_attn_delta")]), what, fails)
            got = slabs_of(ql, c, 2, qkv_shapes(D), what, fails, empty=empty)
            got.dx = q.get("dx")
            Q = B.qkv_bwd_ref(c, form, wide(c.dqkv), wide(c.d_o_in), wide(c.q_in))
            hold(B.items_bwd(Q, got, B.QKV_SLABS, [("dx", "e_dx")]), what, fails)
            refs[form] = (R.d_o, R.g_w1, Q.dx, Q.g_wqkv)
        assert all(np.array_equal(a, b) for f in ("x3", "bf16") for a, b in zip(refs["f32"], refs[f]))       # one reference, three allowances
    # the gathering forward against the two separate calls
    for key in B.GATHER_CASES[:3]:
        c = B.gather_case(*key)
        e = c.emb
        d = Dev(ops, c)
        x = d.out("x", c.M, c.D)
        ed = embed_desc(d, c, e, x)
        call(ops, "cr_embed_fwd", C.byref(ed))
        desc = block_desc(d, c, x=x, **qkv_outs(d, c))
        call(ops, "cr_block_ln_qkv_fwd", C.byref(desc))
        what = "cr_embed_fwd + cr_block_ln_qkv_fwd D %d M %d" % (c.D, c.M)
        d.intact(what, fails)
        hold([("x composed", d.get("x"), c.x_ref, c.e_x)], what, fails)
        hold(B.items_qkv_fwd(c, FORM, qkv_got(d, c), x_got=d.get("x"), x=c.x_ref, e_x=c.e_x), what, fails)
    # tail 1 against cr_block_ln_ffn_fwd followed by the next block's cr_block_ln_qkv_fwd
    for key in B.tile_fwd_cases()[:6]:
        c = B.block_case(*key)
        d = Dev(ops, c)
        y = d.out("y", c.M, c.D)
        desc = block_desc(d, c, o=d.put("o", c.o), f_in=d.out("f_in", c.M, c.D), hid=d.out("hid", c.M, c.D), y=y)
        call(ops, "cr_block_ln_ffn_fwd", C.byref(desc))
        nxt = block_desc(d, c, w=c.next, x=y, **qkv_outs(d, c, "next."))
        call(ops, "cr_block_ln_qkv_fwd", C.byref(nxt))
        what = "cr_block_ln_ffn_fwd + cr_block_ln_qkv_fwd D %d M %d" % (c.D, c.M)
        d.intact(what, fails)
        hold(B.items_tail1(c, FORM, d.get("y"), qkv_got(d, c, "next.")), what, fails)
    fails.report("forms against one reference")

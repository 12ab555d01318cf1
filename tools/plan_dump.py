"""Canonical text of an engine's launch plan, and the case list that compares two checkouts of the planner.

The planner (engine.py, op_embed .. _finalize) compiles a model into flat launch lists.  For the same constructor arguments and
environment two versions of it must produce the same lists: `canonical(eng)` prints everything a step would hand to the C ABI --
every entry, every descriptor field, every pointer as <allocation name>+<byte offset> -- without launching anything.

    python tools/plan_dump.py --out branch.sha [--full branch.txt.gz]                   # this checkout
    python tools/plan_dump.py --tree ../parent --out parent.sha [--full parent.txt.gz]  # another checkout's engine.py
        (--out: one line per case, case id and sha256 of its text; --groups FILE: those lines folded, one line per group of cases)
    python tools/plan_dump.py --diff parent.txt.gz branch.txt.gz                        # the cases that differ, as unified diffs
    python tools/plan_dump.py [--tree DIR] --switch-check                               # tests' switch check on that planner

--tree puts another checkout's root first on sys.path; with CASTREC_LIB pointing at this checkout's built library (same C
sources) no second build is needed.  Constructing an Engine allocates on the device, so all of this needs the GPU.
Only what every version of the engine has is read: fwd, bwd, _l2, _adam, _adam_flat, _reduce, _tgrad, public attributes, _bufs."""
import argparse
import contextlib
import ctypes as C
import difflib
import gc
import gzip
import hashlib
import itertools
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the engine's tensors a launch argument may point into, in lookup order (a view -- lazy_ids over batch_buf -- resolves to the
# allocation listed first); the activation buffers of eng._bufs come before them
ENGINE_TENSORS = ("P", "Mom", "Vel", "Gflat", "Gs", "state", "batch_buf", "static_pe", "_ce_ws", "samples", "item_cdf", "item_logq",
                  "lazy_flags", "lazy_ids", "slab_counts", "_tg_part", "_tg_tickets", "attn_weights")
LISTS = ("fwd", "bwd", "_l2", "_adam", "_adam_flat", "_reduce", "_tgrad")
# every environment switch the engine reads, with the value the cases set it to
SWITCHES = {"CASTREC_TWO_PASS_ATTN_BWD": "1", "CASTREC_NO_TAILS": "1", "CASTREC_NO_EMBED_FUSION": "1", "CASTREC_NO_STACK_KERNEL": "1",
            "CASTREC_NO_STACK_BWD": "1", "CASTREC_NO_WIDE": "1", "CASTREC_NO_BLOCK_BWD": "1", "CASTREC_NO_HEAD_LN": "1",
            "CASTREC_NO_ID_CHECK": "1", "CASTREC_NO_HEAD_FUSION": "1", "CASTREC_WSLABS": "2", "CASTREC_NO_INDEX": "1",
            "CASTREC_WIDE_NO_WGRAD": "1", "CASTREC_WIDE_NO_DELTA": "1", "CASTREC_BF_TWO_KERNELS": "1", "CASTREC_NO_HEAD_DELTA": "1",
            "CASTREC_WIDE_NO_TAILS": "1", "CASTREC_NO_LNF_FUSION": "1", "CASTREC_STACK_PAIR_MAX_B": "2", "CASTREC_LAZY_ADAM": "1",
            "CASTREC_ATTN_PRECISION": "bf16"}
# ... of which CASTREC_NO_ID_CHECK is no planner switch: it turns off set_batch()'s range check of host ids
PLANNER_SWITCHES = [s for s in SWITCHES if s != "CASTREC_NO_ID_CHECK"]


class PlanError(RuntimeError):
    pass


@contextlib.contextmanager
def environment(env):
    """The CASTREC_* switches of `env` set, every other one unset, for the duration of the block."""
    saved = {k: v for k, v in os.environ.items() if k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(saved)


# ---- the canonical text --------------------------------------------------------------------------------------------------
def _buffer_names(eng):
    """eng._bufs name -> canonical name: a gradient buffer's key d@<pointer> becomes d@<name of the activation it belongs to>."""
    owner = {t.data_ptr(): n for n, t in eng._bufs.items() if not n.startswith("d@")}
    names = {}
    for n in eng._bufs:
        if n.startswith("d@"):
            ptr = int(n[2:])
            if ptr not in owner:
                raise PlanError("gradient buffer %s belongs to no named buffer" % n)
            names[n] = "d@" + owner[ptr]
        else:
            names[n] = n
    return names


class _Resolver:
    def __init__(self, eng, extra=None):
        import torch
        names = _buffer_names(eng)
        self.allocs = [(names[n], t.data_ptr(), t.numel() * t.element_size()) for n, t in eng._bufs.items()]
        for n in ENGINE_TENSORS:
            t = getattr(eng, n, None)
            if torch.is_tensor(t) and t.numel():
                self.allocs.append((n, t.data_ptr(), t.numel() * t.element_size()))
        for n, t in (extra or {}).items():
            self.allocs.append((n, t.data_ptr(), t.numel() * t.element_size()))

    def __call__(self, p):
        if not p:
            return "null"
        for name, base, size in self.allocs:
            if base <= p < base + size:
                return "%s+%d" % (name, p - base)
        raise PlanError("pointer 0x%x lies in no allocation of the engine" % p)


def _pointee_count(struct, field):
    """Elements behind a POINTER field: the block and attention arrays of a stack descriptor hold n_blocks, every other one 1."""
    if type(struct).__name__ == "StackDesc" and field in ("blocks", "attn"):
        return struct.n_blocks
    return 1


def _value(v, ctype, R, pad, out, label):
    if ctype is C.c_void_p:
        out.append("%s%s = %s" % (pad, label, R(v.value if isinstance(v, C.c_void_p) else v)))
    elif isinstance(v, C.Structure):
        out.append("%s%s: %s" % (pad, label, type(v).__name__))
        _struct(v, R, pad + "  ", out)
    elif isinstance(v, C.Array):
        out.append("%s%s: array of %d" % (pad, label, len(v)))
        for i, e in enumerate(v):
            _value(e, v._type_, R, pad + "  ", out, "[%d]" % i)
    elif isinstance(v, float):
        out.append("%s%s = %r" % (pad, label, v))
    elif isinstance(v, (int, bytes)) or v is None:
        out.append("%s%s = %r" % (pad, label, v))
    else:
        raise PlanError("%s: a value of type %s has no canonical form" % (label, type(v).__name__))


def _struct(s, R, pad, out):
    for field, ctype in s._fields_:
        v = getattr(s, field)
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            if not v:
                out.append("%s%s = null" % (pad, field))
                continue
            n = _pointee_count(s, field)
            out.append("%s%s -> %d x %s" % (pad, field, n, ctype._type_.__name__))
            for i in range(n):
                _value(v[i], ctype._type_, R, pad + "  ", out, "[%d]" % i)
        else:
            _value(v, ctype, R, pad, out, field)


def _argument(a, ctype, R, out, label):
    pad = "    "
    if a is None:
        out.append("%s%s = null" % (pad, label))
    elif hasattr(a, "_obj"):                                   # byref(structure)
        _value(a._obj, type(a._obj), R, pad, out, label)
    elif isinstance(a, C._Pointer):
        _value(a.contents, type(a.contents), R, pad, out, label)
    elif isinstance(a, (C.Structure, C.Array)):
        _value(a, type(a), R, pad, out, label)
    elif ctype is C.c_void_p:
        _value(a, ctype, R, pad, out, label)
    elif isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        raise PlanError("%s: a bare %r where a %s is expected" % (label, a, ctype.__name__))
    else:
        _value(float(a) if ctype in (C.c_float, C.c_double) else int(a), ctype, R, pad, out, label)


def _launch(entry, R, out):
    name, fn, args = entry
    types = list(fn.argtypes)
    if len(types) != len(args) + 1:                            # (the last parameter is the stream)
        raise PlanError("%s: %d arguments for %d parameters" % (name, len(args), len(types) - 1))
    out.append("  %s" % name)
    for i, (a, t) in enumerate(zip(args, types)):
        _argument(a, t, R, out, "arg%d" % i)


def canonical(eng, extra=None):
    """The plan of `eng` as text.  extra: {name: tensor} of allocations outside the engine that its launches point into (an id
    ring handed to use_id_ring)."""
    R = _Resolver(eng, extra)
    out = ["[derived]"]
    for a in ("n_slabs", "n_wslabs", "use_index", "lazy_adam", "bitwise_reproducible", "bwd_table_done", "fused", "attn_precision",
              "loss", "ce_proposal", "ce_negatives", "gbce_t", "gbce_beta", "row_sparse_adam", "batch_global", "M", "slot_words",
              "index_off"):
        out.append("  %s = %r" % (a, getattr(eng, a, None)))
    out.append("  n_launches = %d" % eng.n_launches())
    out.append("  n_kernel_launches = %d" % eng.n_kernel_launches())
    sc = getattr(eng, "slab_counts", None)
    out.append("  slab_counts = %s" % (None if sc is None else sc.cpu().tolist()))
    out.append("[buffers]")
    names = _buffer_names(eng)
    for n, shape in sorted((names[n], tuple(t.shape)) for n, t in eng._bufs.items()):
        out.append("  %s %s" % (n, shape))
    # the order of allocation decides the device addresses, which the launches' name+offset form cannot show
    out.append("[buffers in order of allocation] %s" % " ".join(names[n] for n in eng._bufs))
    lists = LISTS + (("_ring_next",) if getattr(eng, "_id_ring", None) is not None and getattr(eng, "_ring_next", None) else ())
    for ln in lists:
        lst = getattr(eng, ln, None)
        if lst is None:
            out.append("[%s] none" % ln)
            continue
        lst = lst if isinstance(lst, list) else [lst]
        out.append("[%s] %d" % (ln, len(lst)))
        for entry in lst:
            _launch(entry, R, out)
    return "\n".join(out) + "\n"


def names_of(eng):
    """Entry names of all launch lists of an engine."""
    out = []
    for ln in LISTS:
        lst = getattr(eng, ln, None)
        if lst is not None:
            out += [e[0] for e in (lst if isinstance(lst, list) else [lst])]
    return out


# ---- engines from a small description -----------------------------------------------------------------------------------
def make_engine(E, model="cast_1", D=50, H=1, T=40, L=2, B=3, prec="bf16x3", training=True, n_slabs=5, itemnum=41, max_bins=9,
                hp_kw=None, **kw):
    hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=L, num_heads=H, dropout_rate=0.1, max_bins=max_bins, num_context_blocks=2,
                 lr=1e-3, seed=11, **(hp_kw or {}))
    return E.Engine(model, 9, itemnum, hp, B, training=training, n_slabs=n_slabs, attn_precision=prec, **kw)


def case_text(E, spec, env, steps=()):
    """Header + canonical text of the engine `spec` describes under the switches `env`; a constructor that refuses gives its
    exception's type and message as the text.  steps: "ring" / "noring" -- the plan is dumped again after use_id_ring(ring) / (None)."""
    import torch
    head = "spec %s\nenv %s\n" % (sorted(spec.items()), sorted(env.items()))
    with environment(env), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            eng = make_engine(E, **spec)
        except (ValueError, RuntimeError) as e:
            return head + "raises %s: %s\n" % (type(e).__name__, e)
        text = head + "".join("warns %s: %s\n" % (w.category.__name__, w.message) for w in caught) + canonical(eng)
        ring = None
        for s in steps:
            if s == "ring":
                ring = torch.zeros(4, eng.slot_words, dtype=torch.int32, device=eng.dev)
                eng.use_id_ring(ring)
            else:
                eng.use_id_ring(None)
            text += "== after use_id_ring(%s)\n" % ("ring" if s == "ring" else "None") + canonical(eng, {"ring": ring})
    return text


AWKWARD = [("sasrec", 4, 1, 19, 1, 3), ("cast_1", 5, 1, 33, 2, 3), ("sasrec", 12, 3, 21, 1, 5), ("cast_3", 13, 1, 24, 1, 3),
           ("cast_1", 33, 1, 50, 1, 2), ("sasrec", 47, 1, 70, 2, 2), ("cast_1", 8, 1, 40, 1, 3), ("sasrec", 24, 1, 100, 2, 2),
           ("cast_1", 56, 1, 200, 1, 2), ("cast_8", 63, 3, 31, 1, 3), ("sasrec", 60, 4, 129, 1, 2), ("cast_1", 64, 1, 255, 1, 1),
           ("sasrec", 6, 3, 17, 1, 2), ("sasrec", 66, 1, 18, 1, 2)]       # tests/test_model_gpu.py, test_awkward_hidden_sizes_and_row_counts
PRECS = ("f32", "bf16x3", "bf16")
# base shapes of the switch cases
SWITCH_BASES = [("c1-%s-s%s" % (p, s), dict(model="cast_1", prec=p, n_slabs=s)) for p in ("f32", "bf16x3") for s in (5, None)] + \
               [("sas64", dict(model="sasrec", D=64, H=2, T=50, B=5)), ("sas128", dict(model="sasrec", D=128, H=4)),
                ("sas192", dict(model="sasrec", D=192, H=4, n_slabs=4))]


def cases(E):
    """(case id, spec, env, steps) of every case."""
    out = []
    add = lambda cid, spec, env=None, steps=(): out.append((cid, spec, dict(env or {}), steps))
    for m in E.MODELS:
        for p in PRECS:
            for tr in (True, False):
                for s in (5, None):
                    add("models/%s/%s/%s/s%s" % (m, p, "train" if tr else "eval", s), dict(model=m, prec=p, training=tr, n_slabs=s))
    for m in ("sasrec", "cast_1"):
        for p in PRECS:
            for tr in (True, False):
                add("want_attn/%s/%s/%s" % (m, p, "train" if tr else "eval"), dict(model=m, prec=p, training=tr, want_attn=True))
    for (m, D, H, T, L, B) in AWKWARD:
        for p in ("f32", "bf16x3"):
            add("awkward/%s-D%d-H%d-T%d-L%d-B%d/%s" % (m, D, H, T, L, B, p), dict(model=m, D=D, H=H, T=T, L=L, B=B, prec=p))
    for L in (0, 1, 4, 5):
        add("blocks/%d" % L, dict(model="sasrec", L=L))
    for T in (16, 17, 112, 113, 208, 209, 224, 225, 256, 257, 512):
        for p in ("bf16x3", "bf16"):
            for s in (5, None):
                add("T/%d/%s/s%s" % (T, p, s), dict(model="sasrec", T=T, B=2, prec=p, n_slabs=s))
    add("shape/sas64", dict(model="sasrec", D=64, H=2, T=50, B=5))
    add("shape/bench", dict(model="cast_1", T=200, B=128, n_slabs=None, itemnum=3416, max_bins=200))
    for B in (80, 81, 160, 161):
        add("shape/B%d" % B, dict(model="cast_1", B=B, n_slabs=None))
    for m in ("sasrec", "cast_4"):
        for D, H in ((66, 1), (128, 1), (128, 2), (128, 4), (192, 4), (256, 4)):
            for p in PRECS:
                add("wide/%s-D%d-H%d/%s" % (m, D, H, p), dict(model=m, D=D, H=H, prec=p))
    for bid, base in SWITCH_BASES:
        combos = [(s,) for s in SWITCHES] + list(itertools.combinations(SWITCHES, 2))
        for names in combos:
            env = {n: SWITCHES[n] for n in names}
            spec = dict(base)
            if "CASTREC_ATTN_PRECISION" in env:
                spec["prec"] = None                      # the environment's precision holds only where none is asked for
            add("switch/%s/%s" % (bid, "+".join(n[8:] for n in names)), spec, env)
    for m in ("sasrec", "cast_1"):
        for p in ("bf16x3", "bf16"):
            for loss, kw in (("ce", {}), ("sampled_ce", {}), ("sampled_ce-pop", dict(ce_proposal="popularity")), ("gbce", {})):
                add("loss/%s/%s/%s" % (loss, m, p), dict(model=m, prec=p, loss=loss.split("-")[0], **kw))
        for loss in ("bce", "sampled_ce", "gbce"):
            add("loss/row_sparse/%s/%s" % (loss, m), dict(model=m, loss=loss, row_sparse_adam=True))
        add("loss/row_sparse_hp/%s" % m, dict(model=m, hp_kw=dict(row_sparse_adam=True, loss="gbce", ce_negatives=7, gbce_t=0.5)))
        add("loss/lazy/%s" % m, dict(model=m, lazy_adam=True))
        add("loss/lazy_env/%s" % m, dict(model=m), {"CASTREC_LAZY_ADAM": "1"})
        add("loss/l2/%s" % m, dict(model=m, hp_kw=dict(l2_emb=0.01)))
        for lazy in (False, True):
            add("dp/%s/lazy%d" % (m, lazy), dict(model=m, batch_global=6, row_offset=3, lazy_adam=lazy))
            add("ring/%s/lazy%d" % (m, lazy), dict(model=m, lazy_adam=lazy, n_slabs=None), steps=("ring", "noring"))
    # every refusal of the constructor (a process without a GPU and a failed host allocation apart)
    refusals = [("model", dict(model="cast_10")), ("attn_precision", dict(prec="fp8")), ("loss", dict(loss="mse")),
                ("ce_proposal", dict(ce_proposal="zipf")), ("popularity_needs_sampled_ce", dict(loss="gbce", ce_proposal="popularity")),
                ("ce_row_sparse", dict(loss="ce", row_sparse_adam=True)), ("ce_lazy", dict(loss="ce", lazy_adam=True)),
                ("sampled_lazy", dict(loss="sampled_ce", lazy_adam=True)), ("softmax_dp", dict(loss="gbce", batch_global=6, row_offset=3)),
                ("softmax_dp_global", dict(loss="ce", batch_global=6)), ("ce_hidden", dict(loss="ce", D=4)),
                ("ce_hidden_wide", dict(loss="sampled_ce", D=260, H=4)), ("ce_negatives", dict(loss="sampled_ce", ce_negatives=0)),
                ("ce_negatives_max", dict(loss="gbce", ce_negatives=1 << 20)), ("gbce_t", dict(loss="gbce", gbce_t=1.5)),
                ("gbce_t_nan", dict(loss="gbce", gbce_t=float("nan"))), ("fused_wide", dict(D=128, H=4, fused=True)),
                ("eval_ignores_loss", dict(loss="ce", lazy_adam=True, training=False))]
    for cid, spec in refusals:
        add("refusal/%s" % cid, dict(dict(model="sasrec"), **spec))
    add("refusal/lazy_env", dict(model="sasrec", loss="gbce"), {"CASTREC_LAZY_ADAM": "1"})
    return out


# ---- the switch check of tests/test_model_gpu.py --------------------------------------------------------------------------
_F32 = dict(model="cast_1", prec="f32")
_BF = dict(model="cast_1", prec="bf16x3")
_WIDE = dict(model="sasrec", D=128, H=4)
# switch -> (spec, switches set on BOTH sides, entries it removes, entries it adds): the smallest shape whose default plan takes the
# path the switch turns off
SWITCH_CHECKS = {
    "CASTREC_NO_TAILS": (_F32, {}, ["cr_block_ln_ffn_fwd_tail"], ["cr_block_ln_ffn_fwd"]),
    "CASTREC_TWO_PASS_ATTN_BWD": (_F32, {}, [], []),                      # same entries; no delta / dQ partial in the descriptors
    "CASTREC_NO_EMBED_FUSION": (_F32, {}, ["cr_block_ln_qkv_fwd_gather"], ["cr_embed_fwd"]),
    "CASTREC_NO_HEAD_LN": (_F32, {}, ["cr_head_fwd_bwd_ln"], ["cr_head_fwd_bwd"]),
    "CASTREC_NO_STACK_KERNEL": (_BF, {}, ["cr_stack_fwd"], ["cr_attn_fwd"]),
    "CASTREC_NO_STACK_BWD": (_BF, {}, ["cr_stack_block_bwd"], ["cr_block_ln_ffn_bwd"]),
    "CASTREC_NO_BLOCK_BWD": (_BF, {}, ["cr_stack_block_bwd"], ["cr_stack_ffn_bwd"]),
    # the context stack's final LayerNorm (the trunk's is the head's): its backward leaves the last block's launch for one of its own
    "CASTREC_NO_LNF_FUSION": (_BF, {}, [], ["cr_layernorm_bwd"]),
    "CASTREC_NO_INDEX": (_BF, {}, ["cr_table_grad"], []),
    "CASTREC_NO_HEAD_FUSION": (dict(_BF, n_slabs=None), {}, ["cr_stack_fwd_head"], ["cr_head_fwd_bwd_ln"]),
    "CASTREC_NO_WIDE": (_WIDE, {}, ["cr_wide_ln_qkv_fwd", "cr_wide_ln_ffn_bwd"], ["cr_layernorm_fwd"]),
    "CASTREC_WIDE_NO_WGRAD": (_WIDE, {}, [], ["cr_gemm_wgrad"]),
    "CASTREC_WIDE_NO_DELTA": (_WIDE, {}, [], []),                         # same entries; the FFN backward emits no per-head delta
    "CASTREC_WIDE_NO_TAILS": (_WIDE, {}, ["cr_wide_ln_ffn_fwd_tail"], ["cr_wide_ln_ffn_fwd"]),
    "CASTREC_BF_TWO_KERNELS": (_WIDE, {}, [], []),                        # as CASTREC_WIDE_NO_DELTA (the C side splits the launch)
    # only where cr_gemm_wgrad alone forms the weight gradients and 32 slabs would be too many: through n_wslabs and slab_counts
    "CASTREC_WSLABS": (dict(model="sasrec", D=192, H=4, n_slabs=4), {}, [], []),
    # two heads at D = 64 take the per-head delta only in the three-launch block backward: set up with CASTREC_NO_BLOCK_BWD,
    # whatever cr_stack_block_bwd_supported answers at this shape
    "CASTREC_NO_HEAD_DELTA": (dict(model="sasrec", D=64, H=2, T=50, B=5), {"CASTREC_NO_BLOCK_BWD": "1"}, ["cr_stack_ffn_bwd_heads"], []),
    "CASTREC_STACK_PAIR_MAX_B": (_BF, {}, [], []),                        # changes n_kernel_launches() alone (B = 3 > 2)
    "CASTREC_LAZY_ADAM": (_BF, {}, ["cr_table_grad"], []),                # row-sparse Adam: no occurrence index
    "CASTREC_ATTN_PRECISION": (dict(_BF, prec=None), {}, [], []),         # no precision asked for: the environment's holds
}


def switch_check(E, switch):
    """Asserts that `switch` changes the plan of the engine SWITCH_CHECKS names for it."""
    spec, both, removed, added = SWITCH_CHECKS[switch]
    with environment(both):
        a = make_engine(E, **spec)
        ta, na = canonical(a), names_of(a)
    with environment(dict(both, **{switch: SWITCHES[switch]})):
        b = make_engine(E, **spec)
        tb, nb = canonical(b), names_of(b)
    assert ta != tb, "%s leaves the plan as it is" % switch
    for n in removed:
        assert n in na and n not in nb, "%s: entry %s with the switch %s, without it %s" % (switch, n, n in nb, n in na)
    for n in added:
        assert n in nb, "%s: no entry %s with the switch" % (switch, n)


# ---- command line --------------------------------------------------------------------------------------------------------
def _read_full(path):
    texts, cid = {}, None
    with gzip.open(path, "rt") as f:
        for line in f:
            if line.startswith("#### "):
                cid = line[5:].strip()
                texts[cid] = []
            else:
                texts[cid].append(line)
    return texts


def _diff(a_path, b_path, limit=40):
    a, b = _read_full(a_path), _read_full(b_path)
    bad = [c for c in sorted(set(a) | set(b)) if a.get(c) != b.get(c)]
    print("%d cases on one side, %d on the other, %d differ" % (len(a), len(b), len(bad)))
    for c in bad[:limit]:
        print("---- %s" % c)
        sys.stdout.writelines(list(difflib.unified_diff(a.get(c, []), b.get(c, []), "a", "b", n=2))[:60])
    return 1 if bad else 0


def fold(lines):
    """Per-case lines (case id, sha256) folded into one line per group of cases: group, number of cases, sha256 of the group's
    per-case lines in order.  A group is a case id's first component (its first two under models/ and switch/)."""
    groups = {}
    for line in lines:
        parts = line.split()[0].split("/")
        groups.setdefault("/".join(parts[:2 if parts[0] in ("models", "switch") else 1]), []).append(line)
    return ["%s %d %s\n" % (g, len(ls), hashlib.sha256("".join(ls).encode()).hexdigest()) for g, ls in groups.items()]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", help="root of another checkout whose planner is dumped")
    ap.add_argument("--out", help="file of one line per case: case id, sha256 of its canonical text")
    ap.add_argument("--groups", help="file of one line per group of cases: the --out lines folded (see fold)")
    ap.add_argument("--full", help="gzip file of every case's canonical text")
    ap.add_argument("--only", help="case ids starting with this prefix")
    ap.add_argument("--switch-check", action="store_true", help="run switch_check for every planner switch")
    ap.add_argument("--diff", nargs=2, metavar="FULL", help="compare two --full files")
    a = ap.parse_args(argv)
    if a.diff:
        return _diff(*a.diff)
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import castrec_amd  # noqa: F401
    from castrec_amd import engine as E
    print("planner of %s" % os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))), flush=True)
    if a.switch_check:
        for s in PLANNER_SWITCHES:
            switch_check(E, s)
            print("ok %s" % s, flush=True)
        return 0
    lines, full = [], gzip.open(a.full, "wt") if a.full else None
    todo = [c for c in cases(E) if not a.only or c[0].startswith(a.only)]
    for i, (cid, spec, env, steps) in enumerate(todo):
        text = case_text(E, spec, env, steps)
        lines.append("%s %s\n" % (cid, hashlib.sha256(text.encode()).hexdigest()))
        if full:
            full.write("#### %s\n%s" % (cid, text))
        if i % 100 == 0:
            print("%d / %d  %s" % (i, len(todo), cid), flush=True)
            gc.collect()
    if full:
        full.close()
    for path, text in ((a.out, lines), (a.groups, fold(lines))):
        if path:
            with open(path, "w") as f:
                f.writelines(text)
    if not (a.out or a.groups):
        sys.stdout.writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())

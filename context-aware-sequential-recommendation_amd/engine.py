"""Static forward/backward programs of the SASRec / CAST graphs, composed of libcastrec kernels.

The reference builds a TensorFlow graph once (models/sasrec.py, models/cast_N.py) and runs it with
``sess.run``; here the graph of a model is compiled ONCE into flat lists of pre-built C-ABI launches
over persistent device buffers -- ``fwd`` and ``bwd``, and the single entries that end a step: ``_l2``,
``_adam`` (plain step), ``_tgrad`` / ``_reduce`` / ``_adam_flat`` (data-parallel step) -- which makes
the whole step capturable as a HIP graph (launch-bound problem sizes).  Gradients are hand-derived per
op; there is no autograd and no CPU fallback.

The launch planner is Engine.op_embed .. Engine._finalize: every op_* emits its
forward launches and registers a factory for its backward, which _finalize runs in reverse order; every
environment switch is a field of Switches, read once per engine.

Memory layout (all fp32, resident in HBM for the life of the engine):
  P / M / V   flat parameter, Adam-m, Adam-v vectors: [table section | dense section]
  Gt          table-gradient accumulator (float atomics), zeroed by cr_adam_step after use
  Gs          dense-gradient slabs [n_slabs, n_dense]: every reducing kernel writes slab s from its
              workgroup s (no atomics, bitwise reproducible); cr_adam_step sums the slabs
  activations one [B*T, ld] buffer per tensor of the graph (row = b*T + t)
"""
import ctypes as C
import math
import os
import zlib
from collections import namedtuple
from typing import NamedTuple

import numpy as np
import torch

from . import lib as L
from . import ops as O

# arithmetic of the attention products (castrec.h CR_PREC_*): "f32" = exact fp32 MFMA; "bf16x3" = bf16 MFMA on hi + lo
# split operands (three products, ~1e-5 relative: inside the 1e-3 fp32 bound); "bf16" = plain bf16 operands
ATTN_PRECISIONS = {"f32": L.PREC_F32, "bf16x3": L.PREC_BF16X3, "bf16": L.PREC_BF16}
DEFAULT_ATTN_PRECISION = "bf16x3"
# training objectives: "bce" the reference's pos / neg dot-product BCE with one sampled negative per position (cr_head_fwd_bwd);
# "ce" softmax cross-entropy over the whole item catalogue (cr_softmax_ce)
LOSSES = ("bce", "ce")
# ... and "sampled_ce": softmax cross-entropy over the target and ce_negatives items drawn uniformly for the whole batch
# (cr_sampled_ce)
# ... and "gbce": gSASRec's generalised binary cross-entropy over the target and the same kind of shared negatives, the positive
# term weighted by beta from the sampling rate and gbce_t (cr_gbce)
ALL_LOSSES = LOSSES + ("sampled_ce", "gbce")
SOFTMAX_LOSSES = ("ce", "sampled_ce", "gbce")     # the losses that take the route of "ce" (one launch in op_head, d(seq_emb) stored)
SAMPLED_LOSSES = ("sampled_ce", "gbce")
# the proposal "sampled_ce" draws its shared negatives from: "uniform", or "popularity" -- item weights handed over with
# Engine.set_item_weights, the draw by a search of their cumulative masses and the log-Q correction on every candidate's logit
# (castrec.h cr_sampled_ce)
CE_PROPOSALS = ("uniform", "popularity")

MODELS = ["cast_1", "cast_2", "cast_3", "cast_4", "cast_5", "cast_6", "cast_7", "cast_8", "cast_9",
          "sasrec", "sasrec_static"]          # main.py:28


def site_id(name):
    """Stable 24-bit id of a dropout call site (names follow the graph: 'emb', 'trunk.0.attn', ...)."""
    return zlib.crc32(name.encode()) & 0xFFFFFF


def positional_encoding(dim, length):
    """modules.py:27-37 (sin on even FLAT indices, cos on odd ones; exponent 2*i/dim)."""
    v = np.array([pos / np.power(10000, 2 * i / dim) for pos in range(length) for i in range(dim)])
    v[::2] = np.sin(v[::2])
    v[1::2] = np.cos(v[1::2])
    return v.reshape(length, dim).astype(np.float32)


class Hyper:
    """The fields of the reference's argparse namespace the graphs read (main.py:45-82)."""

    def __init__(self, args=None, **kw):
        d = dict(maxlen=50, hidden_units=50, num_blocks=2, num_heads=1, dropout_rate=0.5, l2_emb=0.0, lr=1e-3,
                 max_bins=200, num_context_blocks=2, seed=42, loss="bce", ce_negatives=256, gbce_t=0.75, ce_proposal="uniform",
                 ce_pop_power=1.0, row_sparse_adam=False)
        for k in d:
            if args is not None and hasattr(args, k):
                d[k] = getattr(args, k)
        d.update(kw)
        self.__dict__.update(d)
        if self.hidden_units % self.num_heads != 0:
            raise ValueError("hidden_units must be divisible by num_heads (tf.split, modules.py:208)")


def auto_slabs(M):
    """Number of gradient slabs = workgroups of every weight-gradient kernel.  The fused backward kernels work on two
    64-row tile groups per workgroup: ceil(M / 128) workgroups have both groups full (M = 25 600: 200 slabs, 0.8 %
    faster end to end than 256 slabs of 100 rows, and 22 % fewer slab bytes for Adam to sum); small problems get one
    64-row tile per workgroup so that enough workgroups exist; never more than one workgroup per CU."""
    n = -(-M // 128)
    if n < 128:
        n = -(-M // 64)
    return max(1, min(256, n))


# ---------------------------------------------------------------------------------------------------
# parameter layout
# ---------------------------------------------------------------------------------------------------
def _stack_entries(prefix, L_, D):
    out = []
    for i in range(L_):
        p = "%s.%d." % (prefix, i)
        out += [(p + "ln1.gamma", (D,), "ones"), (p + "ln1.beta", (D,), "zeros"),
                (p + "wqkv", (D, 3 * D), "glorot3"), (p + "bqkv", (3 * D,), "zeros"),
                (p + "ln2.gamma", (D,), "ones"), (p + "ln2.beta", (D,), "zeros"),
                (p + "w1", (D, D), "glorot"), (p + "b1", (D,), "zeros"),
                (p + "w2", (D, D), "glorot"), (p + "b2", (D,), "zeros")]
    out += [(prefix + ".lnf.gamma", (D,), "ones"), (prefix + ".lnf.beta", (D,), "zeros")]
    return out


def model_structure(model, hp):
    """Which pieces a graph has: context stacks, small tables, mlp width (SURVEY 8a variant table)."""
    L_, Lc = hp.num_blocks, hp.num_context_blocks
    s = dict(ctx={}, small=[], mlp=0, learned_pos=model in ("sasrec", "cast_9"))
    if model in ("cast_1", "cast_2", "cast_3", "cast_4", "cast_5", "cast_6"):
        s["ctx"]["ctx_time"] = L_
    if model == "cast_8":
        s["ctx"].update(ctx_hours=L_, ctx_days=L_)
    if model == "cast_9":
        s["ctx"].update(ctx_hours=Lc, ctx_days=Lc, ctx_time=Lc)
    if "ctx_time" in s["ctx"]:
        s["small"].append(("time_emb", hp.max_bins + 1))
    if model in ("cast_3", "cast_4", "cast_5", "cast_6", "cast_7", "cast_8", "cast_9"):
        s["small"] += [("hours_emb", 25), ("days_emb", 8)]
    s["mlp"] = {"cast_2": 2, "cast_3": 3, "cast_4": 4, "cast_5": 3, "cast_6": 4, "cast_7": 3, "cast_8": 3, "cast_9": 4}.get(model, 0)
    return s


class ParamLayout:
    def __init__(self, model, usernum, itemnum, hp):
        D, T = hp.hidden_units, hp.maxlen
        st = model_structure(model, hp)
        table = [("item_emb", (itemnum + 1, D), "glorot")]
        if st["learned_pos"]:
            table.append(("pos_emb", (T, D), "glorot"))
        dense = [(n, (v, D), "glorot") for n, v in st["small"]]
        for pfx, Lc in st["ctx"].items():
            dense += _stack_entries(pfx, Lc, D)
        if st["mlp"]:
            k = st["mlp"]
            dense += [("mlp.w1", (k * D, k * D), "glorot"), ("mlp.b1", (k * D,), "zeros"),
                      ("mlp.w2", (k * D, D), "glorot"), ("mlp.b2", (D,), "zeros")]
        dense += _stack_entries("trunk", hp.num_blocks, D)
        self.entries, off = {}, 0
        for (n, shape, init) in table:
            self.entries[n] = (off, shape, init, "table"); off += int(np.prod(shape))
        self.n_table = off
        for (n, shape, init) in dense:
            self.entries[n] = (off, shape, init, "dense"); off += int(np.prod(shape))
        self.n_total, self.n_dense, self.D = off, off - self.n_table, D
        # the lookup tables lead the flat vector (item_emb, pos_emb, then the small context tables): the range
        # tf.contrib.layers.l2_regularizer(l2_emb) covers (modules.py:149-153)
        self.n_l2 = self.n_table + sum(int(np.prod(self.entries[n][1])) for n, _ in st["small"])

    def logical_names(self):
        """Names as the oracle / reference variables see them (wq, wk, wv instead of the fused wqkv)."""
        out = []
        for n in self.entries:
            if n.endswith("wqkv"):
                out += [n[:-4] + x for x in ("wq", "wk", "wv")]
            elif n.endswith("bqkv"):
                out += [n[:-4] + x for x in ("bq", "bk", "bv")]
            else:
                out.append(n)
        return out

    def view(self, flat, name):
        """torch view of a (logical) parameter inside a flat [n_total] tensor."""
        D = self.D
        for j, x in enumerate(("q", "k", "v")):
            if name.endswith(".w" + x):
                off, shape, _, _ = self.entries[name[:-2] + "wqkv"]
                return flat[off:off + D * 3 * D].view(D, 3 * D)[:, j * D:(j + 1) * D]
            if name.endswith(".b" + x):
                off, shape, _, _ = self.entries[name[:-2] + "bqkv"]
                return flat[off + j * D:off + (j + 1) * D]
        off, shape, _, _ = self.entries[name]
        return flat[off:off + int(np.prod(shape))].view(*shape)

    def init_host(self, seed):
        """glorot-uniform kernels/tables (TF default of get_variable, tf.layers.dense/conv1d), zero biases,
        LayerNorm gamma=1 / beta=0 (modules.py:75-76)."""
        rs = np.random.RandomState(seed)
        flat = np.zeros(self.n_total, np.float32)
        for n, (off, shape, init, _) in self.entries.items():
            size = int(np.prod(shape))
            if init == "glorot":
                lim = math.sqrt(6.0 / (shape[0] + shape[1]))
                flat[off:off + size] = rs.uniform(-lim, lim, size)
            elif init == "glorot3":       # three independent [D,D] dense kernels side by side
                D = shape[0]
                lim = math.sqrt(6.0 / (D + D))
                flat[off:off + size] = rs.uniform(-lim, lim, size)
            elif init == "ones":
                flat[off:off + size] = 1.0
        return flat


# ---- the launch planner's switches and records ------------------------------------------------------
class Switches(NamedTuple):
    """The environment switches of the engine (field x is CASTREC_X), read once at the top of Engine.__init__.  A flag is on when
    its variable is "1" (bf_two_kernels: when it is set at all); each line says what it turns off and what runs instead."""
    two_pass_attn_bwd: bool    # fp32 attention, one head: no delta / dQ partials from the FFN backward -> two-pass cr_attn_bwd
    no_tails: bool             # the next block's LN1 + QKV, the final LayerNorm inside the FFN kernel -> cr_block_ln_ffn_fwd, own launches
    no_embed_fusion: bool      # a stack's input gathered by its first kernel -> cr_embed_fwd in front of the stack
    no_stack_kernel: bool      # up to four blocks forward in one cr_stack_fwd -> cr_block_* / cr_attn_fwd per block
    no_stack_bwd: bool         # register-layout row phases backward (cr_stack_*_bwd*) and their slab count -> cr_block_ln_*_bwd
    no_wide: bool              # D = 128 / 192 / 256 row phases as cr_wide_* -> cr_layernorm_* / cr_gemm_rows / cr_eltwise
    no_block_bwd: bool         # a block's backward as one cr_stack_block_bwd -> cr_stack_ffn_bwd*, cr_attn_bwd, cr_stack_qkv_bwd*
    no_head_ln: bool           # the final LayerNorm's backward inside the head -> cr_head_fwd_bwd + cr_layernorm_bwd
    no_id_check: bool          # (no planner switch) set_batch() / feed() do not range check host ids
    no_head_fusion: bool       # the head as the tail of the last forward launch (and its 2 B slabs) -> cr_head_fwd_bwd_ln
    wslabs: int                # (default 32) slabs of cr_gemm_wgrad at D > 128 outside the fused path: n_wslabs = min(n_slabs, this)
    no_index: bool             # table gradients by the occurrence index's gather -> float atomics from head and embedding backward
    wide_no_wgrad: bool        # D = 128: cr_wide_* form the weight gradients themselves -> cr_gemm_wgrad
    wide_no_delta: bool        # cr_wide_ln_ffn_bwd emits the per-head delta -> two-launch cr_attn_bwd
    bf_two_kernels: bool       # (also read by the C side) one-launch bf16 attention backward: no per-head delta is asked for
    no_head_delta: bool        # two heads at D = 64: cr_stack_ffn_bwd_heads -> cr_stack_ffn_bwd / _ln, two-launch cr_attn_bwd
    wide_no_tails: bool        # D = 128: cr_wide_ln_ffn_fwd_tail -> cr_wide_ln_ffn_fwd + cr_wide_ln_qkv_fwd / cr_layernorm_fwd
    no_lnf_fusion: bool        # a stack's final LayerNorm backward inside its last block's backward -> cr_layernorm_bwd
    stack_pair_max_b: int      # (default 160) batch sizes up to which n_kernel_launches() counts a launch per block of cr_stack_fwd
    lazy_adam: bool            # default of Engine(lazy_adam=None): row-sparse Adam over seq | pos | neg
    attn_precision: str        # default of Engine(attn_precision=None), in front of hp.attn_precision; None: unset or empty

    @classmethod
    def from_env(cls, env):
        on = lambda f: env.get("CASTREC_" + f.upper()) == "1"
        special = dict(wslabs=int(env.get("CASTREC_WSLABS", "32")), stack_pair_max_b=int(env.get("CASTREC_STACK_PAIR_MAX_B", 160)),
                       bf_two_kernels=env.get("CASTREC_BF_TWO_KERNELS") is not None,
                       lazy_adam=bool(int(env.get("CASTREC_LAZY_ADAM", "0"))), attn_precision=env.get("CASTREC_ATTN_PRECISION") or None)
        return cls(**{f: special[f] if f in special else on(f) for f in cls._fields})


# what op_embed leaves for the first block behind it, which may apply the lookup's backward itself: make_desc(in_block) -> EmbedBwdDesc;
# small: a context table (gradient written as slabs); indexed: the item table's seq lookup under the occurrence index (rows are left)
ScatterRecipe = namedtuple("ScatterRecipe", "make_desc addend small table indexed scale")
# a LayerNorm (input buffer, parameter prefix) whose backward op_head may take over
LnRecipe = namedtuple("LnRecipe", "x pname")
# a stack's final LayerNorm that its last block's backward may apply: yptr = out's pointer at column col, out of pitch ld
LnfIntent = namedtuple("LnfIntent", "yptr pname out ld col")
# what a block's FFN kernel runs behind it: "next" = LN1 + QKV of block pname with output out; "lnf" = LayerNorm pname into out[:, col:]
Tail = namedtuple("Tail", "kind pname out ld col", defaults=(0, 0))
# the gradient rows of the item table's seq lookup, left for the occurrence index's gather: scale * (rows + rows2), rows2 may be None
TgRows = namedtuple("TgRows", "rows rows2 ld scale")
# the activation buffers of one block, eng._bufs[<prefix><field>]; qkv is [3, M, D]: Q rows, K rows, V rows
BlockBufs = namedtuple("BlockBufs", "q_in o f_in hid qkv kvalid qvalid")
# ... and its parameters, in the order of cr_block_desc and (their gradients) cr_block_bwd_desc
BLOCK_PARAMS = ("ln1.gamma", "ln1.beta", "wqkv", "bqkv", "ln2.gamma", "ln2.beta", "w1", "b1", "w2", "b2")


# ---------------------------------------------------------------------------------------------------
class Engine:
    def __init__(self, model, usernum, itemnum, hp, batch_size, training=True, seed=None, n_slabs=None,
                 share=None, batch_global=None, row_offset=0, want_attn=False, device="cuda", fused=None,
                 attn_precision=None, lazy_adam=None, loss=None, ce_negatives=None, gbce_t=None, ce_proposal=None,
                 row_sparse_adam=None):
        """loss: the training objective, "bce" (the default: hp.loss, else "bce") or "ce" -- full-catalogue softmax cross-entropy
        (cr_softmax_ce).  Under "ce" the prediction head is one cr_softmax_ce launch that stores d(seq_emb) and accumulates the item
        table's gradient into Gt; the occurrence index and the head fusions are off, so the embedding backward scatters with float
        atomics and bitwise_reproducible is False.  "ce" refuses row-sparse Adam, data parallelism and hidden sizes outside 8..256
        (ValueError).  Eval engines ignore the option.
        "sampled_ce" takes the route of "ce" with one cr_sampled_ce launch: the softmax over each row's target and ce_negatives
        (default hp.ce_negatives, else 256) item ids drawn uniformly on the device for the whole batch from the engine's seed and step
        word; eng.samples holds the last step's ids.  It refuses what "ce" refuses (row_sparse_adam apart, below) and ce_negatives outside 1..CR_SCE_MAX_SAMPLES.
        "gbce" takes the route of "sampled_ce" with one cr_gbce launch: binary cross-entropy over the target and ce_negatives shared
        uniform negatives, the positive term weighted by eng.gbce_beta = 1 - t (1 - alpha), alpha = min(1, ce_negatives / max(1,
        itemnum - 1)) the sampling rate over the items that are not the target and t = gbce_t (default hp.gbce_t, else 0.75; the
        calibration parameter of gSASRec: 0 is plain BCE, 1 is fully calibrated).  It also refuses gbce_t outside [0, 1].
        ce_proposal: "uniform" (the default: hp.ce_proposal, else "uniform") or "popularity", for "sampled_ce" only (gBCE's beta is
        derived for uniform sampling).  Under "popularity" the samples are drawn from the item weights of set_item_weights() -- a step
        before the first call raises RuntimeError -- and every candidate's logit, the target's included, is corrected by -log Q; the
        device arrays item_cdf / item_logq [itemnum + 1] are allocated here and rewritten in place, so a captured graph follows a new
        set of weights.  Still one cr_sampled_ce launch: the launch list is "sampled_ce"'s.  Eval engines ignore the option.
        row_sparse_adam (default hp.row_sparse_adam, else False): Adam moves only the item rows that have a gradient in the step -- a
        DEVIATION from the reference's dense update.  Taken by "bce" (rows seq | pos | neg: the engine of
        lazy_adam=True), "sampled_ce" and "gbce" (rows seq | pos and the step's samples, read by the Adam launch from eng.samples where
        the loss launch left them: neg has no gradient under these losses and is not listed); "ce" refuses it (every item row has a
        gradient).  It sets eng.lazy_adam.  The older spelling lazy_adam=True / CASTREC_LAZY_ADAM=1 lists seq | pos | neg only and
        stays refused for the three softmax-route losses."""
        self.sw = sw = Switches.from_env(os.environ)
        if model not in MODELS:
            raise ValueError("model must be one of %s" % MODELS)
        if not torch.cuda.is_available():
            raise RuntimeError("castrec_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.model, self.hp, self.B, self.T, self.D = model, hp, batch_size, hp.maxlen, hp.hidden_units
        self.H = hp.num_heads
        self.usernum, self.itemnum, self.training = usernum, itemnum, training
        self._resolve_options(attn_precision, lazy_adam, loss, ce_negatives, gbce_t, ce_proposal, row_sparse_adam, fused,
                              data_parallel=(batch_global is not None and batch_global != batch_size) or bool(row_offset))
        self.M = self.B * self.T
        self.flags_epoch = 0                          # bumped wherever set_step zeroes lazy_flags: a flag then says nothing about earlier steps
        self._pending_embed = {}
        self._scatter_recipe, self._scatter_claimed = {}, set()      # out buffer of an embedding lookup -> ScatterRecipe
        self._ln_recipe, self._ln_claimed = {}, set()                # LayerNorm output pointer -> LnRecipe
        self._lnf_intent = {}                                        # y buffer of a stack's last block -> LnfIntent
        # one launch per block backward (cr_stack_block_bwd): the gradient of a block input then exists as TWO partials;
        # _grad2 maps an activation buffer to the second addend of its gradient until a consumer takes it (see _second_grad)
        self._grad2, self._grad2_bufs = {}, {}        # (the second: data_ptr -> (activation buffer, second-addend buffer))
        self._block_bwd_ranges = []                   # slab-0 float ranges written by cr_stack_block_bwd (one slab per sequence)
        self.dev = torch.device(device)
        self.seed = hp.seed if seed is None else seed
        self.layout = lay = share.layout if share is not None else ParamLayout(model, usernum, itemnum, hp)
        if not n_slabs:
            n_slabs = auto_slabs(batch_size * hp.maxlen)
            # the register-layout backward kernels (cr_stack_bwd.hip) deal (sequence, round) items to the slab workgroups:
            # with a slab per item every workgroup runs one round (B = 128 sequences of 13 tiles: 256 workgroups, 256 CUs)
            if self.fused and self.attn_precision != "f32" and 8 <= self.D <= 64 and self.T <= 224 and not sw.no_stack_bwd:
                items = batch_size * (2 if self.T > 112 else 1)
                if n_slabs < items <= 512:
                    n_slabs = items
                # the prediction head as the tail of the trunk's last forward launch (cr_stack_fwd_head): its two workgroups per sequence
                # write a slab each of the final LayerNorm's gradient
                if training and self.T > 16 and batch_size <= 160 and n_slabs < 2 * batch_size <= 512 and not sw.no_head_fusion:
                    n_slabs = 2 * batch_size
        self.n_slabs = n_slabs
        # cr_gemm_wgrad reduces over rows in n_wslabs workgroups per output tile: at the large hidden sizes of the unfused / wide
        # path (D x D weights, 4 blocks) a slab per 128 rows is 264 MB written and read again per step (config C4); 32 suffice
        # to fill the chip (tiles x slabs workgroups).  cr_adam_step learns per 256-parameter block how many slabs are in use.
        self.n_wslabs = n_slabs if (self.fused or self.D <= 128) else min(n_slabs, sw.wslabs)
        self._wgrad_ranges, self.slab_counts = [], None
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.P = share.P if share is not None else torch.from_numpy(lay.init_host(self.seed)).to(self.dev)
        self.state = torch.zeros(L.CR_STATE_FLOATS, **f32)
        self.state[4:5].view(torch.int32)[0] = 1                      # number of the first step (see set_step)
        if training:
            self.Mom = torch.zeros(lay.n_total, **f32)
            self.Vel = torch.zeros(lay.n_total, **f32)
            # flat gradient bucket [table | dense | loss stats(3) + pad]: the table part receives float atomics
            # directly; the dense part is written by cr_reduce_slabs (data-parallel path only)
            self.Gflat = torch.zeros(lay.n_total + 4, **f32)
            self.Gt = self.Gflat[:lay.n_table]
            self.Gs = torch.zeros(n_slabs, max(lay.n_dense, 1), **f32)
            if self.loss in SOFTMAX_LOSSES:
                nb = (O.softmax_ce_workspace_bytes(self.M, itemnum + 1, self.D) if self.loss == "ce"
                      else O.sampled_ce_workspace_bytes(self.M, self.ce_negatives, self.D) if self.loss == "sampled_ce"
                      else O.gbce_workspace_bytes(self.M, self.ce_negatives, self.D))
                self._ce_ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)
            if self.loss in SAMPLED_LOSSES:
                self.samples = torch.zeros(self.ce_negatives, dtype=torch.int32, device=self.dev)    # the last step's sample ids
            if self.ce_proposal == "popularity":
                # the proposal's two arrays (castrec.h): written in place by set_item_weights, read by every later step
                self.item_cdf = torch.zeros(itemnum + 1, dtype=torch.int32, device=self.dev)         # (the bits of the uint32 masses)
                self.item_logq = torch.zeros(itemnum + 1, **f32)
                self._have_item_weights = False
        self.drop = O.Drop(hp.dropout_rate if training else 0.0, self.seed, self.state, row_offset)
        self.batch_global = self.B if batch_global is None else batch_global
        self.want_attn, self.attn_weights = want_attn, None
        self._bufs, self._keep = {}, []
        self.fwd, self.bwd, self._bwd_factories = [], [], []
        self._grad_written = set()
        i32 = dict(dtype=torch.int32, device=self.dev)
        # the six id inputs of one batch live in ONE [6, M] buffer so a staged batch is a single D2D copy
        self.ID_KEYS = ("seq", "pos", "neg", "time", "hours", "days")
        # The occurrence index of the batch (castrec.h, "occurrence index"; round 5): item -> the rows that hold it as seq / pos /
        # neg id, built on the host beside the batch and travelling with the ids -- a SLOT is [6 M ids | pad | index] -- so that the
        # item (and learned positional) table's gradient is an ordered gather inside cr_adam_step instead of float atomics from the
        # head and the embedding backward.  Off (CASTREC_NO_INDEX=1, row-sparse Adam, hidden sizes the gather does not take): the
        # atomics of rounds 1-4.
        ng, ent = C.c_int(0), C.c_int(0)                        # the gather's geometry at this hidden size (0: a size it does not take)
        self.use_index = bool(training and not self.lazy_adam and self.loss == "bce" and not sw.no_index
                              and L.lib.cr_tgrad_geometry(self.D, C.byref(ng), C.byref(ent)))
        self.ids_words = 6 * self.M
        self.index_off = (self.ids_words + 3) // 4 * 4
        self.index_lay, self._ixb = None, None
        if self.use_index:
            self.index_lay = L.IndexLayout()
            t_pos = self.T if "pos_emb" in self.layout.entries else 0
            L.check(L.lib.cr_batch_index_layout(self.M, itemnum + 1, t_pos, ng.value, ent.value, C.byref(self.index_lay)), "cr_batch_index_layout")
            self._ixb = L.lib.cr_index_builder_create(self.M, itemnum + 1, t_pos, ng.value, ent.value)
            if not self._ixb:
                raise MemoryError("cr_index_builder_create(%d, %d, %d)" % (self.M, itemnum + 1, t_pos))
            # workspace of the rows a batch cuts into slices (a hot item with more occurrences than one workgroup sums)
            self._tg_part = torch.zeros(self.index_lay.cap_blocks, (self.D + 3) // 4 * 4, dtype=torch.float32, device=self.dev)
            self._tg_tickets = torch.zeros(self.index_lay.cap_blocks, dtype=torch.int32, device=self.dev)
        self.slot_words = self.index_off + (int(self.index_lay.total_words) if self.use_index else 0) if self.use_index else self.ids_words
        self.batch_buf = torch.zeros(self.slot_words, **i32)
        self.ids_all = self.batch_buf[:self.ids_words].view(6, self.M)
        self.ids = {k: self.ids_all[i] for i, k in enumerate(self.ID_KEYS)}
        self._host_slot = np.zeros(self.slot_words, np.int32)          # host mirror of the static batch buffer (set_batch builds the index in it)
        self._tg_rows = None                                            # TgRows: the seq lookup's gradient rows
        self.bitwise_reproducible = self.use_index                      # no float atomics left in a step's gradients (loss sums apart)
        self.static_pe = torch.from_numpy(positional_encoding(self.D, self.T)).to(self.dev)
        self._build()
        self._finalize()
        self.graph = None
        self._id_ring, self._ring_next = None, None

    def _resolve_options(self, attn_precision, lazy_adam, loss, ce_negatives, gbce_t, ce_proposal, row_sparse_adam, fused, data_parallel):
        """The constructor's options (argument, else environment, else hp, else default) as attributes, and every refusal."""
        hp, training, itemnum = self.hp, self.training, self.itemnum
        if attn_precision is None:
            attn_precision = self.sw.attn_precision or getattr(hp, "attn_precision", None) or DEFAULT_ATTN_PRECISION
        if attn_precision not in ATTN_PRECISIONS:
            raise ValueError("attn_precision must be one of %s" % sorted(ATTN_PRECISIONS))
        self.attn_precision = attn_precision
        if attn_precision == "f32" and hp.hidden_units > 64:
            import warnings
            warnings.warn("attn_precision='f32' at hidden_units %d leaves the tuned path: the exact-fp32 row phases above 64 columns are "
                          "the unfused kernels (2.6x slower at the C4 shape, 11x at C5; profiles/r02d_other_shapes.log); the "
                          "fp32-grade default is 'bf16x3'" % hp.hidden_units, RuntimeWarning, stacklevel=3)
        # row-sparse Adam on the item table (DEVIATION from the reference's dense update, for tables like C5's 10 M rows;
        # castrec.h cr_adam_desc.lazy_ids): off unless asked for
        self.lazy_adam = self.sw.lazy_adam if lazy_adam is None else bool(lazy_adam)
        from_hp = lambda v, name, default: v if v is not None else (getattr(hp, name, None) or default)
        row_sparse_adam = bool(from_hp(row_sparse_adam, "row_sparse_adam", False))
        loss = from_hp(loss, "loss", "bce")
        if loss not in ALL_LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (ALL_LOSSES, loss))
        self.loss = loss if training else "bce"
        self.ce_negatives = int(from_hp(ce_negatives, "ce_negatives", 256))
        if gbce_t is None:
            gbce_t = getattr(hp, "gbce_t", None)
            gbce_t = 0.75 if gbce_t is None else gbce_t
        self.gbce_t = float(gbce_t)
        ce_proposal = from_hp(ce_proposal, "ce_proposal", "uniform")
        if ce_proposal not in CE_PROPOSALS:
            raise ValueError("ce_proposal must be one of %s, got %r" % (CE_PROPOSALS, ce_proposal))
        self.ce_proposal = ce_proposal if training else "uniform"
        if self.ce_proposal == "popularity" and self.loss != "sampled_ce":
            raise ValueError("ce_proposal='popularity' needs loss='sampled_ce', got loss=%r (gbce's beta is derived for uniform "
                             "sampling; bce and ce draw no shared negatives)" % self.loss)
        if self.loss in SOFTMAX_LOSSES:
            op = {"ce": "cr_softmax_ce", "sampled_ce": "cr_sampled_ce", "gbce": "cr_gbce"}[self.loss]
            if self.loss == "ce" and (self.lazy_adam or row_sparse_adam):
                raise ValueError("loss='%s' does not take row-sparse Adam (lazy_adam): every item row has a gradient" % self.loss)
            if self.lazy_adam:
                raise ValueError("loss='%s' does not take lazy_adam / CASTREC_LAZY_ADAM (its id list is seq | pos | neg: the step's samples "
                                 "have a gradient too); ask for row_sparse_adam=True, which lists them" % self.loss)
            if data_parallel:
                raise ValueError("loss='%s' does not take data parallelism (the item table's gradient is not in the exchanged bucket)"
                                 % self.loss)
            if not 8 <= hp.hidden_units <= 256:
                raise ValueError("loss='%s' needs 8 <= hidden_units <= 256 (%s), got %d" % (self.loss, op, hp.hidden_units))
        if self.loss in SAMPLED_LOSSES and not 1 <= self.ce_negatives <= L.CR_SCE_MAX_SAMPLES:
            raise ValueError("loss='%s' needs 1 <= ce_negatives <= %d (%s), got %d"
                             % (self.loss, L.CR_SCE_MAX_SAMPLES, op, self.ce_negatives))
        if self.loss == "gbce":
            if not 0.0 <= self.gbce_t <= 1.0:                      # (NaN fails too)
                raise ValueError("loss='gbce' needs 0 <= gbce_t <= 1, got %r" % (gbce_t,))
            # the sampling rate over the pool of negatives (the itemnum - 1 items that are not the target), gSASRec eq. for beta
            alpha = min(1.0, self.ce_negatives / max(1, itemnum - 1))
            self.gbce_beta = 1.0 - self.gbce_t * (1.0 - alpha)
        # the public spelling of the row-sparse update: from here on everything (dist.py, models.py, set_step) reads lazy_adam alone
        self.row_sparse_adam = row_sparse_adam
        if row_sparse_adam:
            self.lazy_adam = True
        # fused row-phase kernels (cr_block_*) need the hidden size to fit one 64-column tile
        self.fused = (4 <= hp.hidden_units <= 64) if fused is None else bool(fused)
        if self.fused and not 4 <= hp.hidden_units <= 64:
            raise ValueError("fused block kernels need 4 <= hidden_units <= 64")

    # ---- small helpers -------------------------------------------------------------------------
    def buf(self, name, cols, rows=None):
        if name not in self._bufs:
            self._bufs[name] = torch.zeros(self.M if rows is None else rows, cols, dtype=torch.float32, device=self.dev)
        return self._bufs[name]

    def vec(self, name, n=None):
        if name not in self._bufs:
            self._bufs[name] = torch.zeros(self.M if n is None else n, dtype=torch.float32, device=self.dev)
        return self._bufs[name]

    def p(self, name):
        return self.layout.view(self.P, name)

    def _pptr(self, name):
        off = self.layout.entries[name][0]
        return self.P.data_ptr() + 4 * off

    def _gptr(self, name):
        """slab-0 pointer of a dense parameter's gradient / pointer into Gt for a table parameter."""
        off, _, _, kind = self.layout.entries[name]
        if kind == "table":
            return self.Gt.data_ptr() + 4 * off
        return self.Gs.data_ptr() + 4 * (off - self.layout.n_table)

    def _acc(self, key):
        """Backward-time accumulate flag of a gradient buffer: False for its first writer."""
        first = key not in self._grad_written
        self._grad_written.add(key)
        return 0 if first else 1

    def _call(self, lst, name, *args):
        if name in ("cr_gemm_rows", "cr_gemm_wgrad"):
            # the unfused dense layers (hidden sizes above 64, the CAST mlp) follow the engine's matmul arithmetic
            for i in range(args[1]):
                args[0][i].precision = ATTN_PRECISIONS[self.attn_precision]
        if name == "cr_gemm_wgrad":
            args = args[:3] + (self.n_wslabs,)
            base = self.Gs.data_ptr()
            for i in range(args[1]):                      # the slab-0 float ranges this launch writes
                w = args[0][i]
                o = (w.dW - base) // 4
                self._wgrad_ranges += [(o + k * w.ldw, o + k * w.ldw + w.N) for k in range(w.K)]
                if w.db:
                    self._wgrad_ranges.append(((w.db - base) // 4, (w.db - base) // 4 + w.N))
        fn = getattr(L.lib, name)
        self._keep.append(args)
        lst.append((name, fn, args))
        return lst

    def rng(self, site_name, enabled=True):
        return self.drop.rng(site_id(site_name), enabled and self.training)

    # ---- graph pieces --------------------------------------------------------------------------
    def op_embed(self, ids_key, table, out, ld_out, col_off, scale, pos=None, addend=None, drop_site=None,
                 mask=False, small=False, into_stack=False):
        """modules.py:83-164 + the input composition of each graph. `addend`: a [M, D] buffer added to the looked-up rows.
        into_stack: `out` is the dense input of a transformer stack that follows immediately; on the fused path the
        gather then runs inside the first block's LN1 + QKV kernel (cr_block_ln_qkv_fwd_gather) instead of here."""
        V, D = self.layout.entries[table][1]
        pos_ptr = self.static_pe.data_ptr() if pos == "static" else self._pptr("pos_emb") if pos == "learned" else None
        has_add = addend is not None
        d_add = self._grad_of(addend) if has_add else None
        d = L.EmbedDesc(self.ids[ids_key].data_ptr(), self._pptr(table), self.M, self.T, D, V, 1, float(scale), pos_ptr,
                        addend.data_ptr() if has_add else None, addend.shape[1] if has_add else 0,
                        self.rng(drop_site) if drop_site else O.NO_DROP,
                        self.ids["seq"].data_ptr() if mask else None, out.data_ptr(), ld_out, col_off)
        if into_stack and self.fused and not self.sw.no_embed_fusion and ld_out == D and col_off == 0:
            self._pending_embed[out.data_ptr()] = d                  # emitted by the first block of op_stack
        else:
            self._call(self.fwd, "cr_embed_fwd", C.byref(d))
        if not self.training:
            return

        # the item table's seq lookup under the occurrence index: no table / positional gradient is scattered -- the masked,
        # dropped-out gradient rows are left in a row buffer for the gather (cr_adam_desc.tg / cr_table_grad)
        indexed = self.use_index and table == "item_emb" and ids_key == "seq"
        if indexed:
            assert not small and self._tg_rows is None, "one seq lookup of the item table per graph"

        def make_bwd_desc(in_block=False):
            f = L.EmbedDesc.from_buffer_copy(d)
            f.out = self._grad_of(out).data_ptr()
            dadd = None
            if has_add:
                assert self._acc(id(d_add)) == 0, "addend gradient must be first-written here"
                dadd = d_add.data_ptr()
            g2 = self._second_grad(out) if (ld_out == D and col_off == 0) else None   # a gradient in two partials: the kernels add them
            if indexed:
                if not in_block:
                    # cr_embed_bwd writes the rows as `d_addend` (the addend's gradient where the graph has one -- it IS the row --
                    # else a buffer of their own)
                    if has_add:
                        rows = d_add
                        assert rows.shape[1] % (4 if D % 4 == 0 else (2 if D % 2 == 0 else 1)) == 0
                    else:
                        rows = self.buf("item_rows", D)
                        f.ld_add = D
                        dadd = rows.data_ptr()
                    self._tg_rows = TgRows(rows, None, rows.shape[1], float(scale))
                return L.EmbedBwdDesc(f, None, None, dadd, 0, 0, g2.data_ptr() if g2 is not None else None)
            return L.EmbedBwdDesc(f, self._gptr(table), self._gptr("pos_emb") if pos == "learned" else None, dadd,
                                  self.Gs.shape[1] if small else 0, self.n_slabs if small else 0, g2.data_ptr() if g2 is not None else None)

        # the first block's QKV backward can apply this scatter itself (cr_block_ln_qkv_bwd_scatter): large-table
        # mode only (a learned positional table's gradient is then accumulated with atomics: its slot in the table
        # section is zero at that point); the block's factory (it runs before this one) claims it
        # (a small context table: only cr_stack_block_bwd takes it -- reduced in LDS, written as slabs -- and only with two slabs
        #  per sequence pair to write to)
        if (out.data_ptr() in self._pending_embed and (not has_add or addend.shape[1] == D)
                and (not small or (V <= 256 and D <= 64 and pos is None and self.n_slabs >= 2 * min(self.B, self.n_slabs)))):
            self._scatter_recipe[out.data_ptr()] = ScatterRecipe(make_bwd_desc, addend, small, table, indexed, float(scale))

        def factory():
            if out.data_ptr() in self._scatter_claimed:
                return []
            return self._call([], "cr_embed_bwd", C.byref(make_bwd_desc()))
        factory.pair_aware = ld_out == D and col_off == 0
        self._bwd_factories.append(factory)

    def _grad_of(self, t):
        """gradient buffer paired with activation buffer t (same shape), created on demand."""
        key = "d@%d" % t.data_ptr()
        if key not in self._bufs:
            self._bufs[key] = torch.zeros_like(t)
        return self._bufs[key]

    def _second_grad(self, t):
        """Second addend of the gradient of activation buffer t (or None), handed to a consumer that adds it itself."""
        return self._grad2.pop(t.data_ptr(), None)

    def _fold_pairs(self):
        """cr_eltwise launches that add every pending second addend into its gradient buffer: for consumers that read
        one gradient pointer."""
        lst = []
        for ptr, (t, g2) in list(self._grad2_bufs.items()):
            if ptr in self._grad2:
                g = self._grad_of(t)
                e = L.EltDesc(L.ELT_ADD, g.data_ptr(), g.shape[1], g2.data_ptr(), g2.shape[1], g.data_ptr(), g.shape[1], g.shape[0], g.shape[1],
                              O.NO_DROP, None, 0)
                self._call(lst, "cr_eltwise", C.byref(e))
                del self._grad2[ptr]
                if self._tg_rows is not None and self._tg_rows.rows is g and self._tg_rows.rows2 is g2:
                    # the occurrence index's row pair was this pair: g now holds the SUM (the add above is in place), so the gather
                    # reads one partial
                    self._tg_rows = self._tg_rows._replace(rows=g, rows2=None)
        return lst

    def op_layernorm(self, x, y, y_ld, y_col, pname, flags=None, skip_fwd=False):
        """modules.py:53-80.  y may be a column block of a wider (concat) buffer.  skip_fwd: the forward ran as the
        tail of the producing FFN kernel; only the backward is registered here."""
        M, D = self.M, self.D
        yptr = y.data_ptr() + 4 * y_col
        d = L.LnDesc(x.data_ptr(), D, self._pptr(pname + ".gamma"), self._pptr(pname + ".beta"), yptr, y_ld, M, D, 1e-8,
                     flags[0].data_ptr() if flags else None, flags[1].data_ptr() if flags else None)
        if not skip_fwd:
            self._call(self.fwd, "cr_layernorm_fwd", C.byref(d))
        if not self.training:
            return
        self._ln_recipe[yptr] = LnRecipe(x, pname)    # op_head may take this backward over (cr_head_fwd_bwd_ln)

        def factory():
            if yptr in self._ln_claimed or self._lnf_fused(x):
                return []
            dy, dx = self._grad_of(y), self._grad_of(x)
            bd = self._ln_bwd_desc(x, pname, dy.data_ptr() + 4 * y_col, y_ld, dx.data_ptr(), self._acc(id(dx)))
            return self._call([], "cr_layernorm_bwd", C.byref(bd))
        self._bwd_factories.append(factory)

    def _ln_bwd_desc(self, x, pname, dy_ptr, lddy, dx_ptr, accumulate):
        """Backward descriptor of the LayerNorm with parameters `pname` over the [M, D] rows of buffer x."""
        D = self.D
        return L.LnBwdDesc(x.data_ptr(), D, self._pptr(pname + ".gamma"), dy_ptr, lddy, dx_ptr, D, accumulate,
                           self._gptr(pname + ".gamma"), self._gptr(pname + ".beta"), self.Gs.shape[1], self.n_slabs, self.M, D, 1e-8)

    def _lnf_bwd_desc(self, y, dy):
        """(descriptor, intent) of the final LayerNorm behind block output y, for the block backward kernel that applies it on its way in."""
        it = self._lnf_intent[y.data_ptr()]
        dlo = self._grad_of(it.out)
        nd = self._ln_bwd_desc(y, it.pname, dlo.data_ptr() + 4 * it.col, it.ld, None, 0)
        assert id(dy) not in self._grad_written, "the final LayerNorm must be the only consumer of the stack's output"
        self._keep.append(nd)
        return nd, it

    def _lnf_fused(self, x):
        """True when the final LayerNorm behind buffer x has its backward applied inside the last block's (both factories ask)."""
        it = self._lnf_intent.get(x.data_ptr())
        return it is not None and it.yptr not in self._ln_claimed

    def op_dropout_inplace(self, c, ncols, site):
        """tf.layers.dropout on the first `ncols` columns of concat buffer c (cast_2.py:90-92, cast_4.py:115-124)."""
        ld = c.shape[1]
        d = L.EltDesc(L.ELT_DROPOUT, c.data_ptr(), ld, None, 0, c.data_ptr(), ld, self.M, ncols, self.rng(site), None, 0)
        self._call(self.fwd, "cr_eltwise", C.byref(d))
        if not self.training:
            return

        def factory():
            g = self._grad_of(c)
            bd = L.EltDesc(L.ELT_DROPOUT, g.data_ptr(), ld, None, 0, g.data_ptr(), ld, self.M, ncols, self.rng(site), None, 0)
            return self._call([], "cr_eltwise", C.byref(bd))
        self._bwd_factories.append(factory)

    def op_mlp(self, c, out, k, mask_out=False):
        """modules.py:321-335: relu(dense(relu(dense(c)))), widths kD -> kD -> D."""
        M, D = self.M, self.D
        K = k * D
        h = self.buf("mlp.h", K)
        self._gemm(self.fwd, c, self._pptr("mlp.w1"), K, h, K, K, bias=self._pptr("mlp.b1"), relu=True)
        self._gemm(self.fwd, h, self._pptr("mlp.w2"), D, out, D, K, bias=self._pptr("mlp.b2"), relu=True,
                   mask_ids=self.ids["seq"] if mask_out else None)
        if not self.training:
            return

        def factory():
            lst = []
            dout, dh, dc = self._grad_of(out), self._grad_of(h), self._grad_of(c)
            g2 = self.buf("mlp.g2", D)
            e = L.EltDesc(L.ELT_GRADPREP, dout.data_ptr(), out.shape[1], out.data_ptr(), out.shape[1], g2.data_ptr(), D, M, D,
                          O.NO_DROP, self.ids["seq"].data_ptr() if mask_out else None, 0)
            self._call(lst, "cr_eltwise", C.byref(e))
            self._gemm(lst, g2, self._pptr("mlp.w2"), D, dh, K, D, trans_b=True, accumulate=bool(self._acc(id(dh))))
            e2 = L.EltDesc(L.ELT_GRADPREP, dh.data_ptr(), K, h.data_ptr(), K, dh.data_ptr(), K, M, K, O.NO_DROP, None, 0)
            self._call(lst, "cr_eltwise", C.byref(e2))
            w = (L.WgradDesc * 2)(L.WgradDesc(h.data_ptr(), K, g2.data_ptr(), D, self._gptr("mlp.w2"), D, self._gptr("mlp.b2"), M, D, K),
                                  L.WgradDesc(c.data_ptr(), K, dh.data_ptr(), K, self._gptr("mlp.w1"), K, self._gptr("mlp.b1"), M, K, K))
            self._call(lst, "cr_gemm_wgrad", w, 2, self.Gs.shape[1], self.n_slabs)
            self._gemm(lst, dh, self._pptr("mlp.w1"), K, dc, K, K, trans_b=True, accumulate=bool(self._acc(id(dc))))
            return lst
        self._bwd_factories.append(factory)

    def _gemm(self, lst, A, B, ldb, Cm, N, K, bias=None, **kw):
        """One cr_gemm_rows launch: buffer Cm[M, N] = buffer A[M, K] x the weight at pointer B, pitch ldb; kw: O.gemm_desc's epilogue."""
        d = O.gemm_desc(A, A.shape[1], None, ldb, Cm, Cm.shape[1], self.M, N, K, **kw)
        d.B, d.bias = B, bias
        self._call(lst, "cr_gemm_rows", (L.GemmDesc * 1)(d), 1)

    def op_block(self, x, y, pfx, attn_out=None, skip_qkv=False, tail=None, collect=None):
        """One transformer block (sasrec.py:65-83): y = mask * FFN(LN2(MHA(LN1(x), x))), by one of three routes, each of which emits
        the forward and registers the backward: fused (hidden sizes 4..64), wide (128 / 192 / 256 on bf16 arithmetic), unfused.
        Fused and wide: `skip_qkv` = the LN1 + QKV phase was run as the tail of the previous block's FFN kernel; `tail`: a Tail.
        Fused: `collect` = a list: no forward is emitted; (block desc, attention desc) is appended for op_stack's cr_stack_fwd launch."""
        b = self._block_bufs(pfx)
        bd = self._block_desc(x, y, pfx, b)
        ad = self._attn_desc(pfx, b, attn_out)
        if self.fused:
            return self._block_fused(x, y, pfx, bd, ad, skip_qkv, tail, collect)
        prec = ad.precision
        if self.training and prec != L.PREC_F32:
            # the bf16-MFMA backward recomputes the probabilities from the forward's row statistics
            ad.row_stats = self.vec(pfx + "row_stats", self.H * self.B * self.T * 4).data_ptr()
        if not self.sw.no_wide and prec != L.PREC_F32 and L.lib.cr_wide_supported(C.byref(bd), prec):
            return self._block_wide(x, y, pfx, b, bd, ad, skip_qkv, tail)
        assert not skip_qkv and tail is None, "tails need the fused or the wide (D = 128) row kernels"
        return self._block_unfused(x, y, pfx, b, ad)

    def _block_bufs(self, pfx):
        D = self.D
        return BlockBufs(*(self.buf(pfx + n, D) for n in ("q_in", "o", "f_in", "hid")), self.buf(pfx + "qkv", D, rows=3 * self.M),
                         self.vec(pfx + "kvalid"), self.vec(pfx + "qvalid"))

    def _block_desc(self, x, y, pfx, b):
        """cr_block_desc of the block with parameter prefix `pfx` and buffers b."""
        bufs = (x, b.q_in, b.qkv, b.kvalid, b.qvalid, b.o, b.f_in, b.hid, y, self.ids["seq"])
        return L.BlockDesc(self.M, self.D, *(self._pptr(pfx + n) for n in BLOCK_PARAMS), *(t.data_ptr() for t in bufs),
                           self.rng(pfx[:-1] + ".ffn1"), self.rng(pfx[:-1] + ".ffn2"))

    def _attn_desc(self, pfx, b, attn_out):
        """Attention core of a block (modules.py:208-269) over its [3, M, D] qkv buffer, residual = queries."""
        D, H, MD4 = self.D, self.H, 4 * self.M * self.D
        ad = O.attn_desc(b.qkv, None, None, D, b.kvalid, b.qvalid, b.q_in, D, b.o, D, self.B, self.T, H, D // H,
                         rng=self.rng(pfx + "attn"), batch_global=self.batch_global,
                         dead_ids=None if attn_out is not None else self.ids["seq"], attn_weights=attn_out)
        ad.K, ad.V = b.qkv.data_ptr() + MD4, b.qkv.data_ptr() + 2 * MD4
        ad.precision = ATTN_PRECISIONS[self.attn_precision]
        return ad

    def _tail_desc(self, y, tail):
        """cr_block_tail_desc of a Tail behind the block with output y."""
        if tail.kind == "next":
            nbd = self._block_desc(y, tail.out, tail.pname, self._block_bufs(tail.pname))
            self._keep.append(nbd)
            return L.BlockTailDesc(1, C.pointer(nbd), None, None, None, 0, 0)
        return L.BlockTailDesc(2, None, self._pptr(tail.pname + ".gamma"), self._pptr(tail.pname + ".beta"), tail.out.data_ptr(),
                               tail.ld, tail.col)

    def _attn_bwd_desc(self, ad, pfx, do):
        """cr_attn_bwd_desc of a block: d_o -> dQ | dK | dV, the [3, M, D] rows of its dqkv buffer."""
        M, D, MD4 = self.M, self.D, 4 * self.M * self.D
        dqkv = self.buf(pfx + "dqkv", D, rows=3 * M)
        stats = self.vec(pfx + "stats", self.H * self.B * self.T * 4)
        return L.AttnBwdDesc(L.AttnDesc.from_buffer_copy(ad), do.data_ptr(), D, dqkv.data_ptr(), dqkv.data_ptr() + MD4,
                             dqkv.data_ptr() + 2 * MD4, D, stats.data_ptr())

    def _block_bwd_desc(self, bd, pfx, dy, abd, dx):
        """cr_block_bwd_desc of a block beside its attention backward abd: dy -> d_o, dQ | dK | dV -> dx (first writer of dx or not)."""
        return L.BlockBwdDesc(L.BlockDesc.from_buffer_copy(bd), dy.data_ptr(), abd.dout, abd.dQ, dx.data_ptr(), self._acc(id(dx)),
                              *(self._gptr(pfx + n) for n in BLOCK_PARAMS), self.Gs.shape[1], self.n_slabs)

    def _ffn_wgrad(self, lst, pfx, b, g2, g1):
        """dW2, db2, dW1, db1 of a block by cr_gemm_wgrad."""
        M, D, G = self.M, self.D, self._gptr
        w = (L.WgradDesc * 2)(L.WgradDesc(b.hid.data_ptr(), D, g2.data_ptr(), D, G(pfx + "w2"), D, G(pfx + "b2"), M, D, D),
                              L.WgradDesc(b.f_in.data_ptr(), D, g1.data_ptr(), D, G(pfx + "w1"), D, G(pfx + "b1"), M, D, D))
        self._call(lst, "cr_gemm_wgrad", w, 2, self.Gs.shape[1], self.n_slabs)

    def _qkv_wgrad(self, lst, pfx, b, x, abd):
        """dWq, dbq ; dWk, dbk ; dWv, dbv of a block by cr_gemm_wgrad (column blocks of the fused [D, 3D] weight gradient)."""
        M, D = self.M, self.D
        gw, gb = self._gptr(pfx + "wqkv"), self._gptr(pfx + "bqkv")
        w = (L.WgradDesc * 3)(L.WgradDesc(b.q_in.data_ptr(), D, abd.dQ, D, gw, 3 * D, gb, M, D, D),
                              L.WgradDesc(x.data_ptr(), D, abd.dK, D, gw + 4 * D, 3 * D, gb + 4 * D, M, D, D),
                              L.WgradDesc(x.data_ptr(), D, abd.dV, D, gw + 8 * D, 3 * D, gb + 8 * D, M, D, D))
        self._call(lst, "cr_gemm_wgrad", w, 3, self.Gs.shape[1], self.n_slabs)

    def _block_unfused(self, x, y, pfx, b, ad):
        """The block as the chain cr_layernorm_* / cr_gemm_rows / cr_attn_* / cr_eltwise (any hidden size, exact fp32 above 64)."""
        M, D, P, ids = self.M, self.D, self._pptr, self.ids["seq"]
        wqkv = P(pfx + "wqkv")
        # LN1 (+ data-dependent key / query masks, modules.py:222,248-249)
        ln1 = L.LnDesc(x.data_ptr(), D, P(pfx + "ln1.gamma"), P(pfx + "ln1.beta"), b.q_in.data_ptr(), D, M, D,
                       1e-8, b.kvalid.data_ptr(), b.qvalid.data_ptr())
        self._call(self.fwd, "cr_layernorm_fwd", C.byref(ln1))
        # Q = LN1(x) Wq + bq ; K = x Wk + bk ; V = x Wv + bv   (modules.py:203-205), one batched launch
        gs = []
        for part, src in enumerate((b.q_in, x, x)):
            gd = O.gemm_desc(src, D, None, 3 * D, None, D, M, D, D)
            gd.B, gd.bias, gd.C = wqkv + 4 * part * D, P(pfx + "bqkv") + 4 * part * D, b.qkv.data_ptr() + part * 4 * M * D
            gs.append(gd)
        self._call(self.fwd, "cr_gemm_rows", (L.GemmDesc * 3)(*gs), 3)
        self._call(self.fwd, "cr_attn_fwd", C.byref(ad))
        # LN2 + FFN (modules.py:280-318), residual = LN2 output, then * mask (sasrec.py:83)
        ln2 = L.LnDesc(b.o.data_ptr(), D, P(pfx + "ln2.gamma"), P(pfx + "ln2.beta"), b.f_in.data_ptr(), D, M, D, 1e-8, None, None)
        self._call(self.fwd, "cr_layernorm_fwd", C.byref(ln2))
        self._gemm(self.fwd, b.f_in, P(pfx + "w1"), D, b.hid, D, D, bias=P(pfx + "b1"), relu=True, rng=self.rng(pfx[:-1] + ".ffn1"))
        self._gemm(self.fwd, b.hid, P(pfx + "w2"), D, y, D, D, bias=P(pfx + "b2"), rng=self.rng(pfx[:-1] + ".ffn2"), residual=b.f_in, ldr=D,
                   mask_ids=ids)
        if not self.training:
            return

        def factory():
            lst = []
            dy, dx = self._grad_of(y), self._grad_of(x)
            g2, g1, df, do, dq_in = (self.buf(pfx + n, D) for n in ("g2", "g1", "df", "do", "dq_in"))
            abd = self._attn_bwd_desc(ad, pfx, do)
            # (a) gradient wrt FFN2 pre-dropout output: dy * mask * keep/(1-rate)
            e = L.EltDesc(L.ELT_GRADPREP, dy.data_ptr(), D, None, 0, g2.data_ptr(), D, M, D, self.rng(pfx[:-1] + ".ffn2"), ids.data_ptr(), 0)
            self._call(lst, "cr_eltwise", C.byref(e))
            # (b) dhid = g2 W2^T ; (c) gate by the stored post-dropout ReLU output
            self._gemm(lst, g2, P(pfx + "w2"), D, g1, D, D, trans_b=True)
            e1 = L.EltDesc(L.ELT_GRADPREP, g1.data_ptr(), D, b.hid.data_ptr(), D, g1.data_ptr(), D, M, D, self.rng(pfx[:-1] + ".ffn1"), None, 0)
            self._call(lst, "cr_eltwise", C.byref(e1))
            # (d) dW2, db2, dW1, db1
            self._ffn_wgrad(lst, pfx, b, g2, g1)
            # (e) df_in = (g1 W1^T + dy) * mask     (residual branch of modules.py:313)
            self._gemm(lst, g1, P(pfx + "w1"), D, df, D, D, trans_b=True, residual=dy, ldr=D, mask_ids=ids)
            # (f) LN2 backward -> do
            self._call(lst, "cr_layernorm_bwd", C.byref(self._ln_bwd_desc(b.o, pfx + "ln2", df.data_ptr(), D, do.data_ptr(), 0)))
            # (g) attention backward -> dQ | dK | dV ; (h) their weight gradients
            self._call(lst, "cr_attn_bwd", C.byref(abd))
            self._qkv_wgrad(lst, pfx, b, x, abd)
            # (i) dq_in = dQ Wq^T + do (residual, modules.py:269) ; dx (+)= dK Wk^T, then dx += dV Wv^T
            bq = O.gemm_desc(None, D, None, 3 * D, dq_in, D, M, D, D, trans_b=True, residual=do, ldr=D)
            bq.A, bq.B = abd.dQ, wqkv
            bk = O.gemm_desc(None, D, None, 3 * D, dx, D, M, D, D, trans_b=True, accumulate=bool(self._acc(id(dx))))
            bk.A, bk.B = abd.dK, wqkv + 4 * D
            self._call(lst, "cr_gemm_rows", (L.GemmDesc * 2)(bq, bk), 2)
            bv = O.gemm_desc(None, D, None, 3 * D, dx, D, M, D, D, trans_b=True, accumulate=True)
            bv.A, bv.B = abd.dV, wqkv + 8 * D
            self._call(lst, "cr_gemm_rows", (L.GemmDesc * 1)(bv), 1)
            # (j) LN1 backward accumulates into dx
            self._call(lst, "cr_layernorm_bwd", C.byref(self._ln_bwd_desc(x, pfx + "ln1", dq_in.data_ptr(), D, dx.data_ptr(), 1)))
            return lst
        self._bwd_factories.append(factory)

    def _block_wide(self, x, y, pfx, b, bd, ad, skip_qkv, tail):
        """Hidden sizes 128 / 192 / 256 on bf16 arithmetic: the row phases as ONE launch each (cr_wide.hip)."""
        D, H, T, prec = self.D, self.H, self.T, ad.precision
        if not skip_qkv:                                  # (else: ran as the tail of the previous block's FFN kernel)
            self._call(self.fwd, "cr_wide_ln_qkv_fwd", C.byref(bd), prec)
        self._call(self.fwd, "cr_attn_fwd", C.byref(ad))
        if tail is None:
            self._call(self.fwd, "cr_wide_ln_ffn_fwd", C.byref(bd), prec)
        else:
            self._call(self.fwd, "cr_wide_ln_ffn_fwd_tail", C.byref(bd), C.byref(self._tail_desc(y, tail)), prec)
        if not self.training:
            return

        def factory():
            lst = []
            dy, dx = self._grad_of(y), self._grad_of(x)
            g2, g1, df, do, dq_in = (self.buf(pfx + n, D) for n in ("g2", "g1", "df", "do", "dq_in"))     # (df, dq_in: not read here; kept in eng._bufs)
            abd = self._attn_bwd_desc(ad, pfx, do)
            bbd = self._block_bwd_desc(bd, pfx, dy, abd, dx)
            # dy -> g2, g1, d_o, slabs of dgamma2 dbeta2 (and dW2 db2 dW1 db1 unless left to cr_gemm_wgrad)
            # (the kernels form the weight gradients themselves at D = 128: a [D, D] slab per 128 rows is what an activation
            #  row block costs; at 192 / 256 the slab of a 64-row block is 4 x its rows, and cr_gemm_wgrad reduces more rows
            #  per slab)
            own_w = D == 128 and not self.sw.wide_no_wgrad
            if not own_w:
                bbd.g_w1 = bbd.g_b1 = bbd.g_w2 = bbd.g_b2 = bbd.g_wqkv = bbd.g_bqkv = None
            # The one-launch attention backward (both passes side by side, tiles dealt to eight waves) needs the per-head row
            # term delta up front; the FFN backward emits it (it reads o and q_in once more for that).  C4 shape: 1.136 ->
            # 1.094 ms per step since the fused kernel deals its tiles by iteration count (before that: equal).
            dh = D // H
            fuse_attn = T <= 256 and 8 <= dh <= 64 and dh % 16 == 0 and not self.sw.wide_no_delta and not self.sw.bf_two_kernels
            if fuse_attn:
                bbd.attn_delta = abd.delta = self.vec("attn_delta_heads", H * self.M).data_ptr()
            self._call(lst, "cr_wide_ln_ffn_bwd", C.byref(bbd), g2.data_ptr(), g1.data_ptr(), H if fuse_attn else 0, prec)
            if not own_w:
                self._ffn_wgrad(lst, pfx, b, g2, g1)
            self._call(lst, "cr_attn_bwd", C.byref(abd))
            if not own_w:
                self._qkv_wgrad(lst, pfx, b, x, abd)
            # (dQ | dK | dV, d_o) -> dx (+ dgamma1 / dbeta1 slabs)
            self._call(lst, "cr_wide_ln_qkv_bwd", C.byref(bbd), prec)
            return lst
        self._bwd_factories.append(factory)

    def _block_fused(self, x, y, pfx, bd, ad, skip_qkv, tail, collect):
        """Hidden sizes 4..64 through the fused row-phase kernels (cr_block_*): 3 launches forward; with tails (the next block's
        LN1 + QKV, or the stack's final LayerNorm, inside the FFN kernel) 2; collected for cr_stack_fwd none of its own.  The
        backward is the same in every case: one launch (cr_stack_block_bwd) where the kernel takes the block, else three."""
        D, H, B, T = self.D, self.H, self.B, self.T
        if not skip_qkv and collect is None:
            e = self._pending_embed.pop(x.data_ptr(), None)
            if e is not None:
                self._keep.append(e)
                self._call(self.fwd, "cr_block_ln_qkv_fwd_gather", C.byref(bd), C.byref(e))
            else:
                self._call(self.fwd, "cr_block_ln_qkv_fwd", C.byref(bd))
        # single-pass attention backward (H = 1): the forward saves its row statistics, the FFN backward emits
        # delta, the attention backward returns dQ as two partials that the QKV backward adds
        prec = ad.precision
        bf = prec != L.PREC_F32 and 8 <= D // H <= 64 and T <= 1024     # shapes the bf16-MFMA kernels take
        one_pass = self.training and H == 1 and not self.sw.two_pass_attn_bwd and not bf
        if one_pass or (self.training and bf):
            ad.row_stats = self.vec(pfx + "row_stats", H * B * T * 4).data_ptr()
        if collect is not None:
            collect.append((bd, ad))
        else:
            self._call(self.fwd, "cr_attn_fwd", C.byref(ad))
            if tail is None:
                self._call(self.fwd, "cr_block_ln_ffn_fwd", C.byref(bd))
            else:
                self._call(self.fwd, "cr_block_ln_ffn_fwd_tail", C.byref(bd), C.byref(self._tail_desc(y, tail)))
        if not self.training:
            return

        def factory():
            dy, dx = self._grad_of(y), self._grad_of(x)
            abd = self._attn_bwd_desc(ad, pfx, self.buf(pfx + "do", D))
            bbd = self._block_bwd_desc(bd, pfx, dy, abd, dx)
            if one_pass or (bf and H == 1):
                # one head: the FFN backward emits delta (its row sum IS the head's; shared between the blocks: consumed within the
                # same block); with it the bf16-MFMA backward runs both passes side by side in one launch and dQ comes back whole
                bbd.attn_delta = abd.delta = self.vec("attn_delta", self.M).data_ptr()
            if one_pass:
                bbd.dq_part = abd.dQ_part = self.buf("attn_dq_part", D).data_ptr()
            # bf16 arithmetic: the row phases run on the register-layout kernels (cr_stack_bwd.hip) where they take the shape
            rows_bf = bool(not self.sw.no_stack_bwd and bf and not one_pass and L.lib.cr_stack_bwd_supported(C.byref(bbd), B, T, prec))
            # ... and where the whole block fits one launch (cr_stack_bwd1.hip: one head, D < 64): ffn_bwd -> attn_bwd -> qkv_bwd per
            # sequence on a pair of workgroups; the input gradient leaves as two partials (dx, dx2)
            if (rows_bf and not self.sw.no_block_bwd and (H == 1 or (H == 2 and D == 64))
                    and L.lib.cr_stack_block_bwd_supported(C.byref(bbd), C.byref(abd.f), B, T, prec)):
                return self._block_bwd_one_launch(x, y, pfx, bbd, abd, dy, dx)
            return self._block_bwd_three_launches(x, y, bbd, abd, dy, rows_bf)
        factory.pair_aware = True                      # (takes dy2 where it can; any other pending pair is not its input)
        self._bwd_factories.append(factory)

    def _block_bwd_one_launch(self, x, y, pfx, bbd, abd, dy, dx):
        """cr_stack_block_bwd: the whole block, with the final LayerNorm behind it and the embedding scatter in front of it where
        the graph has them there.  Gradients arrive and leave as two partials each (BlockBwd1Ext)."""
        D, B, T = self.D, self.B, self.T
        dx2 = self.buf(pfx + "dx2", D)
        dy2 = self._second_grad(y)
        ext = L.BlockBwd1Ext(dy2.data_ptr() if dy2 is not None else None, dx2.data_ptr(), None, None)
        nd = None
        if self._lnf_fused(y):
            nd, it = self._lnf_bwd_desc(y, dy)
            assert dy2 is None, "the final LayerNorm must be the only consumer of the stack's output"
            dlo2 = self._second_grad(it.out)
            if dlo2 is not None:
                assert dlo2.shape == it.out.shape
                ext.lnf_dy2 = dlo2.data_ptr() + 4 * it.col
            self._block_slab_range(it.pname + ".gamma", it.pname + ".beta")
        sc = None
        rec = self._scatter_recipe.get(x.data_ptr())
        if rec is not None and not bbd.dx_accumulate:
            self._scatter_claimed.add(x.data_ptr())
            sc = rec.make_desc(in_block=rec.indexed)
            if rec.small:                                          # small table: two slabs per sequence pair
                self._block_slab_range(rec.table, rec.table, 2 * min(self.B, self.n_slabs))
            dadd2 = None
            if sc.d_addend:
                dadd2 = self.buf(pfx + "dadd2", D)
                ext.d_addend2 = dadd2.data_ptr()
                self._grad2[rec.addend.data_ptr()] = dadd2         # the addend's gradient is d_addend + d_addend2
                self._grad2_bufs[rec.addend.data_ptr()] = (rec.addend, dadd2)
            if rec.indexed:
                # occurrence index: the kernel leaves the two masked partials of the input gradient where they wait (the
                # addend's gradient pair, else dx / dx2) and scatters nothing; cr_adam_step gathers scale * (rows + rows2)
                self._tg_rows = TgRows(self._grad_of(rec.addend), dadd2, D, rec.scale) if sc.d_addend else TgRows(dx, dx2, D, rec.scale)
            self._keep.append(sc)
        else:
            self._grad2[x.data_ptr()] = dx2                       # the block input's gradient is dx + dx2
            self._grad2_bufs[x.data_ptr()] = (x, dx2)
        self._keep.append(ext)
        self._block_slab_range(pfx + "ln1.gamma", pfx + "b2")
        return self._call([], "cr_stack_block_bwd", C.byref(bbd), C.byref(abd.f), C.byref(ext), C.byref(nd) if nd is not None else None,
                          C.byref(sc) if sc is not None else None, B, T, abd.f.precision)

    def _block_bwd_three_launches(self, x, y, bbd, abd, dy, rows_bf):
        """FFN backward, attention backward, QKV backward as a launch each: the register-layout kernels (cr_stack_*_bwd*) where
        rows_bf says they take the shape, else the tile kernels (cr_block_ln_*_bwd*)."""
        D, H, B, T, prec = self.D, self.H, self.B, self.T, abd.f.precision
        lst = self._fold_pairs()                               # the kernels below read one gradient pointer
        two_heads = rows_bf and H == 2 and D == 64 and T <= 256 and not self.sw.bf_two_kernels and not self.sw.no_head_delta
        if two_heads:
            # config C3's shape: the register-layout FFN backward emits delta per head ([2, M]), so the attention backward is
            # ONE launch here too
            bbd.attn_delta = abd.delta = self.vec("attn_delta_heads", H * self.M).data_ptr()
        nd = self._lnf_bwd_desc(y, dy)[0] if rows_bf and self._lnf_fused(y) else None
        if two_heads:
            self._call(lst, "cr_stack_ffn_bwd_heads", C.byref(bbd), C.byref(nd) if nd is not None else None, B, T, H, prec)
        elif nd is not None:
            self._call(lst, "cr_stack_ffn_bwd_ln", C.byref(bbd), C.byref(nd), B, T, prec)
        elif rows_bf:
            self._call(lst, "cr_stack_ffn_bwd", C.byref(bbd), B, T, prec)
        else:
            assert not self._lnf_fused(y), "final LayerNorm backward was left to a kernel that does not take it"
            self._call(lst, "cr_block_ln_ffn_bwd", C.byref(bbd))
        self._call(lst, "cr_attn_bwd", C.byref(abd))
        # the embedding scatter of the block's input: the atomic scatter of a large table only (indexed: cr_embed_bwd leaves the
        # rows; a small table: only cr_stack_block_bwd takes it)
        rec = self._scatter_recipe.get(x.data_ptr())
        if rec is not None and not rec.indexed and not rec.small and not bbd.dx_accumulate:
            self._scatter_claimed.add(x.data_ptr())
            if rows_bf:
                self._call(lst, "cr_stack_qkv_bwd_scatter", C.byref(bbd), C.byref(rec.make_desc()), B, T, prec)
            else:
                self._call(lst, "cr_block_ln_qkv_bwd_scatter", C.byref(bbd), C.byref(rec.make_desc()))
        elif rows_bf:
            self._call(lst, "cr_stack_qkv_bwd", C.byref(bbd), B, T, prec)
        else:
            self._call(lst, "cr_block_ln_qkv_bwd", C.byref(bbd))
        return lst

    def _block_slab_range(self, first, last, count=None):
        """Parameters first..last (contiguous in the layout) get their gradient from cr_stack_block_bwd: one slab per sequence
        pair, min(B, n_slabs) slabs in use (cr_adam_desc.slab_counts); `count`: another number of slabs."""
        a = self.layout.entries[first][0] - self.layout.n_table
        off, shape, _, _ = self.layout.entries[last]
        self._block_bwd_ranges.append((a, off + int(np.prod(shape)) - self.layout.n_table, min(self.B, self.n_slabs) if count is None else count))

    def _stack_kernel_fits(self, nblocks, want_attn):
        """Shapes cr_stack_fwd takes (castrec.h): one head (or two of 32 columns), D 8..64, bf16 arithmetic, K / V images +
        weights within the LDS."""
        heads_ok = self.H == 1 or (self.H == 2 and self.D == 64)          # two heads: head dim 32 = one k-step of the score product
        if not (self.fused and not self.sw.no_stack_kernel and nblocks >= 1 and not want_attn and heads_ok and 8 <= self.D <= 64):
            return False
        if self.attn_precision == "f32" or self.T > 256:
            return False
        T16, split = (self.T + 15) // 16 * 16, self.attn_precision == "bf16x3"
        lds = T16 * 64 * 2 * (4 if split else 2) + 3 * 4096 * 2 * (2 if split else 1) + 11 * 64 * 4 + T16 * 4
        if T16 > 208 and (split or self.H != 1):                 # more than 13 tiles: plain bf16, one head (castrec.h)
            return False
        return lds <= 160 * 1024

    def op_stack(self, x, prefix, nblocks, out, out_ld, out_col, want_attn=False):
        """block loop + final LayerNorm (sasrec.py:65-85); returns nothing, writes `out` columns.
        Fused path: block i+1's LN1 + QKV phase and the final LayerNorm run as tails of the FFN kernels; where the
        whole-stack kernel fits (cr_stack_fwd) the forward of up to four blocks + the final LayerNorm is ONE launch."""
        # (the wide row kernels take the same tails at D = 128: cr_wide_ln_ffn_fwd_tail)
        sw = self.sw
        wide_tails = not self.fused and not sw.no_wide and self.attn_precision != "f32" and self.D == 128 and not sw.wide_no_tails
        tails = (self.fused or wide_tails) and not sw.no_tails and nblocks > 0
        stack = self._stack_kernel_fits(nblocks, want_attn)
        emb = None
        if stack and x.data_ptr() in self._pending_embed:                # the stack kernel composes its input itself
            emb = self._pending_embed.pop(x.data_ptr())
        if nblocks == 0 and x.data_ptr() in self._pending_embed:         # no block kernel to carry the gather
            self._call(self.fwd, "cr_embed_fwd", C.byref(self._pending_embed.pop(x.data_ptr())))
        ys = [self.buf("%s.%d.y" % (prefix, i), self.D) for i in range(nblocks)]
        cur = x
        collect = [] if stack else None
        for i in range(nblocks):
            nxt = ys[i]
            aw = None
            if want_attn and i == nblocks - 1:
                aw = self.attn_weights = torch.zeros(self.H * self.B, self.T, self.T, dtype=torch.float32, device=self.dev)
            tail = None
            if tails:
                tail = Tail("next", "%s.%d." % (prefix, i + 1), ys[i + 1]) if i + 1 < nblocks else Tail("lnf", prefix + ".lnf", out, out_ld, out_col)
            self.op_block(cur, nxt, "%s.%d." % (prefix, i), attn_out=aw, skip_qkv=tails and i > 0, tail=tail, collect=collect)
            cur = nxt
        if stack:
            for i0 in range(0, nblocks, 4):
                part = collect[i0:i0 + 4]
                bds = (L.BlockDesc * len(part))(*[bd for bd, _ in part])
                ads = (L.AttnDesc * len(part))(*[ad for _, ad in part])
                fin = i0 + 4 >= nblocks
                sd = L.StackDesc(len(part), C.cast(bds, C.POINTER(L.BlockDesc)), C.cast(ads, C.POINTER(L.AttnDesc)),
                                 self._pptr(prefix + ".lnf.gamma") if fin else None, self._pptr(prefix + ".lnf.beta") if fin else None,
                                 out.data_ptr() if fin else None, out_ld, out_col,
                                 C.pointer(emb) if (emb is not None and i0 == 0) else None)
                self._keep.append(emb)
                if not L.lib.cr_stack_fwd_supported(C.byref(sd)):
                    raise RuntimeError("cr_stack_fwd does not take the stack %s it was sized for" % prefix)
                self._keep.append((bds, ads))
                self._call(self.fwd, "cr_stack_fwd", C.byref(sd))
        if stack and self.training and not sw.no_stack_bwd and self.D <= 64 and self.T <= 224 and not sw.no_lnf_fusion:
            # the register-layout FFN backward of the last block can apply this LayerNorm's backward on its way in
            self._lnf_intent[cur.data_ptr()] = LnfIntent(out.data_ptr() + 4 * out_col, prefix + ".lnf", out, out_ld, out_col)
        self.op_layernorm(cur, out, out_ld, out_col, prefix + ".lnf", skip_fwd=tails or stack)

    def op_head(self, seq_emb):
        """sasrec.py:87-115 (+ unnormalised gradients) / test_logits sasrec.py:93-97."""
        M, D = self.M, self.D
        self.seq_emb = seq_emb
        if not self.training:
            return
        if self.loss in SOFTMAX_LOSSES:
            # softmax cross-entropy: d(seq_emb) is stored (the final LayerNorm's / the MLP's backward reads it), the item table's
            # gradient goes into Gt -- the head route of CASTREC_NO_HEAD_LN=1 with CASTREC_NO_INDEX=1.  "ce" takes the whole
            # catalogue; "sampled_ce" draws its N samples on the device from (seed, state[4]), so every step (captured graphs and the
            # fed multi-step path included) draws its own
            ds = self._grad_of(seq_emb)
            self._grad_written.add(id(ds))
            prec = L.PREC_BF16 if self.attn_precision == "bf16" else L.PREC_BF16X3
            state = self.state.data_ptr()
            head = (seq_emb.data_ptr(), seq_emb.shape[1], self._pptr("item_emb"), self.ids["pos"].data_ptr(), self.ids["neg"].data_ptr(),
                    M, D, self.itemnum + 1)
            tail = (state, ds.data_ptr(), ds.shape[1], self._gptr("item_emb"), None, self._ce_ws.data_ptr(), self._ce_ws.numel())
            if self.loss == "ce":
                return self._call(self.fwd, "cr_softmax_ce", C.byref(L.SoftmaxCeDesc(*head, prec, *tail)))
            draw = (None, self.seed & 0xFFFFFFFF, state + 16, self.samples.data_ptr())       # no ids handed in: drawn from (seed, step)
            if self.loss == "gbce":
                return self._call(self.fwd, "cr_gbce", C.byref(L.GbceDesc(*head, self.ce_negatives, prec, self.gbce_beta, *draw, *tail)))
            pop = self.ce_proposal == "popularity"
            d = L.SampledCeDesc(*head, self.ce_negatives, prec, *draw, *tail,
                                self.item_cdf.data_ptr() if pop else None, self.item_logq.data_ptr() if pop else None)
            return self._call(self.fwd, "cr_sampled_ce", C.byref(d))
        rec = self._ln_recipe.get(seq_emb.data_ptr()) if not self.sw.no_head_ln else None
        dx = ds = self._grad_of(rec.x if rec is not None else seq_emb)      # (allocated in front of head.coef, as ever: buffer order)
        d = L.HeadDesc(seq_emb.data_ptr(), seq_emb.shape[1], self._pptr("item_emb"), self.ids["pos"].data_ptr(),
                       self.ids["neg"].data_ptr(), M, D, self.itemnum + 1, self.state.data_ptr(), None, 0,
                       None if self.use_index else self._gptr("item_emb"), None, None, self._head_coef())
        if rec is not None:
            # seq_emb is the output of a LayerNorm (the stack's final one): its backward runs inside the head kernel,
            # on the gradient rows while they are in registers; d(seq_emb) is never stored
            assert self._acc(id(dx)) == 0
            self._ln_claimed.add(seq_emb.data_ptr())
            n = self._ln_bwd_desc(rec.x, rec.pname, None, 0, dx.data_ptr(), 0)
            # the head as the tail of the stack's last forward launch (cr_stack_fwd_head): no launch of its own.  Needs the occurrence
            # index (nothing is scattered from there) and the launch form with two workgroups per sequence.
            sd = self._stack_desc(self.fwd[-1]) if self.fwd else None
            if (self.use_index and sd is not None and not self.sw.no_head_fusion and sd.out == seq_emb.data_ptr()
                    and L.lib.cr_stack_fwd_head_supported(C.byref(sd), C.byref(d), C.byref(n))):
                self._keep += [d, n]
                self.fwd[-1] = ("cr_stack_fwd_head", L.lib.cr_stack_fwd_head, (C.byref(sd), C.byref(d), C.byref(n)))
                self._block_slab_range(rec.pname + ".gamma", rec.pname + ".beta", 2 * self.B)      # workgroup (sequence, half) writes slab half * B + sequence
                return
            self._call(self.fwd, "cr_head_fwd_bwd_ln", C.byref(d), C.byref(n))
            return
        self._grad_written.add(id(ds))
        d.d_seq_emb, d.ldd = ds.data_ptr(), ds.shape[1]
        self._call(self.fwd, "cr_head_fwd_bwd", C.byref(d))

    @staticmethod
    def _stack_desc(entry):
        """The cr_stack_desc of a cr_stack_fwd / cr_stack_fwd_head launch entry; None for any other entry."""
        return entry[2][0]._obj if entry[0] in ("cr_stack_fwd", "cr_stack_fwd_head") else None

    @staticmethod
    def _scatter_desc(entry):
        """The embedding scatter (EmbedBwdDesc) a backward launch entry applies, or None."""
        name, _, args = entry
        i = 0 if name == "cr_embed_bwd" else 4 if name == "cr_stack_block_bwd" else 1 if name.endswith("_scatter") else None
        return args[i]._obj if i is not None and args[i] is not None else None

    def _head_coef(self):
        """[2, M] d loss_sum / d logit of the pos / neg item per row: what the occurrence index's gather multiplies seq_emb rows with."""
        return self.vec("head.coef", 2 * self.M).data_ptr() if self.use_index else None

    # ---- the eleven graphs -----------------------------------------------------------------------
    def _build(self):
        m, D, T, L_ = self.model, self.D, self.T, self.hp.num_blocks
        sq = math.sqrt(D)    # modules.py:159-160 (num_units ** 0.5)
        st = model_structure(m, self.hp)
        wa_ctx = self.want_attn and m in ("cast_1", "cast_2", "cast_3", "cast_4", "cast_5", "cast_6")
        wa_trunk = self.want_attn and not wa_ctx

        def ctx_stack(table, ids_key, prefix, out, out_ld, out_col, want=False):
            e = self.buf(prefix + ".emb", D)
            self.op_embed(ids_key, table, e, D, 0, sq, small=True, into_stack=True)        # cast_1.py:30-38
            self.op_stack(e, prefix, st["ctx"][prefix], out, out_ld, out_col, want_attn=want)   # cast_1.py:42-60

        if m in ("sasrec", "sasrec_static"):
            x = self.buf("x0", D)
            self.op_embed("seq", "item_emb", x, D, 0, sq, pos="learned" if m == "sasrec" else "static",
                          drop_site="emb", mask=True, into_stack=True)                      # sasrec.py:27-62
            s = self.buf("seq_emb", D)
            self.op_stack(x, "trunk", L_, s, D, 0, want_attn=wa_trunk)
        elif m == "cast_1":
            tseq = self.buf("tseq", D)
            ctx_stack("time_emb", "time", "ctx_time", tseq, D, 0, want=wa_ctx)
            x = self.buf("x0", D)
            self.op_embed("seq", "item_emb", x, D, 0, sq, pos="static", addend=tseq,
                          drop_site="emb", mask=True, into_stack=True)                      # cast_1.py:86-91
            s = self.buf("seq_emb", D)
            self.op_stack(x, "trunk", L_, s, D, 0)
        elif m in ("cast_2", "cast_3", "cast_4", "cast_7", "cast_8", "cast_9"):
            k = st["mlp"]
            c = self.buf("concat", k * D)
            if m == "cast_2":
                ctx_stack("time_emb", "time", "ctx_time", c, k * D, D, want=wa_ctx)
                self.op_embed("seq", "item_emb", c, k * D, 0, sq, pos="static", mask=True)   # cast_2.py:85-86
                self.op_dropout_inplace(c, 2 * D, "concat1")                                # cast_2.py:89-92
            elif m == "cast_3":
                tseq = self.buf("tseq", D)
                ctx_stack("time_emb", "time", "ctx_time", tseq, D, 0, want=wa_ctx)
                self.op_embed("hours", "hours_emb", c, k * D, D, sq, small=True)            # cast_3.py:32-41
                self.op_embed("days", "days_emb", c, k * D, 2 * D, sq, small=True)          # cast_3.py:43-52
                self.op_embed("seq", "item_emb", c, k * D, 0, sq, pos="static", addend=tseq,
                              mask=True)                                                    # cast_3.py:112-114
                self.op_dropout_inplace(c, 3 * D, "concat1")                                # cast_3.py:117-120
            elif m == "cast_4":
                ctx_stack("time_emb", "time", "ctx_time", c, k * D, D, want=wa_ctx)
                self.op_embed("seq", "item_emb", c, k * D, 0, sq, pos="static", mask=True)   # cast_4.py:111-112
                self.op_dropout_inplace(c, 2 * D, "concat1")                                # cast_4.py:115-118
                self.op_embed("hours", "hours_emb", c, k * D, 2 * D, sq, small=True)
                self.op_embed("days", "days_emb", c, k * D, 3 * D, sq, small=True)
                self.op_dropout_inplace(c, 4 * D, "concat2")                                # cast_4.py:121-124
            elif m in ("cast_7", "cast_8"):
                if m == "cast_7":
                    self.op_embed("hours", "hours_emb", c, k * D, D, sq, small=True)        # cast_7.py:30-51
                    self.op_embed("days", "days_emb", c, k * D, 2 * D, sq, small=True)
                else:
                    ctx_stack("hours_emb", "hours", "ctx_hours", c, k * D, D)              # cast_8.py:56-74
                    ctx_stack("days_emb", "days", "ctx_days", c, k * D, 2 * D)             # cast_8.py:78-95
                self.op_embed("seq", "item_emb", c, k * D, 0, sq, pos="static", mask=True)   # cast_7.py:77-78
                self.op_dropout_inplace(c, 3 * D, "concat1")                                # cast_7.py:81-84
            else:  # cast_9
                ctx_stack("hours_emb", "hours", "ctx_hours", c, k * D, 2 * D)              # cast_9.py:56-74
                ctx_stack("days_emb", "days", "ctx_days", c, k * D, 3 * D)                 # cast_9.py:78-95
                ctx_stack("time_emb", "time", "ctx_time", c, k * D, D)                     # cast_9.py:101-129
                self.op_embed("seq", "item_emb", c, k * D, 0, sq, pos="learned")            # cast_9.py:149-160
                self.op_dropout_inplace(c, 4 * D, "concat1")                                # cast_9.py:163-168
            x = self.buf("x0", D)
            self.op_mlp(c, x, k, mask_out=(m == "cast_9"))                                  # cast_2.py:95 / cast_9.py:171-174
            s = self.buf("seq_emb", D)
            self.op_stack(x, "trunk", L_, s, D, 0, want_attn=wa_trunk)
        elif m in ("cast_5", "cast_6"):
            k = st["mlp"]
            c = self.buf("concat", k * D)
            x = self.buf("x0", D)
            if m == "cast_5":
                tseq = self.buf("tseq", D)
                ctx_stack("time_emb", "time", "ctx_time", tseq, D, 0, want=wa_ctx)
                self.op_embed("seq", "item_emb", x, D, 0, sq, pos="static", addend=tseq,
                              into_stack=True)                                              # cast_5.py:113-114
                self.op_stack(x, "trunk", L_, c, k * D, 0)                                  # cast_5.py:118-139
                self.op_embed("hours", "hours_emb", c, k * D, D, sq, small=True)
                self.op_embed("days", "days_emb", c, k * D, 2 * D, sq, small=True)
                self.op_dropout_inplace(c, 3 * D, "concat1")                                # cast_5.py:143-146
            else:
                self.op_embed("seq", "item_emb", x, D, 0, sq, pos="static", into_stack=True)   # cast_6.py:113
                self.op_stack(x, "trunk", L_, c, k * D, 0)                                  # cast_6.py:117-138
                ctx_stack("time_emb", "time", "ctx_time", c, k * D, D, want=wa_ctx)
                self.op_dropout_inplace(c, 2 * D, "concat1")                                # cast_6.py:142-145
                self.op_embed("hours", "hours_emb", c, k * D, 2 * D, sq, small=True)
                self.op_embed("days", "days_emb", c, k * D, 3 * D, sq, small=True)
                self.op_dropout_inplace(c, 4 * D, "concat2")                                # cast_6.py:148-151
            s = self.buf("seq_emb", D)
            self.op_mlp(c, s, k)                                                            # cast_5.py:149
        self.op_head(s)

    def _finalize(self):
        if self.training:
            for fac in reversed(self._bwd_factories):
                lst = fac()
                if lst and self._grad2 and not getattr(fac, "pair_aware", False):
                    self.bwd += self._fold_pairs()            # a consumer with one gradient pointer: fold the pending pairs first
                self.bwd += lst
            assert not self._grad2, "a gradient partial was left without a consumer"
            # data parallelism overlaps the item / positional table's exchange with what is left of the backward once the last
            # launch that adds to the table gradient has been issued: the embedding backward of a looked-up table (its own launch,
            # or inside a block's backward) -- the head's rows are in from the start
            self.bwd_table_done = 0
            for i, entry in enumerate(self.bwd):
                sc = self._scatter_desc(entry)
                if sc is not None and sc.n_slabs == 0:                   # (n_slabs > 0: a small context table, written as slabs)
                    self.bwd_table_done = i + 1
            lay = self.layout
            # the step ends inside Adam (castrec.h, state block): sums and step number are read from the snapshot the
            # head kernel took, and the kernel zeroes the sums and advances the counter -- no cr_step_begin launch
            snap, tsnap = self.state.data_ptr() + 4 * 8, self.state.data_ptr() + 4 * 11
            l2 = float(self.hp.l2_emb)
            n_l2 = lay.n_l2 if l2 != 0.0 else 0
            lazy, lazy2 = (None, 0, 0, 0, None), None
            if self.lazy_adam:
                self.lazy_flags = torch.zeros(self.itemnum + 1, dtype=torch.int32, device=self.dev)
                world = max(1, self.batch_global // self.B)
                # this step's seq | pos | neg ids; under data parallelism the ids of ALL ranks (the sparse exchange hands
                # them over, dist.DataParallel.exchange): every replica must update the same rows
                self.lazy_ids = self.ids_all[:3].reshape(-1) if world == 1 else torch.zeros(world * 3 * self.M, dtype=torch.int32, device=self.dev)
                if self.loss in SAMPLED_LOSSES:
                    # the rows with a gradient: seq (embedding backward) | pos (the target term) and the step's samples, which the
                    # Adam launch reads where the loss launch wrote them (cr_adam_desc.lazy_ids2) -- neg only feeds the AUC here, and
                    # listing it would move rows the loss never touched on their momentum
                    assert world == 1
                    self.lazy_ids = self.ids_all[:2].reshape(-1)
                    lazy2 = self.samples
                lazy = (self.lazy_ids.data_ptr(), self.lazy_ids.numel(), self.itemnum + 1, self.D, self.lazy_flags.data_ptr())
            # slabs in use per 256-parameter block: n_wslabs where cr_gemm_wgrad is the only writer, n_slabs elsewhere
            counts = None
            per = np.full(lay.n_dense, self.n_slabs, np.int32)       # slabs that hold gradient, per dense parameter
            if self.n_wslabs < self.n_slabs:
                for a, b in self._wgrad_ranges:
                    per[a:b] = self.n_wslabs
            for a, b, c in self._block_bwd_ranges:                    # cr_stack_block_bwd: one slab per sequence pair
                per[a:b] = c
            if lay.n_dense and int(per.min()) < self.n_slabs:
                nb = (lay.n_dense + 255) // 256
                pad = np.zeros(nb * 256, np.int32)
                pad[:lay.n_dense] = per
                cnt = pad.reshape(nb, 256).max(1).astype(np.int32)   # a block shared with a parameter of more slabs reads them all (zeros)
                self.slab_counts = torch.from_numpy(cnt).to(self.dev)
                counts = self.slab_counts.data_ptr()

            def adam_desc(dense, n_slabs, stats, slab_counts):
                """cr_adam_desc over the dense gradient `dense` of n_slabs slabs, the loss sums read from `stats`."""
                d = L.AdamDesc(self.P.data_ptr(), self.Mom.data_ptr(), self.Vel.data_ptr(), self.Gt.data_ptr(), dense,
                               lay.n_table, lay.n_dense, n_slabs, float(self.hp.lr), 0.9, 0.98, 1e-8, self.state.data_ptr(),
                               stats, tsnap, l2, n_l2, *lazy, slab_counts)
                if lazy2 is not None:
                    d.lazy_ids2, d.n_lazy_ids2 = lazy2.data_ptr(), lazy2.numel()
                return d
            ad = adam_desc(self.Gs.data_ptr(), self.n_slabs, snap, counts)                  # the plain step: the slabs themselves
            ad1 = adam_desc(self.Gflat.data_ptr() + 4 * lay.n_table, 1, self.Gflat.data_ptr() + 4 * lay.n_total, None)   # the reduced bucket
            self._tgd, self._tgrad = None, None
            if self.use_index:
                # the table section's gradient by gather (castrec.h cr_tgrad_desc): inside the plain step's Adam launch; as a launch of
                # its own (cr_table_grad -> Gt) in front of the data-parallel exchange, and for grads()
                assert self._tg_rows is not None, "occurrence index: no gradient-row buffer for the item table's seq lookup"
                tg, se = self._tg_rows, self.seq_emb
                self._tgd = L.TgradDesc(self.batch_buf.data_ptr() + 4 * self.index_off, None, 0, 0, 0, self.state.data_ptr() + 4 * 4,
                                        self.index_lay, tg.rows.data_ptr(), tg.rows2.data_ptr() if tg.rows2 is not None else None, tg.ld, tg.scale,
                                        se.data_ptr(), se.shape[1], self._head_coef(), self.D, self._tg_part.data_ptr(), self._tg_tickets.data_ptr())
                ad.tg = C.pointer(self._tgd)
                self._tgrad = ("cr_table_grad", L.lib.cr_table_grad, (C.byref(self._tgd), self.Gt.data_ptr()))
            self._adam = ("cr_adam_step", L.lib.cr_adam_step, (C.byref(ad),))
            self._adam_flat = ("cr_adam_step", L.lib.cr_adam_step, (C.byref(ad1),))
            self._reduce = ("cr_reduce_slabs", L.lib.cr_reduce_slabs,
                            (self.Gs.data_ptr(), self.n_slabs, lay.n_dense, self.Gflat.data_ptr() + 4 * lay.n_table,
                             self.state.data_ptr(), self.Gflat.data_ptr() + 4 * lay.n_total, counts))
            # l2_emb != 0: the penalty of the CURRENT parameters, just before Adam moves them (one more launch; every
            # reference run uses 0.0)
            self._l2 = ("cr_l2_penalty", L.lib.cr_l2_penalty, (self.P.data_ptr(), n_l2, 0.5 * l2, self.state.data_ptr())) if n_l2 else None
            self._keep += [ad, ad1]

    # ---- running ---------------------------------------------------------------------------------
    def set_batch(self, seq, pos=None, neg=None, time=None, hours=None, days=None):
        """Copies one batch ([B,T] int arrays, host or device) into the static input buffers.  Host arrays are range
        checked first (the kernels index the tables with these ids unchecked; tf.nn.embedding_lookup raises
        InvalidArgument for an id outside its table -- e.g. unsorted timestamps give negative time bins, and
        sampler.py:66 produces bins up to 200 under --log_scale whatever --max_bins says).  CASTREC_NO_ID_CHECK=1 skips it."""
        limits = dict(seq=self.itemnum, pos=self.itemnum, neg=self.itemnum, time=self.hp.max_bins, hours=24, days=7)
        used = {"seq", "pos", "neg"} | ({"time"} if "time_emb" in self.layout.entries else set()) \
            | ({"hours", "days"} if "hours_emb" in self.layout.entries else set())
        for k, a in (("seq", seq), ("pos", pos), ("neg", neg), ("time", time), ("hours", hours), ("days", days)):
            if a is None:
                continue
            if not self.sw.no_id_check and k in used and not isinstance(a, torch.Tensor):
                a = np.asarray(a)
                if a.size and (int(a.min()) < 0 or int(a.max()) > limits[k]):
                    raise ValueError("%s ids outside [0, %d] (min %d, max %d): the lookup table has %d rows"
                                     % (k, limits[k], int(a.min()), int(a.max()), limits[k] + 1))
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32))
            if self.use_index:
                # the host mirror of the static batch buffer: the index is built from it below, and ids + index go over in ONE copy
                i = self.ID_KEYS.index(k)
                self._host_slot[i * self.M:(i + 1) * self.M] = t.reshape(-1).to(torch.int32).cpu().numpy()
            else:
                self.ids[k].copy_(t.reshape(-1).to(torch.int32), non_blocking=True)
        if self.use_index:
            used = self._build_index(self._host_slot)
            self.batch_buf[:used].copy_(torch.from_numpy(self._host_slot[:used]))

    def _build_index(self, host_slot):
        """host_slot: int32 [slot_words] holding the six id rows; the occurrence index of its seq / pos / neg ids is written behind them."""
        M = self.M
        base = host_slot.ctypes.data
        L.check(L.lib.cr_index_build(self._ixb, base, base + 4 * M, base + 8 * M, base + 4 * self.index_off), "cr_index_build")
        return self.index_off + int(host_slot[self.index_off + 4])     # words of the slot in use: a copy may stop there

    def pack_slot(self, seq, pos, neg, time=None, hours=None, days=None, out=None):
        """One batch as a SLOT of the id ring / the staging area: int32 [slot_words] = the six id rows (+ the batch's occurrence index
        behind them where the engine uses one).  `out`: a host array to fill (e.g. a pinned ring slot's numpy view)."""
        host = np.zeros(self.slot_words, np.int32) if out is None else out
        for i, a in enumerate((seq, pos, neg, time, hours, days)):
            if a is None:
                host[i * self.M:(i + 1) * self.M] = 0
            else:
                host[i * self.M:(i + 1) * self.M] = np.asarray(a).reshape(-1)
        if self.use_index:
            self._build_index(host)
        return host

    def load_slot(self, slot):
        """A packed slot (device tensor [slot_words], pack_slot's layout) into the static batch buffer: ids AND index."""
        self.batch_buf.copy_(slot.reshape(-1))

    def set_step(self, k=1):
        """The next launch runs as step number k (dropout keys, Adam bias correction); loss sums cleared."""
        self.state[:4].zero_()
        self.state[8:].zero_()
        self.state[4:5].view(torch.int32)[0] = k
        if getattr(self, "_feed_ring", None) is not None:
            if self._feed_have:
                raise RuntimeError("set_step(): %d fed batches are waiting (their ring slots follow the step number)" % self._feed_have)
            self._feed_next, self._feed_started, self._feed_first = int(k), False, int(k)
            torch.cuda.synchronize()
            self._feed_done.clear()
        if getattr(self, "_tg_tickets", None) is not None:
            self._tg_tickets.zero_()                     # (every launch leaves them zero; a failed one might not)
        if getattr(self, "lazy_flags", None) is not None:
            # row-sparse Adam claims a row with atomicExch(flag, step) != step: a flag left by an earlier run of the same
            # step number (counter moved back, checkpoint loaded) would read as "already claimed" and skip the row
            self.lazy_flags.zero_()
            self.flags_epoch += 1                        # what the flags said about earlier steps is gone (models.IndexToken)

    def set_item_weights(self, w):
        """ce_proposal="popularity": the proposal of the coming steps from non-negative item weights w [itemnum + 1] (w[0] ignored;
        castrec_amd.proposal.build_proposal states the construction and what it refuses).  The arrays are copied into the buffers the
        launches read (item_cdf, item_logq), behind the steps already queued on the current stream: a captured graph stays valid."""
        if getattr(self, "ce_proposal", "uniform") != "popularity":
            raise RuntimeError("set_item_weights(): this engine was not built with ce_proposal='popularity'")
        from .proposal import build_proposal
        cdf, logq = build_proposal(w, self.itemnum + 1)
        self.item_cdf.copy_(torch.from_numpy(cdf.view(np.int32)))
        self.item_logq.copy_(torch.from_numpy(logq))
        self._have_item_weights = True

    def _need_item_weights(self):
        if self.ce_proposal == "popularity" and not self._have_item_weights:
            raise RuntimeError("ce_proposal='popularity': call set_item_weights() before the first training step")

    def step_number(self):
        """Number of the step the next launch will run (1 + completed optimiser steps)."""
        return int(self.state[4:5].view(torch.int32)[0])

    def _run(self, lst, stream):
        for name, fn, args in lst:
            rc = fn(*args, stream)
            if rc != 0:
                raise RuntimeError("castrec %s failed (%d): %s" % (name, rc, L.lib.cr_last_error().decode()))

    def launch_step(self, apply=True, between=None, capturing=False):
        """forward -> backward -> [between()] -> Adam, on the current stream.  state[4] holds the number of the step
        being run; Adam ends the step (zeroes the loss sums, advances the counter).  Without Adam (apply=False) the
        state is left as the kernels wrote it: call set_step() before running again.  (capturing: recorded into a graph, not run.)"""
        s = torch.cuda.current_stream().cuda_stream
        if self.training and not capturing:
            self._need_item_weights()
        self._run(self.fwd, s)
        if self.training:
            self._run(self.bwd, s)
            if between is not None:
                between()
            if apply:
                self._run(([self._l2] if self._l2 else []) + [self._adam], s)
                if self._id_ring is not None and self.lazy_adam:     # (row-sparse Adam reads this step's ids: the batch moves behind it)
                    self._run([self._ring_next], s)

    # ---- the id batches of the coming steps, resident in HBM -------------------------------------
    def use_id_ring(self, ring):
        """`ring`: int32 device tensor [n_slots, 6, M] (rows in ID_KEYS order), or None to go back to set_batch() per step.
        Slot (k mod n_slots) holds the batch of step number k.  From the next launch_step() / capture() on, a step ends by moving
        the batch of the following step into the static id buffers (inside the cr_adam_step launch): the caller sets the first
        batch with set_batch() and keeps the slots of the coming steps filled -- no copy between two steps."""
        ads = [self._adam[2][0]._obj, self._adam_flat[2][0]._obj]      # the plain step's Adam and the data-parallel one (on the reduced bucket)
        if ring is None:
            self._id_ring = None
            for ad in ads:
                ad.ids_ring, ad.ids_ring_slots, ad.ids_slot_elems, ad.ids_dst, ad.ids_copy_elems = None, 0, 0, None, 0
            if self._tgd is not None:
                self._tgd.ring, self._tgd.ring_slots, self._tgd.slot_words, self._tgd.index_off = None, 0, 0, 0
            return
        assert ring.dtype == torch.int32 and ring.is_cuda and ring.is_contiguous(), ring.shape
        assert int(np.prod(ring.shape[1:])) == self.slot_words, \
            "ring slots of %s words, the engine's slots have %d (pack_slot: 6 x %d ids%s)" % (tuple(ring.shape[1:]), self.slot_words, self.M, " + the occurrence index" if self.use_index else "")
        self._id_ring = ring
        if self.lazy_adam:
            self._ring_next = ("cr_ids_ring_next", L.lib.cr_ids_ring_next,
                               (ring.data_ptr(), int(ring.shape[0]), 6 * self.M, self.ids_all.data_ptr(), self.state.data_ptr() + 4 * 11))
        else:
            # extra workgroups of the Adam launch move the batch (castrec.h cr_adam_desc.ids_ring): no launch of its own.  (A forked
            # graph branch beside Adam was measured first: the fork and join cost 17 us per step, four times the copy they hid.)
            # Only the ids move: the occurrence index of a step is read where it lies, in the ring slot of that step.
            for ad in ads:
                ad.ids_ring, ad.ids_ring_slots, ad.ids_slot_elems, ad.ids_dst = ring.data_ptr(), int(ring.shape[0]), self.slot_words, self.ids_all.data_ptr()
                ad.ids_copy_elems = self.ids_words
            if self._tgd is not None:
                self._tgd.ring, self._tgd.ring_slots, self._tgd.slot_words, self._tgd.index_off = ring.data_ptr(), int(ring.shape[0]), self.slot_words, self.index_off

    # ---- host batches fed AHEAD of the steps that use them --------------------------------------
    def enable_feed(self, n_slots=8, steps_per_graph=1):
        """Turns on the pipelined input path of a training engine: feed() packs a host batch into a pinned buffer and sends
        it -- ONE copy over PCIe, on a copy stream, while earlier steps run -- into a slot of a device ring; train_fed() runs the
        step of the oldest waiting batch, whose tail moves the following batch into the static id buffers (use_id_ring).  With
        one batch fed ahead nothing stands between two steps on the device.  (set_batch() per step: six pageable copies on the
        compute stream, 0.45 ms per step at the headline shape against 0.37 for the device step, tools/e2e_rate.py.)"""
        assert self.training and n_slots >= 4
        # an event behind every `_feed_every`-th step tells feed() that a slot's last reader has finished (behind EVERY step it
        # cost 5 us per step, tools/probes/ev_cost.py); a slot is rewritten n_slots steps after its batch ran
        self._feed_every = 4 if n_slots >= 8 else 1
        self._feed_ring = torch.zeros(n_slots, self.slot_words, dtype=torch.int32, device=self.dev)
        self._feed_host = torch.zeros(n_slots, self.slot_words, dtype=torch.int32).pin_memory()
        self._feed_np = self._feed_host.numpy()
        self._feed_stream = torch.cuda.Stream()
        self._feed_h2d = [None] * n_slots            # per slot: its host -> device copy has finished
        self._feed_done = {}                         # step number -> event behind that step's launch
        recapture = self.graph is not None
        self.use_id_ring(self._feed_ring)
        if recapture:
            # (the ring's address travels in the Adam launch's arguments).  steps_per_graph > 1: train_fed() runs that many steps per
            # graph launch whenever as many batches wait (capture()); the ring must hold them beside the slots being refilled
            assert steps_per_graph == 1 or n_slots >= 2 * steps_per_graph + 4, "ring too small for %d steps per launch" % steps_per_graph
            self.capture(n_steps=steps_per_graph if not self.lazy_adam else 1)
        self._feed_next, self._feed_have, self._feed_started = self.step_number(), 0, False
        self._feed_first = self._feed_next           # steps before it did not read the ring
        used = {"seq", "pos", "neg"} | ({"time"} if "time_emb" in self.layout.entries else set()) \
            | ({"hours", "days"} if "hours_emb" in self.layout.entries else set())
        limits = dict(seq=self.itemnum, pos=self.itemnum, neg=self.itemnum, time=self.hp.max_bins, hours=24, days=7)
        self._feed_limits = [(i, k, limits[k]) for i, k in enumerate(self.ID_KEYS) if k in used]

    def feed(self, seq, pos, neg, time=None, hours=None, days=None):
        """Queues the batch of the next step that has none yet (at most 5 wait at a time in the ring of 8, n_slots - 1 in a ring
        of fewer than 8 slots).  Ids are range checked as set_batch() does."""
        n = self._feed_ring.shape[0]
        # a free slot beside the one the running step's tail reads, and a recorded step in [k - n, last launched]
        if self._feed_have > min(n - self._feed_every, n - 2):
            raise RuntimeError("feed(): %d batches are waiting already (ring of %d slots)" % (self._feed_have, n))
        k = self._feed_next
        slot = k % n
        if self._feed_h2d[slot] is not None:
            self._feed_h2d[slot].synchronize()       # the pinned buffer's previous copy (n batches ago) has left it
        host = self._feed_np[slot]
        hid = host[:self.ids_words].reshape(6, self.M)
        for i, a in enumerate((seq, pos, neg, time, hours, days)):
            if a is None:
                hid[i] = 0
            else:
                hid[i] = np.asarray(a).reshape(-1)
        if not self.sw.no_id_check:
            lo, hi = hid.min(axis=1), hid.max(axis=1)
            for i, key, lim in self._feed_limits:
                if lo[i] < 0 or hi[i] > lim:
                    raise ValueError("%s ids outside [0, %d] (min %d, max %d): the lookup table has %d rows" % (key, lim, lo[i], hi[i], lim + 1))
        used = self.slot_words
        if self.use_index:
            used = self._build_index(host)               # (after the range check: the builder indexes its work arrays with these ids)
        # the slot held batch k - n: read by the tail of step k - n - 1 or, where that step ran with nothing fed ahead, by step
        # k - n's own copy into the static buffers -- the new copy waits for the launch of step k - n
        # (a HOST wait, like the two in train_fed: step k - n ended long ago, while a device-side wait between two streams
        # costs ~10 us of the waiting stream's time on this stack -- measured as 17 us per step for a forked graph branch)
        if k - n >= self._feed_first:
            behind = [j for j in self._feed_done if j >= k - n]
            if behind:
                self._feed_done[min(behind)].synchronize()
            else:
                # no recorded step at or behind the slot's last reader (cannot happen while train_fed records what it says it
                # records; never skip the wait silently): the compute stream itself
                torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(self._feed_stream):
            self._feed_ring[slot][:used].copy_(self._feed_host[slot][:used], non_blocking=True)      # (the index's capacity beyond its use stays behind)
            ev = torch.cuda.Event()
            ev.record()
        self._feed_h2d[slot] = ev
        self._feed_next += 1
        self._feed_have += 1

    def train_fed(self, max_steps=None):
        """Runs the step of the oldest fed batch -- or, where capture(n_steps=G) has made a graph of G steps and at least G batches
        wait (and max_steps allows it), those G steps in one launch.  Returns the number of steps run."""
        if self._feed_have < 1:
            raise RuntimeError("train_fed(): no batch has been fed")
        self._need_item_weights()
        n = self._feed_ring.shape[0]
        k = self._feed_next - self._feed_have
        G = self.graph_steps if (getattr(self, "graph_multi", None) is not None and self.graph is not None) else 1
        if self._feed_have < G or (max_steps is not None and max_steps < G):
            G = 1
        cur = torch.cuda.current_stream()
        if not self._feed_started:
            # nobody moved this batch into the static buffers (first step, or the step before ran with no batch fed ahead)
            self._feed_h2d[k % n].synchronize()
            self.ids_all.copy_(self._feed_ring[k % n][:self.ids_words].view(6, self.M))
        # the tail of step k + j - 1 moves batch k + j: those that are fed (a step or more ago: long there) must have arrived
        for j in range(1, min(G, self._feed_have - 1) + 1):
            self._feed_h2d[(k + j) % n].synchronize()
        self._feed_started = self._feed_have >= G + 1
        if G > 1:
            self.graph_multi.launch()
        elif self.graph is not None:
            self.graph.launch()
        else:
            self.launch_step()
        last = k + G - 1
        # an event behind every step number that is a multiple of _feed_every -- feed()'s admission bound counts on one in every
        # window of that many steps.  A launch of G steps records ONE event at its end and files it under every such step it
        # covers (an upper bound for each of them) and under its last step.
        marks = [j for j in range(k, last + 1) if j % self._feed_every == 0]
        if G > 1 and last not in marks:
            marks.append(last)
        if marks:
            ev = torch.cuda.Event()
            ev.record(cur)
            for j in marks:
                self._feed_done[j] = ev
            for old in [j for j in self._feed_done if j < last - n]:
                del self._feed_done[old]
        self._feed_have -= G
        return G

    # ---- data-parallel pieces (castrec_amd.dist drives them around an RCCL all-reduce) ----------
    def launch_backward_to_flat(self):
        """forward -> backward -> slabs collapsed into Gflat (+ loss stats in its tail)."""
        s = torch.cuda.current_stream().cuda_stream
        self._run(self.fwd, s)
        self._run(self.bwd, s)
        self._run(([self._tgrad] if self._tgrad else []) + [self._reduce], s)

    def launch_adam_from_flat(self):
        """Adam on the (all-reduced) flat bucket; the global loss statistics are read from its tail."""
        self._run(([self._l2] if self._l2 else []) + [self._adam_flat], torch.cuda.current_stream().cuda_stream)

    def capture_dp_phases(self):
        """Three HIP graphs for a data-parallel step: A1 = forward + the backward up to the last launch that adds to the table
        gradient, A2 = the rest of the backward + the slab collapse into the flat bucket, B = Adam on the (reduced) bucket.
        The table exchange runs between A1 and B beside A2 (castrec_amd.dist.DataParallel)."""
        s0 = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(s0)
        k = self.bwd_table_done
        # (occurrence index: the table gradient is WRITTEN into the bucket by cr_table_grad behind the last launch that leaves rows for it)
        progs = [self.fwd + self.bwd[:k] + ([self._tgrad] if self._tgrad else []), self.bwd[k:] + [self._reduce],
                 ([self._l2] if self._l2 else []) + [self._adam_flat]]
        graphs = []
        with torch.cuda.stream(side):
            for prog in progs:
                g = O.Graph()
                g.begin()
                self._run(prog, torch.cuda.current_stream().cuda_stream)
                g.end()
                graphs.append(g)
        s0.wait_stream(side)
        self.dp_graphs, self.dp_progs, self._graph_stream = graphs, progs, side
        return graphs

    def capture(self, dp=False, n_steps=1):
        """Captures launch_step() into a HIP graph (inputs are read from the static id buffers).
        n_steps > 1 (with use_id_ring(): every step's tail moves the next step's batch into the static buffers on the device) captures
        that many consecutive steps into a second graph, `graph_multi`: between two launches of a graph the device idles for the
        7-9 us the command processor needs to start the next one (rocprofv3: gaps of 0.2 us inside a step's graph, 8.7 us between two
        steps); n steps per launch pay that once."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = O.Graph()
        with torch.cuda.stream(side):
            g.begin()
            if dp:
                self.launch_backward_to_flat()
            else:
                self.launch_step(capturing=True)
            g.end()
        self.graph_multi, self.graph_steps = None, 1
        if n_steps > 1:
            assert not dp and self.training and self._id_ring is not None and not self.lazy_adam, "several steps per graph need the id ring (use_id_ring / enable_feed)"
            gm = O.Graph()
            with torch.cuda.stream(side):
                gm.begin()
                for _ in range(n_steps):
                    self.launch_step(capturing=True)
                gm.end()
            self.graph_multi, self.graph_steps = gm, int(n_steps)
        torch.cuda.current_stream().wait_stream(side)
        self.graph, self._graph_stream = g, side
        return g

    def train_step(self, seq, pos, neg, time=None, hours=None, days=None):
        self.set_batch(seq, pos, neg, time, hours, days)
        if self.graph is not None:
            self._need_item_weights()
            self.graph.launch()
        else:
            self.launch_step()

    def loss_auc(self):
        s = self.state.cpu()
        return float(s[5]), float(s[6])

    def forward_eval(self, seq, time=None, hours=None, days=None):
        assert not self.training
        self.set_batch(seq, None, None, time, hours, days)
        self.launch_step()

    def test_logits(self, cand):
        """[B, n_cand] logits of the last position (sasrec.py:93-97); cand int32 device tensor [B, n_cand]."""
        out = torch.empty(self.B, cand.shape[1], dtype=torch.float32, device=self.dev)
        O.test_logits(self.seq_emb, self.seq_emb.shape[1], self.p("item_emb"), cand, self.B, self.T, self.D, out)
        return out

    def topk(self, k, excl_off=None, excl_ids=None, targets=None, index=None, candidates=None):
        """Full-catalogue top-k of the last position of every sequence (after forward_eval): (ids [B, k] int32, scores [B, k] fp32,
        rank [B] int32 or None) as device tensors.  excl_off: host int64 [B + 1] CSR offsets into excl_ids (int32, host or device) --
        the items each row must not return nor count in its target's rank; targets: [B] ids whose rank among the eligible items is
        wanted (-1: excluded).  Scores come from bf16x3 products (fp32-grade; plain bf16 on an engine at attn_precision 'bf16');
        test_logits keeps its exact fp32 form.  index: an ItemIndex of this engine's item table (castrec_amd.index): the scores come
        from it instead of the table, with the same bits.  castrec.h cr_score_topk.  index may also be an ItemSubset of the table:
        the best k among its items only -- ids, exclusions and targets stay global ids, a target outside the subset has rank -1 and
        ranks count the subset's eligible items.  candidates: one iterable of item ids per row, or a prebuilt (off, ids) pair
        (castrec_amd.index.candidates_for): the best k among each row's own candidates minus its exclusions (castrec.h
        cr_score_topk_lists), from the table or from an ItemIndex -- not together with an ItemSubset."""
        from . import index as X
        V, D = self.itemnum + 1, self.D
        cand = (None, None)
        if candidates is not None:
            if isinstance(index, X.ItemSubset):
                raise ValueError("one filter per call: candidates= and an ItemSubset exclude each other")
            cand = X.candidates_for(candidates, self.B, V, excl_off, excl_ids)
            excl_off = excl_ids = None
        if isinstance(index, X.ItemSubset) and (index.parent_V, index.D) != (V, D):
            raise ValueError("subset of a [%d, %d] table, the engine's item table is [%d, %d]" % (index.parent_V, index.D, V, D))
        if isinstance(index, X.ItemIndex) and (index.V, index.D) != (V, D):
            raise ValueError("index of a [%d, %d] table, the engine's item table is [%d, %d]" % (index.V, index.D, V, D))
        ld = self.seq_emb.shape[1]
        query = self.seq_emb[self.T - 1:]                 # row b of the queries: seq_emb row b * T + T - 1
        return X.search(query, self.T * ld, self.B, k, self.p("item_emb") if index is None else index,
                        L.PREC_BF16 if self.attn_precision == "bf16" else L.PREC_BF16X3, self, excl_off, excl_ids, targets,
                        cand_off=cand[0], cand_ids=cand[1])

    # ---- parameter / gradient access (tests, checkpoints) ----------------------------------------
    def get_params(self):
        return {n: self.layout.view(self.P, n).detach().clone() for n in self.layout.logical_names()}

    def load_params(self, d):
        for n in self.layout.logical_names():
            self.layout.view(self.P, n).copy_(torch.tensor(np.asarray(d[n]), dtype=torch.float32).to(self.dev))

    def grads(self):
        """Normalised gradients by logical name, valid after launch_step(apply=False)."""
        n = float(self.state[2])
        if self._tgrad is not None:
            # the plain step never materialises the table gradient (cr_adam_step gathers it row by row): form it now, by the same gather
            self.Gt.zero_()
            self._run([self._tgrad], torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        flat = torch.cat([self.Gt, self.Gs.sum(0)[:self.layout.n_dense]]) / max(n, 1.0)
        return {k: self.layout.view(flat, k).clone() for k in self.layout.logical_names()}

    def n_launches(self):
        """C-ABI calls per step (an entry may launch more than one kernel: n_kernel_launches)."""
        return len(self.fwd) + len(self.bwd) + (1 if self.training else 0) + (1 if self.training and self._l2 else 0)

    def n_kernel_launches(self):
        """Kernel launches per step, as rocprofv3 counts them: cr_stack_fwd launches once per block when a sequence gets two
        workgroups (B <= 160, more than one tile: cr_stack.hip, g_stack_pair_max_b), cr_stack_block_bwd once per min(B, n_slabs)
        sequences; every other entry of the fused path is one kernel."""
        n = 0
        for entry in self.fwd + self.bwd:
            sd = self._stack_desc(entry)
            if sd is not None:
                n += sd.n_blocks if (self.B <= self.sw.stack_pair_max_b and self.T > 16) else 1
            elif entry[0] == "cr_stack_block_bwd":
                per = min(self.B, self.n_slabs)
                n += -(-self.B // per)
            else:
                n += 1
        return n + (1 if self.training else 0) + (1 if self.training and self._l2 else 0)

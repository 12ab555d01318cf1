"""Model classes with the reference's constructor / predict surface (models/sasrec.py:5,127-129,
models/cast_N.py) on top of the native engine.

    model = SASRec(usernum, itemnum, args)              # or CAST1(usernum, itemnum, ratingnum, args) ... CAST9
    auc, loss = model.train_step(u, seq, pos, neg, timeseq, hours_seq, days_seq)    # == sess.run([auc, loss, train_op], feed)
    logits, attn = model.predict(sess, u, seq, item_idx, timeseq=, hours_seq=, days_seq=)

``sess`` is accepted and ignored (there is no TensorFlow session).  ``predict`` takes a whole batch of
users; ``item_idx`` is either the reference's shared list of 101 candidates or a [B, n] array.
"""
import collections
import os

import numpy as np
import torch

from .engine import MODELS, Engine, Hyper

# What an ItemIndex is in step with (ItemIndex.token; Model.refresh_item_index, Model.item_delta).  table_epoch: Model._table_epoch,
# bumped by everything that changes the item table other than a training step (load, load_tf_checkpoint, load_params).  flags_epoch:
# how often the training engine has zeroed row-sparse Adam's flags since it was made (Engine.flags_epoch; 0 before it exists).  step:
# the number of the next training step (Engine.step_number(); 1, a lower bound, before the engine exists), None where Adam is dense.
# lazy_flags[r] is the number of the last step that moved row r, so within one pair of epochs the rows that differ from the index are
# exactly those with a flag >= token.step.
IndexToken = collections.namedtuple("IndexToken", "table_epoch flags_epoch step")


class _Model(object):
    NAME = None

    def __init__(self, usernum, itemnum, args, reuse=None, n_slabs=None, batch_global=None, row_offset=0):
        self.name = self.NAME
        self.usernum, self.itemnum, self.args = usernum, itemnum, args
        self.hp = Hyper(args)
        self._n_slabs, self._batch_global, self._row_offset = n_slabs, batch_global, row_offset
        self._train = None
        self._pending_opt = None              # optimiser state loaded before the training engine exists (load / load_tf_checkpoint)
        self._item_weights = None             # ce_proposal="popularity": the weights of set_item_counts, until the training engine exists
        self._eval = {}
        self._fed = []                        # data parallel: batches handed over by feed() wait here
        self._graph = bool(int(os.environ.get("CASTREC_GRAPH", "1")))
        # parameters exist from construction on (tf.global_variables_initializer, main.py:150)
        self._owner = Engine(self.name, usernum, itemnum, self.hp, 1, training=False)
        self.attention_weights = None
        self._param_version = 0               # bumped by whatever changes the parameters: an ItemIndex records the one it was built at
        self._table_epoch = 0                 # ... and by whatever changes them other than a training step (IndexToken)
        self._flags_epoch0 = 0                # the training engine's flags_epoch when it was made: no step had run yet

    # -- training ---------------------------------------------------------------------------------
    def data_parallel(self, rank, world, process_group=None, sparse=None):
        """One replica per rank (the reference has no multi-GPU path): every rank feeds train_step the SAME
        global batch (one sampler stream, same seed everywhere), takes rows [rank * B / world, (rank + 1) * B / world) of it,
        and the gradients meet in castrec_amd.dist.DataParallel (RCCL all-reduce of one bucket, or the sparse item-row
        exchange for large tables) before an identical Adam step on every rank.  Call before the first train_step."""
        if self._train is not None:
            raise RuntimeError("data_parallel() must be called before the first train_step")
        if getattr(self.hp, "loss", "bce") in ("ce", "sampled_ce", "gbce") and int(world) > 1:
            raise ValueError("loss='%s' does not take data parallelism (castrec_amd.engine.Engine)" % self.hp.loss)
        self._dp_cfg = (int(rank), int(world), process_group, sparse)

    def _train_engine(self, B):
        if self._train is None:
            # the training engine shares the owner's parameter vector: both must live on the device this process runs on
            # (under torch.distributed.run the process group -- which selects cuda:LOCAL_RANK -- comes before build_model)
            cur = torch.device("cuda", torch.cuda.current_device())
            if self._owner.P.device != cur:
                raise RuntimeError("model parameters are on %s but the current device is %s: select the device "
                                   "(castrec_amd.dist.init_from_env / torch.cuda.set_device) before building the model"
                                   % (self._owner.P.device, cur))
            dp_cfg = getattr(self, "_dp_cfg", None)
            if dp_cfg is not None and dp_cfg[1] > 1:
                from . import dist as D_
                rank, world, pg, sparse = dp_cfg
                lo, hi = D_.shard_rows(B, rank, world)
                self._train = Engine(self.name, self.usernum, self.itemnum, self.hp, hi - lo, training=True, share=self._owner,
                                     n_slabs=self._n_slabs, batch_global=B, row_offset=lo * self.hp.maxlen)
                self._dp_rows = (lo, hi, B)
                rep = D_.EngineReplica(self._train, use_graph=self._graph)
                bounce = os.environ.get("CASTREC_DIST_BACKEND") == "gloo"     # gloo cannot reduce device tensors: through host memory
                if bounce:
                    rep = D_.HostBounce(rep)
                self._dp = D_.DataParallel(rep, rank, world, pg, sparse=sparse)
                if bounce:
                    rep.adopt_params()
                if self._graph and not bounce and os.environ.get("CASTREC_DP_ONE_GRAPH") != "0":
                    # the whole step incl. the collectives as one HIP graph: captured and validated inside the FIRST train_step,
                    # on that step's batch (an all-padding batch -- the static id buffers before any set_batch -- moves nothing
                    # and validates nothing); else the three-graph form.  dist.DataParallel.step_form says which one runs.
                    self._dp.request_capture()
                if self._graph:
                    self._train.set_step(1); self._train.Mom.zero_(); self._train.Vel.zero_(); self._train.Gflat.zero_()
                if self._pending_opt is not None:
                    self._apply_opt(*self._pending_opt)
                    self._pending_opt = None
                self._flags_epoch0 = self._train.flags_epoch
                return self._train
            self._train = Engine(self.name, self.usernum, self.itemnum, self.hp, B, training=True, share=self._owner,
                                 n_slabs=self._n_slabs, batch_global=self._batch_global, row_offset=self._row_offset)
            if self._graph and self._batch_global is None:
                self._train.capture()
                self._train.set_step(1); self._train.Mom.zero_(); self._train.Vel.zero_(); self._train.Gflat.zero_()
            if self._pending_opt is not None:          # a checkpoint's Adam slots and step count (saver.restore, main.py:165-175)
                self._apply_opt(*self._pending_opt)
                self._pending_opt = None
            if self._item_weights is not None:
                self._train.set_item_weights(self._item_weights)
            self._flags_epoch0 = self._train.flags_epoch
        if getattr(self, "_dp", None) is not None:
            if self._dp_rows[2] != B:
                raise ValueError("global batch size changed from %d to %d (static graph)" % (self._dp_rows[2], B))
            return self._train
        if self._train.B != B:
            raise ValueError("batch size changed from %d to %d (static graph)" % (self._train.B, B))
        return self._train

    def set_item_counts(self, counts, power=None):
        """--ce_proposal popularity: the sampled softmax draws its negatives with probability proportional to (counts_v + 1)^power
        (counts [itemnum + 1], e.g. each item's occurrences in the training split; power defaults to hp.ce_pop_power; the + 1 gives
        every item mass) and corrects every logit by -log Q (Engine.set_item_weights).  May be called again while training."""
        if getattr(self.hp, "ce_proposal", "uniform") != "popularity":
            raise RuntimeError("set_item_counts(): the model was not built with ce_proposal='popularity'")
        counts = np.asarray(counts, np.float64)
        if counts.shape != (self.itemnum + 1,):
            raise ValueError("counts must have itemnum + 1 = %d entries, got shape %s" % (self.itemnum + 1, counts.shape))
        power = float(getattr(self.hp, "ce_pop_power", 1.0) if power is None else power)
        from .proposal import build_proposal
        w = (counts + 1.0) ** power
        build_proposal(w, self.itemnum + 1)              # (refuses bad counts now, not at the first step)
        self._item_weights = w
        if self._train is not None:
            self._train.set_item_weights(w)

    def train_step(self, u, seq, pos, neg, time_seq=None, hours=None, days=None, fetch=True):
        """One optimisation step (main.py:212-219).  Returns (auc, loss) of the batch like the reference's fetch."""
        seq = np.asarray(seq)
        eng = self._train_engine(seq.shape[0])
        z = np.zeros_like(seq) if (time_seq is None or hours is None or days is None) else None
        arrs = (seq, np.asarray(pos), np.asarray(neg), z if time_seq is None else np.asarray(time_seq),
                z if hours is None else np.asarray(hours), z if days is None else np.asarray(days))
        if getattr(self, "_dp", None) is not None:
            self._dp.step(arrs)                            # this rank's rows -> backward -> exchange -> Adam (loss / auc: global)
        else:
            eng.train_step(*arrs)
        self._param_version += 1
        if fetch:
            loss, auc = eng.loss_auc()
            return auc, loss
        return None

    # -- the same step with its batch handed over AHEAD of time ------------------------------------------------------
    def feed(self, u, seq, pos, neg, time_seq=None, hours=None, days=None):
        """Hands over the batch of a coming step (the sampler's output, as train_step takes it) while earlier steps run:
        one pinned copy over PCIe on a copy stream into a device ring (Engine.enable_feed).  train_fed() then runs the oldest
        waiting batch.  Feeding one batch ahead -- feed(b0); loop: feed(b[i + 1]); train_fed() -- leaves no copy between two
        steps on the device.  Same arithmetic, same batches as train_step: only the transport differs."""
        seq = np.asarray(seq)
        eng = self._train_engine(seq.shape[0])
        if getattr(self, "_dp", None) is not None:
            self._fed.append((u, seq, pos, neg, time_seq, hours, days))     # data parallel: the batch waits on the host
            return
        if getattr(eng, "_feed_ring", None) is None:
            g = self.steps_per_launch
            eng.enable_feed(n_slots=16 if g > 1 else 8, steps_per_graph=g)
        eng.feed(seq, pos, neg, time_seq, hours, days)

    @property
    def steps_per_launch(self):
        """Steps a graph launch of the fed training path runs when as many batches wait (Engine.capture(n_steps)): between two graph
        launches the device idles for the 5-9 us the next launch takes to start, 1-2 % of a 0.33 ms step.  CASTREC_STEPS_PER_GRAPH
        overrides the default of 4; 1 without HIP graphs, with row-sparse Adam, or data parallel."""
        dp_cfg = getattr(self, "_dp_cfg", None)
        data_parallel = getattr(self, "_dp", None) is not None or (dp_cfg is not None and dp_cfg[1] > 1)
        # (row-sparse Adam: the engine's own setting once it exists, before that what it will read -- Engine.__init__)
        lazy = self._train.lazy_adam if self._train is not None else (bool(int(os.environ.get("CASTREC_LAZY_ADAM", "0")))
                                                                       or bool(getattr(getattr(self, "hp", None), "row_sparse_adam", False)))
        if not self._graph or data_parallel or self._batch_global is not None or lazy:
            return 1
        return max(1, int(os.environ.get("CASTREC_STEPS_PER_GRAPH", "4")))

    @property
    def feed_ahead(self):
        """How many fed batches may wait for their steps (main.py keeps that many handed over): one more than steps_per_launch, so that
        a launch's last step finds its successor's batch in place."""
        g = self.steps_per_launch
        return g + 1 if g > 1 else 1

    def train_fed_many(self, max_steps=None):
        """Runs the oldest waiting batch's step -- or steps_per_launch steps in one graph launch when as many batches wait and
        max_steps allows it.  Returns the number of steps run; loss / auc of the last one: loss_auc()."""
        if getattr(self, "_dp", None) is not None:
            self.train_step(*self._fed.pop(0), fetch=False)
            return 1
        eng = self._train
        if eng is None or getattr(eng, "_feed_ring", None) is None:
            raise RuntimeError("train_fed_many(): feed() a batch first")
        self._param_version += 1
        return eng.train_fed(max_steps=max_steps)

    def loss_auc(self):
        """(auc, loss) of the last step run, like train_step's fetch."""
        loss, auc = self._train.loss_auc()
        return auc, loss

    def train_fed(self, fetch=True):
        if getattr(self, "_dp", None) is not None:
            return self.train_step(*self._fed.pop(0), fetch=fetch)
        eng = self._train
        if eng is None or getattr(eng, "_feed_ring", None) is None:
            raise RuntimeError("train_fed(): feed() a batch first")
        self._param_version += 1
        eng.train_fed(max_steps=1)
        if fetch:
            loss, auc = eng.loss_auc()
            return auc, loss
        return None

    # -- inference --------------------------------------------------------------------------------
    def predict(self, sess, u, seq, item_idx, timeseq=None, input_context_seq=None, hours_seq=None, days_seq=None,
                want_attention=True):
        seq = np.asarray(seq)
        if seq.ndim == 1:
            seq = seq[None]
        B = seq.shape[0]
        eng = self._eval_engine(B, want_attention)
        z = np.zeros_like(seq)
        f = lambda a: z if a is None else np.asarray(a).reshape(B, -1)
        eng.forward_eval(seq, f(timeseq), f(hours_seq), f(days_seq))
        cand = np.asarray(item_idx, np.int32)
        if cand.ndim == 1:
            cand = np.tile(cand[None], (B, 1))
        lg = eng.test_logits(torch.from_numpy(np.ascontiguousarray(cand)).to(eng.dev))
        self.attention_weights = eng.attn_weights
        attn = eng.attn_weights.cpu().numpy() if (want_attention and eng.attn_weights is not None) else None
        return lg.cpu().numpy(), attn

    def _eval_engine(self, B, want_attention):
        key = (B, bool(want_attention))
        if key not in self._eval:
            self._eval[key] = Engine(self.name, self.usernum, self.itemnum, self.hp, B, training=False, share=self._owner,
                                     want_attn=want_attention)
        return self._eval[key]

    def build_item_index(self, precision=None, metric="dot"):
        """An ItemIndex (castrec_amd.index) of the current item table for recommend(index=), similar_items(index=) and
        ItemIndex.search / save.  precision: "bf16x3" or "bf16"; by default what the engine's top-K computes in ("bf16" at
        attn_precision "bf16").  metric: "dot", the table's rows as the model scores them, or "cosine", the rows normalised as the
        index is written (item-to-item similarity: similar_items; no normalised copy of the table is made).  The index is a
        snapshot: it records the parameter version, and recommend refuses it once a training step or a load has changed the
        parameters; refresh_item_index brings either kind back in step."""
        from .index import ItemIndex
        if precision is None:
            precision = self._index_precision()
        ix = ItemIndex.build(self._owner.p("item_emb"), precision, version=self._param_version, metric=metric)
        ix.token = self._index_token()
        return ix

    def _index_precision(self):
        """The precision of an index or subset made for one call: what the engine's top-K computes in."""
        return "bf16" if self._owner.attn_precision == "bf16" else "bf16x3"

    def _row_sparse_engine(self):
        """The training engine where it runs row-sparse Adam (its lazy_flags name the rows a step moved), else None."""
        eng = self._train
        return eng if eng is not None and eng.lazy_adam and getattr(eng, "lazy_flags", None) is not None else None

    def _index_token(self):
        """The IndexToken of the item table as it is now."""
        if self._train is None:
            return IndexToken(self._table_epoch, 0, 1)
        eng = self._row_sparse_engine()
        return IndexToken(self._table_epoch, self._train.flags_epoch - self._flags_epoch0, eng.step_number() if eng is not None else None)

    def _sync_refusal(self, token, now):
        """Why the rows moved since `token` cannot be read off row-sparse Adam's flags (a string), or None where they can."""
        if self._row_sparse_engine() is None:
            return "no training engine yet" if self._train is None else "dense Adam moves every row of the item table in every step"
        if token is None or token.step is None or now.step is None:
            return "the index carries no step to count from (it was loaded, built from a bare table, or built under dense Adam)"
        if token.table_epoch != now.table_epoch:
            return ("the item table was replaced since (table epoch %d, now %d: load / load_tf_checkpoint / load_params)"
                    % (token.table_epoch, now.table_epoch))
        if token.flags_epoch != now.flags_epoch:
            return "row-sparse Adam's flags were cleared since (flags epoch %d, now %d: set_step)" % (token.flags_epoch, now.flags_epoch)
        return None

    def refresh_item_index(self, index):
        """Brings an ItemIndex of the item table (build_item_index) in step with the parameters, in place, and returns how: "sync" --
        under row-sparse Adam, when the index's token and the model agree on both epochs, only the 16-row tiles holding a row that a
        step since the token moved are rewritten (ItemIndex.sync with the engine's lazy_flags, since=token.step) -- else "rebuild"
        (ItemIndex.rebuild: the whole blob again, no allocation).  Either way the blob ends as the bytes of a fresh build_item_index()
        of the index's precision and metric (a cosine index is written from the raw table rows, normalised as its build normalised
        them), and index.version / index.token are the model's.  Nothing refreshes by itself: recommend(index=) keeps refusing a stale
        index.  An ItemSubset gathered from the index earlier stays the snapshot it was."""
        from .index import ItemIndex
        if not isinstance(index, ItemIndex):
            raise TypeError("refresh_item_index takes an ItemIndex (an ItemSubset is a snapshot: gather it again)")
        self._check_index_shape(index)
        table, now = self._owner.p("item_emb"), self._index_token()
        if self._sync_refusal(index.token, now) is None:
            index.sync(table, self._train.lazy_flags, since=index.token.step, version=self._param_version)
            how = "sync"
        else:
            index.rebuild(table, version=self._param_version)
            how = "rebuild"
        index.token = now
        return how

    def item_delta(self, token):
        """The item rows that training moved since `token` (an ItemIndex.token, or the token of the last call), for an index held where
        no table is -- an ItemIndex.load-ed serving process runs ix.update(ids, rows=rows), whatever the index's metric (the rows are
        raw table rows; a cosine index normalises them as it writes): returns (ids, rows, token_now), ids an int32
        CUDA tensor [n] (possibly empty), rows float32 [n, D], token_now to pass next time.  RuntimeError, naming the reason, where
        the flags cannot say which rows moved (dense Adam, a table load or cleared flags since the token): send the whole index."""
        now = self._index_token()
        why = self._sync_refusal(token, now)
        if why is not None:
            raise RuntimeError("item_delta: %s; rebuild and send the whole index" % why)
        ids = torch.nonzero(self._train.lazy_flags >= int(token.step)).reshape(-1)
        return ids.to(torch.int32), self._owner.p("item_emb")[ids], now

    def _check_index_shape(self, index):
        V = getattr(index, "parent_V", None) or index.V
        if (V, index.D) != (self.itemnum + 1, self._owner.D):
            raise ValueError("index of a [%d, %d] table, the model's item table is [%d, %d]"
                             % (V, index.D, self.itemnum + 1, self._owner.D))

    def _check_index(self, index):
        """index: None, an ItemIndex or an ItemSubset (its parent_V is the table it refers to)."""
        if index is None:
            return
        self._check_index_shape(index)
        if index.version is not None and index.version != self._param_version:
            raise RuntimeError("stale index: built at parameter version %d, the model is at %d (build_item_index() again)"
                               % (index.version, self._param_version))

    def _allowed(self, allow, index, metric="dot"):
        """What recommend / similar_items search: `index` itself without allow; with allow (an ItemSubset, or an iterable of item ids)
        the ItemSubset -- gathered out of `index` when there is one (it inherits the index's metric), else from the item table's rows
        with `metric`."""
        from .index import ItemSubset
        self._check_index(index)
        if allow is None:
            return index
        if isinstance(allow, ItemSubset):
            self._check_index(allow)
            return allow
        if index is not None:
            if isinstance(index, ItemSubset):
                raise ValueError("allow= with index= an ItemSubset: pass one subset")
            return index.subset(allow)
        return ItemSubset.build(self._owner.p("item_emb"), allow, self._index_precision(), version=self._param_version, metric=metric)

    def similar_items(self, ids, k=10, index=None, allow=None, candidates=None, metric=None):
        """The k items most similar to each given item, the item itself left out.  Returns numpy (ids [n, k], scores [n, k]).
        metric: "dot" -- the largest dot product of the table rows (the model's geometry: the scores of recommend with the item's
        vector as the query; large-norm items come out similar to everything) -- or "cosine" -- the largest cosine, and the scores
        are cosines: the search runs on an index of normalised rows and its scores q . x / ||x|| are divided by the query rows' fp32
        norms (a query row of norm 0 gets scores 0).  None: the metric of the index or ItemSubset that is given, "dot" without one.
        index: an ItemIndex of the table (build_item_index, of either metric) to search instead of one built for this call.  allow:
        an iterable of item ids or an ItemSubset -- the k most similar among those items only (one set for every row).  candidates:
        one iterable of item ids per given item -- the k most similar among that item's own candidates (under "dot" the table's
        rows are gathered unless index is given; under "cosine" an index is built for the call unless one is given); one filter
        per call, allow or candidates.  ValueError when an explicit metric differs from that of a given index or ItemSubset."""
        from .index import ItemIndex, ItemSubset, _metric, search
        ids = np.asarray(ids, np.int64).ravel()
        if ids.size == 0 or ids.min() < 1 or ids.max() > self.itemnum:
            raise ValueError("ids must be item ids in 1 .. %d" % self.itemnum)
        if candidates is not None and allow is not None:
            raise ValueError("one filter per call: allow= or candidates=")
        if metric is not None:
            _metric(metric)
        for what, given in (("index=", index), ("allow=", allow if isinstance(allow, ItemSubset) else None)):
            if given is None:
                continue
            if metric is not None and given.metric != metric:
                raise ValueError("similar_items(metric=%r) with %s of metric %r: search an index of the metric that is asked for, "
                                 "or leave metric=None" % (metric, what + " " + type(given).__name__, given.metric))
            metric = given.metric
        metric = metric or "dot"
        index = self._allowed(allow, index, metric)
        table = self._owner.p("item_emb")
        q = table[torch.from_numpy(ids).to(table.device)]
        if metric == "cosine" and index is None:
            index = ItemIndex.build(table, self._index_precision(), metric="cosine")

        def scores(sc):                                   # q . x / ||x|| -> cosines
            if metric != "cosine":
                return sc
            sc = sc if torch.is_tensor(sc) else torch.from_numpy(sc).to(q.device)
            qn = torch.linalg.vector_norm(q, dim=1, keepdim=True)
            return torch.where(qn > 0, sc / torch.where(qn > 0, qn, torch.ones_like(qn)), torch.zeros_like(sc)).cpu().numpy()
        if candidates is not None:
            from .index import PRECISIONS, _is_prebuilt, candidates_for, excl_csr
            n = ids.size
            cand = candidates_for(candidates, n, self.itemnum + 1, *((None, None) if _is_prebuilt(candidates) else excl_csr([[int(i)] for i in ids], n)))
            prec = index.prec if index is not None else PRECISIONS[self._index_precision()]
            top, sc, _ = search(q, q.shape[1], n, int(k), table if index is None else index, prec, self._owner,
                                cand_off=cand[0], cand_ids=cand[1])
            return top.cpu().numpy(), scores(sc) if metric == "cosine" else sc.cpu().numpy()
        if index is None:
            index = ItemIndex.build(table, self._index_precision())
        top, sc = index.search(q, int(k), exclude=[[int(i)] for i in ids])
        return top, scores(sc)

    def recommend(self, u, seq, k=10, timeseq=None, hours_seq=None, days_seq=None, exclude="history", return_scores=True,
                  targets=None, index=None, allow=None, candidates=None):
        """The k best items of the whole catalogue for each row of a batch (the last position's scores against every item row,
        sasrec.py:93-97 extended from a candidate list to the table; castrec.h cr_score_topk).  exclude: "history" (the nonzero ids
        of each row of seq), None, or one iterable of ids per row.  Returns numpy (ids [B, k], scores [B, k]) -- ids only when
        return_scores is False -- and, with targets ([B] ids), a third array: each target's 0-based rank among the eligible items
        (-1 for an excluded target).  Rows with fewer than k eligible items end in id 0, score -inf.  index: an ItemIndex of the item
        table (build_item_index): same results, the table's rows are not converted again.  An index of metric "cosine" is taken as
        well, for models trained on normalised item scores: the scores are then seq_emb . x / ||x||.  allow: an iterable of item ids or an
        ItemSubset (castrec_amd.index) -- the best k among those items only, one set shared by every row (a list per row goes
        through candidates=); it combines with exclude, a target outside it has rank -1 and ranks count the set's eligible items.
        With an iterable the subset is gathered for this call (out of index when given): keep an ItemSubset to reuse it.
        candidates: one iterable of item ids per row -- the best k among THAT row's candidates (castrec.h cr_score_topk_lists: the
        rows the lists name are gathered from the item table, or from index when given, so the cost follows the lists); it
        combines with exclude ("history" included), a target that is no eligible candidate of its row has rank -1 and ranks count
        the row's eligible candidates.  Or a prebuilt (off, ids) pair (castrec_amd.index.candidate_csr, ids an int32 CUDA tensor of
        distinct ids per row) for large batches: exclude must then be None.  One filter per call: allow or candidates."""
        from .index import ItemSubset, excl_csr
        if candidates is not None and (allow is not None or isinstance(index, ItemSubset)):
            raise ValueError("one filter per call: candidates= together with allow= or an ItemSubset")
        index = self._allowed(allow, index)
        seq = np.asarray(seq)
        if seq.ndim == 1:
            seq = seq[None]
        B = seq.shape[0]
        eng = self._eval_engine(B, False)
        z = np.zeros_like(seq)
        f = lambda a: z if a is None else np.asarray(a).reshape(B, -1)
        eng.forward_eval(seq, f(timeseq), f(hours_seq), f(days_seq))
        if isinstance(exclude, str):
            if exclude != "history":
                raise ValueError("exclude must be 'history', None or a list of per-row id iterables")
            exclude = [r[r != 0] for r in seq.astype(np.int64)]
        top, sc, rk = eng.topk(int(k), *excl_csr(exclude, B), targets, index=index, candidates=candidates)
        out = (top.cpu().numpy(),) + ((sc.cpu().numpy(),) if return_scores else ())
        if targets is not None:
            out = out + (rk.cpu().numpy(),)
        return out if len(out) > 1 else out[0]

    # -- checkpoints (tf.train.Saver, main.py:159,227) ----------------------------------------------
    def state_dict(self):
        d = {"model": self.name, "P": self._owner.P.detach().cpu(), "names": self._owner.layout.logical_names()}
        if self._train is not None:
            d.update(M=self._train.Mom.cpu(), V=self._train.Vel.cpu(), state=self._train.state.cpu())
        return d

    def save(self, path):
        torch.save(self.state_dict(), path)
        return path

    def _apply_opt(self, M, V, next_step):
        self._train.Mom.copy_(M); self._train.Vel.copy_(V)
        self._train.set_step(int(next_step))

    def load(self, path):
        """Parameters AND optimiser state (Adam m / v, step number), like saver.restore (main.py:165-166): a training
        step after load() continues the saved run.  The state is kept aside until the training engine exists."""
        d = torch.load(path, map_location="cpu")
        if d["model"] != self.name or d["P"].numel() != self._owner.P.numel():
            raise ValueError("checkpoint %s does not match model %s" % (path, self.name))
        self._owner.P.copy_(d["P"])
        if "M" in d:
            st = d["state"]
            cur = int(st[4:5].view(torch.int32)[0])
            nxt = cur if st.numel() == 16 else cur + 1   # 8-float state of earlier files: [4] counted COMPLETED steps
            if self._train is not None:
                self._apply_opt(d["M"], d["V"], nxt)
            else:
                self._pending_opt = (d["M"], d["V"], nxt)
        self._param_version += 1
        self._table_epoch += 1

    def load_tf_checkpoint(self, prefix):
        """Loads a checkpoint written by the reference (tf.train.Saver bundle `<prefix>.index` +
        `<prefix>.data-00000-of-00001`, main.py:231-233 there), Adam slots and step count included when the bundle
        holds them (they then seed the next train_step, as saver.restore does before main.py:167-175's one step)."""
        from . import tf_bundle
        params, slot_m, slot_v, steps = tf_bundle.load_logical_with_slots(prefix)
        want = {n: tuple(self._owner.layout.view(self._owner.P, n).shape) for n in self._owner.layout.logical_names()}
        missing, extra = sorted(set(want) - set(params)), sorted(set(params) - set(want))
        if missing or extra:
            raise ValueError("checkpoint %s does not match model %s: missing %s, unexpected %s" % (prefix, self.name, missing, extra))
        for n, shp in want.items():
            if tuple(params[n].shape) != shp:
                raise ValueError("checkpoint %s: %s has shape %s, model expects %s" % (prefix, n, params[n].shape, shp))
        self._owner.load_params(params)
        have_m, have_v = set(slot_m) == set(want), set(slot_v) == set(want)
        if (slot_m or slot_v) and not (have_m and have_v):
            raise ValueError("checkpoint %s holds Adam slots for only part of model %s's variables (m: %d, v: %d of %d)"
                             % (prefix, self.name, len(slot_m), len(slot_v), len(want)))
        if have_m and have_v:
            lay = self._owner.layout
            M, V = torch.zeros(lay.n_total), torch.zeros(lay.n_total)
            for n in want:
                lay.view(M, n).copy_(torch.tensor(np.asarray(slot_m[n], np.float32)))
                lay.view(V, n).copy_(torch.tensor(np.asarray(slot_v[n], np.float32)))
            if self._train is not None:
                self._apply_opt(M, V, steps + 1)
            else:
                self._pending_opt = (M, V, steps + 1)
        self._param_version += 1
        self._table_epoch += 1

    def get_params(self):
        return self._owner.get_params()

    def load_params(self, d):
        self._owner.load_params(d)
        self._param_version += 1
        self._table_epoch += 1


class SASRec(_Model):
    """models/sasrec.py:4-5: SASRec(usernum, itemnum, args, static=False, reuse=None)."""

    def __init__(self, usernum, itemnum, args, static=False, reuse=None, **kw):
        self.NAME = "sasrec_static" if static else "sasrec"
        super().__init__(usernum, itemnum, args, reuse, **kw)


def _cast(n):
    class _C(_Model):
        NAME = "cast_%d" % n
        __doc__ = "models/cast_%d.py: CAST%d(usernum, itemnum, ratingnum, args, reuse=None)." % (n, n)

        def __init__(self, usernum, itemnum, ratingnum, args, reuse=None, **kw):
            self.ratingnum = ratingnum
            super().__init__(usernum, itemnum, args, reuse, **kw)
    _C.__name__ = "CAST%d" % n
    return _C


CAST1, CAST2, CAST3, CAST4, CAST5, CAST6, CAST7, CAST8, CAST9 = (_cast(n) for n in range(1, 10))


def build_model(name, usernum, itemnum, ratingnum, args, **kw):
    """The registry of main.py:121-142."""
    name = name.lower()
    if name not in MODELS:
        raise ValueError("provide model from %s" % MODELS)
    if name == "sasrec":
        return SASRec(usernum, itemnum, args, **kw)
    if name == "sasrec_static":
        return SASRec(usernum, itemnum, args, static=True, **kw)
    return globals()["CAST%s" % name.split("_")[1]](usernum, itemnum, ratingnum, args, **kw)

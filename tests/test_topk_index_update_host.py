"""Keeping an item index in step with training, without a GPU (castrec.h cr_topk_index_update, cr_topk_index_sync; ItemIndex.update;
Model.refresh_item_index / item_delta): both C entries refuse a bad call before any HIP call, ItemIndex.update refuses bad arguments
before it looks at the device, and the token logic decides "sync" or "rebuild" on a stub engine."""
import ctypes
import types

import numpy as np
import pytest
import torch

import castrec_amd  # noqa: F401
from castrec_amd import lib as L
from castrec_amd.index import ItemIndex
from castrec_amd.models import IndexToken, _Model
from topk_harness import rejects
import topk_index_ref as R

P = 0x1000                       # a fake non-NULL pointer: never dereferenced, every call below is refused first
V, D, PREC = 37, 50, L.PREC_BF16X3
NB = R.index_bytes(V, D, PREC)


def _update(src=P, packed=0, V=V, D=D, prec=PREC, index=P, nb=NB, ids=P, n=3):
    return ("cr_topk_index_update", src, packed, V, D, prec, index, nb, ids, n, None)


def _sync(table=P, V=V, D=D, prec=PREC, index=P, nb=NB, flags=P, since=1):
    return ("cr_topk_index_sync", table, V, D, prec, index, nb, flags, since, None)


def test_the_size_is_the_layouts():
    assert L.lib.cr_topk_index_bytes(V, D, PREC) == NB


@pytest.mark.parametrize("kw", [dict(src=None), dict(index=None), dict(ids=None)])
def test_update_refuses_null_pointers(kw):
    rejects(_update(**kw), "NULL")
    rejects(_update(packed=1, **kw), "NULL")


@pytest.mark.parametrize("kw", [dict(table=None), dict(index=None), dict(flags=None)])
def test_sync_refuses_null_pointers(kw):
    rejects(_sync(**kw), "NULL")


@pytest.mark.parametrize("n", [0, -1, -2 ** 31])
def test_update_refuses_an_empty_list(n):
    rejects(_update(n=n), "n=%d" % n, ">= 1")


@pytest.mark.parametrize("call", [_update, _sync])
def test_both_refuse_a_bad_shape_or_precision(call):
    for d in (7, 257, 0, -8):
        rejects(call(D=d, nb=NB), "D=%d" % d, "8 .. 256")
    for v in (0, -1):
        rejects(call(V=v, nb=NB), "V=%d" % v, ">= 1")
    for p in (3, -1, 17):
        rejects(call(prec=p), "unknown precision %d" % p)


@pytest.mark.parametrize("call", [_update, _sync])
def test_both_want_exactly_the_index_bytes(call):
    for nb in (NB - 1, NB + 1, NB + 1024, 0, R.index_bytes(V, D, L.PREC_BF16)):
        rejects(call(nb=nb), "index_bytes=%d" % nb, "%d" % NB)
    rejects(call(prec=L.PREC_BF16), "index_bytes=%d" % NB)             # the split size against a plain index
    rejects(call(V=V + 16), "index_bytes")                             # one tile more
    rejects(call(D=D + 32), "index_bytes")                             # NK 2 -> 4


# ---- ItemIndex.update: arguments are judged before the device -------------------------------------------------------------------
def _cpu_index():
    return ItemIndex(V, D, "bf16x3", torch.zeros(NB, dtype=torch.uint8))


def test_update_takes_exactly_one_source():
    ix = _cpu_index()
    rows = np.zeros((2, D), np.float32)
    with pytest.raises(ValueError, match="neither"):
        ix.update([1, 2])
    with pytest.raises(ValueError, match="both"):
        ix.update([1, 2], rows=rows, table=torch.zeros(V, D))


@pytest.mark.parametrize("ids", [[0], [1, 0, 2], [V], [1, V + 5], [-1], []])
def test_update_refuses_ids_outside_the_items(ids):
    ix = _cpu_index()
    with pytest.raises(ValueError):
        ix.update(ids, rows=np.zeros((len(ids), D), np.float32))
    with pytest.raises(ValueError):
        ix.update(np.asarray(ids, np.int64), table=torch.zeros(V, D))


@pytest.mark.parametrize("shape", [(3, D), (2, D + 1), (2 * D,), (2, D, 1)])
def test_update_refuses_rows_of_the_wrong_shape(shape):
    with pytest.raises(ValueError, match="rows must be"):
        _cpu_index().update([1, 2], rows=np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="rows must be"):
        _cpu_index().update([1, 2], rows=torch.zeros(2, D, dtype=torch.float64))


def test_an_index_loaded_on_the_cpu_is_not_rewritten():
    ix = _cpu_index()
    t = torch.zeros(V, D)
    for call in (lambda: ix.update([1, 2], rows=np.zeros((2, D), np.float32)), lambda: ix.sync(t, torch.zeros(V, dtype=torch.int32), 1),
                 lambda: ix.rebuild(t)):
        with pytest.raises(RuntimeError, match="loaded on the CPU"):
            call()
    assert ix.version is None and ix.token is None


# ---- the token: Model.refresh_item_index and item_delta on a stub engine ------------------------------------------------------
class _Engine(object):
    def __init__(self, lazy=True, step=5):
        self.lazy_adam, self.flags_epoch, self._step = lazy, 3, step
        self.lazy_flags = torch.zeros(V, dtype=torch.int32) if lazy else None

    def step_number(self):
        return self._step


def _stub(engine):
    """A _Model without a device: the attributes refresh_item_index reads, an ItemIndex whose sync / rebuild only record the call."""
    m = object.__new__(_Model)
    m.itemnum, m._param_version, m._table_epoch, m._flags_epoch0, m._train = V - 1, 11, 2, 3, engine
    table = torch.arange(V * D, dtype=torch.float32).reshape(V, D)
    m._owner = types.SimpleNamespace(D=D, p=lambda name: table)
    ix, calls = _cpu_index(), []

    def sync(tab, flags, since, version=None):
        calls.append(("sync", since))
        assert tab is table and flags is engine.lazy_flags
        ix.version = version

    def rebuild(tab, version=None):
        calls.append(("rebuild",))
        assert tab is table
        ix.version = version

    ix.sync, ix.rebuild = sync, rebuild
    return m, ix, calls


def test_a_matching_token_syncs_from_its_step():
    eng = _Engine()
    m, ix, calls = _stub(eng)
    assert m._index_token() == IndexToken(2, 0, 5)
    ix.token = m._index_token()
    eng._step, m._param_version = 8, 14                                  # three steps later
    assert m.refresh_item_index(ix) == "sync" and calls == [("sync", 5)]
    assert ix.version == 14 and ix.token == IndexToken(2, 0, 8)
    assert m.refresh_item_index(ix) == "sync" and calls[-1] == ("sync", 8)


def test_a_token_from_before_the_engine_counts_from_step_one():
    m, ix, calls = _stub(None)
    ix.token = m._index_token()
    assert ix.token == IndexToken(2, 0, 1)
    assert m.refresh_item_index(ix) == "rebuild"                         # no engine, no flags
    # ... and once the engine exists (made with flags_epoch 3, no step run yet), every flag it has set since is >= 1
    m2, ix2, calls2 = _stub(_Engine(step=4))
    ix2.token = IndexToken(2, 0, 1)
    assert m2.refresh_item_index(ix2) == "sync" and calls2 == [("sync", 1)] and ix2.token == IndexToken(2, 0, 4)


@pytest.mark.parametrize("what", ["table_epoch", "flags_epoch", "token step None", "no token", "dense", "step None now"])
def test_everything_else_rebuilds(what):
    eng = _Engine(lazy=(what != "dense"))
    m, ix, calls = _stub(eng)
    ix.token = IndexToken(2, 0, 5)
    if what == "table_epoch":
        m._table_epoch += 1                                              # load / load_tf_checkpoint / load_params
    elif what == "flags_epoch":
        eng.flags_epoch += 1                                             # set_step zeroed the flags
    elif what == "token step None":
        ix.token = IndexToken(2, 0, None)
    elif what == "no token":
        ix.token = None
    elif what == "step None now":
        m._index_token = lambda: IndexToken(2, 0, None)
    eng._step = 9
    assert m.refresh_item_index(ix) == "rebuild" and calls == [("rebuild",)]
    assert ix.version == 11 and ix.token == m._index_token()
    if what != "no token" and what != "token step None":
        with pytest.raises(RuntimeError, match="item_delta: "):
            m.item_delta(IndexToken(2, 0, 5))


def test_refresh_checks_the_shape_first():
    m, ix, calls = _stub(_Engine())
    m.itemnum += 1
    with pytest.raises(ValueError, match="index of a"):
        m.refresh_item_index(ix)
    with pytest.raises(TypeError):
        m.refresh_item_index(None)
    assert calls == []


def test_item_delta_names_the_rows_with_a_flag_from_the_tokens_step_on():
    eng = _Engine(step=9)
    m, ix, _ = _stub(eng)
    eng.lazy_flags[[3, 4, 5, 20]] = torch.tensor([4, 5, 6, 8], dtype=torch.int32)
    ids, rows, now = m.item_delta(IndexToken(2, 0, 5))
    assert ids.dtype == torch.int32 and ids.tolist() == [4, 5, 20] and now == IndexToken(2, 0, 9)
    assert rows.dtype == torch.float32 and torch.equal(rows, m._owner.p("item_emb")[[4, 5, 20]])
    ids, rows, _ = m.item_delta(now)
    assert ids.numel() == 0 and tuple(rows.shape) == (0, D)
    for bad, word in ((IndexToken(1, 0, 5), "table epoch"), (IndexToken(2, 1, 5), "flags epoch")):
        with pytest.raises(RuntimeError, match=word):
            m.item_delta(bad)
    eng.lazy_adam = False
    with pytest.raises(RuntimeError, match="dense Adam"):
        m.item_delta(IndexToken(2, 0, 5))


def test_engine_counts_where_it_clears_the_flags():
    """set_step is the only place that zeroes lazy_flags: the epoch is bumped there and nowhere else."""
    import inspect
    from castrec_amd import engine as E
    src = inspect.getsource(E.Engine.set_step)
    assert src.count("self.lazy_flags.zero_()") == 1 and src.count("self.flags_epoch += 1") == 1
    assert inspect.getsource(E.Engine).count("lazy_flags.zero_()") == 1


def test_main_keeps_one_index(capsys):
    import main as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    assert "keep one item index" in capsys.readouterr().out

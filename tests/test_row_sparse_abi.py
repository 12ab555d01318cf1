"""Row-sparse Adam's second id list (include/castrec.h cr_adam_desc.lazy_ids2) and its public spelling, without a GPU: cr_adam_step
refuses a bad description before any HIP call, Hyper carries the option, main.py lists the flag."""
import ctypes

import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L


def _desc():
    """A description that passes every check in front of the lazy-row ones (host pointers: no launch is reached)."""
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    ad = L.AdamDesc()
    ad.p = ad.m = ad.v = ad.state = ad.table_grad = p
    ad.n_table, ad.lazy_ids, ad.lazy_flags, ad.n_lazy_ids, ad.lazy_rows, ad.lazy_D = 8, p, p, 4, 2, 4
    return ad, p, buf


def _refused(ad):
    rc = L.lib.cr_adam_step(ctypes.byref(ad), None)
    return rc, L.lib.cr_last_error()


def test_second_list_needs_the_first():
    ad, p, _keep = _desc()
    ad.lazy_ids, ad.n_lazy_ids = None, 0
    ad.lazy_ids2, ad.n_lazy_ids2 = p, 4
    rc, msg = _refused(ad)
    assert rc == -1 and b"lazy_ids2" in msg and b"needs lazy_ids" in msg, msg


@pytest.mark.parametrize("n2", [0, -5])
def test_second_list_needs_a_count(n2):
    ad, p, _keep = _desc()
    ad.lazy_ids2, ad.n_lazy_ids2 = p, n2
    rc, msg = _refused(ad)
    assert rc == -1 and b"lazy_ids2" in msg and b"n_lazy_ids2" in msg, msg


@pytest.mark.parametrize("n1,n2", [(2 ** 31 - 1, 1), (2 ** 30, 2 ** 30), (1, 2 ** 31 - 1)])
def test_the_two_counts_must_fit_an_int(n1, n2):
    ad, p, _keep = _desc()
    ad.n_lazy_ids = n1
    ad.lazy_ids2, ad.n_lazy_ids2 = p, n2
    rc, msg = _refused(ad)
    assert rc == -1 and b"lazy_ids2" in msg and b"fit an int" in msg, msg


def test_the_exclusions_of_the_first_list_hold_with_a_second():
    """The id ring inside the Adam launch stays excluded (tests/test_abi.py pins it for one list)."""
    ad, p, _keep = _desc()
    ad.lazy_ids2, ad.n_lazy_ids2 = p, 4
    ad.ids_ring, ad.ids_ring_slots, ad.ids_slot_elems, ad.ids_dst = p, 2, 8, p + 64
    rc, msg = _refused(ad)
    assert rc == -1 and b"exclude each other" in msg, msg


def test_the_fields_close_the_struct():
    """Positional initialisers of the fields in front keep their meaning: the two new ones come last."""
    names = [n for n, _ in L.AdamDesc._fields_]
    assert names[-2:] == ["lazy_ids2", "n_lazy_ids2"] and names[-3] == "tg"
    ad = L.AdamDesc(None, None, None, None, None, 5)
    assert ad.n_table == 5 and not ad.lazy_ids2 and ad.n_lazy_ids2 == 0


def test_hyper_carries_the_option():
    import types
    from castrec_amd.engine import Hyper
    assert Hyper().row_sparse_adam is False
    assert Hyper(row_sparse_adam=True).row_sparse_adam is True
    assert Hyper(types.SimpleNamespace(row_sparse_adam=True)).row_sparse_adam is True


def test_main_lists_the_flag(capsys):
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--row_sparse_adam" in out and "deviation" in out
    base = ["--dataset", "synthetic:tiny", "--train_dir", "t", "--model", "sasrec"]
    assert cli.parse_args(base).row_sparse_adam is False
    assert cli.parse_args(base + ["--row_sparse_adam"]).row_sparse_adam is True

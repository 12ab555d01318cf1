"""The Adam reference and comparator of tests/adam_ref.py, checked without a GPU: the reference against oracle.fpmodel.AdamTF, the
op-by-op fp32 rounding of the reference accepted under the bounds, and every mutant -- a wrong step of the kinds a kernel gets wrong --
rejected with a margin of at least 100 bounds, on one input of every family tests/test_adam_gpu.py runs on the kernel."""
import numpy as np
import pytest

import adam_ref as A

L2 = 0.05
COMMON = ("inv_n_dropped", "beta2_0.999", "t_off_by_one", "l2_dropped", "n_l2_off_by_one")
LAZY_IDS = np.array([3, 7, 7, 0, 9, 12, 3, 41, -2, 40, 7], np.int32)


def _families():
    """name -> (case, the mutants that apply to it).  t = 3 and n_target = 16 or 37: a step early enough and a count large enough
    for `t off by one` (lr_t: 0.895 lr against 0.810 lr) and `inv_n dropped` to matter."""
    f = {}
    f["plain"] = (A.make_case(1, 4099, 130, l2=L2, n_l2=4099 + 8),
                  COMMON + ("one_slab_dropped", "tail_not_updated", "after_table_by_table_rule"))
    f["l2_inside_group"] = (A.make_case(2, 301, 130, l2=L2, n_l2=2), COMMON + ("tail_not_updated",))
    f["dense"] = (A.make_case(3, 301, 1027, n_slabs=17, slab_counts=[0, 1, 17, 17, 5], l2=L2, n_l2=301 + 1027),
                  COMMON + ("slab_counts_ignored", "one_slab_dropped"))      # (block 0 counts no slab: element n_table has G = 0 anyway)
    f["scalars"] = (A.make_case(4, 303, 130, n_target=37.0, stats_mode="self", l2=L2, n_l2=303), COMMON + ("tail_not_updated",))
    f["lazy"] = (A.make_case(5, 41 * 7 + 5 * 7, 130, l2=L2, n_l2=41 * 7 + 5 * 7, lazy=(41, 7, LAZY_IDS)),
                 COMMON + ("lazy_duplicate_twice", "lazy_id0_applied", "tail_not_updated", "one_slab_dropped"))
    f["tg"] = (A.make_case(6, (300 + 25) * 20, 130, l2=L2, n_l2=(300 + 25) * 20 + 8, tg=A.make_tg(6, 20, 300, 25)),
               COMMON + ("unitless_rows_not_moved", "one_slab_dropped", "after_table_by_table_rule"))
    return f


FAMILIES = _families()
PAIRS = [(name, mut) for name, (_, muts) in FAMILIES.items() for mut in muts]


def test_every_mutant_is_used():
    assert {m for _, m in PAIRS} == set(A.MUTANTS)


def test_reference_equals_adamtf_over_three_steps():
    """Hyperparameters that are exact in fp32 (the reference takes them at their float32 values), zero moments, no l2, n_target = 1."""
    import torch
    from oracle import fpmodel as fm
    rs = np.random.RandomState(0)
    nt, nd, ns = 301, 130, 6
    c = A.make_case(0, nt, nd, n_slabs=ns, n_target=1.0, t=1, lr=2.0 ** -7)
    c.beta1, c.beta2, c.eps = 0.875, 0.96875, 2.0 ** -27
    c.m0[:] = 0.0
    c.v0[:] = 0.0
    P = {"w": torch.tensor(c.p0.astype(np.float64))}
    opt = fm.AdamTF(P, lr=c.lr, beta1=c.beta1, beta2=c.beta2, eps=c.eps)
    for step in range(1, 4):
        c.t = step
        c.table_grad = A.dyadic(rs, nt)
        c.slabs = A.dyadic(rs, (ns, nd))
        out = A.reference(c)
        P = opt.step(P, {"w": torch.tensor(np.r_[c.table_grad.astype(np.float64), c.slabs.astype(np.float64).sum(0)])})
        np.testing.assert_allclose(out.p, P["w"].numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(out.m, opt.m["w"].numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(out.v, opt.v["w"].numpy(), rtol=1e-13, atol=1e-15)
        assert out.grad_zeroed.all() and out.updated.all() and out.state04 is None
        c.p0, c.m0, c.v0 = out.p, out.m, out.v


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_fp32_rounded_reference_is_accepted(name):
    """What a correct fp32 kernel may compute -- every operation of the reference rounded to fp32 -- lies within the bounds."""
    c = FAMILIES[name][0]
    ref = A.reference(c)
    r32 = A.reference(c, dtype=np.float32)
    assert r32.p.dtype == np.float32
    ratio, which, i = A.worst_ratio(dict(p=r32.p, m=r32.m, v=r32.v), ref)
    print("%s: fp32 rounding reaches %.3f of the bound (%s[%d])" % (name, ratio, which, i))
    assert ratio <= 1.0, (ratio, which, i)
    assert A.accepted(dict(p=ref.p, m=ref.m, v=ref.v), ref)
    assert (ref.bp[ref.updated] > 0).all() and (ref.bp[~ref.updated] == 0).all()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_large_step_numbers_and_no_targets(name):
    """b1^t underflows to 0 in fp32 at t = 200000 (lr_t = lr); n_target = 0 is a pure momentum step: both accepted when rounded to fp32."""
    import copy
    c = copy.copy(FAMILIES[name][0])
    for t, n_target in ((200000, 16.0), (1000, 0.0), (1, 37.0)):
        c.t, c.n_target = t, n_target
        ref = A.reference(c)
        r32 = A.reference(c, dtype=np.float32)
        assert A.accepted(dict(p=r32.p, m=r32.m, v=r32.v), ref), (t, n_target)
        assert np.isfinite(ref.p).all()
        if n_target == 0.0:
            assert ref.state5 == c.state7 and ref.state6 == 0.0


@pytest.mark.parametrize("name,mutant", PAIRS)
def test_mutant_is_rejected(name, mutant):
    """The comparator under the reference's bounds tells every mutant from the step: some element is off by at least 100 bounds."""
    c = FAMILIES[name][0]
    ref = A.reference(c)
    bad = A.reference(c, mutant=mutant)
    ratio, which, i = A.worst_ratio(dict(p=bad.p, m=bad.m, v=bad.v), ref)
    print("%s / %s: %.3g bounds at %s[%d]" % (name, mutant, ratio, which, i))
    assert not A.accepted(dict(p=bad.p, m=bad.m, v=bad.v), ref)
    assert ratio >= 100.0, (ratio, which, i)
    # ... and from its fp32 rounding as well (the margin does not come from the mutant's fp64 arithmetic)
    bad32 = A.reference(c, mutant=mutant, dtype=np.float32)
    assert A.worst_ratio(dict(p=bad32.p, m=bad32.m, v=bad32.v), ref)[0] >= 100.0


def test_lazy_rows_of_the_reference():
    """Listed ids in 1 .. rows - 1 once; ids 0, rows, negative ignored; unlisted rows keep their gradient."""
    c = FAMILIES["lazy"][0]
    ref = A.reference(c)
    D, rows = c.lazy.D, c.lazy.rows
    touched = np.zeros(rows, bool)
    touched[[3, 7, 9, 12, 40]] = True
    assert np.array_equal(ref.updated[:rows * D].reshape(rows, D).all(1), touched)
    assert np.array_equal(ref.grad_zeroed[:rows * D], np.repeat(touched, D)) and ref.grad_zeroed[rows * D:].all()
    assert ref.updated[rows * D:].all()
    assert np.array_equal(np.flatnonzero(ref.lazy_flags), [3, 7, 9, 12, 40]) and (ref.lazy_flags[touched] == c.t).all()
    assert np.array_equal(ref.p[:D], c.p0[:D].astype(np.float64))

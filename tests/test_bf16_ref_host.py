"""The rounding model of plain bf16 (tests/bf16_ref.py) checked on the CPU: the rounding itself against an integer implementation
over every bf16 bit pattern, RoundedMM with the rounding off against torch.matmul's own autograd, the oracle's product hook at its
default -- and the bound the GPU tests hold the kernels to (tests/test_bf16_envelope_gpu.py): at every shape of bf16_ref.SHAPES it
has ROOM for a correct kernel (the model under seeded stochastic rounding: another realisation of the same noise), its CAP stays at
half the smallest size the round-5 dW2 defect was recorded at, and it has TEETH: one 16 x 16 tile of one weight gradient off by 20 %
fails it, where the global-scale bound it replaces let that pass."""
import numpy as np
import pytest
import torch

import bf16_ref as br
from oracle import fpmodel as fm


# ---------------------------------------------------------------------------------------------------------------------------
# bf16_rne
# ---------------------------------------------------------------------------------------------------------------------------
def rne_bits(u):
    """fp32 bit patterns (uint64 array) -> bf16 bit patterns: add 0x7FFF + lsb, shift; NaN stays NaN"""
    u = u.astype(np.uint64)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint64) & 0xFFFF


def f32_of_bits(u):
    return np.asarray(u, dtype=np.uint64).astype(np.uint32).view(np.float32)


def check_against_integer_rounding(u):
    x = f32_of_bits(u)
    got = br.bf16_rne(torch.tensor(x.astype(np.float64))).numpy()
    want = f32_of_bits(rne_bits(u) << 16).astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))          # -0 stays -0


def test_bf16_rne_on_every_bf16_pattern_its_midpoints_and_their_neighbours():
    pats = np.arange(1 << 16, dtype=np.uint64) << 16
    check_against_integer_rounding(pats)                                            # a bf16 value is a fixed point (subnormals, +-0, +-inf, NaN among them)
    x = f32_of_bits(pats).astype(np.float64)
    fin = np.isfinite(x)
    assert np.array_equal(br.bf16_rne(torch.tensor(x[fin])).numpy(), x[fin])
    for off in (0x8000, 0x7FFF, 0x8001, 1, 0xFFFF):                                 # the midpoint to the next pattern in magnitude (ties to even:
        check_against_integer_rounding(pats + off)                                  # down from an even pattern, up from an odd one), +- 1 fp32 ulp, the ends
    mid = br.bf16_rne(torch.tensor(f32_of_bits(pats + 0x8000).astype(np.float64))).numpy()
    even = (((pats >> 16) & 1) == 0) & ((pats & 0x7F800000) != 0x7F800000)
    assert np.array_equal(mid[even], x[even])
    odd = ~even & ((pats & 0x7F800000) != 0x7F800000)
    assert np.array_equal(mid[odd], f32_of_bits(pats[odd] + 0x10000).astype(np.float64))


def test_bf16_rne_special_values():
    big = float(f32_of_bits([0x7F7F0000])[0])                                       # largest finite bf16
    x = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), big, -big,
                      float(f32_of_bits([0x7F7F8000])[0]), float(f32_of_bits([0x7F7FFFFF])[0]), -float(f32_of_bits([0x7F7F8001])[0]),
                      float(f32_of_bits([0x7F7F7FFF])[0]), 1e39, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -150], dtype=torch.float64)
    y = br.bf16_rne(x).numpy()
    assert y[0] == 0 and not np.signbit(y[0]) and y[1] == 0 and np.signbit(y[1])
    assert y[2] == np.inf and y[3] == -np.inf and np.isnan(y[4]) and y[5] == big and y[6] == -big
    assert y[7] == np.inf and y[8] == np.inf and y[9] == -np.inf                    # fp32 values above the largest finite bf16 (from its midpoint on)
    assert y[10] == big and y[11] == np.inf                                         # (1e39: beyond fp32 as well)
    assert y[12] == 2.0 ** -133 and y[13] == 0.0 and y[14] == 2.0 ** -133 and y[15] == 0.0     # smallest subnormal; its half ties to even = 0
    sub = np.arange(0, 0x00800000, 0x101, dtype=np.uint64)                          # fp32 subnormals, both signs
    check_against_integer_rounding(sub)
    check_against_integer_rounding(sub | 0x80000000)


def test_bf16_rne_jitter_is_seeded_and_bounded():
    x = torch.linspace(-3, 3, 1001, dtype=torch.float64)
    a = br.bf16_rne(x, (torch.Generator().manual_seed(1), 2.0 ** -20))
    b = br.bf16_rne(x, (torch.Generator().manual_seed(1), 2.0 ** -20))
    assert torch.equal(a, b)
    assert bool(((a - x).abs() <= x.abs() * (2.0 ** -8 + 2.0 ** -19)).all())        # half a bf16 ulp (at most 2^-8 of the value) + the jitter
    assert torch.equal(br.bf16_rne(x, (torch.Generator().manual_seed(1), 0.0)), br.bf16_rne(x))


def test_stochastic_rounding_lands_on_a_neighbour_and_is_unbiased():
    x = torch.tensor(np.random.RandomState(0).standard_normal(20000))
    lo = f32_of_bits(x.float().numpy().view(np.uint32).astype(np.uint64) & 0xFFFF0000).astype(np.float64)
    hi = f32_of_bits((x.float().numpy().view(np.uint32).astype(np.uint64) & 0xFFFF0000) + 0x10000).astype(np.float64)
    y = br.bf16_stochastic(torch.Generator().manual_seed(3))(x).numpy()
    assert np.all((y == lo) | (y == hi))
    assert abs(float((y - x.numpy()).mean())) < 4 * 2.0 ** -9 / np.sqrt(20000)


# ---------------------------------------------------------------------------------------------------------------------------
# RoundedMM, the hook
# ---------------------------------------------------------------------------------------------------------------------------
def _operands(kind, rs):
    if kind == "rows x weight":                          # projections, feed-forward, mlp: [N, T, C] @ [C, C']
        return torch.tensor(rs.standard_normal((3, 7, 5))), torch.tensor(rs.standard_normal((5, 6))), lambda b: b
    if kind == "scores":                                 # Q_ @ K_^T: [hN, T, d] @ a transposed view of [hN, T, d]
        return torch.tensor(rs.standard_normal((4, 7, 5))), torch.tensor(rs.standard_normal((4, 7, 5))), lambda b: b.transpose(1, 2)
    return torch.tensor(rs.standard_normal((4, 7, 7))), torch.tensor(rs.standard_normal((4, 7, 5))), lambda b: b      # probabilities @ V_


@pytest.mark.parametrize("kind", ["rows x weight", "scores", "probabilities x V"])
def test_rounded_mm_without_rounding_is_torch_matmul_under_autograd(kind):
    rs = np.random.RandomState(4)
    a0, b0, view = _operands(kind, rs)
    res = []
    for mm in (torch.matmul, lambda a, b: br.RoundedMM.apply(a, b, br.EXACT)):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = mm(a, view(b))
        (y * torch.tensor(np.random.RandomState(5).standard_normal(tuple(y.shape)))).sum().backward()
        res.append((y.detach(), a.grad, b.grad))
    for u, v in zip(*res):
        assert u.shape == v.shape and torch.equal(u, v)


@pytest.mark.parametrize("kind", ["rows x weight", "scores", "probabilities x V"])
def test_rounded_mm_rounds_what_its_switches_say(kind):
    rs = np.random.RandomState(6)
    a0, b0, view = _operands(kind, rs)
    bf = br.bf16_rne
    w = torch.tensor(rs.standard_normal(tuple(torch.matmul(a0, view(b0)).shape)))

    def go(r):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = br.RoundedMM.apply(a, view(b), r)
        y.backward(w)
        return y.detach(), a.grad, b.grad

    def sum_b(x):                                        # the weight's gradient sums over the batch; a 3-D operand's does not
        return x.sum(0) if b0.dim() == 2 else x
    back = (lambda x: x.transpose(1, 2)) if kind == "scores" else (lambda x: x)
    B = view(b0)
    y, ga, gb = go(br.Rounding(fwd=True, bwd=True))
    assert torch.equal(y, torch.matmul(bf(a0), bf(B)))
    assert torch.allclose(ga, torch.matmul(bf(w), bf(B).transpose(-1, -2)), rtol=1e-13, atol=1e-13)
    assert torch.allclose(gb, back(sum_b(torch.matmul(bf(a0).transpose(-1, -2), bf(w)))), rtol=1e-13, atol=1e-13)
    y, ga, gb = go(br.Rounding(fwd=True, bwd=False))     # forward only: the backward products take the values as they are
    assert torch.equal(y, torch.matmul(bf(a0), bf(B)))
    assert torch.allclose(ga, torch.matmul(w, B.transpose(-1, -2)), rtol=1e-13, atol=1e-13)
    assert torch.allclose(gb, back(sum_b(torch.matmul(a0.transpose(-1, -2), w))), rtol=1e-13, atol=1e-13)
    # jitter reaches the operands marked as intermediates and no other
    jit = lambda: (torch.Generator().manual_seed(9), 2.0 ** -9)
    y0 = go(br.Rounding())[0]
    assert torch.equal(go(br.Rounding(jitter=jit()))[0], y0)
    y1 = go(br.Rounding(a_inter=True, jitter=jit()))[0]
    assert not torch.equal(y1, y0) and torch.equal(y1, torch.matmul(bf(a0, jit()), bf(B)))
    y2 = go(br.Rounding(b_inter=True, jitter=jit()))[0]
    assert not torch.equal(y2, y0)
    y3, ga3, gb3 = go(br.Rounding(g_inter=True, jitter=jit()))
    assert torch.equal(y3, y0) and not torch.equal(ga3, go(br.Rounding())[1])


@pytest.mark.parametrize("model", ["sasrec", "cast_1", "cast_4"])
def test_the_product_hook_at_its_default_changes_no_bit(model, monkeypatch):
    rs = np.random.RandomState(2)
    hp = fm.Hyper(maxlen=24, hidden_units=20, num_blocks=2, num_heads=2, dropout_rate=0.0, max_bins=9, num_context_blocks=1)
    P = fm.init_params(model, 9, 37, hp, seed=3)
    P = {k: v + 0.1 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
    batch = fm.to_batch(*br.make_batch(rs, 4, 24, 37, 9))
    assert fm.MM_PRODUCT is None
    out, G = fm.loss_and_grads(model, P, hp, batch)
    sites = []

    def plain(a, b, site):                              # an unhooked run: the operator itself
        sites.append(site)
        return a @ b
    monkeypatch.setattr(fm, "_mm", plain)
    out1, G1 = fm.loss_and_grads(model, P, hp, batch)
    monkeypatch.undo()
    with fm.rounded_products(lambda a, b, site: br.RoundedMM.apply(a, b, br.EXACT)):      # ... and the hook with the rounding off
        out2, G2 = fm.loss_and_grads(model, P, hp, batch)
    assert fm.MM_PRODUCT is None
    for o, g in ((out1, G1), (out2, G2)):
        assert torch.equal(o["loss"], out["loss"]) and torch.equal(o["seq_emb"], out["seq_emb"])
        assert all(torch.equal(g[k], G[k]) for k in G)
    n_stacks = 1 if model == "sasrec" else 2
    assert len(sites) == 7 * 2 * n_stacks + (2 if model == "cast_4" else 0)      # q k v scores pv w1 w2 per block (+ the CAST mlp)
    with fm.rounded_products(br.product()):
        out3, _ = fm.loss_and_grads(model, P, hp, batch)
    assert not torch.equal(out3["loss"], out["loss"])


def test_the_attention_only_variant_rounds_two_products_per_block_and_only_widens_the_envelope():
    shape = ("cast_1", 20, 2, 24, 3, 2)
    P, hp, b = br.draw_case(*shape)
    batch = fm.to_batch(*b)
    gates = br.own_gates("cast_1", P, hp, batch, None)
    rounded = []
    prod = br.product(sites=br.ATTENTION_SITES)
    with fm.rounded_products(lambda a, b_, site: (rounded.append(site) if site.endswith(br.ATTENTION_SITES) else None, prod(a, b_, site))[1]):
        fm.loss_and_grads("cast_1", P, hp, batch)
    assert len(rounded) == 2 * 2 * 2 and all(s.endswith((".attn.scores", ".attn.pv")) for s in rounded)
    _, _, E3, act3, loss3 = br.envelope("cast_1", P, hp, batch, None, gates, None)
    _, _, E4, act4, loss4 = br.envelope("cast_1", P, hp, batch, None, gates, None, fp32_row_phases=True)
    assert all(E4[k] >= E3[k] for k in E3) and act4 >= act3 and loss4 >= loss3
    out0, G0 = br.run("cast_1", P, hp, batch, None, gates, None)
    e, _, _ = br.deviation(*br.run("cast_1", P, hp, batch, None, gates, None, prod), out0, G0, br.denominators(G0))
    assert all(E4[k] >= e[k] for k in e) and max(e.values()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# room, cap, teeth
# ---------------------------------------------------------------------------------------------------------------------------
_CASES = {}
WEIGHTS = (".w1", ".w2", ".wq", ".wk", ".wv")
OLD_GLOBAL_BOUND = 2e-1          # TOL["bf16"]["grad"] of tests/test_model_gpu.py until this bound replaced it: of the GLOBAL gradient scale


def case(shape):
    """One exact run, the envelope's three model runs and the two stand-ins per shape, shared by the tests below (dropout 0, the exact
    run's own ReLU gates in every run: one flipped gate moves w1 / b1 gradients by 6-26 %, which is no rounding error)."""
    if shape not in _CASES:
        model = shape[0]
        P, hp, b = br.draw_case(*shape)
        batch = fm.to_batch(*b)
        gates = br.own_gates(model, P, hp, batch, None)
        out0, G0, E, E_act, E_loss = br.envelope(model, P, hp, batch, None, gates, None)
        stand_ins = [br.run(model, P, hp, batch, None, gates, None, br.product(rnd=br.bf16_stochastic(torch.Generator().manual_seed(seed))))
                     for seed in (1, 2)]
        _CASES[shape] = (out0, G0, E, E_act, E_loss, stand_ins)
    return _CASES[shape]


@pytest.mark.parametrize("shape", br.SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_room_a_correct_kernel_passes_the_bound(shape):
    out0, G0, E, E_act, E_loss, stand_ins = case(shape)
    den = br.denominators(G0)
    for out, G in stand_ins:
        rep = br.grad_report(G, G0, E)
        print(shape, "worst share of the bound: %.2f (%s: error %.3g, E %.3g)" % (rep[0][0], rep[0][1], rep[0][2], rep[0][3]))
        assert rep[0][0] <= 1.0, rep[:4]
        _, act, loss = br.deviation(out, G, out0, G0, den)
        assert act <= br.GRAD_FACTOR * E_act + br.ACT_ABS and loss <= br.GRAD_FACTOR * E_loss + br.LOSS_ABS, (act, E_act, loss, E_loss)


@pytest.mark.parametrize("shape", br.SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_cap_no_bound_reaches_half_the_recorded_defect(shape):
    """A condition on the draw, not a measurement: the round-5 defect was 0.2 to 0.86 of dW2's largest entry."""
    _, G0, E, _, _, _ = case(shape)
    bound = br.grad_bound(E)
    worst = max((bound[k], k) for k in G0 if not k.endswith(".bk"))
    assert worst[0] <= 1e-1, worst


@pytest.mark.parametrize("shape", br.SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_teeth_one_tile_of_one_weight_gradient_off_by_a_fifth(shape):
    _, G0, E, _, _, stand_ins = case(shape)
    G = stand_ins[0][1]
    gmax = max(float(G0[k].abs().max()) for k in G0)
    names = [k for k in G0 if k.endswith(WEIGHTS)]
    assert len(names) >= 5 * shape[5]                   # (the CAST mlp's two weights count as w1 / w2)
    passes_old = []
    for k in names:
        i, j = np.unravel_index(int(G0[k].abs().argmax()), tuple(G0[k].shape))      # the tile that holds the parameter's largest entry
        i, j = i // 16 * 16, j // 16 * 16
        mutant = dict(G)
        mutant[k] = G[k].clone()
        mutant[k][i:i + 16, j:j + 16] *= 1.2
        rep = br.grad_report(mutant, G0, E)
        assert rep[0][0] > 1.0 and rep[0][1] == k, (k, rep[:3])
        if max(float((mutant[n] - G0[n]).abs().max()) for n in G0 if not n.endswith(".bk")) < OLD_GLOBAL_BOUND * gmax:
            passes_old.append(k)
    # the gap being closed: the query projection of the first block (no weight gradient is the largest gradient of its graph -- the
    # embedding tables' and the LayerNorm gains' are) was free to be 20 % off in a tile under the global-scale bound
    assert "trunk.0.wq" in passes_old, passes_old

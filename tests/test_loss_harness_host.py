"""loss_ref.check can fail (no GPU, no native library): on the smallest shape that has a padded row, a repeated target, a duplicate
sample and an accidental hit, each reference's own fp64 values cast to fp32 pass at 4x the bounds, and one element of the per-row
loss, of dh, of tg or of state[0] pushed to 4.5x its bound is refused by name."""
import re

import numpy as np
import pytest

import gbce_ref
import loss_ref

M, D, V, N = 7, 8, 17, 5
SEED = 3              # (the first seed that leaves four live rows of the seven: the makers plant the repeat and the hit from four on)


def _softmax():
    h, E_, pos, neg = loss_ref.ce_case(D, V, M, SEED)
    return pos, None, loss_ref.softmax_ref64(h, E_, pos, neg), "lse", dict(full_catalogue=True)


def _sampled():
    h, E_, pos, neg, s = loss_ref.sampled_case(D, V, M, N, SEED)
    return pos, s, loss_ref.sampled_softmax_ref64(h, E_, pos, neg, s), "lse", {}


def _corrected():
    h, E_, pos, neg, s = loss_ref.sampled_case(D, V, M, N, SEED)
    logq = np.log(np.arange(1, V + 1) / (V * (V + 1) / 2.0)).astype(np.float32)
    return pos, s, loss_ref.sampled_softmax_ref64(h, E_, pos, neg, s, logq), "lse", {}


def _gbce():
    h, E_, pos, neg, s = loss_ref.sampled_case(D, V, M, N, SEED)
    return pos, s, gbce_ref.ref64(h, E_, pos, neg, s, 0.25), "l", {}


@pytest.mark.parametrize("kind", [_softmax, _sampled, _corrected, _gbce])
def test_check_passes_the_reference_and_names_the_tensor_it_refuses(kind):
    pos, s, ref, key, kw = kind()
    live = np.flatnonzero(pos)
    assert len(live) < M and len(set(pos[live])) < len(live)                    # a padded row, a repeated target
    if s is not None:
        assert s[1] == s[0] and np.any(s[:, None] == pos[None, live])          # a duplicate sample, an accidental hit

    def got():
        state = np.zeros(16, np.float32)
        state[0], state[2] = ref["loss"], ref["n"]
        return {key: ref[key].astype(np.float32), "dh": ref["dh"].astype(np.float32), "tg": ref["dE"].astype(np.float32), "state": state}

    assert loss_ref.check(got(), ref, 4.0, key, **kw) <= 1.0
    m, v = live[0], pos[live[0]]                                                # a live row, and a table row with a gradient
    for name, bound, push in ((key, ref["e_" + key][m], lambda g, e: g[key].__setitem__(m, g[key][m] + e)),
                              ("dh", ref["e_dh"][m, 0], lambda g, e: g["dh"].__setitem__((m, 0), g["dh"][m, 0] + e)),
                              ("tg", ref["e_dE"][v, 0], lambda g, e: g["tg"].__setitem__((v, 0), g["tg"][v, 0] + e)),
                              ("state[0]", ref["e_loss"] + (1e-6 * abs(ref["loss"]) + 1e-5) / 4.0,
                               lambda g, e: g["state"].__setitem__(0, g["state"][0] + e))):
        assert bound > 0
        g = got()
        push(g, 4.5 * bound)
        with pytest.raises(AssertionError, match=r"\('" + re.escape(name)):
            loss_ref.check(g, ref, 4.0, key, **kw)

"""Plain bf16 (attn_precision="bf16") against the fp64 oracle on every kernel path only that arithmetic reaches, or that had no
independent comparison under it: each parameter's gradient within (3 E_k + 2e-3) of its OWN largest entry, the forward rows within
3 E_act + 2e-4, the loss within 3 E_loss + 2e-4, where E is what the oracle's rounding model (tests/bf16_ref.py: the operands of every
matrix product rounded to bf16) deviates from the exact oracle at that shape, on the engine's gates and dropout masks
(model_harness._other_shapes).  tests/test_bf16_ref_host.py shows on the CPU that this bound has room for a correct kernel at these
shapes and none for one weight-gradient tile off by 20 %.  The shapes are the smallest that reach each path; every case asserts from
the launch plan that the kernels it names ran.  Measured values: profiles/bf16_envelope.txt (tools/probes/bf16_vs_oracle.py)."""
import pytest

import bf16_ref as br
from model_harness import E, _other_shapes  # noqa: F401  (E: the engine module, a fixture)

pytestmark = pytest.mark.gpu

STACK_FWD = ("cr_stack_fwd", "cr_stack_fwd_head")

# what the plan must hold (any of a tuple) and must not hold, forward and backward, per path
PATHS = {
    # cr_stack.hip routes 14-16 key tiles (T16 in 209..256) to launch_stack<16, false>: plain bf16, one head only
    # (engine._stack_kernel_fits); T = 224 is the last length of the one-launch block backward
    "stack16+block_bwd": dict(fwd=[STACK_FWD], bwd=[("cr_stack_block_bwd",)], no=("cr_attn_fwd", "cr_attn_bwd")),
    # the same forward past the block backward's lengths: FFN / attention / QKV backward as a launch each
    "stack16": dict(fwd=[STACK_FWD], bwd=[("cr_attn_bwd",)], no=("cr_attn_fwd", "cr_stack_block_bwd")),
    # cr_rbwd.hpp wgrad_accum (the code that held the round-5 defect) over 7 and 6 row tiles, family instantiations
    "block_bwd": dict(fwd=[STACK_FWD], bwd=[("cr_stack_block_bwd",)], no=("cr_attn_fwd", "cr_attn_bwd")),
    # two heads of 32 columns (config C3's geometry)
    "two_heads": dict(fwd=[STACK_FWD], bwd=[("cr_stack_ffn_bwd_heads", "cr_stack_block_bwd")], no=("cr_attn_fwd",)),
    "wide": dict(fwd=[("cr_wide_ln_qkv_fwd",), ("cr_wide_ln_ffn_fwd", "cr_wide_ln_ffn_fwd_tail"), ("cr_attn_fwd",)],
                 bwd=[("cr_wide_ln_ffn_bwd",), ("cr_wide_ln_qkv_bwd",)], no=()),
    "wide+mlp": dict(fwd=[("cr_wide_ln_qkv_fwd",), ("cr_gemm_rows",), ("cr_attn_fwd",)], bwd=[("cr_wide_ln_ffn_bwd",), ("cr_gemm_wgrad",)], no=()),
    # hidden sizes above 64 outside 128 / 192 / 256: LayerNorm, cr_gemm_rows / cr_gemm_wgrad (cr_gemm_bf.hip), element-wise kernels
    "unfused": dict(fwd=[("cr_layernorm_fwd",), ("cr_gemm_rows",), ("cr_attn_fwd",)], bwd=[("cr_gemm_rows",), ("cr_gemm_wgrad",), ("cr_attn_bwd",)],
                    no=("cr_wide_ln_qkv_fwd", "cr_wide_ln_ffn_bwd", "cr_stack_fwd")),
}

CASES = [("stack16+block_bwd", 0), ("stack16", 1), ("stack16", 2), ("block_bwd", 3), ("block_bwd", 4), ("two_heads", 5),
         ("wide", 6), ("wide", 7), ("wide", 8), ("wide", 9), ("wide+mlp", 10),
         ("wide", 11),              # T = 300 > 256: K / V stream through the LDS in 256-row chunks (config C5's class)
         ("unfused", 12), ("unfused", 13)]


@pytest.mark.parametrize("path,shape", [(p, br.SHAPES[i]) for p, i in CASES], ids=["%s-%s" % (p, "-".join(str(x) for x in br.SHAPES[i][:5])) for p, i in CASES])
def test_plain_bf16_within_the_rounding_model_of_the_oracle(E, path, shape):
    model, D, H, T, B, L, draw = shape
    eng = _other_shapes(E, model, D, H, T, L, B=B, prec="bf16", dropout=0.2, n_slabs=7 if D <= 64 else 5, draw=draw)
    fwd, bwd = [n for n, _, _ in eng.fwd], [n for n, _, _ in eng.bwd]
    want = PATHS[path]
    assert all(any(n in fwd for n in alt) for alt in want["fwd"]), fwd
    assert all(any(n in bwd for n in alt) for alt in want["bwd"]), bwd
    assert not any(n in fwd + bwd for n in want["no"]), (fwd, bwd)
    if path.startswith("stack16"):
        assert H == 1 and 208 < (T + 15) // 16 * 16 <= 256

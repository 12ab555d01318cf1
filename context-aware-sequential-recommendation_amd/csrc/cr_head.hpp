// The masked BCE row of the prediction head (sasrec.py:100-115), stated ONCE: for the three kernels of cr_head.hip and for the head tail
// of cr_stack.hip's k_stack_fwd.  Gradients are UN-normalised (scaled by n_target): cr_adam_step divides.
#pragma once
#include <math.h>

#include "castrec.h"

struct HeadBce { float sp, sn, dpl, dnl; };              // the two sigmoids; d loss_sum / d pos logit, d loss_sum / d neg logit
struct HeadSums { float loss, auc, n; };                 // a row's terms of state[0..2]

// ist: 1 where the row counts (its pos id is not 0, sasrec.py:104), else 0
__device__ __forceinline__ HeadBce head_bce(float pl, float nl, float ist) {
    HeadBce b;
    b.sp = 1.0f / (1.0f + expf(-pl));
    b.sn = 1.0f / (1.0f + expf(-nl));
    // d/dpl [-log(sig(pl)+e)] = -sig(1-sig)/(sig+e);  d/dnl [-log(1-sig(nl)+e)] = sig(1-sig)/(1-sig+e)
    b.dpl = -ist * b.sp * (1.0f - b.sp) / (b.sp + 1e-24f);
    b.dnl = ist * b.sn * (1.0f - b.sn) / (1.0f - b.sn + 1e-24f);
    return b;
}

// Called by the row's FIRST lane only (evaluated by all lanes the two logf would be paid per lane): the row's terms of the three sums,
// and its entries of the per-row outputs
__device__ __forceinline__ HeadSums head_bce_first_lane(const cr_head_desc& d, int m, float pl, float nl, float ist, const HeadBce& b) {
    HeadSums r;
    r.loss = ist * (-logf(b.sp + 1e-24f) - logf(1.0f - b.sn + 1e-24f));                 // sasrec.py:105-108
    const float dlt = pl - nl;
    const float sgn = (dlt > 0.0f) ? 1.0f : ((dlt < 0.0f) ? -1.0f : 0.0f);
    r.auc = ist * (sgn + 1.0f) * 0.5f;                                                  // sasrec.py:113-115
    r.n = ist;
    if (d.pos_logits) d.pos_logits[m] = pl;
    if (d.neg_logits) d.neg_logits[m] = nl;
    if (d.coef_out) {                                    // the item table's gradient is gathered from the batch's occurrence index
        d.coef_out[m] = b.dpl;
        d.coef_out[(size_t)d.M + m] = b.dnl;
    }
    return r;
}

// One element of the gradient row dy = dpl E[pos] + dnl E[neg].  Element by element on purpose: over a float4 the vector form is a
// packed multiply + in-place packed fma, the chain build.py's ISA scan refuses in the register-layout kernels.
__device__ __forceinline__ float head_dy(const HeadBce& b, float ep, float en) { return fmaf(b.dpl, ep, b.dnl * en); }

// Prediction head (sasrec.py:87-115): pos/neg item gathers, row dot products, masked BCE + AUC sums,
// and -- fused in the same pass -- the gradients wrt the sequence embedding and the item table.
// Gradients are UN-normalised (scaled by n_target); cr_adam_step divides by n_target, which is only
// known after the whole batch (all ranks) has been reduced (sasrec.py:104-108).
//
// Three kernels, one row body.  A lane holds N elements of each of the row's arrays; what is computed on them is written once, below
// (head_row_bce, head_row_ln_bwd, head_scatter, head_sums_fold, head_slab_fold), over a column mapping: HeadColStrided (slot i of lane l
// is column l + LPR i: dword accesses) or HeadColPacked (column N l + i: one 16- or 8-byte access).  The kernels keep what is theirs:
// how rows are dealt to workgroups and how loads and stores are issued.  The BCE formula itself: cr_head.hpp (shared with cr_stack.hip).
#include <math.h>

#include <stdlib.h>
#include "cr_common.hpp"
#include "cr_head.hpp"

// Row mapping as in cr_layernorm.hip: hidden sizes <= 64 give a row 16 lanes (4 rows per wave in flight,
// DPP row sums); larger ones a whole wave.
template <int LPR>
__device__ __forceinline__ float head_row_sum(float v) {
    if (LPR == 16) return cr_row16_sum(v);
    if (LPR == 32) {                                     // two DPP rows of 16 lanes: row sums, then the neighbouring row's
        v = cr_row16_sum(v);
        return v + __shfl_xor(v, 16, 64);
    }
    return wave_sum(v);
}

template <int LPR> struct HeadColStrided { static __device__ __forceinline__ int col(int l, int i) { return l + LPR * i; } };
template <int VEC> struct HeadColPacked { static __device__ __forceinline__ int col(int l, int i) { return VEC * l + i; } };

// (cr_head_desc BY VALUE into the helpers that store through it: behind a reference the compiler no longer knows the descriptor's
// pointers for global ones in k_head<16, 4>, whose stores and atomics then become flat_ instructions)
// The head of one row: s, ep, en hold the lane's elements of the sequence embedding and the two table rows (0 beyond D, 0 for id 0:
// row 0 == zeros, modules.py:154-156).  Adds the row's terms to `acc`, writes its per-row outputs (first lane) and returns the
// coefficients of the gradient row (head_dy) -- 0 unless `grad`.  p: the pos id, 0 for a lane group without a row.
template <int LPR, int N>
__device__ __forceinline__ HeadBce head_row_bce(const cr_head_desc d, int l, int m, bool act, bool grad, int p, const float (&s)[N],
                                                const float (&ep)[N], const float (&en)[N], HeadSums& acc) {
    float pl = 0.0f, nl = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) { pl += ep[i] * s[i]; nl += en[i] * s[i]; }
    pl = head_row_sum<LPR>(pl);                                                // sasrec.py:100
    nl = head_row_sum<LPR>(nl);                                                // sasrec.py:101
    const float ist = (p != 0) ? 1.0f : 0.0f;                                  // sasrec.py:104
    HeadBce b = head_bce(pl, nl, ist);
    if (!grad) { b.dpl = 0.0f; b.dnl = 0.0f; }
    if (l == 0 && act) {
        const HeadSums r = head_bce_first_lane(d, m, pl, nl, ist, b);
        acc.loss += r.loss; acc.auc += r.auc; acc.n += r.n;
    }
    return b;
}

// The gradient row dy and, while it is in registers, the LayerNorm backward of the row (modules.py:74-78; cr_layernorm.hip's arithmetic):
// x -> dx, and the row's terms of dgamma / dbeta onto ag / ab.
template <int LPR, int N, class COL>
__device__ __forceinline__ void head_row_ln_bwd(int l, int D, float invD, float eps, const HeadBce& b, const float (&ep)[N], const float (&en)[N],
                                                const float (&x)[N], const float (&gam)[N], float (&ag)[N], float (&ab)[N], float (&dy)[N],
                                                float (&dx)[N]) {
    float xs = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) xs += x[i];
    const float mean = head_row_sum<LPR>(xs) * invD;
    float v = 0.0f, xh[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        xh[i] = (COL::col(l, i) < D) ? (x[i] - mean) : 0.0f;
        v += xh[i] * xh[i];
    }
    const float rstd = 1.0f / sqrtf(head_row_sum<LPR>(v) * invD + eps);
    float c1 = 0.0f, c2 = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        dy[i] = head_dy(b, ep[i], en[i]);
        xh[i] *= rstd;
        const float dg = dy[i] * gam[i];
        c1 += dg;
        c2 += dg * xh[i];
        ag[i] += dy[i] * xh[i];
        ab[i] += dy[i];
    }
    c1 = head_row_sum<LPR>(c1) * invD;
    c2 = head_row_sum<LPR>(c2) * invD;
#pragma unroll
    for (int i = 0; i < N; ++i) dx[i] = cr_ln_bwd_tail(dy[i] * gam[i], c1, xh[i], c2, rstd);
}

// The item table's gradient by float atomics, for the wave's row group [mb, mb + 64 / LPR) below mend.  16 lanes per row: one CONTIGUOUS
// 4*D-byte burst per table row (lane = column), the shape the atomic units take at full rate -- with the row mapping one instruction
// would carry four 64-byte pieces of four different rows; the row's scalars come from its lane group, its s is re-read (L1 hit).
// Wider rows: the lane's own strided columns.
template <int LPR, int N>
__device__ __forceinline__ void head_scatter(const cr_head_desc d, int lane, int l, int mb, int mend, bool act, int p, int ng,
                                             const HeadBce& b, const float (&s)[N]) {
    if (LPR == 16) {
#pragma unroll
        for (int rr = 0; rr < 64 / LPR; ++rr) {
            const int mr = mb + rr;
            const float gpr = __shfl(b.dpl, rr * LPR, 64), gnr = __shfl(b.dnl, rr * LPR, 64);
            const int pr = __shfl(p, rr * LPR, 64), nr = __shfl(ng, rr * LPR, 64);
            if (mr < mend && pr != 0 && lane < d.D) {                          // a row counts where its pos id is not 0
                const float sv = d.seq_emb[(size_t)mr * d.ld + lane];
                atomicAdd(d.table_grad + (size_t)pr * d.D + lane, gpr * sv);
                if (nr != 0) atomicAdd(d.table_grad + (size_t)nr * d.D + lane, gnr * sv);
            }
        }
    } else if (act && p != 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = l + LPR * i;
            if (c < d.D) {
                atomicAdd(d.table_grad + (size_t)p * d.D + c, b.dpl * s[i]);
                if (ng != 0) atomicAdd(d.table_grad + (size_t)ng * d.D + c, b.dnl * s[i]);
            }
        }
    }
}

// The workgroup's three sums (SLOTS row slots: waves x rows per wave) onto state[0..2].  head_snapshot (cr_common.hpp) must follow once
// the kernel has nothing else to write; the _ln kernels fold their slabs in between, under the atomics' round trip.
template <int SLOTS>
__device__ __forceinline__ void head_sums_fold(float* state, const HeadSums& acc, int l, int slot) {
    __shared__ float red[3][SLOTS];
    if (l == 0) { red[0][slot] = acc.loss; red[1][slot] = acc.auc; red[2][slot] = acc.n; }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = 0.0f;
        for (int i = 0; i < SLOTS; ++i) v += red[threadIdx.x][i];
        if (v != 0.0f) atomicAdd(state + threadIdx.x, v);
    }
}

// dgamma / dbeta of a 16-wave workgroup -> its slab: the wave's row groups by shuffles, then the 16 waves in a fixed order
// (cr_layernorm.hip).  One pass over two [16][COLS] arrays -- except at 512 columns, where the two do not fit the 64 KB of static LDS:
// there one array, dgamma and dbeta in turn.
template <int LPR, int N, class COL>
__device__ __forceinline__ void head_slab_fold(const cr_ln_bwd_desc& n, int D, int wave, int sub, int l, float (&ag)[N], float (&ab)[N]) {
    constexpr int COLS = LPR * N;
    constexpr bool BOTH = COLS <= 256;
    __shared__ float part[BOTH ? 2 : 1][16][COLS];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int o = LPR; o < 64; o <<= 1) {
            ag[i] += __shfl_xor(ag[i], o, 64);
            ab[i] += __shfl_xor(ab[i], o, 64);
        }
    }
#pragma unroll
    for (int pass = 0; pass < (BOTH ? 1 : 2); ++pass) {
        if (pass) __syncthreads();
        if (sub == 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int c = COL::col(l, i);
                part[0][wave][c] = pass == 0 ? ag[i] : ab[i];
                if (BOTH) part[BOTH][wave][c] = ab[i];
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < D; c += 1024) {
            float g = 0.0f, b = 0.0f;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                g += part[0][w][c];
                if (BOTH) b += part[BOTH][w][c];
            }
            (pass == 0 ? n.dgamma : n.dbeta)[(size_t)blockIdx.x * n.slab_stride + c] = g;
            if (BOTH) n.dbeta[(size_t)blockIdx.x * n.slab_stride + c] = b;
        }
    }
}

// The head alone: 256 threads, row groups dealt to the waves of the whole grid in turn.
template <int LPR, int MAXC>
__global__ __launch_bounds__(256) void k_head(cr_head_desc d) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, l = lane % LPR;
    const bool need = d.d_seq_emb || d.table_grad || d.coef_out;
    HeadSums acc = {0.0f, 0.0f, 0.0f};
    for (int mb = (blockIdx.x * 4 + wave) * RPW; mb < d.M; mb += gridDim.x * 4 * RPW) {
        const int m = mb + sub;
        const bool act = m < d.M;
        const int mm = act ? m : d.M - 1;
        const int p = act ? d.pos[mm] : 0, ng = act ? d.neg[mm] : 0;
        float s[MAXC], ep[MAXC], en[MAXC];
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = l + LPR * i;
            const bool ok = c < d.D;
            s[i] = ok ? d.seq_emb[(size_t)mm * d.ld + c] : 0.0f;
            ep[i] = (ok && p != 0) ? d.table[(size_t)p * d.D + c] : 0.0f;
            en[i] = (ok && ng != 0) ? d.table[(size_t)ng * d.D + c] : 0.0f;
        }
        const HeadBce b = head_row_bce<LPR>(d, l, m, act, act && need, p, s, ep, en, acc);
        if (act && d.d_seq_emb) {
#pragma unroll
            for (int i = 0; i < MAXC; ++i)
                if (l + LPR * i < d.D) d.d_seq_emb[(size_t)m * d.ldd + l + LPR * i] = head_dy(b, ep[i], en[i]);
        }
        if (d.table_grad) head_scatter<LPR>(d, lane, l, mb, d.M, act, p, ng, b, s);
    }
    head_sums_fold<4 * RPW>(d.state, acc, l, wave * RPW + sub);
    head_snapshot(d.state, gridDim.x);
}

extern "C" int cr_head_fwd_bwd(const cr_head_desc* d, void* stream) {
    CR_REQUIRE(d && d->seq_emb && d->table && d->pos && d->neg && d->state, "cr_head_fwd_bwd: NULL pointer");
    CR_REQUIRE(d->M > 0 && d->D > 0 && d->V > 0 && d->ld >= d->D, "cr_head_fwd_bwd: bad shape");
    if (d->D > 512) return cr_set_error(CR_ERR_UNSUPPORTED, "cr_head_fwd_bwd: D=%d > 512", d->D);
    const int lpr = d->D <= 64 ? 16 : d->D <= 128 ? 32 : 64;
    int grid = cr_ceil_div(d->M, 4 * (64 / lpr));                              // a workgroup's four waves hold 64 / lpr rows each
    if (grid > 2048) grid = 2048;
    if (lpr == 16) hipLaunchKernelGGL((k_head<16, 4>), dim3(grid), dim3(256), 0, cr_stream(stream), *d);
    else if (lpr == 32) hipLaunchKernelGGL((k_head<32, 4>), dim3(grid), dim3(256), 0, cr_stream(stream), *d);
    else hipLaunchKernelGGL((k_head<64, 8>), dim3(grid), dim3(256), 0, cr_stream(stream), *d);
    return cr_check_launch("cr_head_fwd_bwd");
}

// Head + backward of the LayerNorm that produced seq_emb (sasrec.py:85), in one pass: the gradient row
// dy = dpl * E[pos] + dnl * E[neg] never leaves the registers it is computed in -- it goes straight through the
// LayerNorm backward of cr_layernorm.hip (same row mapping, same arithmetic, same slab reduction: n_slabs workgroups
// of 16 waves, workgroup s owns rows [s*rps, (s+1)*rps) and writes slab s of dgamma / dbeta).
// This form reads a row as LPR-strided dwords and requests the ids of a row group one iteration ahead.
template <int LPR, int MAXC>
__global__ __launch_bounds__(1024) void k_head_ln(cr_head_desc d, cr_ln_bwd_desc n) {
    constexpr int RPW = 64 / LPR;
    using COL = HeadColStrided<LPR>;
    cr_kernarg_touch<sizeof(cr_head_desc) + sizeof(cr_ln_bwd_desc)>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, l = lane % LPR;
    const int rps = (d.M + gridDim.x - 1) / gridDim.x;
    const int m0 = blockIdx.x * rps, m1 = min(d.M, m0 + rps);
    float gam[MAXC], ag[MAXC], ab[MAXC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        gam[i] = (COL::col(l, i) < d.D) ? n.gamma[COL::col(l, i)] : 0.0f;
        ag[i] = 0.0f; ab[i] = 0.0f;
    }
    const float invD = 1.0f / (float)d.D;
    HeadSums acc = {0.0f, 0.0f, 0.0f};
    // the ids of a row group are requested one iteration ahead: id -> table row is a dependent pair of memory round trips, and a
    // wave runs only two iterations (100 rows per workgroup, 16 waves x 4 rows)
    int p_n = 0, ng_n = 0;
    {
        const int m = m0 + wave * RPW + sub;
        if (m < m1) { p_n = d.pos[m]; ng_n = d.neg[m]; }
    }
    for (int mb = m0 + wave * RPW; mb < m1; mb += 16 * RPW) {
        const int m = mb + sub;
        const bool act = m < m1;
        const int mm = act ? m : m0;
        const int p = act ? p_n : 0, ng = act ? ng_n : 0;
        {
            const int mn = m + 16 * RPW;
            p_n = 0; ng_n = 0;
            if (mn < m1) { p_n = d.pos[mn]; ng_n = d.neg[mn]; }
        }
        float s[MAXC], ep[MAXC], en[MAXC], x[MAXC], dy[MAXC], dx[MAXC];
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = COL::col(l, i);
            const bool ok = c < d.D;
            s[i] = ok ? d.seq_emb[(size_t)mm * d.ld + c] : 0.0f;
            x[i] = ok ? n.x[(size_t)mm * n.ldx + c] : 0.0f;
            ep[i] = (ok && p != 0) ? d.table[(size_t)p * d.D + c] : 0.0f;
            en[i] = (ok && ng != 0) ? d.table[(size_t)ng * d.D + c] : 0.0f;
        }
        const HeadBce b = head_row_bce<LPR>(d, l, m, act, act, p, s, ep, en, acc);
        head_row_ln_bwd<LPR, MAXC, COL>(l, d.D, invD, n.eps, b, ep, en, x, gam, ag, ab, dy, dx);
        if (act) {
#pragma unroll
            for (int i = 0; i < MAXC; ++i) {
                const int c = COL::col(l, i);
                if (c < d.D && d.d_seq_emb) d.d_seq_emb[(size_t)m * d.ldd + c] = dy[i];
                if (c < d.D) n.dx[(size_t)m * n.lddx + c] = dx[i];
            }
        }
        if (d.table_grad) head_scatter<LPR>(d, lane, l, mb, m1, act, p, ng, b, s);
    }
    head_sums_fold<16 * RPW>(d.state, acc, l, wave * RPW + sub);
    head_slab_fold<LPR, MAXC, COL>(n, d.D, wave, sub, l, ag, ab);
    head_snapshot(d.state, gridDim.x);
}

// The same kernel with VECTOR row accesses (round 5): a lane owns VEC consecutive columns (16- or 8-byte loads: D a multiple of 4,
// or even), LPR lanes a row (LPR * VEC >= D), and the loop is software-pipelined: the four rows an iteration reads (sequence
// embedding, LayerNorm input, pos row, neg row) are requested one iteration ahead, the ids two.  k_head_ln above reads a row as
// LPR-strided dwords (four load instructions per array and row group) and starts each iteration's loads behind the previous one's
// stores: 14.3 us at the headline shape (two dependent iterations per wave), 81 us for one C5 step's 131 072 table rows (0.52 of the
// HBM roof over all its bytes).  This kernel is bound by load ISSUE and dependent round trips, so both changes go straight to time.
// Nothing scatters from it (the occurrence-index form: no table_grad).
typedef float hd_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float hd_f2 __attribute__((ext_vector_type(2), aligned(4)));
template <int VEC> struct HdVec { float v[VEC]; };
template <int VEC>
__device__ __forceinline__ HdVec<VEC> hd_load(const float* p, bool ok) {
    HdVec<VEC> r;
    if constexpr (VEC == 4) {
        hd_f4 t = (hd_f4){0.f, 0.f, 0.f, 0.f};
        if (ok) t = *reinterpret_cast<const hd_f4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        hd_f2 t = (hd_f2){0.f, 0.f};
        if (ok) t = *reinterpret_cast<const hd_f2*>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void hd_store(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<hd_f4*>(p) = (hd_f4){v[0], v[1], v[2], v[3]};
    else *reinterpret_cast<hd_f2*>(p) = (hd_f2){v[0], v[1]};
}

template <int LPR, int VEC>
__global__ __launch_bounds__(1024) void k_head_ln_v(cr_head_desc d, cr_ln_bwd_desc n) {
    constexpr int RPW = 64 / LPR;
    using COL = HeadColPacked<VEC>;
    cr_kernarg_touch<sizeof(cr_head_desc) + sizeof(cr_ln_bwd_desc)>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, l = lane % LPR;
    const int c0 = VEC * l;
    const bool cok = c0 < d.D;
    const int rps = (d.M + gridDim.x - 1) / gridDim.x;
    const int m0 = blockIdx.x * rps, m1 = min(d.M, m0 + rps);
    const int mz = min(m0, d.M - 1);                      // the row a lane group without a row reads (a workgroup may own none)
    constexpr int STEP = 16 * RPW;                        // rows per iteration of the workgroup
    float gam[VEC], ag[VEC], ab[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) { gam[u] = (c0 + u < d.D) ? n.gamma[c0 + u] : 0.0f; ag[u] = 0.0f; ab[u] = 0.0f; }
    const float invD = 1.0f / (float)d.D;
    HeadSums acc = {0.0f, 0.0f, 0.0f};
    // pipeline: ids of iterations 0 and 1, rows of iteration 0
    const int mfirst = m0 + wave * RPW + sub;
    int p_a = 0, ng_a = 0, p_b = 0, ng_b = 0;             // ids of this iteration / the next one
    if (mfirst < m1) { p_a = d.pos[mfirst]; ng_a = d.neg[mfirst]; }
    if (mfirst + STEP < m1) { p_b = d.pos[mfirst + STEP]; ng_b = d.neg[mfirst + STEP]; }
    HdVec<VEC> s_n, x_n, ep_n, en_n;
    {
        const int mm = mfirst < m1 ? mfirst : mz;
        s_n = hd_load<VEC>(d.seq_emb + (size_t)mm * d.ld + c0, cok);
        x_n = hd_load<VEC>(n.x + (size_t)mm * n.ldx + c0, cok);
        ep_n = hd_load<VEC>(d.table + (size_t)p_a * d.D + c0, cok && p_a != 0);      // row 0 == zeros (modules.py:154-156)
        en_n = hd_load<VEC>(d.table + (size_t)ng_a * d.D + c0, cok && ng_a != 0);
    }
    for (int mb = m0 + wave * RPW; mb < m1; mb += STEP) {
        const int m = mb + sub;
        const bool act = m < m1;
        const int p = act ? p_a : 0;
        const HdVec<VEC> s = s_n, xv = x_n, ep = ep_n, en = en_n;
        // the next iteration's rows (its ids arrived an iteration ago), the ids of the one after
        {
            const int mn = m + STEP;
            const bool actn = mn < m1;
            const int mmn = actn ? mn : m0;
            const int pn = actn ? p_b : 0, nn = actn ? ng_b : 0;
            s_n = hd_load<VEC>(d.seq_emb + (size_t)mmn * d.ld + c0, cok);
            x_n = hd_load<VEC>(n.x + (size_t)mmn * n.ldx + c0, cok);
            ep_n = hd_load<VEC>(d.table + (size_t)pn * d.D + c0, cok && pn != 0);
            en_n = hd_load<VEC>(d.table + (size_t)nn * d.D + c0, cok && nn != 0);
            p_a = p_b; ng_a = ng_b;
            p_b = 0; ng_b = 0;
            if (mn + STEP < m1) { p_b = d.pos[mn + STEP]; ng_b = d.neg[mn + STEP]; }
        }
        float dy[VEC], dx[VEC];
        const HeadBce b = head_row_bce<LPR>(d, l, m, act, act, p, s.v, ep.v, en.v, acc);
        head_row_ln_bwd<LPR, VEC, COL>(l, d.D, invD, n.eps, b, ep.v, en.v, xv.v, gam, ag, ab, dy, dx);
        if (act && cok && d.d_seq_emb) hd_store<VEC>(d.d_seq_emb + (size_t)m * d.ldd + c0, dy);
        if (act && cok) hd_store<VEC>(n.dx + (size_t)m * n.lddx + c0, dx);
    }
    head_sums_fold<16 * RPW>(d.state, acc, l, wave * RPW + sub);
    head_slab_fold<LPR, VEC, COL>(n, d.D, wave, sub, l, ag, ab);
    head_snapshot(d.state, gridDim.x);
}

// Which kernel takes a cr_head_fwd_bwd_ln call: the vector or the strided form, lanes per row, elements per lane (VEC / MAXC)
struct HeadLnForm { bool vec; int lpr, n; };
static HeadLnForm head_ln_form(const cr_head_desc* d, const cr_ln_bwd_desc* n) {
    static const bool no_vec = getenv("CASTREC_HEAD_NO_VEC") != nullptr;
    const int D = d->D, pitch = d->ld | n->ldx | n->lddx | (d->d_seq_emb ? d->ldd : 0);     // (low bits: every pitch even / a multiple of 4)
    // vector row accesses where the shape allows them, and nothing scatters from this kernel (the occurrence-index form)
    // (D = 50: 32 lanes x 8 bytes halve the rows a wave holds per iteration -- four dependent iterations instead of two at the headline
    //  shape: 17.6 against 16.5 us; 16-byte lanes keep four rows per wave up to 64 columns, and above 64 the scalar form's strided dwords
    //  lose outright: 82.2 -> 65.1 us for one C5 step's rows, 0.51 -> 0.65 of the HBM roof, bench.py gather.head_ln)
    if (!no_vec && !d->table_grad && pitch % 2 == 0 && D % 2 == 0 && D <= 256 && (D % 4 == 0 || D > 64)) {
        if (D % 4 == 0 && pitch % 4 == 0) return {true, D <= 64 ? 16 : D <= 128 ? 32 : 64, 4};
        if (D <= 128) return {true, D <= 32 ? 16 : D <= 64 ? 32 : 64, 2};
    }
    // lanes per row: 16 (D <= 64), 32 (D <= 128: two rows per wave and DPP row sums -- with a whole wave per row the eight rows
    // of a wave at config C4 were eight serial gather -> reduce -> atomics passes: 36 us), else 64
    return {false, D <= 64 ? 16 : D <= 128 ? 32 : 64, D <= 128 ? 4 : 8};
}

extern "C" int cr_head_fwd_bwd_ln(const cr_head_desc* d, const cr_ln_bwd_desc* n, void* stream) {
    CR_REQUIRE(d && d->seq_emb && d->table && d->pos && d->neg && d->state, "cr_head_fwd_bwd_ln: NULL pointer");
    CR_REQUIRE(d->M > 0 && d->D > 0 && d->V > 0 && d->ld >= d->D, "cr_head_fwd_bwd_ln: bad shape");
    CR_REQUIRE(n && n->x && n->gamma && n->dx && n->dgamma && n->dbeta, "cr_head_fwd_bwd_ln: NULL LayerNorm pointer");
    CR_REQUIRE(n->M == d->M && n->D == d->D && n->n_slabs > 0 && n->ldx >= d->D && n->lddx >= d->D,
               "cr_head_fwd_bwd_ln: the LayerNorm description must match the head's rows");
    CR_REQUIRE(!n->accumulate, "cr_head_fwd_bwd_ln: accumulate is not supported");
    if (d->D > 512) return cr_set_error(CR_ERR_UNSUPPORTED, "cr_head_fwd_bwd_ln: D=%d > 512", d->D);
    const HeadLnForm f = head_ln_form(d, n);
#define HD_CASE(VEC, K, L, N) \
    if (f.vec == VEC && f.lpr == L && f.n == N) hipLaunchKernelGGL((K<L, N>), dim3(n->n_slabs), dim3(1024), 0, cr_stream(stream), *d, *n)
    HD_CASE(true, k_head_ln_v, 16, 4); HD_CASE(true, k_head_ln_v, 32, 4); HD_CASE(true, k_head_ln_v, 64, 4);
    HD_CASE(true, k_head_ln_v, 16, 2); HD_CASE(true, k_head_ln_v, 32, 2); HD_CASE(true, k_head_ln_v, 64, 2);
    HD_CASE(false, k_head_ln, 16, 4); HD_CASE(false, k_head_ln, 32, 4); HD_CASE(false, k_head_ln, 64, 8);
#undef HD_CASE
    return cr_check_launch("cr_head_fwd_bwd_ln");
}

// test_logits (sasrec.py:93-97): last position of every sequence against its candidate items.
__global__ __launch_bounds__(256) void k_test_logits(const float* seq_emb, int ld, const float* table, const int32_t* cand,
                                                     int B, int T, int D, int n_cand, float* logits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const float* s = seq_emb + (size_t)(b * T + T - 1) * ld;
    for (int j = wave; j < n_cand; j += 4) {
        const int id = cand[(size_t)b * n_cand + j];
        float acc = 0.0f;
        if (id != 0)
            for (int c = lane; c < D; c += 64) acc += s[c] * table[(size_t)id * D + c];
        acc = wave_sum(acc);
        if (lane == 0) logits[(size_t)b * n_cand + j] = acc;
    }
}

// The same for hidden sizes that are multiples of 4 (16-byte rows): a read-only row gather, the form the HBM-read
// roofline of the item table is measured on (bench.py "gather" block).  16 lanes own a candidate row (float4 per lane
// per 64 columns), a wave keeps 4 rows x NR rounds in flight, the row sum is four DPP adds.  NV = D / 64 rounded up.
template <int NV, int NR, bool STREAM>
__global__ __launch_bounds__(256) void k_test_logits_v4(const float* seq_emb, int ld, const float* table, const int32_t* cand,
                                                        int B, int T, int D, int n_cand, float* logits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, grp = (threadIdx.x >> 4);   // 16 groups per block
    const int b = blockIdx.x;
    const float* s = seq_emb + (size_t)(b * T + T - 1) * ld;
    typedef float f4a __attribute__((ext_vector_type(4), aligned(4)));
    f4a sv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * li + 64 * i;
        sv[i] = c < D ? *reinterpret_cast<const f4a*>(s + c) : (f4a){0.f, 0.f, 0.f, 0.f};
    }
    // NR candidates per group and iteration
    for (int j0 = grp * NR; j0 < n_cand; j0 += 16 * NR) {
        int id[NR];
        float4 rv[NR][NV];
#pragma unroll
        for (int r = 0; r < NR; ++r) id[r] = (j0 + r < n_cand) ? cand[(size_t)b * n_cand + j0 + r] : 0;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = 4 * li + 64 * i;
                // STREAM (a table larger than the Infinity Cache: a row is not read again before it has left every cache): streaming loads --
                // 76.7 -> 69.2 us for 425 MB of fresh rows at config C5's table, 69 -> 77 % of the 8 TB/s peak (bench.py gather block).  NOT in
                // cr_embed_fwd, the training-path gather, which writes as many bytes as it reads: there streaming loads cost 5 %, and with
                // both kernels streaming this one's gain was gone as well (tools/probes/run_gather.sh: CASTREC_GATHER_STREAM)
                typedef float f4n __attribute__((ext_vector_type(4)));
                const f4n* src = reinterpret_cast<const f4n*>(table + (size_t)id[r] * D + (c < D ? c : 0));
                const f4n t4 = STREAM ? __builtin_nontemporal_load(src) : *src;
                rv[r][i] = make_float4(t4.x, t4.y, t4.z, t4.w);
            }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const bool ok = 4 * li + 64 * i < D;
                acc += ok ? (sv[i].x * rv[r][i].x + sv[i].y * rv[r][i].y + sv[i].z * rv[r][i].z + sv[i].w * rv[r][i].w) : 0.0f;
            }
            acc = cr_row16_sum(acc);
            if (li == 0 && j0 + r < n_cand) logits[(size_t)b * n_cand + j0 + r] = id[r] != 0 ? acc : 0.0f;   // row 0 reads as zeros
        }
    }
    (void)wave;
}

extern "C" int cr_test_logits(const float* seq_emb, int ld, const float* table, const int32_t* cand, int B, int T, int D,
                              int V, int n_cand, float* logits, void* stream) {
    CR_REQUIRE(seq_emb && table && cand && logits, "cr_test_logits: NULL pointer");
    CR_REQUIRE(B > 0 && T > 0 && D > 0 && V > 0 && n_cand > 0 && ld >= D, "cr_test_logits: bad shape");
    hipStream_t st = cr_stream(stream);
    if (D % 4 == 0 && D <= 256 && (reinterpret_cast<uintptr_t>(table) & 15) == 0) {
        // rows in flight per 16-lane group at D > 128 (1 KB rows): 7 puts the evaluator's 101 candidates of a query into ONE batch
        // (16 groups x 7): 68.2 % / 68.7 % / 70.0 % / 71.1 % of the 8 TB/s HBM peak for 1 / 2 / 4 / 7 at config C5's table
        // (tools/gather_sweep.py, a fresh row set per launch)
        static const int nr = getenv("CASTREC_TL_NR") ? atoi(getenv("CASTREC_TL_NR")) : 7;
        static const char* gs = getenv("CASTREC_GATHER_STREAM");            // (measurement override: 0 / 1)
        const bool big = gs ? atoi(gs) != 0 : (size_t)V * D * 4 >= ((size_t)256 << 20);       // streaming row loads: see k_test_logits_v4
#define TL_LAUNCH(NV, NRR)                                                                                                                    \
    do {                                                                                                                                      \
        if (big) hipLaunchKernelGGL((k_test_logits_v4<NV, NRR, true>), dim3(B), dim3(256), 0, st, seq_emb, ld, table, cand, B, T, D, n_cand, logits);   \
        else hipLaunchKernelGGL((k_test_logits_v4<NV, NRR, false>), dim3(B), dim3(256), 0, st, seq_emb, ld, table, cand, B, T, D, n_cand, logits);     \
    } while (0)
        if (D <= 64) TL_LAUNCH(1, 2);
        else if (D <= 128) TL_LAUNCH(2, 2);
        else if (nr == 4) TL_LAUNCH(4, 4);
        else if (nr == 1) TL_LAUNCH(4, 1);
        else if (nr == 7) TL_LAUNCH(4, 7);
        else TL_LAUNCH(4, 2);
#undef TL_LAUNCH
        return cr_check_launch("cr_test_logits");
    }
    hipLaunchKernelGGL(k_test_logits, dim3(B), dim3(256), 0, st, seq_emb, ld, table, cand, B, T, D, n_cand, logits);
    return cr_check_launch("cr_test_logits");
}

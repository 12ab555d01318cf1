// Adam, TensorFlow-1.15 formulation (tf.train.AdamOptimizer(lr, beta2=0.98), sasrec.py:120):
//   lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//   p -= lr_t * m / (sqrt(v) + eps)
// applied densely to EVERY variable (the reference's zero-padded lookup goes through tf.concat, so
// TF produces dense table gradients and moves every row every step).  Fused here: gradient
// normalisation by n_target, reduction of the dense-parameter slabs, zeroing of the table gradient.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cr_common.hpp"
#include "cr_tgrad.hpp"

int tg_unit_grid(const cr_tgrad_desc* d);     // cr_tgrad.hip

// Sum of the gradient slabs for ADAM_COLS = 256 consecutive dense parameters [j0, j0 + 256): wave w of the block's
// ADAM_WAVES waves adds slabs w, w + 16, w + 32, ... -- each read is 1 KiB contiguous (16 bytes per lane; the first version
// read 256-byte pieces of each slab from 16-lane groups and reached 2.5 TB/s) -- and the wave partials are added in a
// fixed order through LDS: bitwise reproducible.  Result: thread t < 256 returns the sum of column j0 + t.
#define ADAM_COLS 256
#define ADAM_WAVES 16
typedef float f4a __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ float slab_sum256(const float* slabs, int n_slabs, int n_dense, int j0, float (*part)[ADAM_COLS]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = j0 + 4 * lane;
    f4a acc = (f4a){0.f, 0.f, 0.f, 0.f};
    if (j + 3 < n_dense) {
        // every load of the wave's share is issued before the first add (n_slabs <= 256: at most 16 per wave): one
        // memory round trip instead of one per batch of 8
        for (int s0 = w; s0 < n_slabs; s0 += 16 * ADAM_WAVES) {
            f4a v[16];
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (s0 + ADAM_WAVES * u < n_slabs) { v[u] = *reinterpret_cast<const f4a*>(slabs + (size_t)(s0 + ADAM_WAVES * u) * n_dense + j); cnt = u + 1; }
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < cnt) acc += v[u];
        }
    } else {
        for (int s = w; s < n_slabs; s += ADAM_WAVES)
            for (int u = 0; u < 4; ++u)
                if (j + u < n_dense) acc[u] += slabs[(size_t)s * n_dense + j + u];
    }
    part[w][4 * lane + 0] = acc.x; part[w][4 * lane + 1] = acc.y; part[w][4 * lane + 2] = acc.z; part[w][4 * lane + 3] = acc.w;
    __syncthreads();
    float g = 0.0f;
    if (threadIdx.x < ADAM_COLS) {
#pragma unroll
        for (int k = 0; k < ADAM_WAVES; ++k) g += part[k][threadIdx.x];
    }
    return g;
}

// The workgroups of one launch, in block order: nb_dense blocks of 256 dense parameters (slab sums + update), nb_lazy blocks of lazy
// item-table rows, nb_units unit workgroups of the occurrence index, nb_table sweep blocks, nb_ring blocks of the id-ring copy.
// (The order is measured.  The unit workgroups FIRST: 29.7 against 25.8 us at the time -- the dense blocks' slab sums are the other
//  long chain and want the early start; the short sections, id ring and sweep, first: 21.8 against 20.6 us.  The unit grid holds a
//  batch's plan in ONE pass -- 384 workgroups: 260-280 are in use at the headline shape; at 256 a few workgroups ran two passes: 20.6
//  against 19.8 us.)
struct adam_grid { int nb_dense, nb_lazy, nb_units, nb_table, nb_ring; };
#define ADAM_NT (64 * ADAM_WAVES)

// The step's constants, formed once per thread, and 1 / n_target.  They cost two dependent loads (n, t) and two powf: every role forms
// them BEHIND its first loads, which do not depend on them -- one memory round trip of this short kernel's critical path
// (tools/adam_probe.py).  l2 is a REFERENCE into the kernel's argument d, which must outlive the struct (it is not assignable): copied,
// a 16-byte group does its four l2 terms between the other arithmetic and k_adam<true, 0, 1> needs 96 instead of 76 bytes of scratch.
struct adam_consts { float b1, c1, b2, c2, eps; const float& l2; long long n_l2; float lr_t, inv_n; };
__device__ __forceinline__ adam_consts adam_scalars(const cr_adam_desc& d, float n, uint32_t t) {
    const float b1t = powf(d.beta1, (float)t), b2t = powf(d.beta2, (float)t);
    return {d.beta1, 1.0f - d.beta1, d.beta2, 1.0f - d.beta2, d.eps, d.l2, d.n_l2, d.lr * sqrtf(1.0f - b2t) / (1.0f - b1t), n > 0.0f ? 1.0f / n : 0.0f};
}

// THE update, of element i with gradient g: the CALLER has multiplied it by k.inv_n (nothing in here does), or passes a literal 0.0f
// where there is none.  Every role calls it, so every role rounds alike: the compiler contracts these shapes to fma(b1, m, c1 * g) and
// fma(b2, v, (c2 * g) * g), and the bitwise reproducibility of the one-GPU step rests on all roles agreeing.
__device__ __forceinline__ void adam_update(const adam_consts& k, long long i, float g, float& p, float& m, float& v) {
    if (i < k.n_l2) g = fmaf(k.l2, p, g);                // d/dp of l2 * sum(p^2) / 2 on the lookup tables (modules.py:153)
    m = k.b1 * m + k.c1 * g;
    v = k.b2 * v + k.c2 * g * g;
    p = p - k.lr_t * m / (sqrtf(v) + k.eps);
}
// ... of one element in memory
__device__ __forceinline__ void adam_element(const cr_adam_desc& d, const adam_consts& k, long long i, float g) {
    float p = d.p[i], m = d.m[i], v = d.v[i];
    adam_update(k, i, g, p, m, v);
    d.m[i] = m; d.v[i] = v; d.p[i] = p;
}
// ... of one element whose gradient is table_grad[i], which is zeroed for the next step
__device__ __forceinline__ void adam_element_tg(const cr_adam_desc& d, const adam_consts& k, long long i) {
    const float g = d.table_grad[i];
    d.table_grad[i] = 0.0f;
    adam_element(d, k, i, g * k.inv_n);
}

// 16 bytes of a swept section: streaming (STREAM: nothing of the section is read again before 7 x its size has passed) or plain
template <bool STREAM>
__device__ __forceinline__ f4a ld4(const float* q) {
    return STREAM ? __builtin_nontemporal_load(reinterpret_cast<const f4a*>(q)) : *reinterpret_cast<const f4a*>(q);
}
template <bool STREAM>
__device__ __forceinline__ void st4(float* q, const f4a x) {
    if (STREAM) __builtin_nontemporal_store(x, reinterpret_cast<f4a*>(q));
    else *reinterpret_cast<f4a*>(q) = x;
}
// ... updated component by component and stored; g: the four gradients, or one float for all four
__device__ __forceinline__ float adam_comp(const f4a g, int e) { return g[e]; }
__device__ __forceinline__ float adam_comp(float g, int) { return g; }
template <bool STREAM, typename G>
__device__ __forceinline__ void adam_update4(const cr_adam_desc& d, const adam_consts& k, long long i, const G g, f4a p, f4a m, f4a v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_update(k, i + e, adam_comp(g, e), pe, me, ve);
        p[e] = pe; m[e] = me; v[e] = ve;
    }
    st4<STREAM>(d.m + i, m); st4<STREAM>(d.v + i, v); st4<STREAM>(d.p + i, p);
}
// ... with the gradient group g of table_grad, which is zeroed for the next step
template <bool STREAM>
__device__ __forceinline__ void adam_update4_tg(const cr_adam_desc& d, const adam_consts& k, long long i, f4a g, const f4a p, const f4a m, const f4a v) {
    st4<STREAM>(d.table_grad + i, (f4a){0.f, 0.f, 0.f, 0.f});
    g *= k.inv_n;
    adam_update4<STREAM>(d, k, i, g, p, m, v);
}

// ---- the roles of a workgroup (b: its number within the role) -----------------------------------------------------------------
// the next step's ids out of the resident ring (nothing else in this launch reads the static id buffers; the occurrence index of
// the RUNNING step is read from its ring slot, which these blocks do not write)
__device__ __forceinline__ void adam_ring_copy(const cr_adam_desc& d, int b, int nb_ring, uint32_t t) {
    const long long n_copy = d.ids_copy_elems ? d.ids_copy_elems : d.ids_slot_elems;
    const int32_t* src1 = d.ids_ring + (long long)((t + 1u) % (uint32_t)d.ids_ring_slots) * d.ids_slot_elems;
    const long long first = (long long)b * ADAM_NT + threadIdx.x, stride = (long long)nb_ring * ADAM_NT;
    if ((d.ids_slot_elems & 3) == 0 && (n_copy & 3) == 0 && (((uintptr_t)d.ids_ring | (uintptr_t)d.ids_dst) & 15) == 0) {
        const int4* src = reinterpret_cast<const int4*>(src1);
        int4* dst = reinterpret_cast<int4*>(d.ids_dst);
        for (long long i = first; i < (n_copy >> 2); i += stride) dst[i] = src[i];
    } else {                                             // (a slot that is no multiple of 16 bytes: B * T odd)
        for (long long i = first; i < n_copy; i += stride) d.ids_dst[i] = src1[i];
    }
}

// 256 dense parameters: slab sums, then the update
__device__ __forceinline__ void adam_dense_block(const cr_adam_desc& d, int b, float n, uint32_t t, float (*part)[ADAM_COLS]) {
    const int j0 = b * ADAM_COLS;
    const int ns = d.slab_counts ? min(d.slab_counts[b], d.n_slabs) : d.n_slabs;
    // the parameter and its moments are requested BEFORE the slab sum (they do not depend on it): one memory round trip less on
    // the critical path of this short kernel
    const bool mine = threadIdx.x < ADAM_COLS && j0 + (int)threadIdx.x < d.n_dense;
    const long long i0 = d.n_table + j0;                 // (uniform: the three arrays are addressed as a scalar base + a 32-bit lane offset)
    const unsigned c = mine ? threadIdx.x : 0u;
    float p = mine ? (d.p + i0)[c] : 0.0f, m = mine ? (d.m + i0)[c] : 0.0f, v = mine ? (d.v + i0)[c] : 0.0f;
    const float g = slab_sum256(d.dense_slabs, ns, d.n_dense, j0, part);
    const adam_consts k = adam_scalars(d, n, t);
    if (mine) {
        adam_update(k, i0 + c, g * k.inv_n, p, m, v);
        (d.m + i0)[c] = m; (d.v + i0)[c] = v; (d.p + i0)[c] = p;
    }
}

// lazy rows: wave w of the nb_lazy blocks walks ids w, w + W, ...; the first wave to swap the step number into a row's flag owns the
// row (every other occurrence of the id finds it there and moves on).  The ids: lazy_ids followed by lazy_ids2 (where set) -- two
// buffers walked as one list, no copy that joins them (the host has checked that the sum of the counts fits an int)
__device__ __forceinline__ void adam_lazy_rows(const cr_adam_desc& d, int b, int nb_lazy, float n, uint32_t t) {
    const int lane = threadIdx.x & 63, W = nb_lazy * ADAM_WAVES;
    const int n_ids = d.n_lazy_ids + (d.lazy_ids2 ? d.n_lazy_ids2 : 0);
    const adam_consts k = adam_scalars(d, n, t);
    for (int j = b * ADAM_WAVES + (threadIdx.x >> 6); j < n_ids; j += W) {
        const int id = j < d.n_lazy_ids ? d.lazy_ids[j] : d.lazy_ids2[j - d.n_lazy_ids];
        if (id <= 0 || id >= d.lazy_rows) continue;      // row 0: the zero-pad row never has a gradient
        int mine = 0;
        if (lane == 0) mine = atomicExch(&d.lazy_flags[id], t) != t;
        mine = __shfl(mine, 0, 64);
        if (!mine) continue;
        for (int c = lane; c < d.lazy_D; c += 64) adam_element_tg(d, k, (long long)id * d.lazy_D + c);
    }
}

// the rows the batch looked up (occurrence index, cr_tgrad.hpp): gradient = ordered sum over the row's occurrences, update in place.
// (p / m / v requested in front of the batch's loads: 20 bytes of scratch per lane at 16 occurrences in flight, and no faster -- 20.1
// against 20.3 us.)
template <int LPR, int VEC>
__device__ __forceinline__ void adam_unit_blocks(const cr_adam_desc& d, const cr_tgrad_desc& g, int b, int nb_units, float n, uint32_t t, float* part_s) {
    const int32_t* ix = tg_index(g, t);
    const adam_consts k = adam_scalars(d, n, t);
    tg_unit_blocks<LPR, VEC, tg_ent(VEC)>(g, ix, b, nb_units, part_s, reinterpret_cast<int*>(part_s + ADAM_WAVES * ADAM_COLS),
        [&](int row, int col0, const float (&acc)[VEC]) {
            const long long i = (long long)row * g.D + col0;
            float p[VEC], m[VEC], v[VEC];
            tg_load<VEC>(p, d.p + i); tg_load<VEC>(m, d.m + i); tg_load<VEC>(v, d.v + i);
#pragma unroll
            for (int u = 0; u < VEC; ++u) adam_update(k, i + u, acc[u] * k.inv_n, p[u], m[u], v[u]);
            tg_store<VEC>(d.m + i, m); tg_store<VEC>(d.v + i, v); tg_store<VEC>(d.p + i, p);
        });
}

// the rows WITHOUT a unit: the zero-gradient update of TensorFlow's dense Adam (m, v decay, p moves on its momentum) -- no table_grad
// array is read or zeroed (two of the plain sweep's eight streams: config C5's dense step moves 53.8 instead of 71.7 GB)
template <bool STREAM>
__device__ __forceinline__ void adam_bitmap_sweep(const cr_adam_desc& d, const cr_tgrad_desc& g, int b, int nb_table, float n, uint32_t t) {
    const int32_t* ix = tg_index(g, t);
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(ix + ix[6]);
    const long long stride = (long long)nb_table * ADAM_NT;
    const adam_consts k = adam_scalars(d, n, t);
    if ((g.D & 3) == 0) {
        const long long n4 = d.n_table >> 2;
        const unsigned D4 = (unsigned)g.D >> 2;
        const int sh = (D4 & (D4 - 1u)) == 0u ? __builtin_ctz(D4) : -1;      // (128 / 256 columns: a shift instead of a 64-bit division per group)
        constexpr int U = 4;
        // p / m / v of a group are requested WITHOUT waiting for the bitmap word that says whether the row is listed (a dependent
        // round trip in front of every batch of loads: the first version swept config C5's table no faster than the sweep that also
        // read and zeroed a gradient array); a listed row's values are read and dropped (2 % of the rows at C5), only its STORES
        // are skipped -- the unit workgroups write those elements
        for (long long q = (long long)b * ADAM_NT + threadIdx.x; q < n4; q += U * stride) {
            bool in[U];
            uint32_t bw[U], row[U];
            f4a p[U], m[U], v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long qq = q + u * stride;
                in[u] = qq < n4;
                const long long qc = in[u] ? qq : q;
                row[u] = sh >= 0 ? (uint32_t)(qc >> sh) : (uint32_t)((unsigned long long)qc / D4);
                bw[u] = bits[row[u] >> 5];
                p[u] = ld4<STREAM>(d.p + 4 * qc); m[u] = ld4<STREAM>(d.m + 4 * qc); v[u] = ld4<STREAM>(d.v + 4 * qc);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (in[u] && !((bw[u] >> (row[u] & 31)) & 1u)) adam_update4<STREAM>(d, k, 4 * (q + u * stride), 0.0f, p[u], m[u], v[u]);
        }
    } else {
        for (long long i = (long long)b * ADAM_NT + threadIdx.x; i < d.n_table; i += stride) {
            const uint32_t row = (uint32_t)((unsigned long long)i / (unsigned)g.D);
            if (!((bits[row >> 5] >> (row & 31)) & 1u)) adam_element(d, k, i, 0.0f);
        }
    }
}

// the table section with a gradient array: 16 bytes per lane per array (4-byte accesses moved 3.2 TB/s on a 188 MB table; see
// DESIGN.md), two groups of four in flight per thread; the scalar head / tail (a start or an end that is not a multiple of 4) goes to
// the first sweep block.
// STREAM (a swept section of the Infinity Cache's size or more): streaming loads / stores, and four groups instead of two in flight
// per thread.  The 10 M-item table of config C5 (71.7 GB per step): 14.2 -> 13.6 ms.  (Four groups cost 76 bytes of scratch at this
// kernel's 128 registers -- the four arrays' 64-bit addresses; a contiguous region per workgroup, which needs one 32-bit offset only,
// ran the sweep 20 % SLOWER: 256 separate streams per array instead of one moving window.)
template <bool STREAM>
__device__ __forceinline__ void adam_plain_sweep(const cr_adam_desc& d, int b, int nb_table, bool lazy, float n, uint32_t t) {
    const long long first = lazy ? (long long)d.lazy_rows * d.lazy_D : 0;      // the lazy part of the table section is not swept
    const long long a0 = min((first + 3) & ~3ll, d.n_table);
    const long long n4 = (d.n_table - a0) >> 2;
    const long long stride = (long long)nb_table * ADAM_NT;
    long long q = (long long)b * ADAM_NT + threadIdx.x;
    // the thread's first group (its only one on a table of a few hundred thousand entries): requested, THEN the scalars
    const bool have = q < n4;
    const long long i1 = a0 + 4 * (have ? q : 0);
    f4a g1 = (f4a){0.f, 0.f, 0.f, 0.f}, p1 = g1, m1 = g1, v1 = g1;
    if (have) { g1 = ld4<STREAM>(d.table_grad + i1); p1 = ld4<STREAM>(d.p + i1); m1 = ld4<STREAM>(d.m + i1); v1 = ld4<STREAM>(d.v + i1); }
    const adam_consts k = adam_scalars(d, n, t);
    if (have) {
        adam_update4_tg<STREAM>(d, k, i1, g1, p1, m1, v1);
        q += stride;
    }
    constexpr int U = STREAM ? 4 : 2;                     // groups of the four arrays requested before the first update
    for (; q + (U - 1) * stride < n4; q += U * stride) {
        f4a g[U], p[U], m[U], v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i = a0 + 4 * (q + u * stride);
            g[u] = ld4<STREAM>(d.table_grad + i); p[u] = ld4<STREAM>(d.p + i); m[u] = ld4<STREAM>(d.m + i); v[u] = ld4<STREAM>(d.v + i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) adam_update4_tg<STREAM>(d, k, a0 + 4 * (q + u * stride), g[u], p[u], m[u], v[u]);
    }
    for (; q < n4; q += stride) {
        const long long i = a0 + 4 * q;
        const f4a g = ld4<STREAM>(d.table_grad + i), p = ld4<STREAM>(d.p + i), m = ld4<STREAM>(d.m + i), v = ld4<STREAM>(d.v + i);
        adam_update4_tg<STREAM>(d, k, i, g, p, m, v);
    }
    if (b == 0) {
        for (long long i = first + threadIdx.x; i < a0; i += ADAM_NT) adam_element_tg(d, k, i);
        for (long long i = a0 + 4 * n4 + threadIdx.x; i < d.n_table; i += ADAM_NT) adam_element_tg(d, k, i);
    }
}

// One launch, every role (adam_grid).  STREAM: the sweep's accesses.  LPR > 0 (with VEC): the table section's gradient comes from the
// batch's occurrence index `g` (cr_tgrad.hpp) -- unit workgroups and the bitmap sweep; LPR == 0: from table_grad -- lazy rows and the
// plain sweep (the host refuses an index together with lazy rows).
template <bool STREAM, int LPR, int VEC>
__global__ __launch_bounds__(ADAM_NT) void k_adam(cr_adam_desc d, cr_tgrad_desc g, adam_grid gr) {
    __shared__ float part_s[ADAM_WAVES * ADAM_COLS + 4];                         // (+ one word: "this slice arrived last", cr_tgrad.hpp)
    constexpr bool TG = LPR > 0;
    cr_kernarg_touch<sizeof(cr_adam_desc) + (TG ? sizeof(cr_tgrad_desc) : 0)>();
    const uint32_t t = d.step_snapshot ? *d.step_snapshot : *reinterpret_cast<const uint32_t*>(d.state + 4);
    const int bid = (int)blockIdx.x;
    const int b_lazy = gr.nb_dense, b_units = b_lazy + gr.nb_lazy, b_sweep = b_units + gr.nb_units, b_ring = b_sweep + gr.nb_table;
    if (bid >= b_ring) return adam_ring_copy(d, bid - b_ring, gr.nb_ring, t);
    const float* st = d.stats ? d.stats : d.state;
    const float n = st[2];
    if (bid < b_lazy) adam_dense_block(d, bid, n, t, reinterpret_cast<float (*)[ADAM_COLS]>(part_s));
    else if (bid < b_units) adam_lazy_rows(d, bid - b_lazy, gr.nb_lazy, n, t);
    else if constexpr (TG) {
        if (bid < b_sweep) adam_unit_blocks<LPR, VEC>(d, g, bid - b_units, gr.nb_units, n, t, part_s);
        else adam_bitmap_sweep<STREAM>(d, g, bid - b_sweep, gr.nb_table, n, t);
    } else adam_plain_sweep<STREAM>(d, bid - b_sweep, gr.nb_table, gr.nb_lazy > 0, n, t);
    if (bid == 0 && threadIdx.x == 0) {
        d.state[5] = (n > 0.0f ? st[0] / n : 0.0f) + (d.n_l2 > 0 ? d.state[7] : 0.0f);   // loss (sasrec.py:105-110)
        d.state[6] = n > 0.0f ? st[1] / n : 0.0f;        // auc   (sasrec.py:113-115)
        if (d.step_snapshot) {                           // end of the step: no block of this kernel reads state[0..4]
            d.state[0] = 0.0f; d.state[1] = 0.0f; d.state[2] = 0.0f; d.state[3] = 0.0f;
            *reinterpret_cast<uint32_t*>(d.state + 4) = t + 1u;
        }
    }
}

// Checks the lazy-row, id-ring and index arguments (in cr_adam_step's order of old: each count follows from what was just checked) and
// lays out the launch's grid; *n_swept: the table elements its sweep blocks walk (decides between the plain and the streaming forms)
static int adam_grid_of(const cr_adam_desc* d, adam_grid* gr, long long* n_swept) {
    *gr = adam_grid{cr_ceil_div(d->n_dense, ADAM_COLS), 0, 0, 0, 0};
    *n_swept = d->n_table;
    CR_REQUIRE(d->lazy_ids2 == nullptr || d->lazy_ids != nullptr, "cr_adam_step: lazy_ids2 needs lazy_ids (it is a second list of the same row-sparse update)");
    if (d->lazy_ids) {
        CR_REQUIRE(d->lazy_flags && d->n_lazy_ids > 0 && d->lazy_rows > 0 && d->lazy_D > 0 &&
                   (long long)d->lazy_rows * d->lazy_D <= d->n_table, "cr_adam_step: bad lazy-row arguments");
        int n_ids = d->n_lazy_ids;
        if (d->lazy_ids2) {
            CR_REQUIRE(d->n_lazy_ids2 >= 1, "cr_adam_step: lazy_ids2 is set but n_lazy_ids2 = %d (at least one id)", d->n_lazy_ids2);
            CR_REQUIRE((long long)d->n_lazy_ids + d->n_lazy_ids2 <= 0x7fffffffll, "cr_adam_step: lazy_ids2: n_lazy_ids + n_lazy_ids2 does not fit an int");
            n_ids += d->n_lazy_ids2;
        }
        gr->nb_lazy = cr_ceil_div(n_ids, ADAM_WAVES * 8);                    // ~8 ids per wave
        if (gr->nb_lazy > 4096) gr->nb_lazy = 4096;
        *n_swept = d->n_table - (long long)d->lazy_rows * d->lazy_D;
    }
    const long long groups = *n_swept / 4 + 1;                               // 16-byte groups (+ one block's worth of head / tail)
    gr->nb_table = (int)((groups + ADAM_NT - 1) / ADAM_NT > 1024 ? 1024 : (groups + ADAM_NT - 1) / ADAM_NT);
    if (gr->nb_table < 1) gr->nb_table = 1;
    if (d->ids_ring) {
        CR_REQUIRE(d->lazy_ids == nullptr, "cr_adam_step: ids_ring and lazy_ids exclude each other (row-sparse Adam reads the step's ids)");
        CR_REQUIRE(d->ids_dst && d->ids_ring_slots > 0 && d->ids_slot_elems > 0, "cr_adam_step: bad id-ring arguments");
        CR_REQUIRE(d->ids_copy_elems >= 0 && d->ids_copy_elems <= d->ids_slot_elems, "cr_adam_step: ids_copy_elems exceeds the slot");
        const long long slot4 = ((d->ids_copy_elems ? d->ids_copy_elems : d->ids_slot_elems) + 3) / 4;
        gr->nb_ring = (int)((slot4 + ADAM_NT - 1) / ADAM_NT > 256 ? 256 : (slot4 + ADAM_NT - 1) / ADAM_NT);
    }
    if (d->tg) {
        const cr_tgrad_desc* g = d->tg;
        const char* why = tg_unsupported(g);
        CR_REQUIRE(why == nullptr, "cr_adam_step: tg: %s", why ? why : "");
        CR_REQUIRE(d->lazy_ids == nullptr, "cr_adam_step: tg and lazy_ids exclude each other");
        CR_REQUIRE(d->n_table == ((int64_t)g->lay.V + g->lay.T_pos) * g->D, "cr_adam_step: tg: n_table must be (V + T_pos) * D");
        CR_REQUIRE((g->ring != nullptr) == (d->ids_ring != nullptr) && (!g->ring || (g->ring == d->ids_ring && g->ring_slots == d->ids_ring_slots && g->slot_words == d->ids_slot_elems)),
                   "cr_adam_step: tg: the index ring must be the id ring of this launch (or both absent)");
        gr->nb_units = tg_unit_grid(g);
    }
    return 0;
}

template <bool STREAM, int LPR, int VEC>
static void adam_launch(const cr_adam_desc* d, const cr_tgrad_desc& g, const adam_grid& gr, void* stream) {
    hipLaunchKernelGGL((k_adam<STREAM, LPR, VEC>), dim3(gr.nb_dense + gr.nb_lazy + gr.nb_units + gr.nb_table + gr.nb_ring), dim3(ADAM_NT), 0, cr_stream(stream), *d, g, gr);
}

extern "C" int cr_adam_step(const cr_adam_desc* d, void* stream) {
    CR_REQUIRE(d && d->p && d->m && d->v && d->state, "cr_adam_step: NULL pointer");
    CR_REQUIRE(d->n_table >= 0 && d->n_dense >= 0 && d->n_table + d->n_dense > 0, "cr_adam_step: bad sizes");
    CR_REQUIRE(d->n_table == 0 || d->table_grad || d->tg, "cr_adam_step: table_grad is NULL");
    CR_REQUIRE(d->n_dense == 0 || (d->dense_slabs && d->n_slabs > 0), "cr_adam_step: dense_slabs missing");
    CR_REQUIRE(d->step_snapshot == nullptr || d->stats != nullptr, "cr_adam_step: step_snapshot needs stats (a copy of the sums that does not alias state[0..2])");
    adam_grid gr;
    long long n_swept;
    if (const int rc = adam_grid_of(d, &gr, &n_swept)) return rc;
    // read on EVERY call (not cached in a static: a test or a tool that sets it after the process's first step would be ignored);
    // a captured graph keeps the instantiation chosen at capture time -- the variable is not looked at again on replay
    const char* nt_env = getenv("CASTREC_ADAM_STREAM");
    const bool stream_sweep = nt_env ? atoi(nt_env) != 0 : n_swept * 4 >= (256ll << 20);
    cr_tgrad_desc g;
    memset(&g, 0, sizeof(g));
    if (!d->tg) {
        stream_sweep ? adam_launch<true, 0, 1>(d, g, gr, stream) : adam_launch<false, 0, 1>(d, g, gr, stream);
    } else {
        g = *d->tg;
        int lpr = 0, vec = 0, ent = 0;
        tg_shape(g.D, &lpr, &vec, &ent);
        tg_dispatch(lpr, vec, [&](auto L, auto V, auto) {
            constexpr int LPR = decltype(L)::value, VEC = decltype(V)::value;
            // (a STREAM form exists for these two shapes only: ADVICE.md item 4)
            if constexpr (VEC == 4 && LPR >= 32) {
                if (stream_sweep) return adam_launch<true, LPR, VEC>(d, g, gr, stream);
            }
            adam_launch<false, LPR, VEC>(d, g, gr, stream);
        });
    }
    return cr_check_launch("cr_adam_step");
}

// l2 * sum(p^2) / 2 over the lookup tables: ONE workgroup, per-thread strided partial sums, then a fixed-order tree
__global__ __launch_bounds__(1024) void k_l2_penalty(const float* p, long long n, float scale, float* state) {
    __shared__ float red[1024];
    float acc = 0.0f;
    for (long long i = threadIdx.x; i < n; i += 1024) acc = fmaf(p[i], p[i], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) state[7] = scale * red[0];
}

extern "C" int cr_l2_penalty(const float* p, int64_t n, float scale, float* state, void* stream) {
    CR_REQUIRE(p && state && n > 0, "cr_l2_penalty: bad arguments");
    hipLaunchKernelGGL(k_l2_penalty, dim3(1), dim3(1024), 0, cr_stream(stream), p, n, scale, state);
    return cr_check_launch("cr_l2_penalty");
}

__global__ __launch_bounds__(64 * ADAM_WAVES) void k_reduce_slabs(const float* slabs, int n_slabs, int n_dense, float* out,
                                                      const float* state, float* stats_out, const int32_t* slab_counts) {
    __shared__ float part[ADAM_WAVES][ADAM_COLS];
    const int j0 = blockIdx.x * ADAM_COLS;
    const float g = slab_sum256(slabs, slab_counts ? min(slab_counts[blockIdx.x], n_slabs) : n_slabs, n_dense, j0, part);
    if (threadIdx.x < ADAM_COLS && j0 + (int)threadIdx.x < n_dense) out[j0 + threadIdx.x] = g;
    if (blockIdx.x == 0 && threadIdx.x < 3 && stats_out) stats_out[threadIdx.x] = state[threadIdx.x];
}

extern "C" int cr_reduce_slabs(const float* dense_slabs, int n_slabs, int n_dense, float* out, const float* state,
                               float* stats_out, const int32_t* slab_counts, void* stream) {
    CR_REQUIRE(dense_slabs && out && n_slabs > 0 && n_dense > 0, "cr_reduce_slabs: bad arguments");
    CR_REQUIRE(stats_out == nullptr || state != nullptr, "cr_reduce_slabs: state is NULL");
    const int grid = cr_ceil_div(n_dense, ADAM_COLS);
    hipLaunchKernelGGL(k_reduce_slabs, dim3(grid), dim3(64 * ADAM_WAVES), 0, cr_stream(stream), dense_slabs, n_slabs, n_dense, out, state, stats_out, slab_counts);
    return cr_check_launch("cr_reduce_slabs");
}

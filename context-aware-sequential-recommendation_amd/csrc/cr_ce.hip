// Full-catalogue softmax cross-entropy (castrec.h cr_softmax_ce): per batch row m the loss logsumexp_v s_mv - s_{m,pos_m} over the
// items v = 1 .. V-1 with s_mv = h_m . E_v, and its un-normalised gradients wrt h and E, without ever writing the [M, V] scores.
// Up to five launches, each deterministic (no float atomics; every partition is fixed by the shape):
//
//  * lse    (a workgroup per 64 rows, 256 threads).  Each wave keeps its 16 rows as B fragments in registers; the workgroup streams the
//           items through an LDS image of 32 rows (bf16 hi / lo, cr_bf16.hpp img_off<2>), filled from registers loaded a block ahead.
//           A wave scores its rows against the block (tk_tile: the product sequence of cr_topk.hip, so a score has the same bits here
//           as there) and folds the scores into a running base-2 max / sum per lane (exp2 with log2 e folded into the score); the four
//           lane groups of a row merge in a fixed butterfly.  Out: lse2 = log2 sum exp2 per row, the row tile's loss / AUC / target sums.
//  * stats  (one wave).  The row tiles' sums in a fixed order: state[0..2] +=, then the snapshot [8..11] (see cr_softmax_ce below).
//  * dh     (same grid as lse).  The same sweep recomputes each score, p = exp2(s log2 e - lse2) minus the one-hot of pos, and multiplies
//           the [16 rows x 32 items] G block by the item block: A = G straight from the two score tiles' accumulators (k slot 8 lg + j
//           <-> item (j < 4 ? 0 : 16) + 4 lg + (j & 3)), B = the same LDS image read transposed (tr_frag with that k order).
//  * de     (a workgroup per 64 items x a part of the rows).  Each wave keeps its 16 items as B fragments; the batch rows of the part
//           stream through the LDS image.  The score tile is computed with the roles swapped (ce_tile_t: rows as A, items as B, the
//           three products in tk_tile's order), so a lane holds rows against its item -- the A operand of dE = G^T H; B = the row
//           image read transposed.  One part: += into table_grad; several: each writes its slice of the workspace, and
//  * de_sum adds the parts into table_grad in part order.
// One MFMA shape in this file (build.py ISA_CHECKED): v_mfma_f32_16x16x32_bf16.
#include <algorithm>

#include "cr_ce.hpp"

namespace {

constexpr int CE_PART_ELEMS = 32768;        // parts x V of the de pass's partial sums at most (the workspace reserves min(16 V, this) rows)
constexpr int CE_MAX_PARTS = 16;

struct CeArgs {
    const float* h; int64_t ldh;
    const float* E;
    const int32_t* pos; const int32_t* neg;
    int M, D, V;
    float* lse2;                            // [M] log2 sum_v exp2(s_mv log2 e)
    float* stats;                           // [n_rt, 4] loss / auc / target sums per row tile
    float* dh; int64_t ldd;
    float* tg;
    float* part;                            // [parts, V, D] (parts > 1)
    int rpp, parts;                         // batch rows per part of the de pass
    float* lse_out;
    float* state;
    int n_rt;
};

// p - [v = pos] of one score, for a target row (l2: the row's lse2).  The same expression in dh and de: the same bits.
__device__ __forceinline__ float ce_g(float s, float l2, bool hit) {
    return ce_exp2(__builtin_fmaf(s, CE_LOG2E, -l2)) - (hit ? 1.0f : 0.0f);
}

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_lse(CeArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ float red[3][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int q = blockIdx.x * 64 + wave * 16 + li;
    const bool qok = q < a.M;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, a.h, a.ldh, q, qok, q == a.M - 1, a.D);
        tk_row_finish<NK, SPLIT>(v, a.h, a.ldh, q, qok, q == a.M - 1, a.D, bh, bl);
    }
    const int pq = qok ? a.pos[q] : 0, nq = (qok && a.neg) ? a.neg[q] : 0;
    float mx = -INFINITY, s_in = 0.0f, s_out = 0.0f, sp = 0.0f, sn = 0.0f;
    const int rounds = (a.V - 1 + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    blk_issue<NCB>(v, a.E, a.D, 1, a.V, a.V - 1, a.D);
    for (int rd = 0; rd < rounds; ++rd) {
        const int i0 = 1 + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.E, a.D, i0, a.V, a.V - 1, a.D);
        __syncthreads();
        if (rd + 1 < rounds) blk_issue<NCB>(v, a.E, a.D, i0 + CE_BLK, a.V, a.V - 1, a.D);
        float t[2][4];
        float bm = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = i0 + 16 * tt + 4 * lg + r;
                const bool ok = id < a.V;
                sp = (ok && id == pq) ? c[r] : sp;
                sn = (ok && id == nq) ? c[r] : sn;
                t[tt][r] = ok ? c[r] * CE_LOG2E : -INFINITY;
                bm = fmaxf(bm, t[tt][r]);
            }
        }
        if (bm > mx) {                                              // (mx = -inf: the sums are 0 and stay 0)
            const float f = ce_exp2(mx - bm);
            s_in *= f;
            s_out *= f;
            mx = bm;
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_in += t[tt][r] > -INFINITY ? ce_exp2(t[tt][r] - mx) : 0.0f;
        if ((rd & 63) == 63) {                                      // two-level sum: 64 rounds per inner partial
            s_out += s_in;
            s_in = 0.0f;
        }
        __syncthreads();
    }
    float s = s_out + s_in;
    // the row's four lane groups: a fixed butterfly, symmetric in the two partners (every lane ends with the same bits)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(s, o, 64);
        const float m2 = fmaxf(mx, mo);
        s = (mx > -INFINITY ? s * ce_exp2(mx - m2) : 0.0f) + (mo > -INFINITY ? so * ce_exp2(mo - m2) : 0.0f);
        mx = m2;
        sp += __shfl_xor(sp, o, 64);                                // one lane of the four holds the score, the others 0
        sn += __shfl_xor(sn, o, 64);
    }
    const float l2 = mx + __log2f(s);
    const bool ist = qok && pq != 0;
    float lr = 0.0f, ar = 0.0f, nr = 0.0f;
    if (qok && lg == 0) {
        a.lse2[q] = l2;
        if (a.lse_out) a.lse_out[q] = l2 * CE_LN2;
        if (ist) {
            lr = l2 * CE_LN2 - sp;
            const float dlt = sp - sn;                              // neg 0 (or none): row 0 reads as zeros
            ar = a.neg ? ((dlt > 0.0f) ? 1.0f : ((dlt < 0.0f) ? 0.0f : 0.5f)) : 0.0f;
            nr = 1.0f;
        }
    }
    lr = wave_sum(lr);
    ar = wave_sum(ar);
    nr = wave_sum(nr);
    if (lane == 0) { red[0][wave] = lr; red[1][wave] = ar; red[2][wave] = nr; }
    __syncthreads();
    if (threadIdx.x < 3) a.stats[blockIdx.x * 4 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// state[0..2] += the row tiles' sums (fixed order), then the snapshot [8..11] the head kernels take (castrec.h, state block).  One
// workgroup adds and snapshots, so it is the last piece of work by construction; the ticket [12] is left re-armed (0).
__global__ __launch_bounds__(64) void k_ce_stats(CeArgs a) {
    const int lane = threadIdx.x;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int i = lane; i < a.n_rt; i += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += a.stats[i * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float t = a.state[k] + s[k];
            a.state[k] = t;
            a.state[8 + k] = t;
        }
        reinterpret_cast<unsigned*>(a.state)[11] = reinterpret_cast<const unsigned*>(a.state)[4];
        reinterpret_cast<unsigned*>(a.state)[12] = 0u;
    }
}

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_dh(CeArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int q = blockIdx.x * 64 + wave * 16 + li;
    const bool qok = q < a.M;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, a.h, a.ldh, q, qok, q == a.M - 1, a.D);
        tk_row_finish<NK, SPLIT>(v, a.h, a.ldh, q, qok, q == a.M - 1, a.D, bh, bl);
    }
    const int pq = qok ? a.pos[q] : 0;
    const bool ist = qok && pq != 0;
    const float l2 = qok ? a.lse2[q] : 0.0f;
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int rounds = (a.V - 1 + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    blk_issue<NCB>(v, a.E, a.D, 1, a.V, a.V - 1, a.D);
    for (int rd = 0; rd < rounds; ++rd) {
        const int i0 = 1 + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.E, a.D, i0, a.V, a.V - 1, a.D);
        __syncthreads();
        if (rd + 1 < rounds) blk_issue<NCB>(v, a.E, a.D, i0 + CE_BLK, a.V, a.V - 1, a.D);
        float g[2][4];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = i0 + 16 * tt + 4 * lg + r;
                g[tt][r] = (ist && id < a.V) ? ce_g(c[r], l2, id == pq) : 0.0f;
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: row 16 wave + 4 lg + r of the tile, column 16 db + li
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        const int col = 16 * db + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = blockIdx.x * 64 + wave * 16 + 4 * lg + r;
            if (row < a.M && col < a.D) a.dh[(int64_t)row * a.ldd + col] = acc[db][r];
        }
    }
}

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_de(CeArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ float s_l2[CE_BLK];
    __shared__ int s_pos[CE_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int id = 1 + blockIdx.x * 64 + wave * 16 + li;
    const bool iok = id < a.V;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, a.E, a.D, id, iok, id == a.V - 1, a.D);
        tk_row_finish<NK, SPLIT>(v, a.E, a.D, id, iok, id == a.V - 1, a.D, bh, bl);
    }
    const int rb = blockIdx.y * a.rpp, re = min(a.M, rb + a.rpp);
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int rounds = (re - rb + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int npos = 0;
    float nl2 = 0.0f;
    blk_issue<NCB>(v, a.h, a.ldh, rb, re, a.M - 1, a.D);
    if (threadIdx.x < CE_BLK && rb + (int)threadIdx.x < re) { npos = a.pos[rb + threadIdx.x]; nl2 = a.lse2[rb + threadIdx.x]; }
    for (int rd = 0; rd < rounds; ++rd) {
        const int r0 = rb + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.h, a.ldh, r0, re, a.M - 1, a.D);
        if (threadIdx.x < CE_BLK) { s_pos[threadIdx.x] = npos; s_l2[threadIdx.x] = nl2; }
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, a.h, a.ldh, r0 + CE_BLK, re, a.M - 1, a.D);
            const int r = r0 + CE_BLK + threadIdx.x;
            npos = 0;
            nl2 = 0.0f;
            if (threadIdx.x < CE_BLK && r < re) { npos = a.pos[r]; nl2 = a.lse2[r]; }
        }
        float g[2][4];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = ce_tile_t<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 16 * tt + 4 * lg + r;
                const int pr = s_pos[lr];
                g[tt][r] = (iok && pr != 0) ? ce_g(c[r], s_l2[lr], pr == id) : 0.0f;
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: item 16 wave + 4 lg + r of the workgroup's 64, column 16 db + li
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        const int col = 16 * db + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int it = 1 + blockIdx.x * 64 + wave * 16 + 4 * lg + r;
            if (it < a.V && col < a.D) {
                if (a.parts == 1) a.tg[(int64_t)it * a.D + col] += acc[db][r];
                else a.part[((int64_t)blockIdx.y * a.V + it) * a.D + col] = acc[db][r];
            }
        }
    }
}

// table_grad[v, :] += sum of the parts' rows v in part order (rows 1 .. V-1)
__global__ __launch_bounds__(256) void k_ce_de_sum(CeArgs a) {
    const int64_t n = (int64_t)(a.V - 1) * a.D, stride = (int64_t)a.V * a.D;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t e = a.D + i;
        float s = a.part[e];
        for (int p = 1; p < a.parts; ++p) s += a.part[p * stride + e];
        a.tg[e] += s;
    }
}

struct CeGeom {
    int NK, n_rt, n_it, parts, rpp;
};

bool ce_geometry(int M, int V, int D, CeGeom& g) {
    if (M < 1 || V < 2 || D < 8 || D > 256) return false;
    const int nk = (D + 31) / 32;
    g.NK = nk <= 1 ? 1 : nk <= 2 ? 2 : nk <= 4 ? 4 : 8;
    g.n_rt = (M + 63) / 64;
    g.n_it = (V - 1 + 63) / 64;
    // the de pass: about 512 workgroups of (64 items x a part of the rows) where the table is short; parts x V <= CE_PART_ELEMS
    int parts = std::min(CE_MAX_PARTS, CE_PART_ELEMS / V);
    parts = std::max(1, std::min(parts, (M + CE_BLK - 1) / CE_BLK));
    g.rpp = ((M + parts - 1) / parts + CE_BLK - 1) / CE_BLK * CE_BLK;
    g.parts = (M + g.rpp - 1) / g.rpp;
    return true;
}

size_t ce_align(size_t x) { return (x + 255) / 256 * 256; }

// workspace: [lse2 M | row-tile sums n_rt x 4 | de partial rows min(16 V, CE_PART_ELEMS) x D] floats (the last section is reserved for
// every shape so that the size never shrinks as V grows; it is used where parts > 1)
size_t ce_workspace(int M, int V, int D, const CeGeom& g) {
    const size_t part_rows = std::min<size_t>((size_t)CE_MAX_PARTS * V, CE_PART_ELEMS);
    return ce_align(4 * (size_t)M) + ce_align(16 * (size_t)g.n_rt) + ce_align(4 * part_rows * D);
}

template <int NK, bool SPLIT>
void ce_launch(const CeArgs& a, const CeGeom& g, hipStream_t st) {
    hipLaunchKernelGGL((k_ce_lse<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ce_stats, dim3(1), dim3(64), 0, st, a);
    if (a.dh) hipLaunchKernelGGL((k_ce_dh<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    if (a.tg) {
        hipLaunchKernelGGL((k_ce_de<NK, SPLIT>), dim3(g.n_it, g.parts), dim3(256), 0, st, a);
        if (g.parts > 1) {
            const int64_t n = (int64_t)(a.V - 1) * a.D;
            const int grid = (int)std::min<int64_t>(2048, (n + 255) / 256);
            hipLaunchKernelGGL(k_ce_de_sum, dim3(grid), dim3(256), 0, st, a);
        }
    }
}

}  // namespace

extern "C" size_t cr_softmax_ce_workspace(int M, int V, int D) {
    CeGeom g;
    if (!ce_geometry(M, V, D, g)) return 0;
    return ce_workspace(M, V, D, g);
}

extern "C" int cr_softmax_ce(const cr_softmax_ce_desc* d, void* stream) {
    CR_REQUIRE(d, "cr_softmax_ce: NULL descriptor");
    CR_REQUIRE(d->seq_emb && d->table && d->pos && d->state, "cr_softmax_ce: NULL seq_emb, table, pos or state");
    CR_REQUIRE(d->D >= 8 && d->D <= 256, "cr_softmax_ce: D=%d outside 8 .. 256", d->D);
    CR_REQUIRE(d->V >= 2, "cr_softmax_ce: V=%d < 2 (row 0 is padding: no item to score)", d->V);
    CR_REQUIRE(d->M >= 1, "cr_softmax_ce: M=%d <= 0", d->M);
    CR_REQUIRE(d->ld >= d->D, "cr_softmax_ce: ld=%d < D=%d", d->ld, d->D);
    CR_REQUIRE(!d->d_seq_emb || d->ldd >= d->D, "cr_softmax_ce: ldd=%d < D=%d", d->ldd, d->D);
    CR_REQUIRE(d->precision == CR_PREC_F32 || d->precision == CR_PREC_BF16X3 || d->precision == CR_PREC_BF16,
               "cr_softmax_ce: unknown precision %d", d->precision);
    CeGeom g;
    CR_REQUIRE(ce_geometry(d->M, d->V, d->D, g), "cr_softmax_ce: unsupported shape");
    const size_t need = ce_workspace(d->M, d->V, d->D, g);
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_softmax_ce: workspace of %zu bytes, cr_softmax_ce_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    CeArgs a;
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V;
    a.lse2 = reinterpret_cast<float*>(w); w += ce_align(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += ce_align(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w);
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = d->lse_out; a.state = d->state; a.n_rt = g.n_rt;
    hipStream_t st = cr_stream(stream);
    const bool split = d->precision != CR_PREC_BF16;       // CR_PREC_F32: the bf16x3 products (fp32-grade)
#define CE_NK(NK) (split ? ce_launch<NK, true>(a, g, st) : ce_launch<NK, false>(a, g, st))
    if (g.NK == 1) CE_NK(1);
    else if (g.NK == 2) CE_NK(2);
    else if (g.NK == 4) CE_NK(4);
    else CE_NK(8);
#undef CE_NK
    return cr_check_launch("cr_softmax_ce");
}

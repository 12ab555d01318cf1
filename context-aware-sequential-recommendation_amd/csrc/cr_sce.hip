// Sampled softmax cross-entropy with shared uniform negatives (castrec.h cr_sampled_ce): per batch row m the loss
// log(exp z_{m,pos} + sum_{j: s_j != pos_m} exp z_{m,s_j}) - z_{m,pos} over the target and N sample ids shared by the call, and its
// un-normalised gradients wrt h and E.  The passes of cr_ce.hip (cr_ce.hpp: the streamed LDS block, the swapped score tile, the G x
// image product) run against a compact candidate table instead of the catalogue, so the cost is O(M N D), independent of V:
//
//  * ids    (grid-stride over N x D).  Copy or draw the N ids (castrec.h states the draw), write them and samples_out, and gather the
//           N rows of E into the compact fp32 table Es [N, D] of the workspace.
//  * dedup  (a thread per sample; only with table_grad).  For sample j: whether it is its id's first occurrence, and the next j' > j
//           with the same id (a linked list in j order).  Each thread compares its id against all N through LDS chunks: O(N^2) compares,
//           a few microseconds at N = 4096.
//  * lse    (a workgroup per 64 rows, as k_ce_lse).  The sweep streams Es; a sample equal to the row's target is masked.  The target
//           and neg scores come from diagonal tiles of the gathered rows E[pos] / E[neg] against the wave's own rows -- tk_tile, the
//           product sequence of every sweep (cr_score_topk's ranks use the same trick).  The target enters the running max / sum
//           of lane group 0 before the first block.  Out: lse2 per row, gpos = p_pos - 1 per target row, the row tile's sums.
//  * stats  (one wave).  The row tiles' sums in a fixed order into state[0..2], then the snapshot [8..11].
//  * dh     (same grid as lse).  As k_ce_dh over Es with the hit mask; the epilogue adds gpos_m E[pos_m] in fp32.
//  * de     (a workgroup per 64 samples x a part of the rows, as k_ce_de).  Each part writes its [N, D] slice of the workspace.
//  * scatter (a workgroup per sample).  The first occurrence of each id walks its list in j order, adds the parts in part order and
//           += the sum into table_grad[id]: one writer per distinct id, no float atomics.
//  * tgt    (grid-stride over M x D).  dE_{pos_m} += gpos_m h_m with float atomics (the one non-deterministic output).
// One MFMA shape in this file (build.py ISA_CHECKED): v_mfma_f32_16x16x32_bf16.
#include <algorithm>

#include "cr_ce.hpp"

namespace {

constexpr int SCE_PART_ROWS = 65536;        // parts x N of the de pass's partial sums at most
constexpr int SCE_MAX_PARTS = 64;
constexpr int SCE_CHUNK = 2048;             // ids per LDS chunk of the dedup pass

struct SceArgs {
    const float* h; int64_t ldh;
    const float* E;
    const int32_t* pos; const int32_t* neg;
    int M, D, V, N;
    const int32_t* samples;                 // caller's ids, or NULL: drawn from (seed, *step)
    uint32_t seed; const uint32_t* step;
    int32_t* sid;                           // [N] the ids used
    int32_t* samples_out;
    int32_t* nxt;                           // [N] next j' > j with the same id (N: none)
    int32_t* head;                          // [N] 1 where j is its id's first occurrence
    float* Es;                              // [N, D] gathered rows
    float* lse2;                            // [M] log2 of the candidate sum (base-2 exponent of the scores)
    float* gpos;                            // [M] p_pos - 1 for target rows, 0 elsewhere
    float* stats;                           // [n_rt, 4] loss / auc / target sums per row tile
    float* dh; int64_t ldd;
    float* tg;
    float* part;                            // [parts, N, D]
    int rpp, parts;                         // batch rows per part of the de pass
    float* lse_out;
    float* state;
    int n_rt;
};

__global__ __launch_bounds__(256) void k_sce_ids(SceArgs a) {
    const uint32_t key = a.samples ? 0u : cr_site_key(a.seed, *a.step, CR_SCE_SITE);
    const int64_t n = (int64_t)a.N * a.D;
    for (int64_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e / a.D), c = (int)(e % a.D);
        int id;
        if (a.samples) {
            id = a.samples[j];
        } else {
            const uint32_t x = cr_fmix32(key + (uint32_t)j * CR_PHI);
            id = 1 + (int)(uint32_t)(((uint64_t)x * (uint32_t)(a.V - 1)) >> 32);
        }
        a.Es[e] = a.E[(int64_t)id * a.D + c];
        if (c == 0) {
            a.sid[j] = id;
            if (a.samples_out) a.samples_out[j] = id;
        }
    }
}

// (after k_sce_ids) head / nxt of every sample: compares against the N ids in chunks of SCE_CHUNK staged in LDS
__global__ __launch_bounds__(256) void k_sce_dedup(SceArgs a) {
    __shared__ int ids[SCE_CHUNK];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int mine = j < a.N ? a.sid[j] : -1;
    bool first = true;
    int nx = a.N;
    for (int c0 = 0; c0 < a.N; c0 += SCE_CHUNK) {
        const int n = min(SCE_CHUNK, a.N - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) ids[i] = a.sid[c0 + i];
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const int k = c0 + i;
            if (ids[i] == mine) {
                first = first && k >= j;
                nx = (k > j && k < nx) ? k : nx;
            }
        }
    }
    if (j < a.N) {
        a.head[j] = first ? 1 : 0;
        a.nxt[j] = nx;
    }
}

// a wave's diagonal: the score of row (query) li against operand row li of (th, tl), in every lane of the row (tk_tile's bits)
template <int NK, bool SPLIT>
__device__ __forceinline__ float sce_diag(const bf8 (&th)[NK], const bf8 (&tl)[NK], const bf8 (&bh)[NK], const bf8 (&bl)[NK]) {
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const f32x4 c = tk_tile<NK, SPLIT>(th, tl, bh, bl);       // register r of lane (li, lg): operand row 4 lg + r against query li
    const int r = li & 3;
    float x = r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3];
    x = lg == (li >> 2) ? x : 0.0f;
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}

// score of each lane's row against E[id] (id per lane, rok: the lane's row exists)
template <int NK, bool SPLIT>
__device__ __forceinline__ float sce_gathered_score(const SceArgs& a, int id, bool rok, const bf8 (&bh)[NK], const bf8 (&bl)[NK]) {
    bf8 th[NK], tl[NK];
    float v[NK][8];
    tk_row_issue<NK>(v, a.E, a.D, id, rok, id == a.V - 1, a.D);
    tk_row_finish<NK, SPLIT>(v, a.E, a.D, id, rok, id == a.V - 1, a.D, th, tl);
    return sce_diag<NK, SPLIT>(th, tl, bh, bl);
}

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_sce_lse(SceArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ int s_id[CE_BLK];
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
    const float sp = sce_gathered_score<NK, SPLIT>(a, pq, qok, bh, bl);
    float sn = 0.0f;
    if (a.neg) {                                                    // (uniform: the tile runs with every lane on)
        const float x = sce_gathered_score<NK, SPLIT>(a, nq, qok, bh, bl);
        sn = nq != 0 ? x : 0.0f;                                    // neg 0: a zero score, as cr_softmax_ce
    }
    // the target is lane group 0's first candidate
    const float tp = sp * CE_LOG2E;
    float mx = lg == 0 ? tp : -INFINITY, s_in = lg == 0 ? 1.0f : 0.0f, s_out = 0.0f;
    const int rounds = (a.N + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int nid = 0;
    blk_issue<NCB>(v, a.Es, a.D, 0, a.N, a.N - 1, a.D);
    if (threadIdx.x < CE_BLK && (int)threadIdx.x < a.N) nid = a.sid[threadIdx.x];
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.Es, a.D, j0, a.N, a.N - 1, a.D);
        if (threadIdx.x < CE_BLK) s_id[threadIdx.x] = nid;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, a.Es, a.D, j0 + CE_BLK, a.N, a.N - 1, a.D);
            const int j = j0 + CE_BLK + threadIdx.x;
            nid = (threadIdx.x < CE_BLK && j < a.N) ? a.sid[j] : 0;
        }
        float t[2][4];
        float bm = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * tt + 4 * lg + r;
                const bool ok = j0 + jl < a.N && s_id[jl] != pq;
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
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {                            // the fixed butterfly of k_ce_lse
        const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(s, o, 64);
        const float m2 = fmaxf(mx, mo);
        s = (mx > -INFINITY ? s * ce_exp2(mx - m2) : 0.0f) + (mo > -INFINITY ? so * ce_exp2(mo - m2) : 0.0f);
        mx = m2;
    }
    const float l2 = mx + __log2f(s);
    const bool ist = qok && pq != 0;
    float lr = 0.0f, ar = 0.0f, nr = 0.0f;
    if (qok && lg == 0) {
        a.lse2[q] = l2;
        // relative to the target's own base-2 score: a row whose every sample is a hit gets l = 0 and p_pos - 1 = 0 exactly
        a.gpos[q] = ist ? ce_exp2(tp - l2) - 1.0f : 0.0f;
        if (a.lse_out) a.lse_out[q] = l2 * CE_LN2;
        if (ist) {
            lr = (l2 - tp) * CE_LN2;
            const float dlt = sp - sn;
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

// state[0..2] += the row tiles' sums (fixed order), then the snapshot [8..11] (as k_ce_stats; ticket [12] left at 0)
__global__ __launch_bounds__(64) void k_sce_stats(SceArgs a) {
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

// p of a (row, sample) score for a target row (l2: the row's lse2).  The same expression in dh and de: the same bits.
__device__ __forceinline__ float sce_p(float s, float l2) { return ce_exp2(__builtin_fmaf(s, CE_LOG2E, -l2)); }

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_sce_dh(SceArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ int s_id[CE_BLK];
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
    const int rounds = (a.N + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int nid = 0;
    blk_issue<NCB>(v, a.Es, a.D, 0, a.N, a.N - 1, a.D);
    if (threadIdx.x < CE_BLK && (int)threadIdx.x < a.N) nid = a.sid[threadIdx.x];
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.Es, a.D, j0, a.N, a.N - 1, a.D);
        if (threadIdx.x < CE_BLK) s_id[threadIdx.x] = nid;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, a.Es, a.D, j0 + CE_BLK, a.N, a.N - 1, a.D);
            const int j = j0 + CE_BLK + threadIdx.x;
            nid = (threadIdx.x < CE_BLK && j < a.N) ? a.sid[j] : 0;
        }
        float g[2][4];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * tt + 4 * lg + r;
                g[tt][r] = (ist && j0 + jl < a.N && s_id[jl] != pq) ? sce_p(c[r], l2) : 0.0f;
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: row 16 wave + 4 lg + r of the tile, column 16 db + li; plus the target term (p_pos - 1) E_pos
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = blockIdx.x * 64 + wave * 16 + 4 * lg + r;
        if (row >= a.M) continue;
        const int pr = a.pos[row];
        const float gp = a.gpos[row];
        const float* er = a.E + (int64_t)pr * a.D;
#pragma unroll
        for (int db = 0; db < 2 * NK; ++db) {
            const int col = 16 * db + li;
            if (col < a.D) a.dh[(int64_t)row * a.ldd + col] = pr != 0 ? __builtin_fmaf(gp, er[col], acc[db][r]) : 0.0f;
        }
    }
}

template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_sce_de(SceArgs a) {
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ float s_l2[CE_BLK];
    __shared__ int s_pos[CE_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int j = blockIdx.x * 64 + wave * 16 + li;
    const bool jok = j < a.N;
    const int sj = jok ? a.sid[j] : -1;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, a.Es, a.D, j, jok, j == a.N - 1, a.D);
        tk_row_finish<NK, SPLIT>(v, a.Es, a.D, j, jok, j == a.N - 1, a.D, bh, bl);
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
                g[tt][r] = (jok && pr != 0 && pr != sj) ? sce_p(c[r], s_l2[lr]) : 0.0f;
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: sample 16 wave + 4 lg + r of the workgroup's 64, column 16 db + li
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        const int col = 16 * db + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int js = blockIdx.x * 64 + wave * 16 + 4 * lg + r;
            if (js < a.N && col < a.D) a.part[((int64_t)blockIdx.y * a.N + js) * a.D + col] = acc[db][r];
        }
    }
}

// table_grad[s_j] += the sum over the id's samples (j order) of the parts (part order); one workgroup per first occurrence
__global__ __launch_bounds__(256) void k_sce_scatter(SceArgs a) {
    const int j = blockIdx.x;
    if (!a.head[j]) return;
    const int64_t stride = (int64_t)a.N * a.D;
    const int id = a.sid[j];
    for (int c = threadIdx.x; c < a.D; c += 256) {
        float acc = 0.0f;
        for (int k = j; k < a.N; k = a.nxt[k]) {
            const int64_t e = (int64_t)k * a.D + c;
            float s = a.part[e];
            for (int p = 1; p < a.parts; ++p) s += a.part[p * stride + e];
            acc += s;
        }
        a.tg[(int64_t)id * a.D + c] += acc;
    }
}

// dE_{pos_m} += (p_pos - 1) h_m for the target rows (float atomics: rows repeat)
__global__ __launch_bounds__(256) void k_sce_tgt(SceArgs a) {
    const int64_t n = (int64_t)a.M * a.D;
    for (int64_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int m = (int)(e / a.D), c = (int)(e % a.D);
        const int p = a.pos[m];
        if (p != 0) atomicAdd(a.tg + (int64_t)p * a.D + c, a.gpos[m] * a.h[(int64_t)m * a.ldh + c]);
    }
}

struct SceGeom {
    int NK, n_rt, n_jt, parts, rpp;
};

bool sce_geometry(int M, int N, int D, SceGeom& g) {
    if (M < 1 || N < 1 || N > CR_SCE_MAX_SAMPLES || D < 8 || D > 256) return false;
    const int nk = (D + 31) / 32;
    g.NK = nk <= 1 ? 1 : nk <= 2 ? 2 : nk <= 4 ? 4 : 8;
    g.n_rt = (M + 63) / 64;
    g.n_jt = (N + 63) / 64;
    int parts = std::min(SCE_MAX_PARTS, SCE_PART_ROWS / N);
    parts = std::max(1, std::min(parts, (M + CE_BLK - 1) / CE_BLK));
    g.rpp = ((M + parts - 1) / parts + CE_BLK - 1) / CE_BLK * CE_BLK;
    g.parts = (M + g.rpp - 1) / g.rpp;
    return true;
}

size_t sce_align(size_t x) { return (x + 255) / 256 * 256; }
size_t sce_part_rows(int N) { return std::min<size_t>((size_t)SCE_MAX_PARTS * N, std::max<size_t>(N, SCE_PART_ROWS)); }

// workspace: [sid | nxt | head: N ints each | Es N x D | lse2 M | gpos M | row-tile sums n_rt x 4 | de parts min(64 N, 65536) x D]
// (the parts section is sized by N alone, so the total never decreases as M or N grows)
size_t sce_workspace(int M, int N, int D, const SceGeom& g) {
    return 3 * sce_align(4 * (size_t)N) + sce_align(4 * (size_t)N * D) + 2 * sce_align(4 * (size_t)M) + sce_align(16 * (size_t)g.n_rt) +
           sce_align(4 * sce_part_rows(N) * D);
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256)); }

template <int NK, bool SPLIT>
void sce_launch(const SceArgs& a, const SceGeom& g, hipStream_t st) {
    hipLaunchKernelGGL(k_sce_ids, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, a);
    if (a.tg) hipLaunchKernelGGL(k_sce_dedup, dim3((a.N + 255) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_sce_lse<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sce_stats, dim3(1), dim3(64), 0, st, a);
    if (a.dh) hipLaunchKernelGGL((k_sce_dh<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    if (a.tg) {
        hipLaunchKernelGGL((k_sce_de<NK, SPLIT>), dim3(g.n_jt, g.parts), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_sce_scatter, dim3(a.N), dim3(std::min(256, (a.D + 63) / 64 * 64)), 0, st, a);
        hipLaunchKernelGGL(k_sce_tgt, dim3(grid_for((int64_t)a.M * a.D)), dim3(256), 0, st, a);
    }
}

}  // namespace

extern "C" size_t cr_sampled_ce_workspace(int M, int N, int D) {
    SceGeom g;
    if (!sce_geometry(M, N, D, g)) return 0;
    return sce_workspace(M, N, D, g);
}

extern "C" int cr_sampled_ce(const cr_sampled_ce_desc* d, void* stream) {
    CR_REQUIRE(d, "cr_sampled_ce: NULL descriptor");
    CR_REQUIRE(d->seq_emb && d->table && d->pos && d->state, "cr_sampled_ce: NULL seq_emb, table, pos or state");
    CR_REQUIRE(d->D >= 8 && d->D <= 256, "cr_sampled_ce: D=%d outside 8 .. 256", d->D);
    CR_REQUIRE(d->V >= 2, "cr_sampled_ce: V=%d < 2 (row 0 is padding: no item to sample)", d->V);
    CR_REQUIRE(d->M >= 1, "cr_sampled_ce: M=%d <= 0", d->M);
    CR_REQUIRE(d->N >= 1 && d->N <= CR_SCE_MAX_SAMPLES, "cr_sampled_ce: N=%d outside 1 .. %d", d->N, CR_SCE_MAX_SAMPLES);
    CR_REQUIRE(d->ld >= d->D, "cr_sampled_ce: ld=%d < D=%d", d->ld, d->D);
    CR_REQUIRE(!d->d_seq_emb || d->ldd >= d->D, "cr_sampled_ce: ldd=%d < D=%d", d->ldd, d->D);
    CR_REQUIRE(d->precision == CR_PREC_F32 || d->precision == CR_PREC_BF16X3 || d->precision == CR_PREC_BF16,
               "cr_sampled_ce: unknown precision %d", d->precision);
    CR_REQUIRE(d->samples || d->step, "cr_sampled_ce: NULL step with NULL samples (the device draw reads the step word)");
    SceGeom g;
    CR_REQUIRE(sce_geometry(d->M, d->N, d->D, g), "cr_sampled_ce: unsupported shape");
    const size_t need = sce_workspace(d->M, d->N, d->D, g);
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_sampled_ce: workspace of %zu bytes, cr_sampled_ce_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    SceArgs a;
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V; a.N = d->N;
    a.samples = d->samples; a.seed = d->seed; a.step = d->step; a.samples_out = d->samples_out;
    a.sid = reinterpret_cast<int32_t*>(w); w += sce_align(4 * (size_t)d->N);
    a.nxt = reinterpret_cast<int32_t*>(w); w += sce_align(4 * (size_t)d->N);
    a.head = reinterpret_cast<int32_t*>(w); w += sce_align(4 * (size_t)d->N);
    a.Es = reinterpret_cast<float*>(w); w += sce_align(4 * (size_t)d->N * d->D);
    a.lse2 = reinterpret_cast<float*>(w); w += sce_align(4 * (size_t)d->M);
    a.gpos = reinterpret_cast<float*>(w); w += sce_align(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += sce_align(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w);
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = d->lse_out; a.state = d->state; a.n_rt = g.n_rt;
    hipStream_t st = cr_stream(stream);
    const bool split = d->precision != CR_PREC_BF16;       // CR_PREC_F32: the bf16x3 products (fp32-grade)
#define SCE_NK(NK) (split ? sce_launch<NK, true>(a, g, st) : sce_launch<NK, false>(a, g, st))
    if (g.NK == 1) SCE_NK(1);
    else if (g.NK == 2) SCE_NK(2);
    else if (g.NK == 4) SCE_NK(4);
    else SCE_NK(8);
#undef SCE_NK
    return cr_check_launch("cr_sampled_ce");
}

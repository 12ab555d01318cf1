// Softmax cross-entropy without ever writing the [M, candidates] scores, and its un-normalised gradients wrt h and E (castrec.h):
//  * cr_softmax_ce, the full catalogue: per batch row m the loss logsumexp_v s_mv - s_{m,pos_m} over the items v = 1 .. V-1 with
//    s_mv = h_m . E_v;
//  * cr_sampled_ce, shared uniform negatives: log(exp z_{m,pos} + sum_{j: s_j != pos_m} exp z_{m,s_j}) - z_{m,pos} over the target and
//    N sample ids shared by the call, against a compact table of the samples' rows, so the cost is O(M N D), independent of V.
//  * cr_gbce, gSASRec's generalised binary cross-entropy over the same shared negatives: beta softplus(-z_{m,pos}) + sum_{j: s_j !=
//    pos_m} softplus(z_{m,s_j}).  A pointwise objective has no normaliser, so one row sweep gives the loss and dh (gbce_row below) and
//    the item sweep is de without a per-row statistic; ids, dedup, stats, scatter and tgt are the sampled op's.
// The two softmax ops run the same four sweep passes, templated on the candidate kind -- the argument struct: CeArgs, the catalogue, whose candidates
// are the items 1 .. V-1 of E with the target among them; SceArgs, the sampled, whose candidates are the N gathered rows Es with the
// target beside them (a sample equal to a row's target is masked; the target's own terms come separately); ScePopArgs, the sampled
// under a popularity proposal, whose every candidate score carries the log-Q correction -logq[id] (castrec.h) as a base-2 bias that
// travels beside the ids:
//
//  * lse    (a workgroup per 64 rows, 256 threads).  Each wave keeps its 16 rows as B fragments in registers; the workgroup streams the
//           candidates through an LDS image of 32 rows (bf16 hi / lo, cr_bf16.hpp img_off<2>), filled from registers loaded a block
//           ahead.  A wave scores its rows against the block (tk_tile: the product sequence of cr_topk.hip, so a score has the same bits
//           here as there) and folds the scores into a running base-2 max / sum per lane (exp2 with log2 e folded into the score); the
//           four lane groups of a row merge in a fixed butterfly.  Out: lse2 = log2 sum exp2 per row, the row tile's loss / AUC / target
//           sums.  Catalogue: the target and neg scores are picked up as the sweep passes them.  Sampled: they come from diagonal tiles
//           of the gathered rows E[pos] / E[neg] against the wave's own rows (tk_tile again; cr_score_topk's ranks use the same trick),
//           the target enters the running max / sum of lane group 0 before the first block, and gpos = p_pos - 1 is written per row.
//  * stats  (one wave).  The row tiles' sums in a fixed order: state[0..2] +=, then the snapshot [8..11] (see castrec.h, state block).
//  * dh     (same grid as lse).  The same sweep recomputes each score, p = exp2(s log2 e - lse2) (catalogue: minus the one-hot of pos;
//           sampled: 0 at a hit), and multiplies the [16 rows x 32 candidates] G block by the candidate block: A = G straight from the
//           two score tiles' accumulators (k slot 8 lg + j <-> candidate (j < 4 ? 0 : 16) + 4 lg + (j & 3)), B = the same LDS image
//           read transposed (tr_frag with that k order).  Sampled: the epilogue adds gpos_m E[pos_m] in fp32.
//  * de     (a workgroup per 64 candidates x a part of the rows).  Each wave keeps its 16 candidates as B fragments; the batch rows of
//           the part stream through the LDS image.  The score tile is computed with the roles swapped (ce_tile_t: rows as A, candidates
//           as B, the three products in tk_tile's order), so a lane holds rows against its candidate -- the A operand of dE = G^T H;
//           B = the row image read transposed.  Each part writes its slice of the workspace; a catalogue of one part += into table_grad.
// Around the sweeps, per op:
//  * de_sum  (catalogue, parts > 1) adds the parts into table_grad in part order.
//  * ids     (sampled; grid-stride over N x D).  Copy or draw the N ids (castrec.h states the draw), write them and samples_out, and
//            gather the N rows of E into the compact fp32 table Es [N, D] of the workspace.  Popularity proposal (ids_pop): the id of
//            a sample is found once, by the workgroup that holds its first element -- a copy, or the binary search of the cdf -- and
//            handed to the gathering threads through LDS; the same thread writes the sample's bias -logq[id] log2 e.
//  * dedup   (sampled, a thread per sample; only with table_grad).  For sample j: whether it is its id's first occurrence, and the next
//            j' > j with the same id (a linked list in j order).  Each thread compares its id against all N through LDS chunks: O(N^2)
//            compares, a few microseconds at N = 4096.
//  * scatter (sampled, a workgroup per sample).  The first occurrence of each id walks its list in j order, adds the parts in part
//            order and += the sum into table_grad[id]: one writer per distinct id.
//  * tgt     (sampled; grid-stride over M x D).  dE_{pos_m} += gpos_m h_m with float atomics.
//  * gbce_row (gBCE; the grid of lse).  The sweep of dh with g = sigma(score) (0 at a hit) from one exp2 per score, the softplus of the
//            same exponential summed per lane in sweep order, and lse's prologue / epilogue: the target's score from the diagonal
//            tile, gpos = beta (sigma_pos - 1), the row's loss, the row tile's sums, dh += gpos E[pos] in fp32.
// Every partition is fixed by the shape; the sampled tgt is the only pass with float atomics (the one non-deterministic output).
// One MFMA shape in this file (build.py ISA_CHECKED): v_mfma_f32_16x16x32_bf16.
#include <algorithm>

#include "cr_bf16.hpp"

namespace {

constexpr float CE_LOG2E = 1.4426950408889634f;
constexpr float CE_LN2 = 0.6931471805599453f;
constexpr int CE_BLK = 32;                  // rows of the streamed LDS block (candidates in lse / dh, batch rows in de)
constexpr int CE_PART_ELEMS = 32768;        // catalogue: parts x V of the de pass's partial sums at most (the workspace reserves
constexpr int CE_MAX_PARTS = 16;            //   min(16 V, this) rows)
constexpr int SCE_PART_ROWS = 65536;        // sampled: parts x N of the de pass's partial sums at most
constexpr int SCE_MAX_PARTS = 64;
constexpr int SCE_CHUNK = 2048;             // ids per LDS chunk of the dedup pass

struct CeArgs {
    static constexpr bool SAMPLED = false, GBCE = false, POP = false;
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

struct SceArgs {
    static constexpr bool SAMPLED = true, GBCE = false, POP = false;
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

// gBCE: the sampled op's candidates and buffers (lse2 unused; lse_out takes the per-row loss), g = sigma instead of the softmax's p
struct GbceArgs : SceArgs {
    static constexpr bool GBCE = true;
    float beta;                             // weight of the positive term, (0, 1]
};

// sampled softmax under a popularity proposal: z' = z - logq[id] for every candidate, the target included (castrec.h)
struct ScePopArgs : SceArgs {
    static constexpr bool POP = true;
    const uint32_t* cdf;                    // [V] the proposal's cumulative masses in units of 2^-32 (device draw), or NULL
    const float* logq;                      // [V] log Q(v); [0] = 0
    float* sb;                              // [N] the samples' base-2 biases -logq[s_j] log2 e
};

// ---- the streamed block ---------------------------------------------------------------------------------------------------
// CE_BLK rows of an fp32 matrix loaded a block ahead into registers, stored as a bf16 hi / lo LDS image, read back as row operands or
// transposed.  CE_BLK rows x NCB blocks of 64 columns, bf16 hi and lo:
template <int NCB>
struct CeImg {
    __bf16 hi[NCB][CE_BLK * 64];
    __bf16 lo[NCB][CE_BLK * 64];
};

// Rows r0 .. r0 + 31 of src into registers: thread t owns the 8-column chunks t + 256 i (row-major over the image's 8 NCB chunks per
// row).  Rows >= end are read as row 0's last columns and masked to zero (cr_bf16.hpp items); `last`: the matrix's last row.
template <int NCB>
__device__ __forceinline__ void blk_issue(float (&v)[NCB][8], const float* src, int64_t ld, int r0, int end, int last, int D) {
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / (8 * NCB), c = 8 * (idx % (8 * NCB));
        const int r = r0 + row;
        const bool rok = r < end;
        item_issue(v[i], src + (rok ? (int64_t)r * ld : 0), c, D, !rok || item_fix(rok, r == last, c, D));
    }
}
template <int NCB, bool SPLIT>
__device__ __forceinline__ void blk_store(float (&v)[NCB][8], CeImg<NCB>& img, const float* src, int64_t ld, int r0, int end, int last,
                                          int D) {
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / (8 * NCB), ch = idx % (8 * NCB), c = 8 * ch;
        const int r = r0 + row;
        const bool rok = r < end;
        const bool fix = item_fix(rok, r == last, c, D);
        item_mask(v[i], c, D, rok, fix);
        if (fix) item_refill(v[i], src + (int64_t)r * ld, c, D);
        bf8 h, l;
        split8<SPLIT>(v[i], h, l);
        const int off = img_off<2>(row, ch & 7);
        *reinterpret_cast<bf8*>(&img.hi[ch >> 3][off]) = h;
        if (SPLIT) *reinterpret_cast<bf8*>(&img.lo[ch >> 3][off]) = l;
    }
}

// rows row0 + li of the image as an operand with k = columns (k-step ks: columns 32 ks + 8 lg .. + 7, as tk_row_finish lays them out)
template <int NK, int NCB, bool SPLIT>
__device__ __forceinline__ void img_rows(const CeImg<NCB>& img, int row0, bf8 (&h)[NK], bf8 (&l)[NK]) {
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        h[ks] = row_frag<2>(img.hi[ks >> 1], row0, ks & 1);
        l[ks] = SPLIT ? row_frag<2>(img.lo[ks >> 1], row0, ks & 1) : h[ks];
    }
}

// tk_tile with the operands' roles swapped: register r of lane (li, lg) = row 4 lg + r (A) against item li (B).  Per element the
// same three products in the same order (item lo x row hi, item hi x row lo, hi x hi): the MFMA's element function is a sum of exact
// bf16 products in k order, symmetric in its two operands, so an (item, row) pair gets tk_tile's bits.
template <int NK, bool SPLIT>
__device__ __forceinline__ f32x4 ce_tile_t(const bf8 (&rh)[NK], const bf8 (&rl)[NK], const bf8 (&ih)[NK], const bf8 (&il)[NK]) {
    f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        if (SPLIT) {
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rh[ks], il[ks], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl[ks], ih[ks], c, 0, 0, 0);
        }
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rh[ks], ih[ks], c, 0, 0, 0);
    }
    return c;
}

// two score tiles' registers (k slots 8 lg + j: tile j >> 2, register j & 3) as one operand of a k = 32 product
template <bool SPLIT>
__device__ __forceinline__ void g_frag(const float (&g)[2][4], bf8& h, bf8& l) {
    const float x[8] = {g[0][0], g[0][1], g[0][2], g[0][3], g[1][0], g[1][1], g[1][2], g[1][3]};
    split8<SPLIT>(x, h, l);
    if (!SPLIT) l = h;
}

// acc[db] += G x (the image read transposed: k = image row in g_frag's order, columns 16 db .. + 15), for the column blocks below D
template <int NK, int NCB, bool SPLIT>
__device__ __forceinline__ void g_times_img(f32x4 (&acc)[2 * NK], const bf8& gh, const bf8& gl, const CeImg<NCB>& img, int D) {
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        if (16 * db < D) {                                          // uniform: every lane reads (ds_read_b64_tr_b16 wants EXEC full)
            const bf8 bh = tr_frag<2>(img.hi[db >> 2], 0, 16, db & 3);
            const bf8 bl = SPLIT ? tr_frag<2>(img.lo[db >> 2], 0, 16, db & 3) : bh;
            acc[db] = mma<SPLIT>(gh, gl, bh, bl, acc[db]);
        }
    }
}

__device__ __forceinline__ float ce_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// p of one (row, candidate) score for a target row (l2: the row's lse2).  The same expression in dh and de: the same bits.
__device__ __forceinline__ float ce_p(float s, float l2) { return ce_exp2(__builtin_fmaf(s, CE_LOG2E, -l2)); }
// ... of a corrected score (b: the candidate's base-2 bias)
__device__ __forceinline__ float ce_pb(float s, float b, float l2) { return ce_exp2(__builtin_fmaf(s, CE_LOG2E, b) - l2); }
// catalogue: p - [v = pos] (a sampled hit is masked instead)
__device__ __forceinline__ float ce_g(float s, float l2, bool hit) { return ce_p(s, l2) - (hit ? 1.0f : 0.0f); }

// gBCE: e = exp(-|s|) serves both sigma(s) and softplus(s) = max(s, 0) + log(1 + e).  Below 2^-12 the log is the series e - e^2 / 2
// (1 + e would round e away: truncation e^3 / 3 < 2^-25 e); above it 1 + e carries e to 2^-12 relative at worst, 2^-24 absolute.
__device__ __forceinline__ float gb_e(float s) { return ce_exp2(-fabsf(s) * CE_LOG2E); }
__device__ __forceinline__ float gb_sigma(float s, float e) {
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    return s >= 0.0f ? r : e * r;
}
__device__ __forceinline__ float gb_softplus(float s, float e) {
    const float l = e < 0x1p-12f ? __builtin_fmaf(-0.5f * e, e, e) : __log2f(1.0f + e) * CE_LN2;
    return fmaxf(s, 0.0f) + l;
}

// ---- the sampled-only pieces around the sweeps ---------------------------------------------------------------------------
template <uint32_t SITE>
__global__ __launch_bounds__(256) void k_sce_ids(SceArgs a) {
    const uint32_t key = a.samples ? 0u : cr_site_key(a.seed, *a.step, SITE);
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

// Popularity proposal.  A workgroup takes 256 consecutive elements of [N, D] per round: they span at most 256 / 8 + 1 samples, whose
// ids the first threads copy or draw -- s_j = the smallest s in [1, V-1] with x_j < cdf[s], cdf[V-1] read as 2^32: ceil(log2 V)
// dependent loads, once per sample -- and leave in LDS for the gather.  The workgroup that holds a sample's column 0 writes its id,
// samples_out and bias (one writer per sample).
constexpr int SCE_POP_IDS = 256 / 8 + 1;
__global__ __launch_bounds__(256) void k_sce_ids_pop(ScePopArgs a) {
    __shared__ int s_ids[SCE_POP_IDS];
    const uint32_t key = a.samples ? 0u : cr_site_key(a.seed, *a.step, CR_SCE_SITE);
    const int64_t n = (int64_t)a.N * a.D;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int jf = (int)(base / a.D), jl = (int)(std::min<int64_t>(base + 255, n - 1) / a.D);
        __syncthreads();                                            // (the round before has read s_ids)
        if ((int)threadIdx.x <= jl - jf) {
            const int j = jf + threadIdx.x;
            int id;
            if (a.samples) {
                id = a.samples[j];
            } else {
                const uint32_t x = cr_fmix32(key + (uint32_t)j * CR_PHI);
                int lo = 1, hi = a.V - 1;                           // (cdf[V-1] is never read: it stands for 2^32 > x)
                while (lo < hi) {
                    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                    if (x < a.cdf[mid]) hi = mid;
                    else lo = mid + 1;
                }
                id = lo;
            }
            s_ids[threadIdx.x] = id;
            if ((int64_t)j * a.D >= base) {
                a.sid[j] = id;
                if (a.samples_out) a.samples_out[j] = id;
                a.sb[j] = -a.logq[id] * CE_LOG2E;
            }
        }
        __syncthreads();
        const int64_t e = base + threadIdx.x;
        if (e < n) {
            const int j = (int)(e / a.D), c = (int)(e % a.D);
            a.Es[e] = a.E[(int64_t)s_ids[j - jf] * a.D + c];
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

// popularity: what a thread stages for the block of samples j0 .. j0 + 31 -- threads 0 .. 31 the ids, threads 32 .. 63 the biases'
// bits (one register for both, as the ids alone take)
__device__ __forceinline__ int sce_pop_stage(const ScePopArgs& a, int j0) {
    const int j = j0 + (threadIdx.x & (CE_BLK - 1));
    if (threadIdx.x >= 2 * CE_BLK || j >= a.N) return 0;
    return threadIdx.x < CE_BLK ? a.sid[j] : __float_as_int(a.sb[j]);
}

// ---- the sweep passes (A: CeArgs, SceArgs or ScePopArgs) ------------------------------------------------------------------
template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_lse(A a) {
    constexpr bool S = A::SAMPLED, P = A::POP;
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ int s_id[P ? 2 * CE_BLK : CE_BLK];                   // (sampled; popularity: the biases' bits behind the ids)
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
    float sp = 0.0f, sn = 0.0f;
    if constexpr (S) {
        sp = sce_gathered_score<NK, SPLIT>(a, pq, qok, bh, bl);
        if (a.neg) {                                                // (uniform: the tile runs with every lane on)
            const float x = sce_gathered_score<NK, SPLIT>(a, nq, qok, bh, bl);
            sn = nq != 0 ? x : 0.0f;                                // neg 0: a zero score, as the catalogue's row 0
        }
    }
    // sampled: the target is lane group 0's first candidate (popularity: corrected as every candidate; a padded row reads logq[0] = 0)
    float tp = sp * CE_LOG2E;
    if constexpr (P) tp = __builtin_fmaf(sp, CE_LOG2E, -a.logq[pq] * CE_LOG2E);
    float mx = (S && lg == 0) ? tp : -INFINITY, s_in = (S && lg == 0) ? 1.0f : 0.0f, s_out = 0.0f;
    const float* src;                                               // the candidates: rows c0 .. end - 1 of src (catalogue: the
    int c0, end;                                                    // items 1 .. V-1 of E; sampled: the N gathered rows Es)
    if constexpr (S) { src = a.Es; c0 = 0; end = a.N; }
    else { src = a.E; c0 = 1; end = a.V; }
    const int rounds = (end - c0 + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int nid = 0;                                                    // (sampled: the ids of the next block, staged through LDS)
    blk_issue<NCB>(v, src, a.D, c0, end, end - 1, a.D);
    if constexpr (P) nid = sce_pop_stage(a, 0);
    else if constexpr (S) if (threadIdx.x < CE_BLK && (int)threadIdx.x < a.N) nid = a.sid[threadIdx.x];
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = c0 + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, src, a.D, j0, end, end - 1, a.D);
        if constexpr (P) { if (threadIdx.x < 2 * CE_BLK) s_id[threadIdx.x] = nid; }
        else if constexpr (S) if (threadIdx.x < CE_BLK) s_id[threadIdx.x] = nid;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, src, a.D, j0 + CE_BLK, end, end - 1, a.D);
            if constexpr (P) {
                nid = sce_pop_stage(a, j0 + CE_BLK);
            } else if constexpr (S) {
                const int j = j0 + CE_BLK + threadIdx.x;
                nid = (threadIdx.x < CE_BLK && j < a.N) ? a.sid[j] : 0;
            }
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
                bool ok;
                if constexpr (S) {
                    ok = j0 + jl < end && s_id[jl] != pq;           // a sample equal to the target is masked
                } else {
                    const int id = j0 + 16 * tt + 4 * lg + r;
                    ok = id < end;
                    sp = (ok && id == pq) ? c[r] : sp;
                    sn = (ok && id == nq) ? c[r] : sn;
                }
                if constexpr (P) t[tt][r] = ok ? __builtin_fmaf(c[r], CE_LOG2E, __int_as_float(s_id[CE_BLK + jl])) : -INFINITY;
                else t[tt][r] = ok ? c[r] * CE_LOG2E : -INFINITY;
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
        if constexpr (!S) {
            sp += __shfl_xor(sp, o, 64);                            // one lane of the four holds the score, the others 0
            sn += __shfl_xor(sn, o, 64);
        }
    }
    const float l2 = mx + __log2f(s);
    const bool ist = qok && pq != 0;
    float lr = 0.0f, ar = 0.0f, nr = 0.0f;
    if (qok && lg == 0) {
        a.lse2[q] = l2;
        // sampled: relative to the target's own base-2 score, so a row whose every sample is a hit gets l = 0 and p_pos - 1 = 0 exactly
        if constexpr (S) a.gpos[q] = ist ? ce_exp2(tp - l2) - 1.0f : 0.0f;
        if (a.lse_out) a.lse_out[q] = l2 * CE_LN2;
        if (ist) {
            lr = S ? (l2 - tp) * CE_LN2 : l2 * CE_LN2 - sp;
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
template <class A>
__global__ __launch_bounds__(64) void k_ce_stats(A a) {
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

template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_dh(A a) {
    constexpr bool S = A::SAMPLED, P = A::POP;
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ int s_id[P ? 2 * CE_BLK : CE_BLK];                   // (sampled; popularity: the biases' bits behind the ids)
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
    const float* src;                                               // the candidates: rows c0 .. end - 1 of src (catalogue: the
    int c0, end;                                                    // items 1 .. V-1 of E; sampled: the N gathered rows Es)
    if constexpr (S) { src = a.Es; c0 = 0; end = a.N; }
    else { src = a.E; c0 = 1; end = a.V; }
    const int rounds = (end - c0 + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int nid = 0;                                                    // (sampled: the ids of the next block, staged through LDS)
    blk_issue<NCB>(v, src, a.D, c0, end, end - 1, a.D);
    if constexpr (P) nid = sce_pop_stage(a, 0);
    else if constexpr (S) if (threadIdx.x < CE_BLK && (int)threadIdx.x < a.N) nid = a.sid[threadIdx.x];
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = c0 + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, src, a.D, j0, end, end - 1, a.D);
        if constexpr (P) { if (threadIdx.x < 2 * CE_BLK) s_id[threadIdx.x] = nid; }
        else if constexpr (S) if (threadIdx.x < CE_BLK) s_id[threadIdx.x] = nid;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, src, a.D, j0 + CE_BLK, end, end - 1, a.D);
            if constexpr (P) {
                nid = sce_pop_stage(a, j0 + CE_BLK);
            } else if constexpr (S) {
                const int j = j0 + CE_BLK + threadIdx.x;
                nid = (threadIdx.x < CE_BLK && j < a.N) ? a.sid[j] : 0;
            }
        }
        float g[2][4];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (P) {
                    const int jl = 16 * tt + 4 * lg + r;
                    g[tt][r] = (ist && j0 + jl < end && s_id[jl] != pq) ? ce_pb(c[r], __int_as_float(s_id[CE_BLK + jl]), l2) : 0.0f;
                } else if constexpr (S) {
                    const int jl = 16 * tt + 4 * lg + r;
                    g[tt][r] = (ist && j0 + jl < end && s_id[jl] != pq) ? ce_p(c[r], l2) : 0.0f;     // a hit is masked
                } else {
                    const int id = j0 + 16 * tt + 4 * lg + r;
                    g[tt][r] = (ist && id < end) ? ce_g(c[r], l2, id == pq) : 0.0f;
                }
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: row 16 wave + 4 lg + r of the tile, column 16 db + li
    if constexpr (S) {
        // plus the target term (p_pos - 1) E_pos
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
    } else {
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
}

// gBCE: loss and dh from one sweep of the candidates (the sweep of k_ce_dh<SceArgs>, the prologue and epilogue of k_ce_lse<SceArgs>)
template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_gbce_row(GbceArgs a) {
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
    const bool ist = qok && pq != 0;
    const float sp = sce_gathered_score<NK, SPLIT>(a, pq, qok, bh, bl);
    float sn = 0.0f;
    if (a.neg) {                                                    // (uniform: the tile runs with every lane on)
        const float x = sce_gathered_score<NK, SPLIT>(a, nq, qok, bh, bl);
        sn = nq != 0 ? x : 0.0f;                                    // neg 0: a zero score, as the catalogue's row 0
    }
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float ls = 0.0f;                                                // softplus of this lane's candidates, in sweep order
    const int end = a.N;
    const int rounds = (end + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    int nid = 0;                                                    // the ids of the next block, staged through LDS
    blk_issue<NCB>(v, a.Es, a.D, 0, end, end - 1, a.D);
    if (threadIdx.x < CE_BLK && (int)threadIdx.x < a.N) nid = a.sid[threadIdx.x];
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.Es, a.D, j0, end, end - 1, a.D);
        if (threadIdx.x < CE_BLK) s_id[threadIdx.x] = nid;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, a.Es, a.D, j0 + CE_BLK, end, end - 1, a.D);
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
                const bool live = ist && j0 + jl < end && s_id[jl] != pq;       // a hit is masked
                const float e = gb_e(c[r]);
                g[tt][r] = live ? gb_sigma(c[r], e) : 0.0f;
                ls += live ? gb_softplus(c[r], e) : 0.0f;
            }
        }
        if (a.dh) {
            bf8 gh, gl;
            g_frag<SPLIT>(g, gh, gl);
            g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        }
        __syncthreads();
    }
    // the row's four lane groups: a butterfly symmetric in the two partners (every lane ends with the same bits)
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    // the target: beta softplus(-z_pos), coefficient beta (sigma(z_pos) - 1) = -beta sigma(-z_pos)
    const float et = gb_e(sp);
    const float gp = ist ? -a.beta * gb_sigma(-sp, et) : 0.0f;
    const float l = ist ? __builtin_fmaf(a.beta, gb_softplus(-sp, et), ls) : 0.0f;
    float lr = 0.0f, ar = 0.0f, nr = 0.0f;
    if (qok && lg == 0) {
        a.gpos[q] = gp;
        if (a.lse_out) a.lse_out[q] = l;
        if (ist) {
            lr = l;
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
    if (!a.dh) return;
    // acc[db] register r: row 16 wave + 4 lg + r of the tile (its gpos sits in lane 4 lg + r), column 16 db + li; plus gpos E_pos
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gpr = __shfl(gp, 4 * lg + r, 64);
        const int row = blockIdx.x * 64 + wave * 16 + 4 * lg + r;
        if (row >= a.M) continue;
        const int pr = a.pos[row];
        const float* er = a.E + (int64_t)pr * a.D;
#pragma unroll
        for (int db = 0; db < 2 * NK; ++db) {
            const int col = 16 * db + li;
            if (col < a.D) a.dh[(int64_t)row * a.ldd + col] = pr != 0 ? __builtin_fmaf(gpr, er[col], acc[db][r]) : 0.0f;
        }
    }
}

template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_de(A a) {
    constexpr bool S = A::SAMPLED, G = A::GBCE, P = A::POP;         // (gBCE: no per-row statistic, so no s_l2)
    constexpr int NCB = (NK + 1) / 2;
    __shared__ __attribute__((aligned(16))) CeImg<NCB> img;
    __shared__ float s_l2[G ? 1 : CE_BLK];
    __shared__ int s_pos[CE_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const float* src;                                               // the candidates: rows c0 .. end - 1 of src (catalogue: the
    int c0, end;                                                    // items 1 .. V-1 of E; sampled: the N gathered rows Es)
    if constexpr (S) { src = a.Es; c0 = 0; end = a.N; }
    else { src = a.E; c0 = 1; end = a.V; }
    const int j = c0 + blockIdx.x * 64 + wave * 16 + li;
    const bool jok = j < end;
    int id = j;                                                     // the candidate's item id
    if constexpr (S) id = jok ? a.sid[j] : -1;
    float bj = 0.0f;                                                // (popularity: the candidate's base-2 bias)
    if constexpr (P) bj = jok ? a.sb[j] : 0.0f;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, src, a.D, j, jok, j == end - 1, a.D);
        tk_row_finish<NK, SPLIT>(v, src, a.D, j, jok, j == end - 1, a.D, bh, bl);
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
    if (threadIdx.x < CE_BLK && rb + (int)threadIdx.x < re) {
        npos = a.pos[rb + threadIdx.x];
        if constexpr (!G) nl2 = a.lse2[rb + threadIdx.x];
    }
    for (int rd = 0; rd < rounds; ++rd) {
        const int r0 = rb + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, a.h, a.ldh, r0, re, a.M - 1, a.D);
        if (threadIdx.x < CE_BLK) {
            s_pos[threadIdx.x] = npos;
            if constexpr (!G) s_l2[threadIdx.x] = nl2;
        }
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, a.h, a.ldh, r0 + CE_BLK, re, a.M - 1, a.D);
            const int r = r0 + CE_BLK + threadIdx.x;
            npos = 0;
            nl2 = 0.0f;
            if (threadIdx.x < CE_BLK && r < re) {
                npos = a.pos[r];
                if constexpr (!G) nl2 = a.lse2[r];
            }
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
                if constexpr (P) g[tt][r] = (jok && pr != 0 && pr != id) ? ce_pb(c[r], bj, s_l2[lr]) : 0.0f;
                else if constexpr (G) g[tt][r] = (jok && pr != 0 && pr != id) ? gb_sigma(c[r], gb_e(c[r])) : 0.0f;
                else if constexpr (S) g[tt][r] = (jok && pr != 0 && pr != id) ? ce_p(c[r], s_l2[lr]) : 0.0f;
                else g[tt][r] = (jok && pr != 0) ? ce_g(c[r], s_l2[lr], pr == id) : 0.0f;
            }
        }
        bf8 gh, gl;
        g_frag<SPLIT>(g, gh, gl);
        g_times_img<NK, NCB, SPLIT>(acc, gh, gl, img, a.D);
        __syncthreads();
    }
    // acc[db] register r: candidate 16 wave + 4 lg + r of the workgroup's 64, column 16 db + li
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        const int col = 16 * db + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jr = c0 + blockIdx.x * 64 + wave * 16 + 4 * lg + r;
            if (jr < end && col < a.D) {
                if (!S && a.parts == 1) a.tg[(int64_t)jr * a.D + col] += acc[db][r];
                else a.part[((int64_t)blockIdx.y * end + jr) * a.D + col] = acc[db][r];
            }
        }
    }
}

// ---- the op-specific reductions of the de pass -------------------------------------------------------------------------
// catalogue: table_grad[v, :] += sum of the parts' rows v in part order (rows 1 .. V-1)
__global__ __launch_bounds__(256) void k_ce_de_sum(CeArgs a) {
    const int64_t n = (int64_t)(a.V - 1) * a.D, stride = (int64_t)a.V * a.D;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t e = a.D + i;
        float s = a.part[e];
        for (int p = 1; p < a.parts; ++p) s += a.part[p * stride + e];
        a.tg[e] += s;
    }
}

// sampled: table_grad[s_j] += the sum over the id's samples (j order) of the parts (part order); one workgroup per first occurrence
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

// sampled: dE_{pos_m} += (p_pos - 1) h_m for the target rows (float atomics: rows repeat)
__global__ __launch_bounds__(256) void k_sce_tgt(SceArgs a) {
    const int64_t n = (int64_t)a.M * a.D;
    for (int64_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int m = (int)(e / a.D), c = (int)(e % a.D);
        const int p = a.pos[m];
        if (p != 0) atomicAdd(a.tg + (int64_t)p * a.D + c, a.gpos[m] * a.h[(int64_t)m * a.ldh + c]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct CeGeom {
    int NK, n_rt, n_ct, parts, rpp;         // n_ct: the de pass's workgroups of 64 candidates
};

// Candidates c0 .. end - 1 (cands()).  The de pass: about 512 workgroups of (64 candidates x a part of the rows) where the candidates
// are few; its partial sums are at most max_parts slices of `end` rows, parts x end <= part_rows.
bool ce_geometry(int M, int c0, int end, int D, int max_parts, int part_rows, CeGeom& g) {
    if (M < 1 || end <= c0 || D < 8 || D > 256) return false;
    g.NK = tk_nk(D);
    g.n_rt = (M + 63) / 64;
    g.n_ct = (end - c0 + 63) / 64;
    int parts = std::min(max_parts, part_rows / end);
    parts = std::max(1, std::min(parts, (M + CE_BLK - 1) / CE_BLK));
    g.rpp = ((M + parts - 1) / parts + CE_BLK - 1) / CE_BLK * CE_BLK;
    g.parts = (M + g.rpp - 1) / g.rpp;
    return true;
}

// catalogue workspace: [lse2 M | row-tile sums n_rt x 4 | de partial rows min(16 V, CE_PART_ELEMS) x D] floats (the last section is
// reserved for every shape so that the size never shrinks as V grows; it is used where parts > 1).  0: an unsupported shape.
size_t ce_workspace(int M, int V, int D, CeGeom& g) {
    if (!ce_geometry(M, 1, V, D, CE_MAX_PARTS, CE_PART_ELEMS, g)) return 0;
    const size_t part_rows = std::min<size_t>((size_t)CE_MAX_PARTS * V, CE_PART_ELEMS);
    return cr_align256(4 * (size_t)M) + cr_align256(16 * (size_t)g.n_rt) + cr_align256(4 * part_rows * D);
}

size_t sce_part_rows(int N) { return std::min<size_t>((size_t)SCE_MAX_PARTS * N, std::max<size_t>(N, SCE_PART_ROWS)); }

// sampled workspace: [sid | nxt | head: N ints each | Es N x D | lse2 M | gpos M | row-tile sums n_rt x 4 | de parts min(64 N, 65536)
// x D | the samples' biases N (popularity proposal)] (the parts section is sized by N alone, so the total never decreases as M or N
// grows).  0: an unsupported shape.
size_t sce_workspace(int M, int N, int D, CeGeom& g) {
    if (N > CR_SCE_MAX_SAMPLES || !ce_geometry(M, 0, N, D, SCE_MAX_PARTS, SCE_PART_ROWS, g)) return 0;
    return 3 * cr_align256(4 * (size_t)N) + cr_align256(4 * (size_t)N * D) + 2 * cr_align256(4 * (size_t)M) +
           cr_align256(16 * (size_t)g.n_rt) + cr_align256(4 * sce_part_rows(N) * D) + cr_align256(4 * (size_t)N);
}

// gBCE workspace: the sampled one without lse2
size_t gbce_workspace(int M, int N, int D, CeGeom& g) {
    if (N > CR_SCE_MAX_SAMPLES || !ce_geometry(M, 0, N, D, SCE_MAX_PARTS, SCE_PART_ROWS, g)) return 0;
    return 3 * cr_align256(4 * (size_t)N) + cr_align256(4 * (size_t)N * D) + cr_align256(4 * (size_t)M) +
           cr_align256(16 * (size_t)g.n_rt) + cr_align256(4 * sce_part_rows(N) * D);
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256)); }

template <class A, int NK, bool SPLIT>
void ce_launch(const A& a, const CeGeom& g, hipStream_t st) {
    constexpr bool S = A::SAMPLED;
    if constexpr (S) {
        if constexpr (A::POP) hipLaunchKernelGGL(k_sce_ids_pop, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_sce_ids<CR_SCE_SITE>, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, a);
        if (a.tg) hipLaunchKernelGGL(k_sce_dedup, dim3((a.N + 255) / 256), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL((k_ce_lse<A, NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ce_stats<A>, dim3(1), dim3(64), 0, st, a);
    if (a.dh) hipLaunchKernelGGL((k_ce_dh<A, NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    if (a.tg) {
        hipLaunchKernelGGL((k_ce_de<A, NK, SPLIT>), dim3(g.n_ct, g.parts), dim3(256), 0, st, a);
        if constexpr (S) {
            hipLaunchKernelGGL(k_sce_scatter, dim3(a.N), dim3(std::min(256, (a.D + 63) / 64 * 64)), 0, st, a);
            hipLaunchKernelGGL(k_sce_tgt, dim3(grid_for((int64_t)a.M * a.D)), dim3(256), 0, st, a);
        } else if (g.parts > 1) {
            const int64_t n = (int64_t)(a.V - 1) * a.D;
            const int grid = (int)std::min<int64_t>(2048, (n + 255) / 256);
            hipLaunchKernelGGL(k_ce_de_sum, dim3(grid), dim3(256), 0, st, a);
        }
    }
}

// gBCE: seven launches (no lse / dh pair: one row sweep)
template <int NK, bool SPLIT>
void gbce_launch(const GbceArgs& a, const CeGeom& g, hipStream_t st) {
    const SceArgs& s = a;
    hipLaunchKernelGGL(k_sce_ids<CR_GBCE_SITE>, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, s);
    if (a.tg) hipLaunchKernelGGL(k_sce_dedup, dim3((a.N + 255) / 256), dim3(256), 0, st, s);
    hipLaunchKernelGGL((k_gbce_row<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ce_stats<SceArgs>, dim3(1), dim3(64), 0, st, s);
    if (a.tg) {
        hipLaunchKernelGGL((k_ce_de<GbceArgs, NK, SPLIT>), dim3(g.n_ct, g.parts), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_sce_scatter, dim3(a.N), dim3(std::min(256, (a.D + 63) / 64 * 64)), 0, st, s);
        hipLaunchKernelGGL(k_sce_tgt, dim3(grid_for((int64_t)a.M * a.D)), dim3(256), 0, st, s);
    }
}

// the passes for the descriptor's precision (CR_PREC_F32: the bf16x3 products, fp32-grade) and tk_nk's k-steps
template <class A>
void ce_run(const A& a, const CeGeom& g, int precision, hipStream_t st) {
    tk_dispatch(g.NK, precision != CR_PREC_BF16, [&](auto nk, auto split) { ce_launch<A, nk, split>(a, g, st); });
}

}  // namespace

extern "C" size_t cr_softmax_ce_workspace(int M, int V, int D) {
    CeGeom g;
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
    const size_t need = ce_workspace(d->M, d->V, d->D, g);
    CR_REQUIRE(need, "cr_softmax_ce: unsupported shape");
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_softmax_ce: workspace of %zu bytes, cr_softmax_ce_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    CeArgs a;
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V;
    a.lse2 = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += cr_align256(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w);
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = d->lse_out; a.state = d->state; a.n_rt = g.n_rt;
    ce_run(a, g, d->precision, cr_stream(stream));
    return cr_check_launch("cr_softmax_ce");
}

extern "C" size_t cr_sampled_ce_workspace(int M, int N, int D) {
    CeGeom g;
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
    CR_REQUIRE(!d->cdf || d->logq, "cr_sampled_ce: cdf without logq (a proposal is both: the draw and its log-Q correction)");
    CR_REQUIRE(d->samples || !d->logq || d->cdf, "cr_sampled_ce: logq with NULL samples needs the cdf (the device draw searches it)");
    CeGeom g;
    const size_t need = sce_workspace(d->M, d->N, d->D, g);
    CR_REQUIRE(need, "cr_sampled_ce: unsupported shape");
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_sampled_ce: workspace of %zu bytes, cr_sampled_ce_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    SceArgs a;
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V; a.N = d->N;
    a.samples = d->samples; a.seed = d->seed; a.step = d->step; a.samples_out = d->samples_out;
    a.sid = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.nxt = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.head = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.Es = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->N * d->D);
    a.lse2 = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->M);
    a.gpos = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += cr_align256(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w); w += cr_align256(4 * sce_part_rows(d->N) * d->D);
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = d->lse_out; a.state = d->state; a.n_rt = g.n_rt;
    if (d->logq) {                                                  // popularity proposal: the corrected candidates
        ScePopArgs p;
        static_cast<SceArgs&>(p) = a;
        p.cdf = d->cdf; p.logq = d->logq;
        p.sb = reinterpret_cast<float*>(w);
        ce_run(p, g, d->precision, cr_stream(stream));
    } else {
        ce_run(a, g, d->precision, cr_stream(stream));
    }
    return cr_check_launch("cr_sampled_ce");
}

extern "C" size_t cr_gbce_workspace(int M, int N, int D) {
    CeGeom g;
    return gbce_workspace(M, N, D, g);
}

extern "C" int cr_gbce(const cr_gbce_desc* d, void* stream) {
    CR_REQUIRE(d, "cr_gbce: NULL descriptor");
    CR_REQUIRE(d->seq_emb && d->table && d->pos && d->state, "cr_gbce: NULL seq_emb, table, pos or state");
    CR_REQUIRE(d->D >= 8 && d->D <= 256, "cr_gbce: D=%d outside 8 .. 256", d->D);
    CR_REQUIRE(d->V >= 2, "cr_gbce: V=%d < 2 (row 0 is padding: no item to sample)", d->V);
    CR_REQUIRE(d->M >= 1, "cr_gbce: M=%d <= 0", d->M);
    CR_REQUIRE(d->N >= 1 && d->N <= CR_SCE_MAX_SAMPLES, "cr_gbce: N=%d outside 1 .. %d", d->N, CR_SCE_MAX_SAMPLES);
    CR_REQUIRE(d->ld >= d->D, "cr_gbce: ld=%d < D=%d", d->ld, d->D);
    CR_REQUIRE(!d->d_seq_emb || d->ldd >= d->D, "cr_gbce: ldd=%d < D=%d", d->ldd, d->D);
    CR_REQUIRE(d->precision == CR_PREC_F32 || d->precision == CR_PREC_BF16X3 || d->precision == CR_PREC_BF16,
               "cr_gbce: unknown precision %d", d->precision);
    CR_REQUIRE(d->beta > 0.0f && d->beta <= 1.0f, "cr_gbce: beta=%g outside (0, 1]", (double)d->beta);     // (NaN fails both)
    CR_REQUIRE(d->samples || d->step, "cr_gbce: NULL step with NULL samples (the device draw reads the step word)");
    CeGeom g;
    const size_t need = gbce_workspace(d->M, d->N, d->D, g);
    CR_REQUIRE(need, "cr_gbce: unsupported shape");
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_gbce: workspace of %zu bytes, cr_gbce_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    GbceArgs a;
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V; a.N = d->N; a.beta = d->beta;
    a.samples = d->samples; a.seed = d->seed; a.step = d->step; a.samples_out = d->samples_out;
    a.sid = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.nxt = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.head = reinterpret_cast<int32_t*>(w); w += cr_align256(4 * (size_t)d->N);
    a.Es = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->N * d->D);
    a.lse2 = nullptr;
    a.gpos = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += cr_align256(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w);
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = d->loss_out; a.state = d->state; a.n_rt = g.n_rt;
    tk_dispatch(g.NK, d->precision != CR_PREC_BF16, [&](auto nk, auto split) { gbce_launch<nk, split>(a, g, cr_stream(stream)); });
    return cr_check_launch("cr_gbce");
}

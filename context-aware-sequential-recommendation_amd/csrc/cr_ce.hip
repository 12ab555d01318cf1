// The candidate-sweep losses: none writes the [M, candidates] scores; each gives the loss sums and the un-normalised gradients wrt h
// and E (castrec.h).  A score is s_mv = h_m . E_v; pos_m is row m's target (0: the row is padding).
//
// The skeleton, written once:
//  * stream  (ce_stream).  A workgroup of 256 threads streams rows of an fp32 matrix through an LDS image of 32 rows (bf16 hi / lo,
//            cr_bf16.hpp img_off<2>), filled from registers loaded a block ahead, with up to two words per row beside it (ids, biases,
//            pos, lse2), staged the same way.  Each wave holds 16 rows of the other operand as B fragments and scores them against
//            the block in two tiles (tk_tile: the product sequence of cr_topk.hip, so a score has the same bits here as there); the
//            caller gives what happens to a score tile and what happens once per block while the image is still there.
//  * row kernels (a workgroup per 64 batch rows; ce_row: the wave's rows, ce_row_scores: neg and the diagonal scores, ce_tile_stats:
//            the row tile's loss / AUC / target sums, ce_store_dh).  The candidates (ce_cands) stream past the wave's batch rows.
//  * de      (k_ce_de, a workgroup per 64 candidates x a part of the rows).  Each wave keeps 16 candidates; the batch rows of the part
//            stream past with pos (and lse2) beside them.  The score tile has the roles swapped (ce_tile_t: the three products in
//            tk_tile's order), so a lane holds rows against its candidate -- the A operand of dE = G^T H (g_times_img: A = G straight
//            from the two score tiles' accumulators, k slot 8 lg + j <-> image row (j < 4 ? 0 : 16) + 4 lg + (j & 3); B = the image
//            read transposed, tr_frag with that k order).  Each part writes its slice of the workspace; a catalogue of one part +=
//            into table_grad.
//  * stats   (k_ce_stats, one wave).  The row tiles' sums in a fixed order: state[0..2] +=, then the snapshot [8..11] (castrec.h).
// The ops are kinds of candidates -- the argument struct -- and what they do per score:
//  * cr_softmax_ce, CeArgs: the items 1 .. V-1 of E with the target among them.  Loss logsumexp_v s_mv - s_{m,pos_m}.
//      lse     per lane a running base-2 max / sum (exp2 with log2 e folded into the score; 64 blocks per inner partial), the four
//              lane groups of a row merged in a fixed butterfly; the target and neg scores are picked up as the sweep passes them.
//              Out: lse2 = log2 sum exp2 per row, the row tile's sums.
//      dh      the same sweep recomputes each score, g = exp2(s log2 e - lse2) - [v = pos], dh = G x the block (g_times_img).
//      de      g as in dh; de_sum (parts > 1) adds the parts into table_grad in part order.
//  * cr_sampled_ce, SceArgs: N sample ids shared by the call, as the gathered rows Es [N, D], the target beside them: log(exp z_pos +
//    sum_{j: s_j != pos_m} exp z_{m,s_j}) - z_pos, O(M N D) independent of V.  The deltas:
//      ids     (grid-stride over N x D) copies or draws the ids (castrec.h states the draw), writes them and samples_out, gathers Es.
//      dedup   (a thread per sample; only with table_grad) whether sample j is its id's first occurrence, and the next j' > j with
//              the same id: each thread compares against all N ids through LDS chunks, a few microseconds at N = 4096.
//      lse     a sample equal to the row's target is masked; the target and neg scores come from diagonal tiles of E[pos] / E[neg]
//              against the wave's own rows (tk_tile again; cr_score_topk's ranks use the same trick); the target enters the running
//              max / sum of lane group 0 before the first block; gpos = p_pos - 1 is written per row.
//      dh      g = 0 at a hit; the store adds gpos_m E[pos_m] in fp32.
//      de      every part writes its slice; scatter (a workgroup per sample): the first occurrence of each id walks its list in j
//              order, adds the parts in part order and += the sum into table_grad[id], one writer per distinct id; tgt (grid-stride
//              over M x D): dE_{pos_m} += gpos_m h_m with float atomics.
//  * ... under a popularity proposal, ScePopArgs: every candidate score carries the log-Q correction -logq[id] (castrec.h) as a base-2
//    bias, the second word beside a sample's id.  ids_pop: the id of a sample is found once, by the workgroup that holds its first
//    element -- a copy, or the binary search of the cdf -- and handed to the gathering threads through LDS; the same thread writes
//    the bias -logq[id] log2 e.
//  * cr_gbce, GbceArgs: gSASRec's generalised binary cross-entropy over the sampled op's candidates, beta softplus(-z_pos) +
//    sum_{j: s_j != pos_m} softplus(z_{m,s_j}).  A pointwise objective has no normaliser, so one row kernel (k_gbce_row) stands for
//    lse and dh: g = sigma(score) (0 at a hit) from one exp2 per score, the softplus of the same exponential summed per lane in sweep
//    order; gpos = beta (sigma_pos - 1).  de: g = sigma, no lse2 beside pos.  ids (its own draw site), dedup, stats, scatter, tgt: the
//    sampled op's.
// Every partition is fixed by the shape; tgt is the only pass with float atomics (the one non-deterministic output).
// One MFMA shape in this file (build.py ISA_CHECKED): v_mfma_f32_16x16x32_bf16.
#include <algorithm>

#include "cr_bf16.hpp"

namespace {

constexpr float CE_LOG2E = 1.4426950408889634f;
constexpr float CE_LN2 = 0.6931471805599453f;
constexpr int CE_BLK = 32;                  // rows of the streamed LDS block (candidates in the row kernels, batch rows in de)
constexpr int CE_PART_ELEMS = 32768;        // catalogue: parts x V of the de pass's partial sums at most (the workspace reserves
constexpr int CE_MAX_PARTS = 16;            //   min(16 V, this) rows)
constexpr int SCE_PART_ROWS = 65536;        // sampled: parts x N of the de pass's partial sums at most
constexpr int SCE_MAX_PARTS = 64;
constexpr int SCE_CHUNK = 2048;             // ids per LDS chunk of the dedup pass

// what every kind has
struct CeBase {
    const float* h; int64_t ldh;
    const float* E;
    const int32_t* pos; const int32_t* neg;
    int M, D, V;
    float* lse2;                            // [M] log2 of the candidate sum (base-2 exponent of the scores); gBCE: none
    float* stats;                           // [n_rt, 4] loss / auc / target sums per row tile
    float* dh; int64_t ldd;
    float* tg;
    float* part;                            // [parts, V or N, D] (catalogue: parts > 1)
    int rpp, parts;                         // batch rows per part of the de pass
    float* lse_out;                         // [M] or NULL (gBCE: the per-row loss)
    float* state;
    int n_rt;
};

struct CeArgs : CeBase {
    static constexpr bool SAMPLED = false, GBCE = false, POP = false;
};

struct SceArgs : CeBase {
    static constexpr bool SAMPLED = true, GBCE = false, POP = false;
    static constexpr uint32_t SITE = CR_SCE_SITE;
    int N;
    const int32_t* samples;                 // caller's ids, or NULL: drawn from (seed, *step)
    uint32_t seed; const uint32_t* step;
    int32_t* sid;                           // [N] the ids used
    int32_t* samples_out;
    int32_t* nxt;                           // [N] next j' > j with the same id (N: none)
    int32_t* head;                          // [N] 1 where j is its id's first occurrence
    float* Es;                              // [N, D] gathered rows
    float* gpos;                            // [M] the target term's coefficient (p_pos - 1) for target rows, 0 elsewhere
};

// gBCE: the sampled op's candidates and buffers, g = sigma instead of the softmax's p
struct GbceArgs : SceArgs {
    static constexpr bool GBCE = true;
    static constexpr uint32_t SITE = CR_GBCE_SITE;
    float beta;                             // weight of the positive term, (0, 1]
};

// sampled softmax under a popularity proposal: z' = z - logq[id] for every candidate, the target included (castrec.h)
struct ScePopArgs : SceArgs {
    static constexpr bool POP = true;
    const uint32_t* cdf;                    // [V] the proposal's cumulative masses in units of 2^-32 (device draw), or NULL
    const float* logq;                      // [V] log Q(v); [0] = 0
    float* sb;                              // [N] the samples' base-2 biases -logq[s_j] log2 e
};

struct CeStatsArgs {
    float* stats; float* state;
    int n_rt;
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

// acc[db] += G x (the image read transposed), for the column blocks below D.  G: two score tiles' registers as the A operand of a
// k = 32 product (k slot 8 lg + j: tile j >> 2, register j & 3); the image's rows in that k order, columns 16 db .. + 15.
template <int NK, bool SPLIT>
__device__ __forceinline__ void g_times_img(f32x4 (&acc)[2 * NK], const float (&g)[2][4], const CeImg<(NK + 1) / 2>& img, int D) {
    const float x[8] = {g[0][0], g[0][1], g[0][2], g[0][3], g[1][0], g[1][1], g[1][2], g[1][3]};
    bf8 gh, gl;
    split8<SPLIT>(x, gh, gl);
    if (!SPLIT) gl = gh;
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

// ---- the stream ----------------------------------------------------------------------------------------------------------------
// Rows r0 .. end - 1 of src (`last`: the matrix's last row, blk_issue), with NSIDE words beside row j: w0[j], then the bits of w1[j].
struct CeStream {
    const float* src; int64_t ld;
    int r0, end, last;
    const int32_t* w0; const float* w1;
};

// the candidates of a kind: the items 1 .. V-1 of E; the N gathered rows Es with their ids (popularity: and biases) beside them
template <class A>
constexpr int CE_NSIDE = A::SAMPLED ? (A::POP ? 2 : 1) : 0;
template <class A>
__device__ __forceinline__ CeStream ce_cands(const A& a) {
    if constexpr (A::POP) return {a.Es, a.D, 0, a.N, a.N - 1, a.sid, a.sb};
    else if constexpr (A::SAMPLED) return {a.Es, a.D, 0, a.N, a.N - 1, a.sid, nullptr};
    else return {a.E, a.D, 1, a.V, a.V - 1, nullptr, nullptr};
}

// what a thread stages for the block of rows j0 .. j0 + 31: threads 0 .. 31 the first words, threads 32 .. 63 the second (one
// register either way)
template <int NSIDE>
__device__ __forceinline__ int ce_side_stage(const CeStream& s, int j0) {
    const int j = j0 + (threadIdx.x & (CE_BLK - 1));
    if (threadIdx.x >= NSIDE * CE_BLK || j >= s.end) return 0;
    if (NSIDE == 2 && threadIdx.x >= CE_BLK) return __float_as_int(s.w1[j]);
    return s.w0[j];
}

// The sweep every pass shares.  Per block: the image and side[32 k + i] = word k of row j0 + i, then tile(j0, tt, c) for the score
// tiles tt = 0, 1 of image rows 16 tt .. + 15 against the wave's fragments (bh, bl) -- tk_tile: register r of lane (li, lg) = image
// row 16 tt + 4 lg + r against the wave's row li; SWAP: ce_tile_t -- then block(rd) with the image still resident.
template <int NK, bool SPLIT, int NSIDE, bool SWAP, class Tile, class Block>
__device__ __forceinline__ void ce_stream(const CeStream& s, int D, CeImg<(NK + 1) / 2>& img, int* side, const bf8 (&bh)[NK],
                                          const bf8 (&bl)[NK], Tile&& tile, Block&& block) {
    constexpr int NCB = (NK + 1) / 2;
    const int rounds = (s.end - s.r0 + CE_BLK - 1) / CE_BLK;
    float v[NCB][8];
    blk_issue<NCB>(v, s.src, s.ld, s.r0, s.end, s.last, D);
    int nw = ce_side_stage<NSIDE>(s, s.r0);
    for (int rd = 0; rd < rounds; ++rd) {
        const int j0 = s.r0 + rd * CE_BLK;
        blk_store<NCB, SPLIT>(v, img, s.src, s.ld, j0, s.end, s.last, D);
        if (NSIDE > 0 && threadIdx.x < NSIDE * CE_BLK) side[threadIdx.x] = nw;
        __syncthreads();
        if (rd + 1 < rounds) {
            blk_issue<NCB>(v, s.src, s.ld, j0 + CE_BLK, s.end, s.last, D);
            nw = ce_side_stage<NSIDE>(s, j0 + CE_BLK);
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            bf8 ah[NK], al[NK];
            img_rows<NK, NCB, SPLIT>(img, 16 * tt, ah, al);
            tile(j0, tt, SWAP ? ce_tile_t<NK, SPLIT>(ah, al, bh, bl) : tk_tile<NK, SPLIT>(ah, al, bh, bl));
        }
        block(rd);
        __syncthreads();
    }
}

// ---- the row kernels' shared pieces ---------------------------------------------------------------------------------------------
// What lane (li, lg) of a wave holds of batch row q = 64 blockIdx.x + 16 wave + li, beside the row itself as a B fragment (bh, bl)
struct CeRow {
    int q, pq, nq;                          // the row, its target, its neg (0: none)
    bool qok, ist;                          // the row exists; ... and has a target
    float sp, sn;                           // the scores of pos and neg (catalogue: as the sweep passes them)
};

template <class A, int NK, bool SPLIT>
__device__ __forceinline__ void ce_row(const A& a, CeRow& w, bf8 (&bh)[NK], bf8 (&bl)[NK]) {
    w.q = blockIdx.x * 64 + (threadIdx.x >> 6) * 16 + (threadIdx.x & 15);
    w.qok = w.q < a.M;
    float v[NK][8];
    tk_row_issue<NK>(v, a.h, a.ldh, w.q, w.qok, w.q == a.M - 1, a.D);
    tk_row_finish<NK, SPLIT>(v, a.h, a.ldh, w.q, w.qok, w.q == a.M - 1, a.D, bh, bl);
    w.pq = w.qok ? a.pos[w.q] : 0;
    w.ist = w.qok && w.pq != 0;
    w.nq = 0;
    w.sp = w.sn = 0.0f;
}

// (after ce_row) neg, and for the sampled kinds the scores of E[pos] and E[neg]: diagonal tiles against the wave's own rows
template <class A, int NK, bool SPLIT>
__device__ __forceinline__ void ce_row_scores(const A& a, CeRow& w, const bf8 (&bh)[NK], const bf8 (&bl)[NK]) {
    w.nq = (w.qok && a.neg) ? a.neg[w.q] : 0;
    if constexpr (A::SAMPLED) {
        w.sp = sce_gathered_score<NK, SPLIT>(a, w.pq, w.qok, bh, bl);
        if (a.neg) {                                                // (uniform: the tile runs with every lane on)
            const float x = sce_gathered_score<NK, SPLIT>(a, w.nq, w.qok, bh, bl);
            w.sn = w.nq != 0 ? x : 0.0f;                            // neg 0: a zero score, as the catalogue's row 0
        }
    }
}

// The row tile's loss / AUC / target sums to stats: l, the loss of the lane's row, counts once per target row (lane group 0)
template <class A>
__device__ __forceinline__ void ce_tile_stats(const A& a, const CeRow& w, float l, float (&red)[3][4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lr = 0.0f, ar = 0.0f, nr = 0.0f;
    if (w.ist && lane < 16) {
        lr = l;
        const float dlt = w.sp - w.sn;                              // neg 0 (or none): row 0 reads as zeros
        ar = a.neg ? ((dlt > 0.0f) ? 1.0f : ((dlt < 0.0f) ? 0.0f : 0.5f)) : 0.0f;
        nr = 1.0f;
    }
    lr = wave_sum(lr);
    ar = wave_sum(ar);
    nr = wave_sum(nr);
    if (lane == 0) { red[0][wave] = lr; red[1][wave] = ar; red[2][wave] = nr; }
    __syncthreads();
    if (threadIdx.x < 3) a.stats[blockIdx.x * 4 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// dh from acc[db] register r: row 16 wave + 4 lg + r of the tile, column 16 db + li.  Sampled kinds: plus the target term
// gpos(r, row) E[pos] in fp32 (gpos is asked for every r with all lanes on, before the row is known to exist).
template <class A, int NK, class Gpos>
__device__ __forceinline__ void ce_store_dh(const A& a, const f32x4 (&acc)[2 * NK], Gpos&& gpos) {
    const int wave = threadIdx.x >> 6, li = threadIdx.x & 15, lg = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = blockIdx.x * 64 + wave * 16 + 4 * lg + r;
        const float gp = gpos(r, row);
        if (row >= a.M) continue;
        const int pr = A::SAMPLED ? a.pos[row] : 0;
        const float* er = a.E + (int64_t)pr * a.D;
#pragma unroll
        for (int db = 0; db < 2 * NK; ++db) {
            const int col = 16 * db + li;
            if (col >= a.D) continue;
            if constexpr (A::SAMPLED) a.dh[(int64_t)row * a.ldd + col] = pr != 0 ? __builtin_fmaf(gp, er[col], acc[db][r]) : 0.0f;
            else a.dh[(int64_t)row * a.ldd + col] = acc[db][r];
        }
    }
}

// ---- the passes (A: CeArgs, SceArgs, ScePopArgs or GbceArgs) -------------------------------------------------------------------
template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_lse(A a) {
    constexpr bool S = A::SAMPLED, P = A::POP;
    constexpr int NSIDE = CE_NSIDE<A>;
    __shared__ __attribute__((aligned(16))) CeImg<(NK + 1) / 2> img;
    __shared__ int s_id[NSIDE ? NSIDE * CE_BLK : 1];                // (sampled: the block's ids; popularity: the biases' bits behind)
    __shared__ float red[3][4];
    const int lg = (threadIdx.x & 63) >> 4;
    CeRow w;
    bf8 bh[NK], bl[NK];
    ce_row<A, NK, SPLIT>(a, w, bh, bl);
    ce_row_scores<A, NK, SPLIT>(a, w, bh, bl);
    // sampled: the target is lane group 0's first candidate (popularity: corrected as every candidate; a padded row reads logq[0] = 0)
    float tp = w.sp * CE_LOG2E;
    if constexpr (P) tp = __builtin_fmaf(w.sp, CE_LOG2E, -a.logq[w.pq] * CE_LOG2E);
    float mx = (S && lg == 0) ? tp : -INFINITY, s_in = (S && lg == 0) ? 1.0f : 0.0f, s_out = 0.0f;
    const CeStream cd = ce_cands(a);
    float t[2][4];
    float bm = -INFINITY;
    ce_stream<NK, SPLIT, NSIDE, false>(
        cd, a.D, img, s_id, bh, bl,
        [&](int j0, int tt, const f32x4& c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * tt + 4 * lg + r;
                bool ok;
                if constexpr (S) {
                    ok = (j0 + jl < cd.end) & (s_id[jl] != w.pq);   // a sample equal to the target is masked (&, here and in
                                                                    //   dh and gBCE: no branch round the LDS read of the id)
                } else {
                    const int id = j0 + jl;
                    ok = id < cd.end;
                    w.sp = (ok && id == w.pq) ? c[r] : w.sp;
                    w.sn = (ok && id == w.nq) ? c[r] : w.sn;
                }
                if constexpr (P) t[tt][r] = ok ? __builtin_fmaf(c[r], CE_LOG2E, __int_as_float(s_id[CE_BLK + jl])) : -INFINITY;
                else t[tt][r] = ok ? c[r] * CE_LOG2E : -INFINITY;
                bm = fmaxf(bm, t[tt][r]);
            }
        },
        [&](int rd) {
            if (bm > mx) {                                          // (mx = -inf: the sums are 0 and stay 0)
                const float f = ce_exp2(mx - bm);
                s_in *= f;
                s_out *= f;
                mx = bm;
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s_in += t[tt][r] > -INFINITY ? ce_exp2(t[tt][r] - mx) : 0.0f;
            if ((rd & 63) == 63) {                                  // two-level sum: 64 rounds per inner partial
                s_out += s_in;
                s_in = 0.0f;
            }
            bm = -INFINITY;
        });
    float s = s_out + s_in;
    // the row's four lane groups: a fixed butterfly, symmetric in the two partners (every lane ends with the same bits)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(s, o, 64);
        const float m2 = fmaxf(mx, mo);
        s = (mx > -INFINITY ? s * ce_exp2(mx - m2) : 0.0f) + (mo > -INFINITY ? so * ce_exp2(mo - m2) : 0.0f);
        mx = m2;
        if constexpr (!S) {
            w.sp += __shfl_xor(w.sp, o, 64);                        // one lane of the four holds the score, the others 0
            w.sn += __shfl_xor(w.sn, o, 64);
        }
    }
    const float l2 = mx + __log2f(s);
    if (w.qok && lg == 0) {
        a.lse2[w.q] = l2;
        // sampled: relative to the target's own base-2 score, so a row whose every sample is a hit gets l = 0 and p_pos - 1 = 0 exactly
        if constexpr (S) a.gpos[w.q] = w.ist ? ce_exp2(tp - l2) - 1.0f : 0.0f;
        if (a.lse_out) a.lse_out[w.q] = l2 * CE_LN2;
    }
    ce_tile_stats(a, w, S ? (l2 - tp) * CE_LN2 : l2 * CE_LN2 - w.sp, red);
}

// state[0..2] += the row tiles' sums (fixed order), then the snapshot [8..11] the head kernels take (castrec.h, state block).  One
// workgroup adds and snapshots, so it is the last piece of work by construction; the ticket [12] is left re-armed (0).
__global__ __launch_bounds__(64) void k_ce_stats(CeStatsArgs a) {
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

// (NK = 1: held to five waves per SIMD -- the branch-free g below would otherwise cost the sampled kinds' bf16x3 kernels their fifth)
template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256, NK == 1 ? 5 : 1) void k_ce_dh(A a) {
    constexpr bool S = A::SAMPLED, P = A::POP;
    constexpr int NSIDE = CE_NSIDE<A>;
    __shared__ __attribute__((aligned(16))) CeImg<(NK + 1) / 2> img;
    __shared__ int s_id[NSIDE ? NSIDE * CE_BLK : 1];                // (sampled: the block's ids; popularity: the biases' bits behind)
    const int lg = (threadIdx.x & 63) >> 4;
    CeRow w;
    bf8 bh[NK], bl[NK];
    ce_row<A, NK, SPLIT>(a, w, bh, bl);
    const float l2 = w.qok ? a.lse2[w.q] : 0.0f;
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const CeStream cd = ce_cands(a);
    float g[2][4];
    ce_stream<NK, SPLIT, NSIDE, false>(
        cd, a.D, img, s_id, bh, bl,
        [&](int j0, int tt, const f32x4& c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * tt + 4 * lg + r, id = j0 + jl;  // (catalogue: the item's id)
                bool live = w.ist && id < cd.end;
                if constexpr (S) live = live & (s_id[jl] != w.pq);  // a hit is masked
                float p;                                            // (computed for every score: selects, no branches)
                if constexpr (P) p = ce_pb(c[r], __int_as_float(s_id[CE_BLK + jl]), l2);
                else if constexpr (S) p = ce_p(c[r], l2);
                else p = ce_g(c[r], l2, id == w.pq);
                g[tt][r] = live ? p : 0.0f;
            }
        },
        [&](int) { g_times_img<NK, SPLIT>(acc, g, img, a.D); });
    ce_store_dh<A, NK>(a, acc, [&](int, int row) {
        if constexpr (S) return row < a.M ? a.gpos[row] : 0.0f;
        else return 0.0f;
    });
}

// gBCE: loss and dh from one sweep of the candidates
template <int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_gbce_row(GbceArgs a) {
    __shared__ __attribute__((aligned(16))) CeImg<(NK + 1) / 2> img;
    __shared__ int s_id[CE_BLK];
    __shared__ float red[3][4];
    const int lg = (threadIdx.x & 63) >> 4;
    CeRow w;
    bf8 bh[NK], bl[NK];
    ce_row<GbceArgs, NK, SPLIT>(a, w, bh, bl);
    ce_row_scores<GbceArgs, NK, SPLIT>(a, w, bh, bl);
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float ls = 0.0f;                                                // softplus of this lane's candidates, in sweep order
    const CeStream cd = ce_cands(a);
    float g[2][4];
    ce_stream<NK, SPLIT, 1, false>(
        cd, a.D, img, s_id, bh, bl,
        [&](int j0, int tt, const f32x4& c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * tt + 4 * lg + r;
                const bool live = (w.ist && j0 + jl < cd.end) & (s_id[jl] != w.pq);        // a hit is masked
                const float e = gb_e(c[r]);
                g[tt][r] = live ? gb_sigma(c[r], e) : 0.0f;
                ls += live ? gb_softplus(c[r], e) : 0.0f;
            }
        },
        [&](int) { if (a.dh) g_times_img<NK, SPLIT>(acc, g, img, a.D); });
    // the row's four lane groups: a butterfly symmetric in the two partners (every lane ends with the same bits)
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    // the target: beta softplus(-z_pos), coefficient beta (sigma(z_pos) - 1) = -beta sigma(-z_pos)
    const float et = gb_e(w.sp);
    const float gp = w.ist ? -a.beta * gb_sigma(-w.sp, et) : 0.0f;
    const float l = w.ist ? __builtin_fmaf(a.beta, gb_softplus(-w.sp, et), ls) : 0.0f;
    if (w.qok && lg == 0) {
        a.gpos[w.q] = gp;
        if (a.lse_out) a.lse_out[w.q] = l;
    }
    ce_tile_stats(a, w, l, red);
    if (!a.dh) return;
    ce_store_dh<GbceArgs, NK>(a, acc, [&](int r, int) { return __shfl(gp, 4 * lg + r, 64); });     // (row 4 lg + r's gpos: lane 4 lg + r)
}

template <class A, int NK, bool SPLIT>
__global__ __launch_bounds__(256) void k_ce_de(A a) {
    constexpr bool S = A::SAMPLED, G = A::GBCE, P = A::POP;
    constexpr int NSIDE = G ? 1 : 2;                                // (gBCE: no per-row statistic, so no lse2 beside pos)
    __shared__ __attribute__((aligned(16))) CeImg<(NK + 1) / 2> img;
    __shared__ int s_row[NSIDE * CE_BLK];                           // the block's pos; the bits of its lse2 behind
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const CeStream cd = ce_cands(a);
    const int j = cd.r0 + blockIdx.x * 64 + wave * 16 + li;
    const bool jok = j < cd.end;
    int id = j;                                                     // the candidate's item id
    if constexpr (S) id = jok ? a.sid[j] : -1;
    float bj = 0.0f;                                                // (popularity: the candidate's base-2 bias)
    if constexpr (P) bj = jok ? a.sb[j] : 0.0f;
    bf8 bh[NK], bl[NK];
    {
        float v[NK][8];
        tk_row_issue<NK>(v, cd.src, a.D, j, jok, j == cd.last, a.D);
        tk_row_finish<NK, SPLIT>(v, cd.src, a.D, j, jok, j == cd.last, a.D, bh, bl);
    }
    const int rb = blockIdx.y * a.rpp, re = min(a.M, rb + a.rpp);
    f32x4 acc[2 * NK];
#pragma unroll
    for (int i = 0; i < 2 * NK; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float g[2][4];
    ce_stream<NK, SPLIT, NSIDE, true>(
        CeStream{a.h, a.ldh, rb, re, a.M - 1, a.pos, a.lse2}, a.D, img, s_row, bh, bl,
        [&](int, int tt, const f32x4& c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 16 * tt + 4 * lg + r;
                const int pr = s_row[lr];
                if constexpr (P) g[tt][r] = (jok && pr != 0 && pr != id) ? ce_pb(c[r], bj, __int_as_float(s_row[CE_BLK + lr])) : 0.0f;
                else if constexpr (G) g[tt][r] = (jok && pr != 0 && pr != id) ? gb_sigma(c[r], gb_e(c[r])) : 0.0f;
                else if constexpr (S) g[tt][r] = (jok && pr != 0 && pr != id) ? ce_p(c[r], __int_as_float(s_row[CE_BLK + lr])) : 0.0f;
                else g[tt][r] = (jok && pr != 0) ? ce_g(c[r], __int_as_float(s_row[CE_BLK + lr]), pr == id) : 0.0f;
            }
        },
        [&](int) { g_times_img<NK, SPLIT>(acc, g, img, a.D); });
    // acc[db] register r: candidate 16 wave + 4 lg + r of the workgroup's 64, column 16 db + li
#pragma unroll
    for (int db = 0; db < 2 * NK; ++db) {
        const int col = 16 * db + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jr = cd.r0 + blockIdx.x * 64 + wave * 16 + 4 * lg + r;
            if (jr < cd.end && col < a.D) {
                if (!S && a.parts == 1) a.tg[(int64_t)jr * a.D + col] += acc[db][r];
                else a.part[((int64_t)blockIdx.y * cd.end + jr) * a.D + col] = acc[db][r];
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

// Candidates c0 .. end - 1 (ce_cands).  The de pass: about 512 workgroups of (64 candidates x a part of the rows) where the
// candidates are few; its partial sums are at most max_parts slices of `end` rows, parts x end <= part_rows.
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

// sampled workspace: [sid | nxt | head: N ints each | Es N x D | lse2 M (softmax) | gpos M | row-tile sums n_rt x 4 | de parts
// min(64 N, 65536) x D | the samples' biases N (softmax: the popularity proposal's)] (the parts section is sized by N alone, so the
// total never decreases as M or N grows).  softmax: cr_sampled_ce; gBCE has neither lse2 nor biases.  0: an unsupported shape.
size_t sce_workspace(int M, int N, int D, bool softmax, CeGeom& g) {
    if (N > CR_SCE_MAX_SAMPLES || !ce_geometry(M, 0, N, D, SCE_MAX_PARTS, SCE_PART_ROWS, g)) return 0;
    return 3 * cr_align256(4 * (size_t)N) + cr_align256(4 * (size_t)N * D) + (softmax ? 2 : 1) * cr_align256(4 * (size_t)M) +
           cr_align256(16 * (size_t)g.n_rt) + cr_align256(4 * sce_part_rows(N) * D) + (softmax ? cr_align256(4 * (size_t)N) : 0);
}

// What the three entry points check alike, in two steps: the descriptor's fields before an op's own checks, the workspace after them
// (the order of the checks is the order every op has had).  `items`: what the op does with the table's rows; n: the sampled kinds' N.
template <class Desc>
int ce_check_desc(const char* op, const char* items, const Desc* d, const int* n = nullptr) {
    CR_REQUIRE(d, "%s: NULL descriptor", op);
    CR_REQUIRE(d->seq_emb && d->table && d->pos && d->state, "%s: NULL seq_emb, table, pos or state", op);
    CR_REQUIRE(d->D >= 8 && d->D <= 256, "%s: D=%d outside 8 .. 256", op, d->D);
    CR_REQUIRE(d->V >= 2, "%s: V=%d < 2 (row 0 is padding: no item to %s)", op, d->V, items);
    CR_REQUIRE(d->M >= 1, "%s: M=%d <= 0", op, d->M);
    CR_REQUIRE(!n || (*n >= 1 && *n <= CR_SCE_MAX_SAMPLES), "%s: N=%d outside 1 .. %d", op, n ? *n : 0, CR_SCE_MAX_SAMPLES);
    CR_REQUIRE(d->ld >= d->D, "%s: ld=%d < D=%d", op, d->ld, d->D);
    CR_REQUIRE(!d->d_seq_emb || d->ldd >= d->D, "%s: ldd=%d < D=%d", op, d->ldd, d->D);
    CR_REQUIRE(d->precision == CR_PREC_F32 || d->precision == CR_PREC_BF16X3 || d->precision == CR_PREC_BF16,
               "%s: unknown precision %d", op, d->precision);
    return CR_OK;
}
template <class Desc>
int ce_check_workspace(const char* op, const Desc* d, size_t need) {
    CR_REQUIRE(need, "%s: unsupported shape", op);
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "%s: workspace of %zu bytes, %s_workspace says %zu", op,
               d->workspace ? d->workspace_bytes : (size_t)0, op, need);
    return CR_OK;
}

// the fields every kind has, from a descriptor; out: the optional per-row output
template <class Desc>
void ce_fill(CeBase& a, const Desc* d, float* out, const CeGeom& g) {
    a.h = d->seq_emb; a.ldh = d->ld; a.E = d->table; a.pos = d->pos; a.neg = d->neg;
    a.M = d->M; a.D = d->D; a.V = d->V;
    a.dh = d->d_seq_emb; a.ldd = d->ldd; a.tg = d->table_grad;
    a.rpp = g.rpp; a.parts = g.parts;
    a.lse_out = out; a.state = d->state; a.n_rt = g.n_rt;
}

// ... and the sampled kinds' own, carved from the workspace in sce_workspace's order.  Returns the biases' place.
template <class Desc>
float* sce_fill(SceArgs& a, const Desc* d, float* out, bool softmax, const CeGeom& g) {
    ce_fill(a, d, out, g);
    a.N = d->N;
    a.samples = d->samples; a.seed = d->seed; a.step = d->step; a.samples_out = d->samples_out;
    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    auto take = [&](size_t bytes) { void* p = w; w += cr_align256(bytes); return p; };
    a.sid = static_cast<int32_t*>(take(4 * (size_t)d->N));
    a.nxt = static_cast<int32_t*>(take(4 * (size_t)d->N));
    a.head = static_cast<int32_t*>(take(4 * (size_t)d->N));
    a.Es = static_cast<float*>(take(4 * (size_t)d->N * d->D));
    a.lse2 = softmax ? static_cast<float*>(take(4 * (size_t)d->M)) : nullptr;
    a.gpos = static_cast<float*>(take(4 * (size_t)d->M));
    a.stats = static_cast<float*>(take(16 * (size_t)g.n_rt));
    a.part = static_cast<float*>(take(4 * sce_part_rows(d->N) * d->D));
    return reinterpret_cast<float*>(w);
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256)); }

// The launches of one op.  Sampled: eight (ids, dedup, lse, stats, dh, de, scatter, tgt); gBCE: seven (one row kernel for lse and dh).
template <class A, int NK, bool SPLIT>
void ce_launch(const A& a, const CeGeom& g, hipStream_t st) {
    constexpr bool S = A::SAMPLED;
    if constexpr (S) {
        if constexpr (A::POP) hipLaunchKernelGGL(k_sce_ids_pop, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_sce_ids<A::SITE>, dim3(grid_for((int64_t)a.N * a.D)), dim3(256), 0, st, a);
        if (a.tg) hipLaunchKernelGGL(k_sce_dedup, dim3((a.N + 255) / 256), dim3(256), 0, st, a);
    }
    if constexpr (A::GBCE) hipLaunchKernelGGL((k_gbce_row<NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_ce_lse<A, NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ce_stats, dim3(1), dim3(64), 0, st, CeStatsArgs{a.stats, a.state, a.n_rt});
    if constexpr (!A::GBCE) if (a.dh) hipLaunchKernelGGL((k_ce_dh<A, NK, SPLIT>), dim3(g.n_rt), dim3(256), 0, st, a);
    if (a.tg) {
        hipLaunchKernelGGL((k_ce_de<A, NK, SPLIT>), dim3(g.n_ct, g.parts), dim3(256), 0, st, a);
        if constexpr (S) {
            hipLaunchKernelGGL(k_sce_scatter, dim3(a.N), dim3(std::min(256, (a.D + 63) / 64 * 64)), 0, st, a);
            hipLaunchKernelGGL(k_sce_tgt, dim3(grid_for((int64_t)a.M * a.D)), dim3(256), 0, st, a);
        } else if (g.parts > 1) {
            hipLaunchKernelGGL(k_ce_de_sum, dim3(grid_for((int64_t)(a.V - 1) * a.D)), dim3(256), 0, st, a);
        }
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
    if (const int rc = ce_check_desc("cr_softmax_ce", "score", d)) return rc;
    CeGeom g;
    if (const int rc = ce_check_workspace("cr_softmax_ce", d, ce_workspace(d->M, d->V, d->D, g))) return rc;

    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    CeArgs a;
    ce_fill(a, d, d->lse_out, g);
    a.lse2 = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->M);
    a.stats = reinterpret_cast<float*>(w); w += cr_align256(16 * (size_t)g.n_rt);
    a.part = reinterpret_cast<float*>(w);
    ce_run(a, g, d->precision, cr_stream(stream));
    return cr_check_launch("cr_softmax_ce");
}

extern "C" size_t cr_sampled_ce_workspace(int M, int N, int D) {
    CeGeom g;
    return sce_workspace(M, N, D, true, g);
}

extern "C" int cr_sampled_ce(const cr_sampled_ce_desc* d, void* stream) {
    if (const int rc = ce_check_desc("cr_sampled_ce", "sample", d, d ? &d->N : nullptr)) return rc;
    CR_REQUIRE(d->samples || d->step, "cr_sampled_ce: NULL step with NULL samples (the device draw reads the step word)");
    CR_REQUIRE(!d->cdf || d->logq, "cr_sampled_ce: cdf without logq (a proposal is both: the draw and its log-Q correction)");
    CR_REQUIRE(d->samples || !d->logq || d->cdf, "cr_sampled_ce: logq with NULL samples needs the cdf (the device draw searches it)");
    CeGeom g;
    if (const int rc = ce_check_workspace("cr_sampled_ce", d, sce_workspace(d->M, d->N, d->D, true, g))) return rc;

    ScePopArgs p;                                                   // (uniform: launched as its SceArgs base, which carries none of sb, cdf, logq)
    p.sb = sce_fill(p, d, d->lse_out, true, g);
    p.cdf = d->cdf; p.logq = d->logq;
    if (d->logq) ce_run(p, g, d->precision, cr_stream(stream));     // popularity proposal: the corrected candidates
    else ce_run(static_cast<const SceArgs&>(p), g, d->precision, cr_stream(stream));
    return cr_check_launch("cr_sampled_ce");
}

extern "C" size_t cr_gbce_workspace(int M, int N, int D) {
    CeGeom g;
    return sce_workspace(M, N, D, false, g);
}

extern "C" int cr_gbce(const cr_gbce_desc* d, void* stream) {
    if (const int rc = ce_check_desc("cr_gbce", "sample", d, d ? &d->N : nullptr)) return rc;
    CR_REQUIRE(d->beta > 0.0f && d->beta <= 1.0f, "cr_gbce: beta=%g outside (0, 1]", (double)d->beta);     // (NaN fails both)
    CR_REQUIRE(d->samples || d->step, "cr_gbce: NULL step with NULL samples (the device draw reads the step word)");
    CeGeom g;
    if (const int rc = ce_check_workspace("cr_gbce", d, sce_workspace(d->M, d->N, d->D, false, g))) return rc;

    GbceArgs a;
    sce_fill(a, d, d->loss_out, false, g);
    a.beta = d->beta;
    ce_run(a, g, d->precision, cr_stream(stream));
    return cr_check_launch("cr_gbce");
}

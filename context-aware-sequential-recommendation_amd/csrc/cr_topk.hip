// Full-catalogue top-K (castrec.h cr_score_topk): s[b, i] = q_b . item_i for every item of the table, a per-query top-K and the
// rank of one target per query, without ever writing the [B, V] score matrix.  Two launches:
//
//  * sweep  (grid: query tile x item chunk, 256 threads).  The workgroup splits its QT = 16 QB queries into bf16 hi / lo once and
//    keeps them in LDS as ready-made B fragments (one 16-byte read per lane, product and k-step).  Each wave streams 16 item rows
//    of its chunk per round straight from global memory into A fragments (cr_bf16.hpp items: any D >= 8, zero fill past D),
//    prefetching the next round's rows, and runs v_mfma_f32_16x16x32_bf16 products against every query block: three per k-step
//    (CR_PREC_BF16X3) or one (CR_PREC_BF16).  A score that reaches its query's running threshold (the K-th best of the chunk so far)
//    goes to the query's candidate buffer in LDS; after a round, a wave per query folds a buffer that might not hold another
//    round into the query's sorted top-K (exclusion check, then a merge by ranks), and the threshold rises.  Beside that every
//    score is compared with the query's target score (integer counts in registers).  The chunk's sorted top-K and count go to the
//    workspace.
//  * merge  (a wave per query).  K steps of a tournament over the chunks' sorted lists; the rank: the chunks' counts summed, minus
//    the distinct excluded items that beat the target (their scores from the same product path).
//
// Determinism: a chunk's top-K is the exact top-K of its eligible items under the total order (score desc, id asc), whatever the
// order in which candidates reached the buffer; the chunk partition is fixed by the shape; counts are integers.
// One MFMA shape in this file (build.py ISA_CHECKED): v_mfma_f32_16x16x32_bf16.
//
// Row source (TkSrc, tk_source): where an item row's A fragments come from.  Either the fp32 table -- rows loaded, masked past D and
// split by cr_bf16.hpp's tk_row_issue / tk_row_finish -- or (IDX) an item index (castrec.h cr_topk_index_build, cr_topk_desc.index):
// those same fragments made once and stored in fragment order, a wave's 64 lanes of one (tile of 16 rows, k-step) 1 KB contiguous, the
// lo halves a second plane.  One row per lane -- targets, excluded rows, the rows an index is written from -- comes from tk_src_row;
// the sweep's tile, one round ahead, is spelled out in its round loop (issue / finish of table rows, or tk_idx_tile): that keeps the
// loop's instruction sequence what it was measured with; as a pair of functions it is scheduled differently, not measurably slower
// (DESIGN.md section 10).  Everything after the A operand is the same code, so a score has the same bits from either source.  A
// row's fragments depend on that row alone: k_topk_index_write makes the index of a table from rows 16 tile + li and a gathered
// sub-index (castrec.h cr_topk_index_gather) from rows ids[]; a search of it is the two launches above on fewer rows.
#include <algorithm>

#include "cr_bf16.hpp"

namespace {

constexpr int TK_CAP = 128;                 // candidate buffer per query; a round appends at most 64 (4 waves x 16 items)
constexpr int TK_PAD = 0x7fffffff;          // id of an empty list entry (score -inf): worse than every item
constexpr int TK_MAX_CHUNKS = 256;

// The row source: the fp32 table [V, D], or (IDX kernels) its index in 16-byte groups, the lo plane `plane` groups after the hi plane
// (unread by a plain search).  Made by tk_source alone, which leaves no member unset for either kind of kernel.
struct TkSrc {
    const float* table;
    const bf8* idx;
    int64_t plane;
    int n_tiles;
    int V, D;
};

struct TkArgs {
    const float* q; int64_t ldq;
    TkSrc src;
    int B, K;
    const int64_t* off;                     // device copy of the CSR offsets, or null
    const int32_t* excl;
    const int32_t* tgt;
    float* part_s; int32_t* part_id;        // [n_chunks, B, K]
    int32_t* part_cnt;                      // [n_chunks, B]
    float* st_ws;                           // [B] target scores (written by chunk 0's workgroups)
    int32_t* top_ids; float* top_scores; int32_t* rank;
    int chunk, n_chunks;
};

// a better than b: higher score, equal scores -> smaller id (empty entries carry TK_PAD, the largest id)
__device__ __forceinline__ bool tk_better(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

// (tk_row_issue / tk_row_finish / tk_tile: cr_bf16.hpp, shared with cr_ce.hip)

// A fragments of the 16 rows of tile `tile` from the index: group ((h n_tiles + tile) NK + ks) 64 + lane.  A tile past the table (the
// idle waves of a chunk's last round) reads tile 0: its ids are not eligible, its scores are dropped.
template <int NK, bool SPLIT>
__device__ __forceinline__ void tk_idx_tile(const TkSrc& s, int tile, bf8 (&hi)[NK], bf8 (&lo)[NK]) {
    const bf8* p = s.idx + (int64_t)(tile < s.n_tiles ? tile : 0) * (NK * 64) + (threadIdx.x & 63);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        hi[ks] = p[ks * 64];
        if (SPLIT) lo[ks] = p[s.plane + ks * 64];
    }
}
// ... and the wave's store of tile `tile` of an index whose lo plane lies `plane` groups after the hi plane
template <int NK, bool SPLIT>
__device__ __forceinline__ void tk_idx_store(bf8* idx, int64_t plane, int tile, const bf8 (&hi)[NK], const bf8 (&lo)[NK]) {
    bf8* p = idx + (int64_t)tile * (NK * 64) + (threadIdx.x & 63);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        p[ks * 64] = hi[ks];
        if (SPLIT) p[plane + ks * 64] = lo[ks];
    }
}

// The cosine form of tk_row_finish (castrec.h CR_INDEX_COSINE; the index writers alone): the masked row is scaled by the reciprocal of
// its norm before the split, so the index holds the fragments of x / ||x||.  The arithmetic is fixed -- tests/topk_cosine_ref.py
// restates it in numpy and the blob is compared byte for byte -- and nothing of it may be contracted into an fma (hipcc's default):
//   lane (li, lg):  p = 0; for ks ascending, j = 0 .. 7 ascending: p = p + v * v     (a rounded product, then a rounded sum)
//   the row's four lanes:  p += p of lane ^ 16, then p += p of lane ^ 32: ss = (p_lg + p_lg^1) + (p_lg^2 + p_lg^3), the same bits in all four
//   inv = ss > 0 ? 1 / sqrt(ss) : 0   (correctly rounded square root, then correctly rounded division);  y = v * inv
// A zero row -- row 0, a lane without a row, an ss that underflows to 0 -- stays zero.  The two exchanges need all 64 lanes of the wave
// active: the callers' exits ahead of this are wave-uniform, and the one divergent branch here (the last row's refill) has ended.
template <int NK>
__device__ __forceinline__ float tk_inv_norm(const float (&v)[NK][8]) {
#pragma clang fp contract(off)
    float p = 0.0f;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sq = v[ks][j] * v[ks][j];
            p = p + sq;
        }
    }
    p = p + __shfl_xor(p, 16, 64);
    p = p + __shfl_xor(p, 32, 64);
    return p > 0.0f ? 1.0f / sqrtf(p) : 0.0f;
}
template <int NK, bool SPLIT>
__device__ __forceinline__ void tk_row_finish_cos(float (&v)[NK][8], const float* src, int64_t ld, int row, bool rok, bool last, int D,
                                                  bf8 (&hi)[NK], bf8 (&lo)[NK]) {
#pragma clang fp contract(off)
    const int lg = (threadIdx.x & 63) >> 4;
    const float* p = src + (rok ? (int64_t)row * ld : 0);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        const int c = 32 * ks + 8 * lg;
        const bool fix = item_fix(rok, last, c, D);
        item_mask(v[ks], c, D, rok, fix);
        if (fix) item_refill(v[ks], p, c, D);          // the partial chunk of the matrix's last row (one lane group of the grid)
    }
    const float inv = tk_inv_norm<NK>(v);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[ks][j] = v[ks][j] * inv;      // rounded here: split8's x - hi never sees an unrounded product
        split8<SPLIT>(v[ks], hi[ks], lo[ks]);
    }
}

// The fragments of one row per lane (li): from the table as tk_row_issue / tk_row_finish give them (COS: tk_row_finish_cos, the
// writers of a cosine index), from the index by 16-byte gathers of the same groups; a lane without a row (!rok) gets zeros.
template <int NK, bool SPLIT, bool IDX, bool COS = false>
__device__ __forceinline__ void tk_src_row(const TkSrc& s, int row, bool rok, bf8 (&hi)[NK], bf8 (&lo)[NK]) {
    if constexpr (IDX) {
        const int lg = (threadIdx.x & 63) >> 4, r = rok ? row : 0;
        const bf8* p = s.idx + (int64_t)(r >> 4) * (NK * 64) + (lg * 16 + (r & 15));
        const bf8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            const bf8 h = p[ks * 64];
            hi[ks] = rok ? h : z;
            if (SPLIT) {
                const bf8 l = p[s.plane + ks * 64];
                lo[ks] = rok ? l : z;
            }
        }
    } else {
        float v[NK][8];
        tk_row_issue<NK>(v, s.table, s.D, row, rok, row == s.V - 1, s.D);
        if constexpr (COS) tk_row_finish_cos<NK, SPLIT>(v, s.table, s.D, row, rok, row == s.V - 1, s.D, hi, lo);
        else tk_row_finish<NK, SPLIT>(v, s.table, s.D, row, rok, row == s.V - 1, s.D, hi, lo);
    }
}

__device__ __forceinline__ float tk_pick(const f32x4& c, int r) { return r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3]; }

// LDS ordering between the lanes of ONE wave (the fold below runs a wave per query, other waves on other queries)
__device__ __forceinline__ void tk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool tk_excluded(const int32_t* excl, int64_t e0, int64_t e1, int id) {
    bool ex = false;
    for (int64_t j = e0; j < e1; ++j) ex |= excl[j] == id;           // uniform addresses: one scalar load serves the wave
    return ex;
}

struct TkLds {
    bf8* img_hi; bf8* img_lo;
    float* top_s; int* top_id;              // [QT, K] sorted best first
    float* buf_s; int* buf_id;              // [QT, TK_CAP]
    int* cnt; float* thr; float* st; int* tq;
    float* scr_s; int* scr_id;              // [4 waves, K]
};
__host__ __device__ inline size_t tk_lds_bytes(int QT, int NK, int K) {
    return (size_t)QT * NK * 64 * 16 * 2 / 16 + (size_t)QT * K * 8 + (size_t)QT * TK_CAP * 8 + (size_t)QT * 16 + (size_t)4 * K * 8;
}
__device__ inline TkLds tk_lds(unsigned char* base, int QT, int NK, int K) {
    TkLds l;
    l.img_hi = reinterpret_cast<bf8*>(base);
    l.img_lo = l.img_hi + (QT / 16) * NK * 64;
    l.top_s = reinterpret_cast<float*>(l.img_lo + (QT / 16) * NK * 64);
    l.top_id = reinterpret_cast<int*>(l.top_s + QT * K);
    l.buf_s = reinterpret_cast<float*>(l.top_id + QT * K);
    l.buf_id = reinterpret_cast<int*>(l.buf_s + QT * TK_CAP);
    l.cnt = l.buf_id + QT * TK_CAP;
    l.thr = reinterpret_cast<float*>(l.cnt + QT);
    l.st = l.thr + QT;
    l.tq = reinterpret_cast<int*>(l.st + QT);
    l.scr_s = reinterpret_cast<float*>(l.tq + QT);
    l.scr_id = reinterpret_cast<int*>(l.scr_s + 4 * K);
    return l;
}

// Folds query qi's n buffered candidates into its sorted top-K (one wave).  Excluded candidates are dropped first; then every
// surviving candidate's place is (better candidates) + (better list entries, a binary search), every list entry's place is its index
// + (better candidates), and whatever lands below K is written to the wave's scratch and copied back.  Ids are distinct within a chunk,
// so the places of the real entries are a bijection onto the merged order; empty list entries go last.
__device__ void tk_fold(const TkLds& l, int qi, int n, int K, const TkArgs& a, int b, int wave) {
    const int lane = threadIdx.x & 63;
    float* bs = l.buf_s + qi * TK_CAP;
    int* bi = l.buf_id + qi * TK_CAP;
    float* ts = l.top_s + qi * K;
    int* ti = l.top_id + qi * K;
    float* ss = l.scr_s + wave * K;
    int* si = l.scr_id + wave * K;
    if (a.off) {
        const int64_t e0 = a.off[b], e1 = a.off[b + 1];
        for (int i = lane; i < n; i += 64)
            if (tk_excluded(a.excl, e0, e1, bi[i])) { bs[i] = -INFINITY; bi[i] = TK_PAD; }
        tk_wave_sync();
    }
    for (int i = lane; i < n; i += 64) {
        const float s = bs[i];
        const int id = bi[i];
        if (id == TK_PAD) continue;
        int pos = 0;
        for (int j = 0; j < n; ++j) pos += tk_better(bs[j], bi[j], s, id) ? 1 : 0;
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tk_better(ts[mid], ti[mid], s, id)) lo = mid + 1; else hi = mid;
        }
        pos += lo;
        if (pos < K) { ss[pos] = s; si[pos] = id; }
    }
    for (int k = lane; k < K; k += 64) {
        const float s = ts[k];
        const int id = ti[k];
        int pos = k;
        for (int j = 0; j < n; ++j) pos += tk_better(bs[j], bi[j], s, id) ? 1 : 0;
        if (pos < K) { ss[pos] = s; si[pos] = id; }
    }
    tk_wave_sync();
    for (int k = lane; k < K; k += 64) { ts[k] = ss[k]; ti[k] = si[k]; }
    tk_wave_sync();
    if (lane == 0) { l.cnt[qi] = 0; l.thr[qi] = ts[K - 1]; }
    tk_wave_sync();
}

template <int NK, int QB, bool SPLIT, bool IDX>
__global__ __launch_bounds__(256) void k_topk_sweep(TkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QT = 16 * QB;
    const int K = a.K;
    const TkLds l = tk_lds(smem, QT, NK, K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * QT;
    const int nq = min(QT, a.B - q0);
    const int c0 = blockIdx.y * a.chunk, c1 = min(a.src.V, c0 + a.chunk);

    // the query tile as B fragments, once
    for (int qb = wave; qb < QB; qb += 4) {
        const int row = q0 + qb * 16 + li;
        const bool rok = row < a.B;
        float v[NK][8];
        bf8 h[NK], lo[NK];
        tk_row_issue<NK>(v, a.q, a.ldq, row, rok, row == a.B - 1, a.src.D);
        tk_row_finish<NK, SPLIT>(v, a.q, a.ldq, row, rok, row == a.B - 1, a.src.D, h, lo);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            l.img_hi[(qb * NK + ks) * 64 + lane] = h[ks];
            if (SPLIT) l.img_lo[(qb * NK + ks) * 64 + lane] = lo[ks];
        }
    }
    for (int i = threadIdx.x; i < QT * K; i += 256) { l.top_s[i] = -INFINITY; l.top_id[i] = TK_PAD; }
    for (int i = threadIdx.x; i < QT; i += 256) {
        int t = -1;
        if (a.tgt && i < nq) t = a.tgt[q0 + i];
        l.tq[i] = (t >= 1 && t < a.src.V) ? t : -1;
        l.cnt[i] = 0;
        l.thr[i] = i < nq ? -INFINITY : INFINITY;          // a query row past B takes no candidates
        l.st[i] = 0.0f;
    }
    __syncthreads();

    // target scores: the diagonal of (target rows of the block's queries) x (the block's queries)
    if (a.tgt) {
        for (int qb = wave; qb < QB; qb += 4) {
            const int t = l.tq[qb * 16 + li];
            bf8 ah[NK], al[NK], bh[NK], bl[NK];
            tk_src_row<NK, SPLIT, IDX>(a.src, t, t > 0, ah, al);
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                bh[ks] = l.img_hi[(qb * NK + ks) * 64 + lane];
                bl[ks] = SPLIT ? l.img_lo[(qb * NK + ks) * 64 + lane] : bh[ks];
            }
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
            const int r = li - 4 * lg;
            if (r >= 0 && r < 4) {
                l.st[qb * 16 + li] = tk_pick(c, r);
                if (blockIdx.y == 0 && qb * 16 + li < nq) a.st_ws[q0 + qb * 16 + li] = tk_pick(c, r);
            }
        }
        __syncthreads();
    }

    int rk[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) rk[qb] = 0;
    const int n_rounds = (c1 - c0 + 63) / 64;
    float v[NK][8];                                        // the round ahead: table rows in flight, or (IDX) the fragments themselves
    bf8 nh[NK], nl[NK];
    if constexpr (IDX) {
        tk_idx_tile<NK, SPLIT>(a.src, (c0 + wave * 16) >> 4, nh, nl);       // chunks start at multiples of 64 rows
    } else {
        const int row = c0 + wave * 16 + li;
        tk_row_issue<NK>(v, a.src.table, a.src.D, row, row < c1, row == a.src.V - 1, a.src.D);
    }
    for (int round = 0; round < n_rounds; ++round) {
        const int it0 = c0 + round * 64 + wave * 16;
        bf8 ah[NK], al[NK];
        if constexpr (IDX) {
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                ah[ks] = nh[ks];
                if (SPLIT) al[ks] = nl[ks];
            }
            if (round + 1 < n_rounds) tk_idx_tile<NK, SPLIT>(a.src, (it0 + 64) >> 4, nh, nl);
        } else {
            {
                const int row = it0 + li;
                tk_row_finish<NK, SPLIT>(v, a.src.table, a.src.D, row, row < c1, row == a.src.V - 1, a.src.D, ah, al);
            }
            if (round + 1 < n_rounds) {
                const int row = it0 + 64 + li;
                tk_row_issue<NK>(v, a.src.table, a.src.D, row, row < c1, row == a.src.V - 1, a.src.D);
            }
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            bf8 bh[NK], bl[NK];
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                bh[ks] = l.img_hi[(qb * NK + ks) * 64 + lane];
                bl[ks] = SPLIT ? l.img_lo[(qb * NK + ks) * 64 + lane] : bh[ks];
            }
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
            const int qi = qb * 16 + li;
            const float th = l.thr[qi], s_t = l.st[qi];
            const int t = l.tq[qi];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = it0 + 4 * lg + r;
                const bool ok = id >= 1 && id < c1;
                if (ok && c[r] >= th) {
                    const int k = atomicAdd(&l.cnt[qi], 1);
                    l.buf_s[qi * TK_CAP + k] = c[r];
                    l.buf_id[qi * TK_CAP + k] = id;
                }
                rk[qb] += (t > 0 && ok && id != t && (c[r] > s_t || (c[r] == s_t && id < t))) ? 1 : 0;
            }
        }
        __syncthreads();
        // the wave's queries wave, wave + 4, ... : one LDS read for all of them, then a fold per set bit
        const bool last = round + 1 == n_rounds;
        const int my_q = wave + 4 * lane;
        const bool full = my_q < nq && l.cnt[my_q] > (last ? 0 : TK_CAP - 64);
        for (uint64_t m = __ballot(full); m; m &= m - 1) {
            const int qi = wave + 4 * (int)__builtin_ctzll(m);
            tk_fold(l, qi, __builtin_amdgcn_readfirstlane(l.cnt[qi]), K, a, q0 + qi, wave);
        }
        __syncthreads();
    }

    // the chunk's list and target count (every buffer is empty now: cnt[] = 0)
    const size_t slot = (size_t)blockIdx.y * a.B;
    for (int i = threadIdx.x; i < nq * K; i += 256) {
        const int qi = i / K, k = i - qi * K;
        a.part_s[(slot + q0 + qi) * K + k] = l.top_s[i];
        a.part_id[(slot + q0 + qi) * K + k] = l.top_id[i];
    }
    if (a.tgt) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
            if (rk[qb]) atomicAdd(&l.cnt[qb * 16 + li], rk[qb]);        // integer sums: the same total in any order
        __syncthreads();
        for (int i = threadIdx.x; i < nq; i += 256) a.part_cnt[slot + q0 + i] = l.cnt[i];
    }
}

// wave-wide best of (s, id): butterfly, every lane ends with the winner
__device__ __forceinline__ void tk_wave_best(float& s, int& id) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64);
        const int oi = __shfl_xor(id, o, 64);
        if (tk_better(os, oi, s, id)) { s = os; id = oi; }
    }
}

template <int NK, bool SPLIT, bool IDX>
__global__ __launch_bounds__(256) void k_topk_merge(TkArgs a) {
    __shared__ float sc[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;                                  // wave-uniform; no workgroup barrier below
    const int K = a.K;
    constexpr int J = TK_MAX_CHUNKS / 64;
    int head[J];
    float hs[J];
    int hid[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        head[j] = 0;
        const bool ok = c < a.n_chunks;
        hs[j] = ok ? a.part_s[((size_t)c * a.B + b) * K] : -INFINITY;
        hid[j] = ok ? a.part_id[((size_t)c * a.B + b) * K] : TK_PAD;
    }
    int k = 0;
    for (; k < K; ++k) {
        float s = hs[0];
        int id = hid[0];
#pragma unroll
        for (int j = 1; j < J; ++j)
            if (tk_better(hs[j], hid[j], s, id)) { s = hs[j]; id = hid[j]; }
        tk_wave_best(s, id);
        if (id == TK_PAD) break;                           // every list is exhausted
        if (lane == 0) { a.top_ids[(size_t)b * K + k] = id; a.top_scores[(size_t)b * K + k] = s; }
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (hid[j] == id) {                            // ids are distinct across chunks: exactly one head holds the winner
                const int c = lane + 64 * j;
                const int h = ++head[j];
                hs[j] = h < K ? a.part_s[((size_t)c * a.B + b) * K + h] : -INFINITY;
                hid[j] = h < K ? a.part_id[((size_t)c * a.B + b) * K + h] : TK_PAD;
            }
    }
    for (int kk = k + lane; kk < K; kk += 64) { a.top_ids[(size_t)b * K + kk] = 0; a.top_scores[(size_t)b * K + kk] = -INFINITY; }

    if (!a.tgt) return;
    const int t = a.tgt[b];
    const int64_t e0 = a.off ? a.off[b] : 0, e1 = a.off ? a.off[b + 1] : 0;
    int raw = 0;
    for (int c = lane; c < a.n_chunks; c += 64) raw += a.part_cnt[(size_t)c * a.B + b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) raw += __shfl_xor(raw, o, 64);
    bool hit_t = false;
    for (int64_t j = e0 + lane; j < e1; j += 64) hit_t |= a.excl[j] == t;
    const bool bad = !(t >= 1 && t < a.src.V) || __any(hit_t);
    if (bad) {
        if (lane == 0) a.rank[b] = -1;
        return;
    }
    // distinct excluded items (1 <= e < V, e != t) that beat the target, 16 rows at a time against the query in every column
    const float s_t = a.st_ws[b];
    int sub = 0;
    if (e1 > e0) {
        float qv[NK][8];
        bf8 bh[NK], bl[NK];
        tk_row_issue<NK>(qv, a.q, a.ldq, b, true, b == a.B - 1, a.src.D);
        tk_row_finish<NK, SPLIT>(qv, a.q, a.ldq, b, true, b == a.B - 1, a.src.D, bh, bl);
        for (int64_t p0 = e0; p0 < e1; p0 += 16) {
            const int64_t p = p0 + li;
            const int e = p < e1 ? a.excl[p] : 0;
            const bool rok = e >= 1 && e < a.src.V;
            bf8 ah[NK], al[NK];
            tk_src_row<NK, SPLIT, IDX>(a.src, e, rok, ah, al);
            const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
            if (li == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[wave][4 * lg + r] = c[r];
            }
            tk_wave_sync();
            bool hit = false;
            if (lane < 16 && rok && e != t) {
                const float s = sc[wave][lane];
                if (s > s_t || (s == s_t && e < t)) {
                    hit = true;
                    for (int64_t j = e0; j < p; ++j)
                        if (a.excl[j] == e) { hit = false; break; }       // counted at its first occurrence
                }
            }
            sub += __popcll(__ballot(hit));
            tk_wave_sync();
        }
    }
    if (lane == 0) a.rank[b] = raw - sub;
}

// Writing an index (castrec.h cr_topk_index_build, cr_topk_index_gather): a wave per destination tile, lane (li, lg) stores the
// fragments of its source row where the sweep's lane reads destination row r = 16 tile + li.  Without ids the source row is r itself
// (the build: rows >= V and columns >= D are +0); with ids it is ids[r - 1], the index of the table {0; row ids[0]; ...; row
// ids[n - 1]} -- no source row, so +0, for r = 0, r > n and an id outside 1 .. V-1.  A row's fragments depend on that row alone, so
// the gathered bytes are the build's on the gathered table, whether they come from the table or (IDX) from an index of it.
template <int NK, bool SPLIT, bool IDX, bool COS>
__global__ __launch_bounds__(256) void k_topk_index_write(TkSrc s, const int32_t* ids, int n, bf8* idx, int64_t plane, int n_tiles) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                           // wave-uniform
    const int r = tile * 16 + (threadIdx.x & 15);
    const int row = !ids ? r : (r >= 1 && r <= n) ? ids[r - 1] : 0;
    const bool rok = row < s.V && (!ids || row >= 1);
    bf8 h[NK], lo[NK];
    tk_src_row<NK, SPLIT, IDX, COS>(s, row, rok, h, lo);   // (a lane without a row reads nothing at `row`)
    tk_idx_store<NK, SPLIT>(idx, plane, tile, h, lo);
}

// Keeping an index in step with its table (castrec.h cr_topk_index_update, cr_topk_index_sync).  A row's groups are its own, so a row
// is rewritten in place.  tk_idx_row_store is the store that mirrors the IDX branch of tk_src_row: lane (li, lg) puts the fragments
// of ITS row r where that gather reads them, group (r >> 4) NK 64 + ks 64 + 16 lg + (r & 15), the lo plane `plane` groups further
// on; every offset 64-bit; a lane without a row (!rok) stores nothing and forms no address from r.
template <int NK, bool SPLIT>
__device__ __forceinline__ void tk_idx_row_store(bf8* idx, int64_t plane, int r, bool rok, const bf8 (&hi)[NK], const bf8 (&lo)[NK]) {
    if (!rok) return;
    const int lg = (threadIdx.x & 63) >> 4;
    bf8* p = idx + (int64_t)(r >> 4) * (NK * 64) + (lg * 16 + (r & 15));
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        p[ks * 64] = hi[ks];
        if (SPLIT) p[plane + ks * 64] = lo[ks];
    }
}

// The rows a list names: a wave takes 16 ids, lane li the id ids[16 w + li].  s is the fp32 source: the [V, D] table (source row =
// the id) or, packed, the [n, D] rows in list order (source row = the position; s.V == n, so the re-read of the source's last row is
// the build's).  An id outside 0 .. V-1, and a lane past the list, has no row: nothing of it is read or written.
template <int NK, bool SPLIT, bool COS>
__global__ __launch_bounds__(256) void k_topk_index_update(TkSrc s, int packed, int V, const int32_t* ids, int n, bf8* idx, int64_t plane) {
    const int64_t j = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (threadIdx.x & 15);
    const int id = j < n ? ids[j] : -1;
    const bool rok = (unsigned)id < (unsigned)V;
    const int row = !rok ? 0 : packed ? (int)j : id;
    bf8 h[NK], lo[NK];
    tk_src_row<NK, SPLIT, false, COS>(s, row, rok, h, lo);
    tk_idx_row_store<NK, SPLIT>(idx, plane, id, rok, h, lo);
}

// The tiles a flag array names: a wave per tile, rewritten whole -- the build's body, full 1 KB runs -- when any of its rows r < V has
// (uint32_t)flags[r] >= since (cr_adam_desc.lazy_flags: the number of the last step that moved row r).  The test is wave-uniform; a
// tile without such a row is left alone and its table rows are not read.
template <int NK, bool SPLIT, bool COS>
__global__ __launch_bounds__(256) void k_topk_index_sync(TkSrc s, const int32_t* flags, uint32_t since, bf8* idx, int64_t plane) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= s.n_tiles) return;                         // wave-uniform
    const int r = tile * 16 + (threadIdx.x & 15);
    const bool rok = r < s.V;
    const bool hit = rok && (uint32_t)flags[rok ? r : 0] >= since;
    if (__ballot(hit) == 0) return;                        // wave-uniform
    bf8 h[NK], lo[NK];
    tk_src_row<NK, SPLIT, false, COS>(s, r, rok, h, lo);
    tk_idx_store<NK, SPLIT>(idx, plane, tile, h, lo);
}

// planes of an index of `precision`: 2 (hi + lo; CR_PREC_F32 as CR_PREC_BF16X3), 1 (plain bf16), 0 for anything else
int tk_index_planes(int precision) {
    return (precision == CR_PREC_BF16X3 || precision == CR_PREC_F32) ? 2 : precision == CR_PREC_BF16 ? 1 : 0;
}

// an index of a [V, D] table: k-steps, tiles of 16 rows, and the 16-byte groups of one plane
struct TkIdxGeom {
    int NK, n_tiles;
    int64_t plane;
};
TkIdxGeom tk_index_geom(int V, int D) {
    TkIdxGeom g;
    g.NK = tk_nk(D);
    g.n_tiles = (int)(((int64_t)V + 15) / 16);
    g.plane = (int64_t)g.n_tiles * g.NK * 64;
    return g;
}
TkSrc tk_source(const float* table, const void* index, int V, int D) {
    const TkIdxGeom g = tk_index_geom(V, D);
    return TkSrc{table, static_cast<const bf8*>(index), g.plane, g.n_tiles, V, D};
}

// what every entry point `who` asks of a table's shape and of a precision
int tk_check_shape(const char* who, int V, int D, int precision) {
    CR_REQUIRE(D >= 8 && D <= 256, "%s: D=%d outside 8 .. 256", who, D);
    CR_REQUIRE(V >= 1, "%s: V=%d must be >= 1", who, V);
    CR_REQUIRE(tk_index_planes(precision) != 0, "%s: unknown precision %d", who, precision);
    return CR_OK;
}

// A writer's `precision` argument (castrec.h CR_INDEX_COSINE): the CR_PREC_* value alone, or the flag OR-ed onto CR_PREC_BF16X3 /
// CR_PREC_BF16 for an index of normalised rows.  Strips the flag from exactly those two values; anything else -- the flag alone, another
// bit, a negative number -- stays whole for tk_check_shape to refuse as the unknown precision it is.
bool tk_writer_cosine(int& precision) {
    const int base = precision ^ CR_INDEX_COSINE;
    if (base != CR_PREC_BF16X3 && base != CR_PREC_BF16) return false;
    precision = base;
    return true;
}

struct TkGeom {
    int NK, QB, n_qt, n_chunks, chunk;
    size_t lds;
};

bool tk_geometry(int B, int V, int D, int K, TkGeom& g) {
    if (B < 1 || V < 1 || D < 8 || D > 256 || K < 1 || K > CR_TOPK_MAX) return false;
    g.NK = tk_nk(D);
    g.QB = 4;
    while (g.QB > 1 && (tk_lds_bytes(16 * g.QB, g.NK, K) > 160 * 1024 || 16 * (g.QB / 2) >= B)) g.QB /= 2;
    g.lds = tk_lds_bytes(16 * g.QB, g.NK, K);
    if (g.lds > 160 * 1024) return false;
    g.n_qt = (B + 16 * g.QB - 1) / (16 * g.QB);
    // about 512 workgroups, chunks of at least 2 048 items (a chunk's first rounds fill its list: short chunks repeat that work)
    int nc = (512 + g.n_qt - 1) / g.n_qt;
    nc = std::min(nc, std::min(TK_MAX_CHUNKS, (V + 2047) / 2048));
    nc = std::max(nc, 1);
    g.chunk = ((V + nc - 1) / nc + 63) / 64 * 64;
    g.n_chunks = (V + g.chunk - 1) / g.chunk;
    return true;
}

// workspace: [offsets (B + 1) int64 | target scores B | chunk lists n_chunks B K (float, int32) | chunk counts n_chunks B]
size_t tk_workspace(int B, const TkGeom& g, int K) {
    const size_t nb = (size_t)g.n_chunks * B;
    return cr_align256(8 * ((size_t)B + 1)) + cr_align256(4 * (size_t)B) + 2 * cr_align256(nb * K * 4) + cr_align256(nb * 4);
}

template <int NK, bool SPLIT, bool IDX>
void tk_launch(const TkArgs& a, const TkGeom& g, hipStream_t st) {
    const dim3 grid(g.n_qt, g.n_chunks);
    if (g.QB == 4) hipLaunchKernelGGL((k_topk_sweep<NK, 4, SPLIT, IDX>), grid, dim3(256), g.lds, st, a);
    else if (g.QB == 2) hipLaunchKernelGGL((k_topk_sweep<NK, 2, SPLIT, IDX>), grid, dim3(256), g.lds, st, a);
    else hipLaunchKernelGGL((k_topk_sweep<NK, 1, SPLIT, IDX>), grid, dim3(256), g.lds, st, a);
    hipLaunchKernelGGL((k_topk_merge<NK, SPLIT, IDX>), dim3((a.B + 3) / 4), dim3(256), 0, st, a);
}

// the index of `rows` rows in `planes` planes, written from src: row for row (ids NULL) or from rows ids[0 .. n-1] behind a zero row;
// cosine: table rows are normalised (the rows of an index source are what they are)
void tk_index_write(const TkSrc& src, const int32_t* ids, int n, void* out, int rows, int planes, bool cosine, hipStream_t st) {
    const TkIdxGeom g = tk_index_geom(rows, src.D);
    const dim3 grid((g.n_tiles + 3) / 4);
    bf8* idx = static_cast<bf8*>(out);
    tk_dispatch(g.NK, planes == 2, [&](auto nk, auto sp) {
        if (src.idx) hipLaunchKernelGGL((k_topk_index_write<nk, sp, true, false>), grid, dim3(256), 0, st, src, ids, n, idx, g.plane, g.n_tiles);
        else if (cosine) hipLaunchKernelGGL((k_topk_index_write<nk, sp, false, true>), grid, dim3(256), 0, st, src, ids, n, idx, g.plane, g.n_tiles);
        else hipLaunchKernelGGL((k_topk_index_write<nk, sp, false, false>), grid, dim3(256), 0, st, src, ids, n, idx, g.plane, g.n_tiles);
    });
}

}  // namespace

extern "C" size_t cr_topk_index_bytes(int V, int D, int precision) {
    const int planes = tk_index_planes(precision);
    if (V < 1 || D < 8 || D > 256 || planes == 0) return 0;
    return (size_t)planes * (size_t)tk_index_geom(V, D).plane * 16;
}

extern "C" int cr_topk_index_build(const float* table, int V, int D, int precision, void* index, size_t index_bytes, void* stream) {
    CR_REQUIRE(table && index, "cr_topk_index_build: NULL table or index");
    const bool cosine = tk_writer_cosine(precision);
    if (const int rc = tk_check_shape("cr_topk_index_build", V, D, precision)) return rc;
    const size_t need = cr_topk_index_bytes(V, D, precision);
    CR_REQUIRE(index_bytes >= need, "cr_topk_index_build: index of %zu bytes, cr_topk_index_bytes says %zu", index_bytes, need);
    tk_index_write(tk_source(table, nullptr, V, D), nullptr, 0, index, V, tk_index_planes(precision), cosine, cr_stream(stream));
    return cr_check_launch("cr_topk_index_build");
}

extern "C" int cr_topk_index_gather(const float* table, const void* index, int index_precision, int V, int D, const int32_t* ids,
                                    int n, int precision, void* out_index, size_t out_bytes, void* stream) {
    CR_REQUIRE((table != nullptr) != (index != nullptr), "cr_topk_index_gather: exactly one source, table or index, must be non-NULL (%s)",
               table ? "both given" : "both NULL");
    CR_REQUIRE(ids && out_index, "cr_topk_index_gather: NULL ids or out_index");
    const bool cosine = tk_writer_cosine(precision);      // (an index source is copied: its rows carry their metric already)
    if (const int rc = tk_check_shape("cr_topk_index_gather", V, D, precision)) return rc;
    CR_REQUIRE(n >= 1 && n < 0x7fffffff, "cr_topk_index_gather: n=%d must be >= 1 (and n + 1 an int)", n);
    const int planes = tk_index_planes(precision);
    if (index) {
        const int sp = tk_index_planes(index_precision);
        CR_REQUIRE(sp != 0, "cr_topk_index_gather: unknown index_precision %d", index_precision);
        CR_REQUIRE(planes <= sp, "cr_topk_index_gather: a plain bf16 index has no lo plane for a sub-index of precision %d", precision);
    }
    const size_t need = cr_topk_index_bytes(n + 1, D, precision);
    CR_REQUIRE(out_bytes >= need, "cr_topk_index_gather: out_index of %zu bytes, cr_topk_index_bytes(n + 1 = %d) says %zu", out_bytes,
               n + 1, need);
    tk_index_write(tk_source(table, index, V, D), ids, n, out_index, n + 1, planes, cosine, cr_stream(stream));
    return cr_check_launch("cr_topk_index_gather");
}

extern "C" int cr_topk_index_update(const float* src, int packed, int V, int D, int precision, void* index, size_t index_bytes,
                                    const int32_t* ids, int n, void* stream) {
    CR_REQUIRE(src && index && ids, "cr_topk_index_update: NULL src, index or ids");
    const bool cosine = tk_writer_cosine(precision);
    if (const int rc = tk_check_shape("cr_topk_index_update", V, D, precision)) return rc;
    CR_REQUIRE(n >= 1, "cr_topk_index_update: n=%d must be >= 1", n);
    const size_t need = cr_topk_index_bytes(V, D, precision);
    CR_REQUIRE(index_bytes == need, "cr_topk_index_update: index_bytes=%zu, cr_topk_index_bytes(V=%d, D=%d) says %zu", index_bytes, V, D,
               need);
    const TkIdxGeom g = tk_index_geom(V, D);
    const TkSrc s = tk_source(src, nullptr, packed ? n : V, D);          // the source's own rows: its last row is re-read as the build's
    const dim3 grid((unsigned)(((int64_t)n + 63) / 64));
    bf8* idx = static_cast<bf8*>(index);
    hipStream_t st = cr_stream(stream);
    tk_dispatch(g.NK, tk_index_planes(precision) == 2, [&](auto nk, auto sp) {
        if (cosine) hipLaunchKernelGGL((k_topk_index_update<nk, sp, true>), grid, dim3(256), 0, st, s, packed ? 1 : 0, V, ids, n, idx, g.plane);
        else hipLaunchKernelGGL((k_topk_index_update<nk, sp, false>), grid, dim3(256), 0, st, s, packed ? 1 : 0, V, ids, n, idx, g.plane);
    });
    return cr_check_launch("cr_topk_index_update");
}

extern "C" int cr_topk_index_sync(const float* table, int V, int D, int precision, void* index, size_t index_bytes, const int32_t* flags,
                                  uint32_t since, void* stream) {
    CR_REQUIRE(table && index && flags, "cr_topk_index_sync: NULL table, index or flags");
    const bool cosine = tk_writer_cosine(precision);
    if (const int rc = tk_check_shape("cr_topk_index_sync", V, D, precision)) return rc;
    const size_t need = cr_topk_index_bytes(V, D, precision);
    CR_REQUIRE(index_bytes == need, "cr_topk_index_sync: index_bytes=%zu, cr_topk_index_bytes(V=%d, D=%d) says %zu", index_bytes, V, D,
               need);
    const TkSrc s = tk_source(table, nullptr, V, D);
    const dim3 grid((s.n_tiles + 3) / 4);
    bf8* idx = static_cast<bf8*>(index);
    hipStream_t st = cr_stream(stream);
    tk_dispatch(tk_nk(D), tk_index_planes(precision) == 2, [&](auto nk, auto sp) {
        if (cosine) hipLaunchKernelGGL((k_topk_index_sync<nk, sp, true>), grid, dim3(256), 0, st, s, flags, since, idx, s.plane);
        else hipLaunchKernelGGL((k_topk_index_sync<nk, sp, false>), grid, dim3(256), 0, st, s, flags, since, idx, s.plane);
    });
    return cr_check_launch("cr_topk_index_sync");
}

extern "C" size_t cr_score_topk_workspace(int B, int V, int D, int K) {
    TkGeom g;
    if (!tk_geometry(B, V, D, K, g)) return 0;
    return tk_workspace(B, g, K);
}

extern "C" int cr_score_topk(const cr_topk_desc* d, void* stream) {
    CR_REQUIRE(d, "cr_score_topk: NULL descriptor");
    CR_REQUIRE(d->K >= 1 && d->K <= CR_TOPK_MAX, "cr_score_topk: K=%d outside 1 .. CR_TOPK_MAX (%d)", d->K, CR_TOPK_MAX);
    CR_REQUIRE(d->B >= 1 && d->V >= 1, "cr_score_topk: B=%d, V=%d must be >= 1", d->B, d->V);
    if (const int rc = tk_check_shape("cr_score_topk", d->V, d->D, d->precision)) return rc;
    CR_REQUIRE(d->ld >= d->D, "cr_score_topk: ld=%d < D=%d", d->ld, d->D);
    if (d->index) CR_REQUIRE(d->query, "cr_score_topk: NULL query");
    else CR_REQUIRE(d->query && d->table, "cr_score_topk: NULL query or table");
    CR_REQUIRE(d->top_ids && d->top_scores, "cr_score_topk: NULL output (top_ids / top_scores)");
    CR_REQUIRE(!d->targets || d->rank, "cr_score_topk: targets given but rank is NULL");
    if (d->index) {
        const int planes = tk_index_planes(d->index_precision);
        CR_REQUIRE(planes != 0, "cr_score_topk: unknown index_precision %d", d->index_precision);
        CR_REQUIRE(planes == 2 || d->precision == CR_PREC_BF16,
                   "cr_score_topk: a plain bf16 index serves precision CR_PREC_BF16 only, not %d", d->precision);
        const size_t ib = cr_topk_index_bytes(d->V, d->D, d->index_precision);
        CR_REQUIRE(d->index_bytes == ib, "cr_score_topk: index_bytes=%zu, cr_topk_index_bytes(V=%d, D=%d) says %zu", d->index_bytes,
                   d->V, d->D, ib);
    }
    if (d->excl_off) {
        CR_REQUIRE(d->excl_off[0] >= 0, "cr_score_topk: excl_off[0]=%lld < 0", (long long)d->excl_off[0]);
        for (int b = 0; b < d->B; ++b)
            CR_REQUIRE(d->excl_off[b + 1] >= d->excl_off[b], "cr_score_topk: excl_off decreases at row %d (%lld -> %lld)", b,
                       (long long)d->excl_off[b], (long long)d->excl_off[b + 1]);
        CR_REQUIRE(d->excl_ids || d->excl_off[d->B] == d->excl_off[0], "cr_score_topk: excl_off names ids but excl_ids is NULL");
    }
    TkGeom g;
    CR_REQUIRE(tk_geometry(d->B, d->V, d->D, d->K, g), "cr_score_topk: unsupported shape");
    const size_t need = tk_workspace(d->B, g, d->K);
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need, "cr_score_topk: workspace of %zu bytes, cr_score_topk_workspace says %zu",
               d->workspace ? d->workspace_bytes : (size_t)0, need);

    hipStream_t st = cr_stream(stream);
    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    const size_t nb = (size_t)g.n_chunks * d->B;
    TkArgs a;
    a.q = d->query; a.ldq = d->ld; a.src = tk_source(d->table, d->index, d->V, d->D);
    a.B = d->B; a.K = d->K;
    a.off = nullptr;
    if (d->excl_off && d->excl_off[d->B] > d->excl_off[0]) {
        int64_t* off = reinterpret_cast<int64_t*>(w);
        const hipError_t e = hipMemcpyAsync(off, d->excl_off, 8 * ((size_t)d->B + 1), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return cr_set_error(CR_ERR_HIP, "cr_score_topk: offsets copy: %s", hipGetErrorString(e));
        a.off = off;
    }
    w += cr_align256(8 * ((size_t)d->B + 1));
    a.st_ws = reinterpret_cast<float*>(w); w += cr_align256(4 * (size_t)d->B);
    a.part_s = reinterpret_cast<float*>(w); w += cr_align256(nb * d->K * 4);
    a.part_id = reinterpret_cast<int32_t*>(w); w += cr_align256(nb * d->K * 4);
    a.part_cnt = reinterpret_cast<int32_t*>(w);
    a.excl = d->excl_ids; a.tgt = d->targets;
    a.top_ids = d->top_ids; a.top_scores = d->top_scores; a.rank = d->rank;
    a.chunk = g.chunk; a.n_chunks = g.n_chunks;
    const bool split = d->precision != CR_PREC_BF16;       // CR_PREC_F32: the bf16x3 products (fp32-grade)
    tk_dispatch(g.NK, split, [&](auto nk, auto sp) {
        if (d->index) tk_launch<nk, sp, true>(a, g, st);
        else tk_launch<nk, sp, false>(a, g, st);
    });
    return cr_check_launch("cr_score_topk");
}

// ---- top-K over per-query candidate lists (castrec.h cr_score_topk_lists) -------------------------------------------------------------
// "The best K among THIS row's candidates."  Grid: (query b) x (segment of the row's list), 256 threads.  Every wave forms the query's
// B fragments once the way k_topk_merge does for the excluded rows -- row b in every lane, so the query stands in every column -- and
// takes 16 candidates per round: lane li reads cand[p + li], tk_src_row gives that row's A fragments (zeros for an id outside
// 1 .. V-1, whose row is not read), one tk_tile gives the 16 scores, item 4 lg + r in c[r] of every lane of group lg.  The lane with
// li == 4 lg + r owns that item: it holds the id it loaded and picks c[r].  Ids are requested two rounds ahead and rows one round
// ahead, so a round's gather is in flight while the round before it is selected.  Selection is the sweep's on a TkLds of one query
// (threshold, TK_CAP buffer, tk_fold by wave 0 whenever the buffer could not take another round of 64 and after the last round);
// beside it every score is compared with the target's (integer counts, and a "target seen" flag).  No exclusions here: the host
// subtracts them from the lists, so TkArgs.off stays NULL for the fold.  A score has the sweep's bits: one item row, one query, tk_tile.
// One segment: the workgroup writes the final outputs.  More: its sorted list, count and flag go to the workspace, k_topk_merge (as it
// is, without targets) runs the tournament and k_topk_lists_rank sums the counts.
namespace {

struct TlArgs {
    TkArgs a;                               // q, ldq, src, B, K, tgt, part_*, top_*, rank; off = excl = NULL; n_chunks = segments
    const int64_t* coff;                    // device copy of cand_off
    const int32_t* cand;
    int32_t* part_seen;                     // [n_seg, B]: the segment held the target
    int seg_len;
};

template <int NK, bool SPLIT, bool IDX>
__global__ __launch_bounds__(256) void k_topk_lists(TlArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TkArgs& a = g.a;
    const int K = a.K, V = a.src.V;
    const TkLds l = tk_lds(smem, 1, NK, K);                // one query: no operand image (the fragments stay in registers)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x;
    const int64_t p0 = g.coff[b] + (int64_t)blockIdx.y * g.seg_len;
    const int64_t p1 = min(g.coff[b + 1], p0 + g.seg_len);
    const int n_rounds = p1 > p0 ? (int)((p1 - p0 + 63) / 64) : 0;
    int t = a.tgt ? a.tgt[b] : -1;
    t = (t >= 1 && t < V) ? t : -1;

    bf8 bh[NK], bl[NK];
    {
        float qv[NK][8];
        tk_row_issue<NK>(qv, a.q, a.ldq, b, true, b == a.B - 1, a.src.D);
        tk_row_finish<NK, SPLIT>(qv, a.q, a.ldq, b, true, b == a.B - 1, a.src.D, bh, bl);
    }
    for (int i = threadIdx.x; i < K; i += 256) { l.top_s[i] = -INFINITY; l.top_id[i] = TK_PAD; }
    if (threadIdx.x == 0) { l.cnt[0] = 0; l.thr[0] = -INFINITY; l.st[0] = 0.0f; l.tq[0] = 0; }      // tq: "target seen"
    if (wave == 0 && t > 0) {                              // the target's score: its row in every lane, one tile
        bf8 ah[NK], al[NK];
        tk_src_row<NK, SPLIT, IDX>(a.src, t, true, ah, al);
        const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
        if (lane == 0) l.st[0] = c[0];
    }
    __syncthreads();
    const float s_t = l.st[0];

    // candidate p0 + 64 round + 16 wave + li of the segment; 0 (not eligible) past its end
    auto cand_at = [&](int round) {
        const int64_t p = p0 + (int64_t)round * 64 + wave * 16 + li;
        return p < p1 ? g.cand[p] : 0;
    };
    int id_c = cand_at(0), id_n = cand_at(1);
    float v[NK][8];                                        // the round ahead: table rows in flight, or (IDX) the fragments themselves
    bf8 nh[NK], nl[NK];
    if (n_rounds > 0) {
        const bool rok = id_c >= 1 && id_c < V;
        if constexpr (IDX) tk_src_row<NK, SPLIT, true>(a.src, id_c, rok, nh, nl);
        else tk_row_issue<NK>(v, a.src.table, a.src.D, id_c, rok, id_c == V - 1, a.src.D);
    }
    int rk = 0;
    bool seen = false;
    for (int round = 0; round < n_rounds; ++round) {
        const int id = id_c;
        const bool rok = id >= 1 && id < V;
        bf8 ah[NK], al[NK];
        if constexpr (IDX) {
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                ah[ks] = nh[ks];
                if (SPLIT) al[ks] = nl[ks];
            }
        } else {
            tk_row_finish<NK, SPLIT>(v, a.src.table, a.src.D, id, rok, id == V - 1, a.src.D, ah, al);
        }
        if (round + 1 < n_rounds) {
            id_c = id_n;
            const bool nok = id_c >= 1 && id_c < V;
            if constexpr (IDX) tk_src_row<NK, SPLIT, true>(a.src, id_c, nok, nh, nl);
            else tk_row_issue<NK>(v, a.src.table, a.src.D, id_c, nok, id_c == V - 1, a.src.D);
            id_n = cand_at(round + 2);
        }
        const f32x4 c = tk_tile<NK, SPLIT>(ah, al, bh, bl);
        const int r = li - 4 * lg;
        if (r >= 0 && r < 4 && rok) {                      // the lane that owns item 4 lg + r = li of the tile
            const float s = tk_pick(c, r);
            if (s >= l.thr[0]) {
                const int k = atomicAdd(&l.cnt[0], 1);
                l.buf_s[k] = s;
                l.buf_id[k] = id;
            }
            if (t > 0) {
                if (id == t) seen = true;
                else rk += (s > s_t || (s == s_t && id < t)) ? 1 : 0;
            }
        }
        __syncthreads();
        const int n = l.cnt[0];
        if (wave == 0 && n > (round + 1 == n_rounds ? 0 : TK_CAP - 64)) tk_fold(l, 0, n, K, a, b, 0);
        __syncthreads();
    }

    // every buffer is empty now (cnt = 0): the counts of the target's betters are summed there
    if (a.tgt) {
        if (rk) atomicAdd(&l.cnt[0], rk);                  // integer sums: the same total in any order
        if (seen) l.tq[0] = 1;
        __syncthreads();
    }
    if (a.n_chunks == 1) {
        for (int k = threadIdx.x; k < K; k += 256) {
            const int id = l.top_id[k];
            a.top_ids[(size_t)b * K + k] = id == TK_PAD ? 0 : id;
            a.top_scores[(size_t)b * K + k] = l.top_s[k];
        }
        if (a.tgt && threadIdx.x == 0) a.rank[b] = l.tq[0] ? l.cnt[0] : -1;
    } else {
        const size_t slot = (size_t)blockIdx.y * a.B + b;
        for (int k = threadIdx.x; k < K; k += 256) {
            a.part_s[slot * K + k] = l.top_s[k];
            a.part_id[slot * K + k] = l.top_id[k];
        }
        if (a.tgt && threadIdx.x == 0) { a.part_cnt[slot] = l.cnt[0]; g.part_seen[slot] = l.tq[0]; }
    }
}

// the rank of a segmented row: the segments' counts summed; -1 unless exactly one segment held the target
__global__ __launch_bounds__(256) void k_topk_lists_rank(const int32_t* part_cnt, const int32_t* part_seen, int B, int n_seg, int32_t* rank) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int cnt = 0, seen = 0;
    for (int s = 0; s < n_seg; ++s) {
        cnt += part_cnt[(size_t)s * B + b];
        seen += part_seen[(size_t)s * B + b];
    }
    rank[b] = seen == 1 ? cnt : -1;
}

// the partition of lists whose longest has max_len candidates: segments of seg_len candidates, n_seg of them
struct TlGeom {
    int n_seg, seg_len;
};
bool tl_geometry(int B, int64_t max_len, TlGeom& g) {
    if (B < 1 || max_len < 0 || max_len > 0x7fffffff) return false;
    int64_t n = std::min<int64_t>(TK_MAX_CHUNKS, (max_len + 2047) / 2048);
    n = std::max<int64_t>(1, std::min<int64_t>(n, std::max(1, (1024 + B - 1) / B)));
    g.seg_len = (int)std::max<int64_t>(1, (max_len + n - 1) / n);
    g.n_seg = (int)std::max<int64_t>(1, (max_len + g.seg_len - 1) / g.seg_len);
    return true;
}

// workspace: [offsets (B + 1) int64 | with more than one segment: lists n_seg B K (float, int32), counts and flags n_seg B]
size_t tl_workspace(int B, const TlGeom& g, int K) {
    const size_t nb = g.n_seg > 1 ? (size_t)g.n_seg * B : 0;
    return cr_align256(8 * ((size_t)B + 1)) + 2 * cr_align256(nb * K * 4) + 2 * cr_align256(nb * 4);
}

template <int NK, bool SPLIT, bool IDX>
void tl_launch(const TlArgs& g, hipStream_t st) {
    const TkArgs& a = g.a;
    hipLaunchKernelGGL((k_topk_lists<NK, SPLIT, IDX>), dim3(a.B, a.n_chunks), dim3(256), tk_lds_bytes(1, NK, a.K), st, g);
    if (a.n_chunks == 1) return;
    TkArgs m = a;
    m.tgt = nullptr;                                       // the tournament alone: the ranks need the segments' flags
    hipLaunchKernelGGL((k_topk_merge<NK, SPLIT, IDX>), dim3((a.B + 3) / 4), dim3(256), 0, st, m);
    if (a.tgt) hipLaunchKernelGGL(k_topk_lists_rank, dim3((a.B + 255) / 256), dim3(256), 0, st, a.part_cnt, g.part_seen, a.B, a.n_chunks, a.rank);
}

}  // namespace

extern "C" int cr_topk_lists_segments(int B, int64_t max_len) {
    TlGeom g;
    return tl_geometry(B, max_len, g) ? g.n_seg : 0;
}

extern "C" size_t cr_score_topk_lists_workspace(int B, int64_t max_len, int D, int K) {
    TlGeom g;
    if (D < 8 || D > 256 || K < 1 || K > CR_TOPK_MAX || !tl_geometry(B, max_len, g)) return 0;
    return tl_workspace(B, g, K);
}

extern "C" int cr_score_topk_lists(const cr_topk_lists_desc* d, void* stream) {
    const char* who = "cr_score_topk_lists";
    CR_REQUIRE(d, "cr_score_topk_lists: NULL descriptor");
    CR_REQUIRE(d->K >= 1 && d->K <= CR_TOPK_MAX, "cr_score_topk_lists: K=%d outside 1 .. CR_TOPK_MAX (%d)", d->K, CR_TOPK_MAX);
    CR_REQUIRE(d->B >= 1 && d->V >= 1, "cr_score_topk_lists: B=%d, V=%d must be >= 1", d->B, d->V);
    if (const int rc = tk_check_shape(who, d->V, d->D, d->precision)) return rc;
    CR_REQUIRE(d->ld >= d->D, "cr_score_topk_lists: ld=%d < D=%d", d->ld, d->D);
    if (d->index) CR_REQUIRE(d->query, "cr_score_topk_lists: NULL query");
    else CR_REQUIRE(d->query && d->table, "cr_score_topk_lists: NULL query or table");
    CR_REQUIRE(d->top_ids && d->top_scores, "cr_score_topk_lists: NULL output (top_ids / top_scores)");
    CR_REQUIRE(!d->targets || d->rank, "cr_score_topk_lists: targets given but rank is NULL");
    CR_REQUIRE(d->cand_off, "cr_score_topk_lists: NULL cand_off");
    CR_REQUIRE(d->cand_off[0] >= 0, "cr_score_topk_lists: cand_off[0]=%lld < 0", (long long)d->cand_off[0]);
    int64_t max_len = 0;
    for (int b = 0; b < d->B; ++b) {
        const int64_t n = d->cand_off[b + 1] - d->cand_off[b];
        CR_REQUIRE(n >= 0, "cr_score_topk_lists: cand_off decreases at row %d (%lld -> %lld)", b, (long long)d->cand_off[b],
                   (long long)d->cand_off[b + 1]);
        CR_REQUIRE(n <= 0x7fffffff, "cr_score_topk_lists: row %d names %lld candidates, 2^31 - 1 at most", b, (long long)n);
        max_len = std::max(max_len, n);
    }
    CR_REQUIRE(d->cand_ids || max_len == 0, "cr_score_topk_lists: cand_off names ids but cand_ids is NULL");
    if (d->index) {
        const int planes = tk_index_planes(d->index_precision);
        CR_REQUIRE(planes != 0, "cr_score_topk_lists: unknown index_precision %d", d->index_precision);
        CR_REQUIRE(planes == 2 || d->precision == CR_PREC_BF16,
                   "cr_score_topk_lists: a plain bf16 index serves precision CR_PREC_BF16 only, not %d", d->precision);
        const size_t ib = cr_topk_index_bytes(d->V, d->D, d->index_precision);
        CR_REQUIRE(d->index_bytes == ib, "cr_score_topk_lists: index_bytes=%zu, cr_topk_index_bytes(V=%d, D=%d) says %zu", d->index_bytes,
                   d->V, d->D, ib);
    }
    TlGeom g;
    CR_REQUIRE(tl_geometry(d->B, max_len, g), "cr_score_topk_lists: unsupported shape");
    const size_t need = tl_workspace(d->B, g, d->K);
    CR_REQUIRE(d->workspace && d->workspace_bytes >= need,
               "cr_score_topk_lists: workspace of %zu bytes, cr_score_topk_lists_workspace says %zu", d->workspace ? d->workspace_bytes : (size_t)0,
               need);

    hipStream_t st = cr_stream(stream);
    unsigned char* w = static_cast<unsigned char*>(d->workspace);
    int64_t* off = reinterpret_cast<int64_t*>(w);
    const hipError_t e = hipMemcpyAsync(off, d->cand_off, 8 * ((size_t)d->B + 1), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return cr_set_error(CR_ERR_HIP, "cr_score_topk_lists: offsets copy: %s", hipGetErrorString(e));
    w += cr_align256(8 * ((size_t)d->B + 1));
    const size_t nb = g.n_seg > 1 ? (size_t)g.n_seg * d->B : 0;
    TlArgs t;
    TkArgs& a = t.a;
    a.q = d->query; a.ldq = d->ld; a.src = tk_source(d->table, d->index, d->V, d->D);
    a.B = d->B; a.K = d->K;
    a.off = nullptr; a.excl = nullptr; a.tgt = d->targets; a.st_ws = nullptr;
    a.part_s = reinterpret_cast<float*>(w); w += cr_align256(nb * d->K * 4);
    a.part_id = reinterpret_cast<int32_t*>(w); w += cr_align256(nb * d->K * 4);
    a.part_cnt = reinterpret_cast<int32_t*>(w); w += cr_align256(nb * 4);
    t.part_seen = reinterpret_cast<int32_t*>(w);
    a.top_ids = d->top_ids; a.top_scores = d->top_scores; a.rank = d->rank;
    a.chunk = 0; a.n_chunks = g.n_seg;
    t.coff = off; t.cand = d->cand_ids; t.seg_len = g.seg_len;
    const bool split = d->precision != CR_PREC_BF16;       // CR_PREC_F32: the bf16x3 products (fp32-grade)
    tk_dispatch(tk_nk(d->D), split, [&](auto nk, auto sp) {
        if (d->index) tl_launch<nk, sp, true>(t, st);
        else tl_launch<nk, sp, false>(t, st);
    });
    return cr_check_launch("cr_score_topk_lists");
}

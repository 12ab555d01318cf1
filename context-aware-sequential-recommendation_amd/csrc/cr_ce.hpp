// The streamed-block machinery of the softmax sweeps (cr_ce.hip: the full catalogue; cr_sce.hip: a sampled candidate table):
// 32 rows of an fp32 matrix loaded a block ahead into registers, stored as a bf16 hi / lo LDS image, read back as row operands or
// transposed, the score tile with the operands' roles swapped, and the G x image product of the gradient passes.
#pragma once
#include "cr_bf16.hpp"

namespace {

constexpr float CE_LOG2E = 1.4426950408889634f;
constexpr float CE_LN2 = 0.6931471805599453f;
constexpr int CE_BLK = 32;                  // rows of the streamed LDS block (items in lse / dh, batch rows in de)

// CE_BLK rows x NCB blocks of 64 columns, bf16 hi and lo
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

}  // namespace

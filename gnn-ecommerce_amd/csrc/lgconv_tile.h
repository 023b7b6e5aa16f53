// lgconv_tile.h -- the 64 x 128 x 32 fp32-MFMA tile of the scoring units (lgconv_similar.hip, lgconv_fullrank.hip,
// lgconv_softmax.hip, lgconv_retrieve.hip; DESIGN.md sections 12a and 19).  The prologue (which ids index which table), the loop over tiles and
// slices and the tile's epilogue are the unit's own; what they share is here, one definition each (Tile::product is the one
// piece two of the kernels restate, for the registers a call costs them).
//
// A workgroup of kBlock threads owns kTileBM query rows: gathered and staged once in LDS as Qs[kTileBM][dp + 4], whole
// width, zero-padded to dp = dim rounded up to 16 columns.  Tiles of kTileBN table rows ("items") pass through
// Bs[kTileBN][kTileBS] in chunks of kTileKC columns; the next chunk is already in registers (kTileStage float4 groups a
// thread) while the current one is multiplied.  Wavefront w scores all kTileBM rows against items [32 w, 32 w + 32) of the
// tile: 4 x 2 accumulators of v_mfma_f32_16x16x4_f32, all independent.  Lane l = (c = l & 15, q = l >> 4) holds
// A[row c][k = q] and B[k = q][item c]; one instruction adds k = 0, 1, 2, 3 in that order to the chain, so a 16-column group
// is four instructions and the chain runs over d ascending from +0 -- lgc_score_rows' chain (score_chain) with the query row
// the first factor.  Inside a 16-column group both LDS images hold column 4 j + q at position 4 q + j (store4_perm), so that
// the four operands lane quarter q needs (steps j = 0 .. 3) are ONE 16-byte read.  After a tile's last chunk acc[mi][nj][r]
// is the score of row 16 mi + 4 q + r against item 32 w + 16 nj + c.
#pragma once
#include "lgconv_common.h"

namespace {

constexpr int kTileBM = 64, kTileBN = 128, kTileKC = 32;
constexpr int kTileBS = kTileKC + 4;          // floats; (stride / 4) odd: 16 consecutive rows hit 16 different bank quads
constexpr int kTileStage = kTileBN * (kTileKC / 4) / kBlock;   // float4 groups of a chunk a thread holds
static_assert(kTileStage * kBlock == kTileBN * (kTileKC / 4), "a chunk is dealt evenly over the workgroup");

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int tile_dp(int dim) { return (dim + 15) & ~15; }
// floats of Qs and Bs together, the head of every user's dynamic LDS
inline size_t tile_lds_floats(int dp) { return (size_t)kTileBM * (dp + 4) + (size_t)kTileBN * kTileBS; }

// The slice count in use for `rows` query rows over `items` table rows: the one asked for, or with 0 the smallest that
// gives about 512 workgroups (two for every CU); never more than 64 or than there are item tiles.
inline int tile_slices(int64_t rows, int64_t items, int asked) {
    const int64_t item_tiles = (items + kTileBN - 1) / kTileBN, row_tiles = std::max<int64_t>(1, (rows + kTileBM - 1) / kTileBM);
    int64_t s = asked > 0 ? asked : (512 + row_tiles - 1) / row_tiles;
    s = std::min<int64_t>(s, 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, item_tiles));
}

// what the sliced entry points accept: 32-bit row and item counts, at least one item, 0 (= choose) to 64 slices
inline bool tile_sizes_ok(int64_t rows, int64_t items, int slices) {
    return rows >= 0 && items >= 1 && rows < INT32_MAX && items < INT32_MAX && slices >= 0 && slices <= 64;
}

// columns c0 .. c0 + 3 (c0 % 4 == 0) of a row image whose 16-column groups hold column 4 j + q at position 4 q + j
__device__ __forceinline__ void store4_perm(float *row, int c0, f4 v) {
    float *g = row + (c0 & ~15) + ((c0 & 15) >> 2);
    g[0] = v.x;
    g[4] = v.y;
    g[8] = v.z;
    g[12] = v.w;
}

// What a thread holds of the tile; the kernel makes one at its top, over the head of its dynamic LDS (tile_lds_floats).
struct Tile {
    float *Qs, *Bs;                           // [kTileBM][sq] and [kTileBN][kTileBS]
    int sq, tid, w, c, q;                     // sq = dp + 4; wavefront w, lane (c, q)
    f4 stage[kTileStage];                     // the chunk in flight
    f32x4 acc[4][2];

    __device__ __forceinline__ Tile(float *lds, int dp) : Qs(lds), Bs(lds + kTileBM * (dp + 4)), sq(dp + 4), tid(threadIdx.x) {
        const int lane = tid & (kWave - 1);
        w = tid >> 6;
        c = lane & 15;
        q = lane >> 4;
    }
    __device__ __forceinline__ float *lds_end() const { return Bs + kTileBN * kTileBS; }   // the unit's own LDS starts here

    // Qs <- the kTileBM query rows, whole width.  row_of(row) gives the row's index in `table`, negative for "no row": zeros,
    // and no address is formed from it.
    template <typename RowOf>
    __device__ __forceinline__ void stage_rows(const float *__restrict__ table, int64_t stride, int dim, RowOf row_of) {
        const int qgroups = (sq - 4) / 4;
        for (int e = tid; e < kTileBM * qgroups; e += kBlock) {
            const int row = e / qgroups, g = e - row * qgroups;
            const int id = row_of(row);
            store4_perm(Qs + row * sq, 4 * g, load4_if(table + (int64_t)max(id, 0) * stride, 4 * g, dim, id >= 0 && 4 * g < dim));
        }
    }

    // stage <- columns [32 ch, 32 ch + 32) of the tile's items.  item_of(it) gives the table row of the tile's item it,
    // negative for "none" (past the table's end, or an id the prologue has refused): zeros, nothing read.
    template <typename ItemOf>
    __device__ __forceinline__ void load_chunk(const float *__restrict__ table, int64_t stride, int dim, int ch, ItemOf item_of) {
#pragma unroll
        for (int i = 0; i < kTileStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            const int item = item_of(it), d = ch * kTileKC + 4 * g;
            stage[i] = load4_if(table + (int64_t)max(item, 0) * stride, d, dim, item >= 0 && d < dim);
        }
    }

    // Bs <- stage
    __device__ __forceinline__ void store_chunk() {
#pragma unroll
        for (int i = 0; i < kTileStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            store4_perm(Bs + it * kTileBS, 4 * g, stage[i]);
        }
    }

    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    // acc += Qs[:, chunk ch] . Bs^T for this wavefront's 32 items: the chunk's 16-column groups that lie below dp, ascending.
    // k_rank_sweep and k_sm_logits restate this loop in place: called, it costs them registers.
    __device__ __forceinline__ void product(int ch) {
        const int groups = min(kTileKC / 16, (sq - 4) / 16 - ch * (kTileKC / 16));
        for (int g = 0; g < groups; ++g) {
            f4 a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                a[mi] = *reinterpret_cast<const f4 *>(Qs + (16 * mi + c) * sq + ch * kTileKC + 16 * g + 4 * q);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
                b[nj] = *reinterpret_cast<const f4 *>(Bs + (32 * w + 16 * nj + c) * kTileBS + 16 * g + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], acc[mi][nj], 0, 0, 0);
        }
    }
};

}  // namespace

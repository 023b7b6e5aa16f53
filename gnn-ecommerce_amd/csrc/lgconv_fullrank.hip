// lgconv_fullrank.hip -- full-rank evaluation: the exact place of a held-out item among the whole catalogue, by counting.
// Per (user, item) pair the number of candidates that precede the item in lgc_mask_topk's total order; the users x catalogue
// dot products run on the fp32 matrix cores and no score is ever written to memory.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// Geometry: section 19's without the selection.  Three launches in stream order.
//   k_rank_thresholds  one lane per pair: the pair's own score, lgc_score_rows' chain in one lane; with lists a binary search
//                      says whether p is seen.  Writes the threshold m(u, p), zeroes the counters, voids a bad pair.
//   k_rank_sweep       a workgroup owns kFrBM pairs as query rows (the user row gathered through pair_users) and a slice of
//                      the catalogue, which passes through LDS in tiles of kFrBN items, each in chunks of kFrKC columns.
//                      Wavefront w scores all rows against items [32 w, 32 w + 32) of the tile with 4 x 2 accumulators of
//                      v_mfma_f32_16x16x4_f32 (the operand layout of lgconv_similar.hip: one instruction adds k = 0 .. 3 in
//                      order, so the sum is the chain over d ascending from +0).  A lane sees 16 distinct rows: their
//                      thresholds, items p and both counters stay in registers for the whole slice; the epilogue of a tile
//                      is one float compare a score, the exact key and index test only where that compare cannot decide.
//   k_rank_seen        only with lists, one wavefront per pair, lane = list entry in rounds of 64: takes back what the
//                      sweep counted for a seen item's raw score and, in mode ZERO, counts its masked score instead.
constexpr int kFrBM = 64, kFrBN = 128, kFrKC = 32;
constexpr int kFrBS = kFrKC + 4;              // floats; (stride / 4) odd: 16 consecutive rows hit 16 different bank quads
constexpr int kFrStage = kFrBN * (kFrKC / 4) / kBlock;   // float4 groups of a chunk a thread holds
constexpr int kFrRows = kBlock / kWave;       // pairs of a k_rank_seen workgroup
constexpr int kFrRowMax = 256;                // floats of a staged user row: lgc_dim_ok's widest, a multiple of 4
static_assert(kFrStage * kBlock == kFrBN * (kFrKC / 4), "a chunk is dealt evenly over the workgroup");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct FrArgs {
    const float *users, *items;
    int64_t user_stride, item_stride;
    const int64_t *pair_users, *pair_items, *seen_ptr, *seen_items;
    int32_t *rank, *n_equal, *n_cand;
    float *value;
    float *thr;                               // workspace: m(u, p) of every pair
    int32_t *status;
    int32_t n_user_rows, n_items, n_pairs, dim, dp;   // dp = dim rounded up to 16
    int32_t seen_mode, slices, item_tiles;
};

// lgc_mask_topk's total order (lgconv_serve.hip): ascending with the value, every NaN the one top key, -0 = +0
__device__ __forceinline__ uint32_t fr_order_key(float v) {
    const float w = __fadd_rn(v, 0.0f);
    const uint32_t u = __float_as_uint(w);
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return w != w ? 0xFFFFFFFFu : key;
}

// Four floats of a table row starting at column d (d % 4 == 0); columns >= dim read as 0 and are never touched (the row
// may end there: padding columns, the next row, or the end of the allocation).  VEC: the width is a multiple of 4 and every
// row starts on 16 bytes, one aligned 16-byte load.
template <bool VEC>
__device__ __forceinline__ f4 fr_load4(const float *__restrict__ row, int d, int dim) {
    if (VEC) return *reinterpret_cast<const f4 *>(row + d);
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (d + 4 <= dim) {
        v = *reinterpret_cast<const f4u *>(row + d);
    } else {
        if (d + 0 < dim) v.x = row[d + 0];
        if (d + 1 < dim) v.y = row[d + 1];
        if (d + 2 < dim) v.z = row[d + 2];
    }
    return v;
}

__device__ __forceinline__ f4 fr_load4_if(const float *__restrict__ row, int d, int dim, bool live) {
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (live) v = fr_load4<false>(row, d, dim);
    return v;
}

// columns c0 .. c0 + 3 (c0 % 4 == 0) of a row image whose 16-column groups hold column 4 j + q at position 4 q + j
__device__ __forceinline__ void fr_store4(float *row, int c0, f4 v) {
    float *g = row + (c0 & ~15) + ((c0 & 15) >> 2);
    g[0] = v.x;
    g[4] = v.y;
    g[8] = v.z;
    g[12] = v.w;
}

// does the item with key ki and index i precede the one with key kp and index p
__device__ __forceinline__ bool fr_precedes(uint32_t ki, int i, uint32_t kp, int p) { return ki > kp || (ki == kp && i < p); }

// ----------------------------------------------------------------------------------------
// thresholds: lane = pair
// ----------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_rank_thresholds(const FrArgs p) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= p.n_pairs) return;
    const int64_t u = p.pair_users[r], it = p.pair_items[r];
    if (u < 0 || u >= p.n_user_rows || it < 0 || it >= p.n_items) {   // range-checked before any address is formed
        atomicOr(p.status, LGC_ST_INDEX_OOB);
        p.rank[r] = -1;
        if (p.n_equal) p.n_equal[r] = -1;
        if (p.n_cand) p.n_cand[r] = 0;
        if (p.value) p.value[r] = 0.0f;
        p.thr[r] = 0.0f;
        return;
    }
    // lgc_score_rows' chain: v_fma over d = 0 .. groups * 4 - 1 ascending from +0, zeros past dim, the user's value the first
    // factor.  No step runs past groups * 4: fma(0, 0, -0) is +0, an extra step could change a sign.
    const float *urow = p.users + u * p.user_stride, *irow = p.items + it * p.item_stride;
    const int groups = (p.dim + 3) / 4;
    float acc = 0.0f;
    for (int g = 0; g < groups; ++g) {
        const f4 a = fr_load4<VEC>(urow, 4 * g, p.dim), b = fr_load4<VEC>(irow, 4 * g, p.dim);
        acc = __fmaf_rn(a.x, b.x, acc);
        acc = __fmaf_rn(a.y, b.y, acc);
        acc = __fmaf_rn(a.z, b.z, acc);
        acc = __fmaf_rn(a.w, b.w, acc);
    }
    bool seen = false;
    if (p.seen_ptr) {                                        // binary search in the ascending list; never leaves [b, e)
        const int64_t b = p.seen_ptr[u], e = p.seen_ptr[u + 1];
        int64_t lo = b, hi = e;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (p.seen_items[mid] < it) lo = mid + 1; else hi = mid;
        }
        seen = lo < e && p.seen_items[lo] == it;
    }
    const float m = (seen && p.seen_mode == LGC_RANK_SEEN_ZERO) ? __fmul_rn(acc, 0.0f) : acc;
    p.thr[r] = m;
    p.rank[r] = 0;                                           // the sweep adds to these; k_rank_seen voids a removed p
    if (p.n_equal) p.n_equal[r] = 0;
    if (p.n_cand) p.n_cand[r] = p.n_items;
    if (p.value) p.value[r] = m;
}

// ----------------------------------------------------------------------------------------
// the sweep
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rank_sweep(const FrArgs p) {
    extern __shared__ __attribute__((aligned(16))) float fr_lds[];
    const int sq = p.dp + 4, dim = p.dim;
    float *Qs = fr_lds;                                      // [kFrBM][sq]: the user rows of the pairs
    float *Bs = Qs + kFrBM * sq;                             // [kFrBN][kFrBS]: a chunk of the item tile
    float *thv = Bs + kFrBN * kFrBS;                         // [kFrBM]: m(u, p)
    int *pid = reinterpret_cast<int *>(thv + kFrBM);         // [kFrBM]: the item p of a row, -1 = no row
    int *uid = pid + kFrBM;                                  // [kFrBM]: its user row
    int *cntp = uid + kFrBM;                                 // [kFrBM]: candidates that precede p
    int *cnte = cntp + kFrBM;                                // [kFrBM]: candidates with p's key
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kFrBM;

    if (tid < kFrBM) {
        const int64_t r = row0 + tid;
        int64_t u = -1, it = -1;
        if (r < p.n_pairs) {
            u = p.pair_users[r];
            it = p.pair_items[r];
            if (u < 0 || u >= p.n_user_rows || it < 0 || it >= p.n_items) u = it = -1;   // k_rank_thresholds has said so
        }
        uid[tid] = (int)u;
        pid[tid] = (int)it;
        thv[tid] = it >= 0 ? p.thr[r] : INFINITY;
        cntp[tid] = 0;
        cnte[tid] = 0;
    }
    __syncthreads();
    const int qgroups = p.dp / 4;
    for (int e = tid; e < kFrBM * qgroups; e += kBlock) {
        const int row = e / qgroups, g = e - row * qgroups;
        const int u = uid[row];
        fr_store4(Qs + row * sq, 4 * g, fr_load4_if(p.users + (int64_t)max(u, 0) * p.user_stride, 4 * g, dim, u >= 0 && 4 * g < dim));
    }

    // this slice's item tiles, and the steps (tile, chunk) over them
    const int t_lo = (int)((int64_t)p.item_tiles * blockIdx.y / p.slices);
    const int t_hi = (int)((int64_t)p.item_tiles * (blockIdx.y + 1) / p.slices);
    const int nch = (p.dp + kFrKC - 1) / kFrKC;
    const int n_steps = (t_hi - t_lo) * nch;

    f4 stage[kFrStage];
    auto load_chunk = [&](int step) {
        const int tile = t_lo + step / nch, ch = step % nch;
#pragma unroll
        for (int i = 0; i < kFrStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            const uint32_t item = (uint32_t)tile * kFrBN + it;               // below 2^31 + 128: unsigned, no overflow
            const int d = ch * kFrKC + 4 * g;
            const bool live = item < (uint32_t)p.n_items && d < dim;
            stage[i] = fr_load4_if(p.items + (int64_t)(live ? item : 0) * p.item_stride, d, dim, live);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < kFrStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            fr_store4(Bs + it * kFrBS, 4 * g, stage[i]);
        }
    };

    // what a lane keeps of its 16 rows (row 16 mi + 4 q + r is x = 4 mi + r) for the whole slice
    float tv[16];
    int pp[16], prec[16], eq[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int row = 16 * (x >> 2) + 4 * q + (x & 3);
        tv[x] = thv[row];
        pp[x] = pid[row];
        prec[x] = 0;
        eq[x] = 0;
    }

    f32x4 acc[4][2];
    int item[2];
    bool iok[2];
    if (n_steps > 0) load_chunk(0);
    for (int step = 0; step < n_steps; ++step) {
        const int tile = t_lo + step / nch, ch = step % nch;
        if (ch == 0) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                const uint32_t col = (uint32_t)tile * kFrBN + 32 * w + 16 * nj + c;   // below 2^31 + 128: unsigned
                iok[nj] = col < (uint32_t)p.n_items;
                item[nj] = (int)col;                                 // counts only where iok
            }
        }
        __syncthreads();                                     // the previous chunk is consumed
        store_chunk();
        __syncthreads();                                     // also orders the user rows before their first use
        if (step + 1 < n_steps) load_chunk(step + 1);        // in flight during this chunk's products
        const int groups = min(kFrKC / 16, p.dp / 16 - ch * (kFrKC / 16));
        for (int g = 0; g < groups; ++g) {
            f4 a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                a[mi] = *reinterpret_cast<const f4 *>(Qs + (16 * mi + c) * sq + ch * kFrKC + 16 * g + 4 * q);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
                b[nj] = *reinterpret_cast<const f4 *>(Bs + (32 * w + 16 * nj + c) * kFrBS + 16 * g + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], acc[mi][nj], 0, 0, 0);
        }
        if (ch != nch - 1) continue;

        // The tile's scores are whole: lane (c, q) holds rows 16 mi + 4 q + r of items 32 w + 16 nj + c.  A score ABOVE its
        // row's threshold precedes p: one compare and an add.  A score neither above nor below it -- an equal value, either
        // zero against the other, a NaN on either side -- goes on to the exact test.  A column past n_items competes as
        // -inf, which is above nothing, and p itself is left out by its index.
        uint32_t rare = 0u;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                const float s = iok[nj] ? acc[x >> 2][nj][x & 3] : -INFINITY;
                const bool above = s > tv[x], below = s < tv[x];
                prec[x] += (above && item[nj] != pp[x]) ? 1 : 0;
                rare |= (above || below) ? 0u : 1u << (2 * x + nj);
            }
        }
        if (__ballot(rare != 0u) == 0ull) continue;          // the usual case, decided once for the wavefront
#pragma unroll
        for (int x = 0; x < 16; ++x) {
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                if (!(rare & (1u << (2 * x + nj)))) continue;
                if (!iok[nj] || item[nj] == pp[x]) continue;
                const uint32_t ks = fr_order_key(acc[x >> 2][nj][x & 3]), kt = fr_order_key(tv[x]);
                prec[x] += fr_precedes(ks, item[nj], kt, pp[x]) ? 1 : 0;
                eq[x] += ks == kt ? 1 : 0;
            }
        }
    }

    // a row's counts lie in the 16 lanes of a quarter, in four wavefronts: summed once, here
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        int a = prec[x], b = eq[x];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            a += __shfl_xor(a, m, kWave);
            b += __shfl_xor(b, m, kWave);
        }
        if (c == 0) {
            const int row = 16 * (x >> 2) + 4 * q + (x & 3);
            if (a) atomicAdd(&cntp[row], a);
            if (b) atomicAdd(&cnte[row], b);
        }
    }
    __syncthreads();
    if (tid < kFrBM && pid[tid] >= 0) {                      // integer sums: the order of the slices does not show
        const int64_t r = row0 + tid;
        if (cntp[tid]) atomicAdd(p.rank + r, cntp[tid]);
        if (p.n_equal && cnte[tid]) atomicAdd(p.n_equal + r, cnte[tid]);
    }
}

// ----------------------------------------------------------------------------------------
// the seen correction: wavefront = pair, lane = list entry
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int fr_wave_sum(int v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_rank_seen(const FrArgs p) {
    __shared__ __attribute__((aligned(16))) float fr_user[kFrRows][kFrRowMax];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = (int64_t)blockIdx.x * kFrRows + wv;    // the wavefront's pair
    const int groups = (p.dim + 3) / 4;
    int64_t u = -1, it = -1;
    if (r < p.n_pairs) {
        u = p.pair_users[r];
        it = p.pair_items[r];
        if (u < 0 || u >= p.n_user_rows || it < 0 || it >= p.n_items) u = it = -1;
    }
    const bool ok = u >= 0;
    {
        const float *urow = p.users + (ok ? u : 0) * p.user_stride;
        for (int d = lane; d < 4 * groups; d += kWave) fr_user[wv][d] = (ok && d < p.dim) ? urow[d] : 0.0f;
    }
    __syncthreads();                                         // the kernel's only barrier: every wavefront reaches it
    if (!ok) return;
    const float *ur = fr_user[wv];
    const int pi = (int)it;
    const uint32_t kt = fr_order_key(p.thr[r]);
    const int64_t b = p.seen_ptr[u], e = p.seen_ptr[u + 1];
    int d_rank = 0, d_eq = 0, n_seen = 0, p_seen = 0;
    for (int64_t j0 = b; j0 < e; j0 += kWave) {
        const int64_t j = j0 + lane;
        int64_t i = -1;
        if (j < e) {
            i = p.seen_items[j];
            if (i < 0 || i >= p.n_items || (j > b && p.seen_items[j - 1] == i)) i = -1;   // ignored; a repeat is skipped
        }
        if (i < 0) continue;
        n_seen += 1;
        if (i == it) {
            p_seen = 1;
            continue;
        }
        // the raw score of the seen item, lgc_score_rows' chain in this lane: the sweep compared these bits with p's
        const float *row = p.items + i * p.item_stride;
        float s = 0.0f;
        for (int g = 0; g < groups; ++g) {
            const f4 a = *reinterpret_cast<const f4 *>(ur + 4 * g), v = fr_load4<VEC>(row, 4 * g, p.dim);
            s = __fmaf_rn(a.x, v.x, s);
            s = __fmaf_rn(a.y, v.y, s);
            s = __fmaf_rn(a.z, v.z, s);
            s = __fmaf_rn(a.w, v.w, s);
        }
        const uint32_t ks = fr_order_key(s);
        d_rank -= fr_precedes(ks, (int)i, kt, pi) ? 1 : 0;
        d_eq -= ks == kt ? 1 : 0;
        if (p.seen_mode == LGC_RANK_SEEN_ZERO) {
            const uint32_t km = fr_order_key(__fmul_rn(s, 0.0f));
            d_rank += fr_precedes(km, (int)i, kt, pi) ? 1 : 0;
            d_eq += km == kt ? 1 : 0;
        }
    }
    d_rank = fr_wave_sum(d_rank);
    d_eq = fr_wave_sum(d_eq);
    n_seen = fr_wave_sum(n_seen);
    p_seen = fr_wave_sum(p_seen);
    if (lane != 0) return;
    const bool remove = p.seen_mode == LGC_RANK_SEEN_REMOVE;
    if (remove && p_seen) {                                  // p is no candidate: a property of the data, not an error
        p.rank[r] = -1;
        if (p.n_equal) p.n_equal[r] = -1;
    } else {
        if (d_rank) p.rank[r] += d_rank;
        if (p.n_equal && d_eq) p.n_equal[r] += d_eq;
    }
    if (remove && p.n_cand) p.n_cand[r] = p.n_items - n_seen;
}

bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// The slice count in use: the one asked for, or with 0 the smallest that gives about 512 workgroups (two for every CU);
// never more than there are item tiles.
inline int fr_slices(int64_t n_pairs, int64_t n_items, int slices) {
    const int64_t item_tiles = (n_items + kFrBN - 1) / kFrBN, row_tiles = std::max<int64_t>(1, (n_pairs + kFrBM - 1) / kFrBM);
    int64_t s = slices > 0 ? slices : (512 + row_tiles - 1) / row_tiles;
    s = std::min<int64_t>(s, 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, item_tiles));
}

inline bool fr_sizes_ok(int64_t n_pairs, int64_t n_items, int slices) {
    return n_pairs >= 0 && n_items >= 1 && n_pairs < INT32_MAX && n_items < INT32_MAX && slices >= 0 && slices <= 64;
}

unsigned long long lds_ok_rank_sweep;

}  // namespace

extern "C" {

size_t lgc_rank_positions_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t slices) {
    if (!fr_sizes_ok(n_pairs, n_items, slices)) return 0;
    return (size_t)n_pairs * sizeof(float);                  // the thresholds; the slices add to the outputs themselves
}

int lgc_rank_positions(const float *users, int64_t user_stride, int64_t n_user_rows, const float *items, int64_t item_stride,
                       int64_t n_items, int32_t dim, const int64_t *pair_users, const int64_t *pair_items, int64_t n_pairs,
                       const int64_t *seen_ptr, const int64_t *seen_items, int32_t seen_mode, int32_t slices, int32_t *rank,
                       int32_t *n_equal, int32_t *n_cand, float *value, void *workspace, size_t workspace_bytes,
                       int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!users || !items || !pair_users || !pair_items || !rank || !status || n_pairs < 0 || n_user_rows < 0 ||
        user_stride < dim || item_stride < dim || (seen_mode != LGC_RANK_SEEN_ZERO && seen_mode != LGC_RANK_SEEN_REMOVE) ||
        (seen_ptr && !seen_items))
        return LGC_E_INVAL;
    if (!fr_sizes_ok(n_pairs, n_items, slices) || n_user_rows >= INT32_MAX) return LGC_E_RANGE;
    if (!seen_ptr) seen_items = nullptr;                     // ignored without lists, its alignment too
    if (!aligned_to(users, 4) || !aligned_to(items, 4) || !aligned_to(rank, 4) || !aligned_to(n_equal, 4) ||
        !aligned_to(n_cand, 4) || !aligned_to(value, 4) || !aligned_to(workspace, 4) || !aligned_to(status, 4) ||
        !aligned_to(pair_users, 8) || !aligned_to(pair_items, 8) || !aligned_to(seen_ptr, 8) || !aligned_to(seen_items, 8))
        return LGC_E_ALIGN;
    const size_t need = (size_t)n_pairs * sizeof(float);
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    if (n_pairs == 0) return 0;

    FrArgs p{};
    p.users = users;
    p.items = items;
    p.user_stride = user_stride;
    p.item_stride = item_stride;
    p.pair_users = pair_users;
    p.pair_items = pair_items;
    p.seen_ptr = seen_ptr;
    p.seen_items = seen_items;
    p.rank = rank;
    p.n_equal = n_equal;
    p.n_cand = n_cand;
    p.value = value;
    p.thr = reinterpret_cast<float *>(workspace);
    p.status = status;
    p.n_user_rows = (int32_t)n_user_rows;
    p.n_items = (int32_t)n_items;
    p.n_pairs = (int32_t)n_pairs;
    p.dim = dim;
    p.dp = (dim + 15) & ~15;
    p.seen_mode = seen_mode;
    p.slices = fr_slices(n_pairs, n_items, slices);
    p.item_tiles = (int32_t)((n_items + kFrBN - 1) / kFrBN);
    hipStream_t stream = as_stream(stream_);
    const bool vec = dim % 4 == 0 && user_stride % 4 == 0 && item_stride % 4 == 0 && aligned_to(users, 16) && aligned_to(items, 16);

    hipLaunchKernelGGL(vec ? k_rank_thresholds<true> : k_rank_thresholds<false>, dim3(ceil_div(n_pairs, kBlock)), dim3(kBlock),
                       0, stream, p);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;

    const size_t lds = sizeof(float) * ((size_t)kFrBM * (p.dp + 4) + (size_t)kFrBN * kFrBS + kFrBM) + sizeof(int) * 4 * kFrBM;
    if (lds > 48 * 1024) {
        const int rc_attr = allow_big_lds(reinterpret_cast<const void *>(k_rank_sweep), 96 * 1024, &lds_ok_rank_sweep);
        if (rc_attr != 0) return rc_attr;
    }
    const int64_t row_tiles = (n_pairs + kFrBM - 1) / kFrBM;
    hipLaunchKernelGGL(k_rank_sweep, dim3((unsigned)row_tiles, (unsigned)p.slices), dim3(kBlock), lds, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0 || !seen_ptr) return rc;

    hipLaunchKernelGGL(vec ? k_rank_seen<true> : k_rank_seen<false>, dim3(ceil_div(n_pairs, kFrRows)), dim3(kBlock), 0, stream, p);
    return (int)hipGetLastError();
}

}  // extern "C"

// lgconv_fullrank.hip -- full-rank evaluation: the exact place of a held-out item among the whole catalogue, by counting.
// Per (user, item) pair the number of candidates that precede the item in lgc_mask_topk's total order; the users x catalogue
// dot products run on the fp32 matrix cores and no score is ever written to memory.
// C ABI: include/lgconv_hip.h
#include "lgconv_tile.h"

namespace {

// Geometry.  Three launches in stream order.
//   k_rank_thresholds  one lane per pair: the pair's own score, lgc_score_rows' chain in one lane; with lists a binary search
//                      says whether p is seen.  Writes the threshold m(u, p), zeroes the counters, voids a bad pair.
//   k_rank_sweep       the tile of lgconv_tile.h: a workgroup owns kTileBM pairs as query rows (the user row gathered
//                      through pair_users) and a slice of the catalogue's tiles.  A lane sees 16 distinct rows: their
//                      thresholds, items p and both counters stay in registers for the whole slice; the epilogue of a tile
//                      is one float compare a score, the exact key and index test only where that compare cannot decide.
//   k_rank_seen        only with lists, one wavefront per pair, lane = list entry in rounds of 64: takes back what the
//                      sweep counted for a seen item's raw score and, in mode ZERO, counts its masked score instead.
constexpr int kFrRows = kBlock / kWave;       // pairs of a k_rank_seen workgroup
constexpr int kFrRowMax = 256;                // floats of a staged user row: lgc_dim_ok's widest, a multiple of 4

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

// order_key's total order: does the item with key ki and index i precede the one with key kp and index p
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
    // lgc_score_rows' chain (score_chain) in this lane, the user's value the first factor
    const float *urow = p.users + u * p.user_stride, *irow = p.items + it * p.item_stride;
    const int groups = (p.dim + 3) / 4;
    float acc = 0.0f;
    for (int g = 0; g < groups; ++g) acc = score_chain(load4<VEC>(urow, 4 * g, p.dim), load4<VEC>(irow, 4 * g, p.dim), acc);
    bool seen = false;
    if (p.seen_ptr) seen = in_sorted(p.seen_items, p.seen_ptr[u], p.seen_ptr[u + 1], it);
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
    const int dim = p.dim;
    Tile tl(fr_lds, p.dp);                                   // Qs: the user rows of the pairs; Bs: a chunk of the item tile
    float *thv = tl.lds_end();                               // [kTileBM]: m(u, p)
    int *pid = reinterpret_cast<int *>(thv + kTileBM);       // [kTileBM]: the item p of a row, -1 = no row
    int *uid = pid + kTileBM;                                // [kTileBM]: its user row
    int *cntp = uid + kTileBM;                               // [kTileBM]: candidates that precede p
    int *cnte = cntp + kTileBM;                              // [kTileBM]: candidates with p's key
    const int tid = tl.tid, w = tl.w, c = tl.c, q = tl.q;
    const int64_t row0 = (int64_t)blockIdx.x * kTileBM;

    if (tid < kTileBM) {
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
    tl.stage_rows(p.users, p.user_stride, dim, [&](int row) { return uid[row]; });

    // this slice's item tiles, and the steps (tile, chunk) over them
    const int t_lo = (int)((int64_t)p.item_tiles * blockIdx.y / p.slices);
    const int t_hi = (int)((int64_t)p.item_tiles * (blockIdx.y + 1) / p.slices);
    const int nch = (p.dp + kTileKC - 1) / kTileKC;
    const int n_steps = (t_hi - t_lo) * nch;

    auto load_chunk = [&](int step) {
        const int tile = t_lo + step / nch;
        tl.load_chunk(p.items, p.item_stride, dim, step % nch, [&](int it) {
            const uint32_t item = (uint32_t)tile * kTileBN + it;                 // below 2^31 + 128: unsigned, no overflow
            return item < (uint32_t)p.n_items ? (int)item : -1;
        });
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

    int item[2];
    bool iok[2];
    if (n_steps > 0) load_chunk(0);
    for (int step = 0; step < n_steps; ++step) {
        const int tile = t_lo + step / nch, ch = step % nch;
        if (ch == 0) {
            tl.reset();
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                const uint32_t col = (uint32_t)tile * kTileBN + 32 * w + 16 * nj + c;   // below 2^31 + 128: unsigned
                iok[nj] = col < (uint32_t)p.n_items;
                item[nj] = (int)col;                                 // counts only where iok
            }
        }
        __syncthreads();                                     // the previous chunk is consumed
        tl.store_chunk();
        __syncthreads();                                     // also orders the user rows before their first use
        if (step + 1 < n_steps) load_chunk(step + 1);        // in flight during this chunk's products
        // Tile::product (lgconv_tile.h), restated: as a call it costs this kernel 28 VGPRs and 4 % of its time (DESIGN.md
        // section 12a)
        const int groups = min(kTileKC / 16, p.dp / 16 - ch * (kTileKC / 16));
        for (int g = 0; g < groups; ++g) {
            f4 a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                a[mi] = *reinterpret_cast<const f4 *>(tl.Qs + (16 * mi + c) * tl.sq + ch * kTileKC + 16 * g + 4 * q);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
                b[nj] = *reinterpret_cast<const f4 *>(tl.Bs + (32 * w + 16 * nj + c) * kTileBS + 16 * g + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        tl.acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], tl.acc[mi][nj], 0, 0, 0);
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
                const float s = iok[nj] ? tl.acc[x >> 2][nj][x & 3] : -INFINITY;
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
                const uint32_t ks = order_key(tl.acc[x >> 2][nj][x & 3]), kt = order_key(tv[x]);
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
    if (tid < kTileBM && pid[tid] >= 0) {                      // integer sums: the order of the slices does not show
        const int64_t r = row0 + tid;
        if (cntp[tid]) atomicAdd(p.rank + r, cntp[tid]);
        if (p.n_equal && cnte[tid]) atomicAdd(p.n_equal + r, cnte[tid]);
    }
}

// ----------------------------------------------------------------------------------------
// the seen correction: wavefront = pair, lane = list entry
// ----------------------------------------------------------------------------------------
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
    const uint32_t kt = order_key(p.thr[r]);
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
            const f4 a = *reinterpret_cast<const f4 *>(ur + 4 * g), v = load4<VEC>(row, 4 * g, p.dim);
            s = score_chain(a, v, s);
        }
        const uint32_t ks = order_key(s);
        d_rank -= fr_precedes(ks, (int)i, kt, pi) ? 1 : 0;
        d_eq -= ks == kt ? 1 : 0;
        if (p.seen_mode == LGC_RANK_SEEN_ZERO) {
            const uint32_t km = order_key(__fmul_rn(s, 0.0f));
            d_rank += fr_precedes(km, (int)i, kt, pi) ? 1 : 0;
            d_eq += km == kt ? 1 : 0;
        }
    }
    d_rank = wave_sum(d_rank);
    d_eq = wave_sum(d_eq);
    n_seen = wave_sum(n_seen);
    p_seen = wave_sum(p_seen);
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

unsigned long long lds_ok_rank_sweep;

}  // namespace

extern "C" {

size_t lgc_rank_positions_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t slices) {
    if (!tile_sizes_ok(n_pairs, n_items, slices)) return 0;
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
    if (!tile_sizes_ok(n_pairs, n_items, slices) || n_user_rows >= INT32_MAX) return LGC_E_RANGE;
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
    p.dp = tile_dp(dim);
    p.seen_mode = seen_mode;
    p.slices = tile_slices(n_pairs, n_items, slices);
    p.item_tiles = (int32_t)((n_items + kTileBN - 1) / kTileBN);
    hipStream_t stream = as_stream(stream_);
    const bool vec = dim % 4 == 0 && user_stride % 4 == 0 && item_stride % 4 == 0 && aligned_to(users, 16) && aligned_to(items, 16);

    hipLaunchKernelGGL(vec ? k_rank_thresholds<true> : k_rank_thresholds<false>, dim3(ceil_div(n_pairs, kBlock)), dim3(kBlock),
                       0, stream, p);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;

    const size_t lds = sizeof(float) * (tile_lds_floats(p.dp) + kTileBM) + sizeof(int) * 4 * kTileBM;
    rc = allow_lds(reinterpret_cast<const void *>(k_rank_sweep), lds, 48 * 1024, 96 * 1024, &lds_ok_rank_sweep);
    if (rc != 0) return rc;
    const int64_t row_tiles = (n_pairs + kTileBM - 1) / kTileBM;
    hipLaunchKernelGGL(k_rank_sweep, dim3((unsigned)row_tiles, (unsigned)p.slices), dim3(kBlock), lds, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0 || !seen_ptr) return rc;

    hipLaunchKernelGGL(vec ? k_rank_seen<true> : k_rank_seen<false>, dim3(ceil_div(n_pairs, kFrRows)), dim3(kBlock), 0, stream, p);
    return (int)hipGetLastError();
}

}  // extern "C"

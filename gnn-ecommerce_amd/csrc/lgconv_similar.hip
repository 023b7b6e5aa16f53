// lgconv_similar.hip -- similar items: the k nearest rows of the item table by dot product or cosine, scored on the fp32
// matrix cores and selected in the same launch; no score is ever written to memory.
// C ABI: include/lgconv_hip.h
#include "lgconv_select.h"
#include "lgconv_tile.h"

namespace {

// Geometry: the tile of lgconv_tile.h.  A workgroup owns kTileBM query rows, gathered through
// query_ids, and a slice of the catalogue's tiles; the epilogue of a tile selects.
constexpr int kNbRowsPerWave = kTileBM / (kBlock / kWave);
static_assert(LGC_NEIGHBORS_MAX_K <= kSelectMaxK, "compact_row holds a buffer in two registers a lane");

struct NbArgs {
    const float *items;
    int64_t item_stride;
    const int64_t *query_ids;
    const float *scale;
    const uint8_t *item_ok;
    int64_t *out_index;
    float *out_value;
    u64 *ws;
    int32_t *status;
    int32_t n_items, n_queries, dim, dp;      // dp = dim rounded up to 16
    int32_t exclude_self, k, slices, cap, item_tiles;
};

__global__ __launch_bounds__(kBlock) void k_item_neighbors(const NbArgs p) {
    extern __shared__ __attribute__((aligned(16))) float nb_lds[];
    const int cap = p.cap, k = p.k, dim = p.dim;
    Tile tl(nb_lds, p.dp);                                   // Qs: the query rows; Bs: a chunk of the item tile
    u64 *buf = reinterpret_cast<u64 *>(tl.lds_end());        // [kTileBM][cap]: the candidates of a row
    u64 *thr = buf + kTileBM * cap;                          // [kTileBM]: what a new candidate has to beat
    int *cnt = reinterpret_cast<int *>(thr + kTileBM);       // [kTileBM]
    int *qid = cnt + kTileBM;                                // [kTileBM]: the item a row asks about, -1 = no row
    float *qsc = reinterpret_cast<float *>(qid + kTileBM);   // [kTileBM]: scale[query]
    float *thv = qsc + kTileBM;                              // [kTileBM]: the value of thr's key (-inf while there is none)
    const int tid = tl.tid, lane = tid & (kWave - 1), w = tl.w, c = tl.c, q = tl.q;
    const int64_t row0 = (int64_t)blockIdx.x * kTileBM;

    if (tid < kTileBM) {
        const int64_t r = row0 + tid;
        int64_t id = -1;
        if (r < p.n_queries) {
            id = p.query_ids ? p.query_ids[r] : r;
            if (id < 0 || id >= p.n_items) {                 // range-checked before any address is formed from it
                atomicOr(p.status, LGC_ST_INDEX_OOB);
                id = -1;
            }
        }
        qid[tid] = (int)id;
        qsc[tid] = (id >= 0 && p.scale) ? p.scale[id] : 1.0f;
        cnt[tid] = 0;
        thr[tid] = 0ull;
        thv[tid] = -INFINITY;
    }
    __syncthreads();
    tl.stage_rows(p.items, p.item_stride, dim, [&](int row) { return qid[row]; });

    // this slice's item tiles, and the steps (tile, chunk) over them
    const int t_lo = (int)((int64_t)p.item_tiles * blockIdx.y / p.slices);
    const int t_hi = (int)((int64_t)p.item_tiles * (blockIdx.y + 1) / p.slices);
    const int nch = (p.dp + kTileKC - 1) / kTileKC;
    const int n_steps = (t_hi - t_lo) * nch;

    auto load_chunk = [&](int step) {
        const int tile = t_lo + step / nch;
        tl.load_chunk(p.items, p.item_stride, dim, step % nch, [&](int it) {
            const uint32_t item = (uint32_t)tile * kTileBN + it;                   // below 2^31 + 128: unsigned, no overflow
            return item < (uint32_t)p.n_items ? (int)item : -1;
        });
    };

    int item[2];
    bool iok[2];
    float isc[2];
    if (n_steps > 0) load_chunk(0);
    for (int step = 0; step < n_steps; ++step) {
        const int tile = t_lo + step / nch, ch = step % nch;
        if (ch == 0) {
            tl.reset();
            // what the epilogue needs of this lane's two items, requested a whole tile of products ahead
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                item[nj] = tile * kTileBN + 32 * w + 16 * nj + c;
                const bool inside = (uint32_t)item[nj] < (uint32_t)p.n_items;   // below 2^31 + 128: compared unsigned
                iok[nj] = inside && (!p.item_ok || p.item_ok[item[nj]] != 0);
                isc[nj] = (p.scale && inside) ? p.scale[item[nj]] : 1.0f;
            }
        }
        __syncthreads();                                     // the previous chunk is consumed
        tl.store_chunk();
        __syncthreads();                                     // also orders the query rows before their first use
        if (step + 1 < n_steps) load_chunk(step + 1);        // in flight during this chunk's products
        tl.product(ch);
        if (ch != nch - 1) continue;

        // The tile's scores are whole: lane (c, q) holds rows 16 mi + 4 q + r of items 32 w + 16 nj + c.  First the filter,
        // two multiplies and a compare per score: a score BELOW the value of its row's threshold is dropped in registers
        // (a NaN, an equal value and either zero against the other are not below: they go on to the exact comparison).
        uint32_t todo = 0u;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mi + 4 * q + r;
                const float tv = thv[row], rs = qsc[row];
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) {
                    float s = tl.acc[mi][nj][r];
                    if (p.scale) s = __fmul_rn(__fmul_rn(s, rs), isc[nj]);
                    tl.acc[mi][nj][r] = s;
                    todo |= (s < tv) ? 0u : 1u << ((mi * 4 + r) * 2 + nj);
                }
            }
        }
        // The rest, rare once the thresholds have risen: a candidate that beats the row's threshold in the total order
        // goes to the row's buffer.  A lane whose row is full keeps its candidate, the full rows are compacted, and it
        // tries again: no candidate is ever lost, so the result does not depend on the order of arrival.
        while (true) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                if (__ballot((todo >> (8 * mi)) & 0xFFu) == 0ull) continue;   // the usual case, decided once for the wavefront
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj) {
                        const uint32_t bit = 1u << ((mi * 4 + r) * 2 + nj);
                        if (!(todo & bit)) continue;
                        const int row = 16 * mi + 4 * q + r;
                        const int id = qid[row];
                        bool pending = false;
                        if (id >= 0 && iok[nj] && !(p.exclude_self && item[nj] == id)) {
                            const u64 e = pack_candidate(tl.acc[mi][nj][r], item[nj]);
                            if (e > thr[row]) {
                                const int pos = atomicAdd(&cnt[row], 1);
                                if (pos < cap) buf[row * cap + pos] = e;
                                else pending = true;
                            }
                        }
                        if (!pending) todo &= ~bit;
                    }
                }
            }
            if (!__syncthreads_or(todo != 0u)) break;        // block-uniform
            for (int rr = 0; rr < kNbRowsPerWave; ++rr) {
                const int row = kNbRowsPerWave * w + rr;
                const int n = cnt[row];                      // the same for every lane of the wavefront
                if (n >= cap) {
                    const int m = compact_row(buf + row * cap, cap, k, lane, thr + row, thv + row);
                    if (lane == 0) cnt[row] = m;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // every row sorted, its k best out: to the result, or to this slice's place in the workspace
    for (int rr = 0; rr < kNbRowsPerWave; ++rr) {
        const int row = kNbRowsPerWave * w + rr;
        const int64_t r = row0 + row;
        if (r >= p.n_queries) break;                         // the same for every lane
        const int m = compact_row(buf + row * cap, min(cnt[row], cap), k, lane, nullptr, nullptr);
        if (lane < k) {
            const u64 e = lane < m ? buf[row * cap + lane] : 0ull;
            if (p.slices == 1) write_candidate(p.out_index, p.out_value, r * k + lane, e);
            else p.ws[(r * p.slices + blockIdx.y) * k + lane] = e;
        }
    }
}

// One wavefront per query row merges the slices' candidates (merge_row).
__global__ __launch_bounds__(kBlock) void k_neighbors_merge(const NbArgs p) {
    __shared__ u64 mbuf[kBlock / kWave][kNbCapMax];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, k = p.k;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + w;
    if (r >= p.n_queries) return;
    merge_row(mbuf[w], p.ws + r * p.slices * k, p.slices * k, k, lane, p.out_index, p.out_value, r * k);
}

// ss = one chain of fused multiply-adds over d ascending from +0; out = 1 / sqrt(ss), both correctly rounded, inf -> 0
__global__ __launch_bounds__(kBlock) void k_row_rnorm(const float *__restrict__ table, int64_t stride, int64_t n_rows,
                                                     int32_t dim, float *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    const float *row = table + r * stride;
    float ss = 0.0f;
    for (int d = 0; d < dim; ++d) {
        const float x = row[d];
        ss = __fmaf_rn(x, x, ss);
    }
    float v = __fdiv_rn(1.0f, __fsqrt_rn(ss));
    if (v == INFINITY) v = 0.0f;
    out[r] = v;
}

inline bool nb_sizes_ok(int64_t n_queries, int64_t n_items, int k, int slices) {
    return tile_sizes_ok(n_queries, n_items, slices) && k >= 1 && k <= LGC_NEIGHBORS_MAX_K;
}

unsigned long long lds_ok_neighbors;

}  // namespace

extern "C" {

int lgc_row_rnorm(const float *table, int64_t stride, int64_t n_rows, int32_t dim, float *out, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!table || !out || n_rows < 0 || stride < dim) return LGC_E_INVAL;
    if (n_rows >= INT32_MAX) return LGC_E_RANGE;
    if (!aligned_to(table, 4) || !aligned_to(out, 4)) return LGC_E_ALIGN;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_row_rnorm, dim3(ceil_div(n_rows, kBlock)), dim3(kBlock), 0, as_stream(stream_), table, stride,
                       n_rows, dim, out);
    return (int)hipGetLastError();
}

size_t lgc_item_neighbors_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t slices) {
    if (!nb_sizes_ok(n_queries, n_items, k, slices)) return 0;
    const int64_t item_tiles = (n_items + kTileBN - 1) / kTileBN;
    int64_t places;                                          // candidate lists of k places
    if (slices > 0) {
        const int64_t s = std::min<int64_t>(slices, item_tiles);
        places = s > 1 ? n_queries * s : 0;
    } else {
        // what the chosen count needs is not monotonic in n_queries (more row tiles, fewer slices); its two bounds are
        const int64_t s_max = std::min<int64_t>(64, item_tiles);
        places = s_max > 1 ? std::min<int64_t>(n_queries * s_max, n_queries + 512 * (int64_t)kTileBM) : 0;
    }
    return (size_t)places * (size_t)k * sizeof(u64);
}

int lgc_item_neighbors(const float *items, int64_t item_stride, int64_t n_items, int32_t dim, const int64_t *query_ids,
                       int64_t n_queries, const float *scale, const uint8_t *item_ok, int32_t exclude_self, int32_t k,
                       int32_t slices, int64_t *out_index, float *out_value, void *workspace, size_t workspace_bytes,
                       int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!items || !out_index || !status || n_queries < 0 || item_stride < dim || (exclude_self != 0 && exclude_self != 1))
        return LGC_E_INVAL;
    if (!nb_sizes_ok(n_queries, n_items, k, slices)) return LGC_E_RANGE;
    if (!aligned_to(items, 4) || !aligned_to(scale, 4) || !aligned_to(out_value, 4) || !aligned_to(out_index, 8) ||
        !aligned_to(workspace, 8))
        return LGC_E_ALIGN;
    const int s = tile_slices(n_queries, n_items, slices);
    const size_t need = s > 1 ? (size_t)n_queries * s * k * sizeof(u64) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    if (n_queries == 0) return 0;

    NbArgs p{};
    p.items = items;
    p.item_stride = item_stride;
    p.query_ids = query_ids;
    p.scale = scale;
    p.item_ok = item_ok;
    p.out_index = out_index;
    p.out_value = out_value;
    p.ws = reinterpret_cast<u64 *>(workspace);
    p.status = status;
    p.n_items = (int32_t)n_items;
    p.n_queries = (int32_t)n_queries;
    p.dim = dim;
    p.dp = tile_dp(dim);
    p.exclude_self = exclude_self;
    p.k = k;
    p.slices = s;
    p.cap = select_cap(k);
    p.item_tiles = (int32_t)((n_items + kTileBN - 1) / kTileBN);
    const size_t lds = sizeof(float) * tile_lds_floats(p.dp) + sizeof(u64) * ((size_t)kTileBM * p.cap + kTileBM) +
                       (sizeof(int) * 2 + sizeof(float) * 2) * kTileBM;
    int rc = allow_lds(reinterpret_cast<const void *>(k_item_neighbors), lds, 48 * 1024, 144 * 1024, &lds_ok_neighbors);
    if (rc != 0) return rc;
    const int64_t row_tiles = (n_queries + kTileBM - 1) / kTileBM;
    hipLaunchKernelGGL(k_item_neighbors, dim3((unsigned)row_tiles, (unsigned)s), dim3(kBlock), lds, as_stream(stream_), p);
    rc = (int)hipGetLastError();
    if (rc != 0 || s == 1) return rc;
    hipLaunchKernelGGL(k_neighbors_merge, dim3((unsigned)ceil_div(n_queries, kBlock / kWave)), dim3(kBlock), 0,
                       as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

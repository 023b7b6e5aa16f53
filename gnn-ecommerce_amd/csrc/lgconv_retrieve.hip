// lgconv_retrieve.hip -- cross-table retrieval: per query row of one table the k best rows of another (user -> items with
// the catalogue filter and the purchase lists removed, item -> users for an audience, user -> users), scored on the fp32
// matrix cores and selected in the same launch; no score is ever written to memory.
// C ABI: include/lgconv_hip.h
#include "lgconv_select.h"
#include "lgconv_tile.h"

namespace {

// Geometry (DESIGN.md sections 19 and 26): the tile of lgconv_tile.h and the selection of lgconv_select.h.  A workgroup owns
// kTileBM query rows, gathered through query_ids from the query table, and a range of the candidate table's tiles; the
// epilogue of a tile selects.  What is this unit's own: two tables, one scale per side, the skipped id and the exclusion
// list of a row -- a binary search that only a candidate which already beats its row's threshold pays for.
constexpr int kRtRowsPerWave = kTileBM / (kBlock / kWave);
static_assert(LGC_RETRIEVE_MAX_K <= kSelectMaxK, "compact_row holds a buffer in two registers a lane");

struct RtArgs {
    const float *queries;
    const float *cands;
    int64_t query_stride, cand_stride;
    const int64_t *query_ids;
    const float *query_scale;
    const float *cand_scale;
    const uint8_t *cand_ok;
    const int64_t *list_ptr;
    const int64_t *list_items;
    const int64_t *list_rows;
    const int64_t *skip_id;
    int64_t *out_index;
    float *out_value;
    u64 *ws;
    int32_t *status;
    int32_t n_query_rows, n_cand, n_queries, n_lists, dim, dp;   // dp = dim rounded up to 16
    int32_t k, slices, cap, cand_tiles;
};

__global__ __launch_bounds__(kBlock) void k_retrieve(const RtArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rt_lds[];
    const int cap = p.cap, k = p.k, dim = p.dim;
    Tile tl(rt_lds, p.dp);                                   // Qs: the query rows; Bs: a chunk of the candidate tile
    u64 *buf = reinterpret_cast<u64 *>(tl.lds_end());        // [kTileBM][cap]: the candidates of a row
    u64 *thr = buf + kTileBM * cap;                          // [kTileBM]: what a new candidate has to beat
    int64_t *lb = reinterpret_cast<int64_t *>(thr + kTileBM);   // [kTileBM]: the row's exclusion list is list_items[lb, le)
    int64_t *le = lb + kTileBM;                              // [kTileBM]
    int *cnt = reinterpret_cast<int *>(le + kTileBM);        // [kTileBM]
    int *qid = cnt + kTileBM;                                // [kTileBM]: the row of the query table, -1 = no row
    int *skp = qid + kTileBM;                                // [kTileBM]: the candidate the row skips, -1 = none
    float *qsc = reinterpret_cast<float *>(skp + kTileBM);   // [kTileBM]: query_scale[id]
    float *thv = qsc + kTileBM;                              // [kTileBM]: the value of thr's key (-inf while there is none)
    const int tid = tl.tid, lane = tid & (kWave - 1), w = tl.w, c = tl.c, q = tl.q;
    const int64_t row0 = (int64_t)blockIdx.x * kTileBM;

    if (tid < kTileBM) {
        const int64_t r = row0 + tid;
        int64_t id = -1, b = 0, e = 0, skip = -1;
        if (r < p.n_queries) {
            id = p.query_ids ? p.query_ids[r] : r;
            if (id < 0 || id >= p.n_query_rows) {            // range-checked before any address is formed from it
                atomicOr(p.status, LGC_ST_INDEX_OOB);
                id = -1;
            }
            if (id >= 0 && p.list_ptr) {
                const int64_t l = p.list_rows ? p.list_rows[r] : id;
                if (l >= 0 && l < p.n_lists) {
                    b = p.list_ptr[l];
                    e = p.list_ptr[l + 1];
                } else if (l != -1) {                        // a filter that cannot be found: the row is not answered
                    atomicOr(p.status, LGC_ST_INDEX_OOB);
                    id = -1;
                }
            }
            if (p.skip_id) {
                skip = p.skip_id[r];
                if (skip < 0 || skip >= p.n_cand) skip = -1;
            }
        }
        qid[tid] = (int)id;
        skp[tid] = (int)skip;
        lb[tid] = b;
        le[tid] = e;
        qsc[tid] = (id >= 0 && p.query_scale) ? p.query_scale[id] : 1.0f;
        cnt[tid] = 0;
        thr[tid] = 0ull;
        thv[tid] = -INFINITY;
    }
    __syncthreads();
    tl.stage_rows(p.queries, p.query_stride, dim, [&](int row) { return qid[row]; });

    // this range's candidate tiles, and the steps (tile, chunk) over them
    const int t_lo = (int)((int64_t)p.cand_tiles * blockIdx.y / p.slices);
    const int t_hi = (int)((int64_t)p.cand_tiles * (blockIdx.y + 1) / p.slices);
    const int nch = (p.dp + kTileKC - 1) / kTileKC;
    const int n_steps = (t_hi - t_lo) * nch;

    auto load_chunk = [&](int step) {
        const int tile = t_lo + step / nch;
        tl.load_chunk(p.cands, p.cand_stride, dim, step % nch, [&](int it) {
            const uint32_t cand = (uint32_t)tile * kTileBN + it;                   // below 2^31 + 128: unsigned, no overflow
            return cand < (uint32_t)p.n_cand ? (int)cand : -1;
        });
    };

    int cand[2];
    bool cok[2];
    float csc[2];
    if (n_steps > 0) load_chunk(0);
    for (int step = 0; step < n_steps; ++step) {
        const int tile = t_lo + step / nch, ch = step % nch;
        if (ch == 0) {
            tl.reset();
            // what the epilogue needs of this lane's two candidates, requested a whole tile of products ahead
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                cand[nj] = tile * kTileBN + 32 * w + 16 * nj + c;
                const bool inside = (uint32_t)cand[nj] < (uint32_t)p.n_cand;    // below 2^31 + 128: compared unsigned
                cok[nj] = inside && (!p.cand_ok || p.cand_ok[cand[nj]] != 0);
                csc[nj] = (p.cand_scale && inside) ? p.cand_scale[cand[nj]] : 1.0f;
            }
        }
        __syncthreads();                                     // the previous chunk is consumed
        tl.store_chunk();
        __syncthreads();                                     // also orders the query rows before their first use
        if (step + 1 < n_steps) load_chunk(step + 1);        // in flight during this chunk's products
        tl.product(ch);
        if (ch != nch - 1) continue;

        // The tile's scores are whole: lane (c, q) holds rows 16 mi + 4 q + r of candidates 32 w + 16 nj + c.  First the
        // filter, two multiplies and a compare per score: a score BELOW the value of its row's threshold is dropped in
        // registers (a NaN, an equal value and either zero against the other are not below: they go on).
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
                    if (p.query_scale) s = __fmul_rn(__fmul_rn(s, rs), csc[nj]);
                    tl.acc[mi][nj][r] = s;
                    todo |= (s < tv) ? 0u : 1u << ((mi * 4 + r) * 2 + nj);
                }
            }
        }
        // The rest, rare once the thresholds have risen: the exact comparison in the total order, and LAST, for a candidate
        // that has beaten its row's threshold, the search in the row's exclusion list.  A lane whose row is full keeps its
        // candidate, the full rows are compacted, and it tries again: no candidate is ever lost, so the result does not
        // depend on the order of arrival.
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
                        bool pending = false;
                        if (qid[row] >= 0 && cok[nj] && cand[nj] != skp[row]) {
                            const u64 e = pack_candidate(tl.acc[mi][nj][r], cand[nj]);
                            if (e > thr[row] && !in_sorted(p.list_items, lb[row], le[row], (int64_t)cand[nj])) {
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
            for (int rr = 0; rr < kRtRowsPerWave; ++rr) {
                const int row = kRtRowsPerWave * w + rr;
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

    // every row sorted, its k best out: to the result, or to this range's place in the workspace
    for (int rr = 0; rr < kRtRowsPerWave; ++rr) {
        const int row = kRtRowsPerWave * w + rr;
        const int64_t r = row0 + row;
        if (r >= p.n_queries) break;                         // the same for every lane
        const int m = compact_row(buf + row * cap, min(cnt[row], cap), k, lane, nullptr, nullptr);
        if (lane < k) {
            const u64 e = lane < m ? buf[row * cap + lane] : 0ull;
            if (p.slices == 1) write_candidate(p.out_index, p.out_value, r * k + lane, e);
            else p.ws[((int64_t)r * p.slices + blockIdx.y) * k + lane] = e;
        }
    }
}

// One wavefront per query row merges the ranges' candidates (merge_row).
__global__ __launch_bounds__(kBlock) void k_retrieve_merge(const RtArgs p) {
    __shared__ u64 mbuf[kBlock / kWave][kNbCapMax];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, k = p.k;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + w;
    if (r >= p.n_queries) return;
    merge_row(mbuf[w], p.ws + r * p.slices * k, p.slices * k, k, lane, p.out_index, p.out_value, r * k);
}

inline int64_t rt_cand_tiles(int64_t n_cand) { return (n_cand + kTileBN - 1) / kTileBN; }

// The range count in use: the one asked for, or with 0 the smallest that gives about 512 workgroups (two for every CU);
// never more than LGC_RETRIEVE_MAX_SLICES or than there are candidate tiles.  Its own rule beside tile_slices: an audience
// request is one tile of queries over thousands of candidate tiles, and 64 ranges would leave three quarters of the CUs idle.
inline int rt_slices(int64_t n_queries, int64_t n_cand, int asked) {
    const int64_t row_tiles = std::max<int64_t>(1, (n_queries + kTileBM - 1) / kTileBM);
    int64_t s = asked > 0 ? asked : (512 + row_tiles - 1) / row_tiles;
    s = std::min<int64_t>(s, LGC_RETRIEVE_MAX_SLICES);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, rt_cand_tiles(n_cand)));
}

inline bool rt_sizes_ok(int64_t n_queries, int64_t n_cand, int k, int slices) {
    return n_queries >= 0 && n_cand >= 1 && n_queries < INT32_MAX && n_cand < INT32_MAX && slices >= 0 &&
           slices <= LGC_RETRIEVE_MAX_SLICES && k >= 1 && k <= LGC_RETRIEVE_MAX_K;
}

unsigned long long lds_ok_retrieve;

}  // namespace

extern "C" {

size_t lgc_retrieve_workspace_bytes(int64_t n_queries, int64_t n_cand, int32_t k, int32_t slices) {
    if (!rt_sizes_ok(n_queries, n_cand, k, slices)) return 0;
    int64_t places;                                          // candidate lists of k places
    if (slices > 0) {
        const int64_t s = std::min<int64_t>(slices, rt_cand_tiles(n_cand));
        places = s > 1 ? n_queries * s : 0;
    } else {
        // what the chosen count needs is not monotonic in n_queries (more row tiles, fewer ranges); its two bounds are
        const int64_t s_max = std::min<int64_t>(512, rt_cand_tiles(n_cand));
        places = s_max > 1 ? std::min<int64_t>(n_queries * s_max, n_queries + 512 * (int64_t)kTileBM) : 0;
    }
    return (size_t)places * (size_t)k * sizeof(u64);
}

int lgc_retrieve_topk(const float *queries, int64_t query_stride, int64_t n_query_rows, const float *cands,
                      int64_t cand_stride, int64_t n_cand, int32_t dim, const int64_t *query_ids, int64_t n_queries,
                      const float *query_scale, const float *cand_scale, const uint8_t *cand_ok, const int64_t *list_ptr,
                      const int64_t *list_items, const int64_t *list_rows, int64_t n_lists, const int64_t *skip_id,
                      int32_t k, int32_t slices, int64_t *out_index, float *out_value, void *workspace,
                      size_t workspace_bytes, int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!queries || !cands || !out_index || !status || n_queries < 0 || n_query_rows < 0 || n_lists < 0 ||
        query_stride < dim || cand_stride < dim || (query_scale == nullptr) != (cand_scale == nullptr) ||
        (list_ptr && !list_items))
        return LGC_E_INVAL;
    if (!rt_sizes_ok(n_queries, n_cand, k, slices) || n_query_rows >= INT32_MAX || n_lists >= INT32_MAX) return LGC_E_RANGE;
    if (!aligned_to(queries, 4) || !aligned_to(cands, 4) || !aligned_to(query_scale, 4) || !aligned_to(cand_scale, 4) ||
        !aligned_to(out_value, 4) || !aligned_to(query_ids, 8) || !aligned_to(list_ptr, 8) || !aligned_to(list_items, 8) ||
        !aligned_to(list_rows, 8) || !aligned_to(skip_id, 8) || !aligned_to(out_index, 8) || !aligned_to(workspace, 8))
        return LGC_E_ALIGN;
    const int s = rt_slices(n_queries, n_cand, slices);
    const size_t need = s > 1 ? (size_t)n_queries * s * k * sizeof(u64) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    if (n_queries == 0) return 0;

    RtArgs p{};
    p.queries = queries;
    p.cands = cands;
    p.query_stride = query_stride;
    p.cand_stride = cand_stride;
    p.query_ids = query_ids;
    p.query_scale = query_scale;
    p.cand_scale = cand_scale;
    p.cand_ok = cand_ok;
    p.list_ptr = list_ptr;
    p.list_items = list_ptr ? list_items : nullptr;
    p.list_rows = list_ptr ? list_rows : nullptr;
    p.skip_id = skip_id;
    p.out_index = out_index;
    p.out_value = out_value;
    p.ws = reinterpret_cast<u64 *>(workspace);
    p.status = status;
    p.n_query_rows = (int32_t)n_query_rows;
    p.n_cand = (int32_t)n_cand;
    p.n_queries = (int32_t)n_queries;
    p.n_lists = (int32_t)n_lists;
    p.dim = dim;
    p.dp = tile_dp(dim);
    p.k = k;
    p.slices = s;
    p.cap = select_cap(k);
    p.cand_tiles = (int32_t)rt_cand_tiles(n_cand);
    const size_t lds = sizeof(float) * tile_lds_floats(p.dp) + sizeof(u64) * ((size_t)kTileBM * p.cap + kTileBM) +
                       (sizeof(int64_t) * 2 + sizeof(int) * 3 + sizeof(float) * 2) * kTileBM;
    int rc = allow_lds(reinterpret_cast<const void *>(k_retrieve), lds, 48 * 1024, 144 * 1024, &lds_ok_retrieve);
    if (rc != 0) return rc;
    const int64_t row_tiles = (n_queries + kTileBM - 1) / kTileBM;
    hipLaunchKernelGGL(k_retrieve, dim3((unsigned)row_tiles, (unsigned)s), dim3(kBlock), lds, as_stream(stream_), p);
    rc = (int)hipGetLastError();
    if (rc != 0 || s == 1) return rc;
    hipLaunchKernelGGL(k_retrieve_merge, dim3((unsigned)ceil_div(n_queries, kBlock / kWave)), dim3(kBlock), 0,
                       as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

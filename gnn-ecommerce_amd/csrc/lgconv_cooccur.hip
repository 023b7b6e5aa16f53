// lgconv_cooccur.hip -- bought together: per query item the k items that share most buyers with it, counted from the two
// purchase CSRs alone (item -> buyers, user -> items) with integer LDS adds, scored (count, cosine, Jaccard) and selected in
// the same launch; no count is ever written to memory except those of the returned items.
// C ABI: include/lgconv_hip.h
#include "lgconv_select.h"

namespace {

// Geometry.  A workgroup of kCoBlock threads owns one (query, band): `band` uint32 counters of
// consecutive items in LDS.  It clears them, walks the query's buyers -- kCoGroup lanes per buyer, kCoBuyers buyers at a
// time: the walk is a chain of dependent loads, and what hides it is buyers in flight -- adding 1 per entry of a buyer's item
// list that falls into the band; then its first four wavefronts scan every fourth run of 64 counters each, score the
// eligible ones and keep their k best (the candidate word and compact_row of lgconv_select.h); wavefront 0 merges the four
// lists.  One band: that is the result, and the counts of the returned items are still in LDS.  Several bands: the list
// goes to the workspace and k_cooccur_merge merges the bands' lists of a query; it counts the returned items again for
// out_count, since a place of the workspace has no room for a count.
constexpr int kCoGroup = 16;                                 // lanes that walk one buyer's list
constexpr int kCoBlock = 1024;                               // 16 wavefronts: with two workgroups a CU, all it can hold
constexpr int kCoBuyers = kCoBlock / kCoGroup;               // buyers a workgroup walks at a time
constexpr int kCoSearch = 4 * kCoGroup;                      // a longer list is narrowed to the band by two searches
constexpr int kCoWaves = 4;                                  // wavefronts that scan and select
constexpr int kCoAutoBand = 16384;                           // the fastest of 8192 / 16384 / 32768 over a whole catalogue
constexpr int64_t kCoMaxBands = 1 << 20;                     // bands * k places of one query are merged with an int count
constexpr int64_t kCoMaxGrid = 1 << 22;                      // workgroups of one launch
constexpr size_t kCoLdsFixed = sizeof(u64) * (kCoWaves * kNbCapMax + kCoWaves * kSelectMaxK + kCoWaves) + sizeof(float) * kCoWaves;
static_assert(LGC_COOCCUR_MAX_K <= kSelectMaxK, "compact_row holds a buffer in two registers a lane");
static_assert(kCoLdsFixed % 16 == 0 && kCoLdsFixed + sizeof(uint32_t) * LGC_COOCCUR_MAX_BAND <= 144 * 1024,
              "the largest band fits the LDS opt-in");
static_assert(LGC_COOCCUR_MAX_BAND % kWave == 0 && kCoAutoBand % kWave == 0 && kCoAutoBand <= LGC_COOCCUR_MAX_BAND, "bands are runs of 64");

struct CoArgs {
    const int64_t *buyer_ptr;
    const int64_t *buyer_users;
    const int64_t *seen_ptr;
    const int64_t *seen_items;
    const int64_t *query_ids;
    const uint8_t *item_ok;
    int64_t *out_index;
    float *out_value;
    int32_t *out_count;
    u64 *ws;
    int32_t *status;
    int64_t first;                                           // the launch's first workgroup (k_cooccur) or query (merge)
    int64_t n_items, n_users;
    int32_t min_count, measure, k, band, bands;
};

// the query item of row r and its buyer list buyer_users[bp, be); an id outside the catalogue has no buyers
__device__ __forceinline__ int64_t co_query(const CoArgs &p, int64_t r, int64_t *bp, int64_t *be) {
    const int64_t q = p.query_ids ? p.query_ids[r] : r;
    const bool inside = q >= 0 && q < p.n_items;             // range-checked before any address is formed from it
    *bp = inside ? p.buyer_ptr[q] : 0;
    *be = inside ? p.buyer_ptr[q + 1] : 0;
    return inside ? q : -1;
}

// The workgroup walks buyer_users[bp, be): group g = tid / kCoGroup takes buyers g, g + kCoBuyers, ... and its lanes the
// entries of that buyer's item list, add(j) for every entry j in [lo, hi).  A list of more than kCoSearch entries is
// narrowed to the part that can hold [lo, hi) by two searches (dependent loads; up to kCoSearch entries cost less read
// whole), which `first` (nothing below lo is in the catalogue) and
// `last` (nothing at or above hi is) spare; a shorter one is read whole.  Every buyer and every entry is range-checked
// before it is used: one outside its table is skipped and sets LGC_ST_INDEX_OOB (an entry only where this walk reads it: in
// an ascending list the band of item 0 reads the negative ones and the last band those past the catalogue).  The buyer two
// steps ahead and the list bounds of the next one are requested before the current list is read.
template <typename F>
__device__ __forceinline__ void co_walk(const CoArgs &p, int64_t bp, int64_t be, int64_t lo, int64_t hi, bool first, bool last,
                                        int tid, F add) {
    const int sub = tid % kCoGroup;
    int64_t i = bp + tid / kCoGroup;
    int64_t u = i < be ? p.buyer_users[i] : -1;
    int64_t un = i + kCoBuyers < be ? p.buyer_users[i + kCoBuyers] : -1;
    int64_t sb = 0, se = 0;
    if ((uint64_t)u < (uint64_t)p.n_users) {
        sb = p.seen_ptr[u];
        se = p.seen_ptr[u + 1];
    }
    while (i < be) {
        const int64_t u2 = i + 2 * kCoBuyers < be ? p.buyer_users[i + 2 * kCoBuyers] : -1;
        int64_t sbn = 0, sen = 0;
        if ((uint64_t)un < (uint64_t)p.n_users) {
            sbn = p.seen_ptr[un];
            sen = p.seen_ptr[un + 1];
        }
        if ((uint64_t)u >= (uint64_t)p.n_users) {
            if (sub == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
        } else {
            int64_t e0 = sb, e1 = se;
            if (se - sb > kCoSearch) {
                if (!first) e0 = lower_bound(p.seen_items, sb, se, lo);
                if (!last) e1 = lower_bound(p.seen_items, e0, se, hi);
            }
            for (int64_t e = e0 + sub; e < e1; e += kCoGroup) {
                const int64_t j = p.seen_items[e];
                if ((uint64_t)j >= (uint64_t)p.n_items) atomicOr(p.status, LGC_ST_INDEX_OOB);
                else if (j >= lo && j < hi) add(j);
            }
        }
        i += kCoBuyers;
        u = un;
        un = u2;
        sb = sbn;
        se = sen;
    }
}

__global__ __launch_bounds__(kCoBlock) void k_cooccur(const CoArgs p) {
    extern __shared__ __attribute__((aligned(16))) u64 co_lds[];
    u64 *buf = co_lds;                                       // [kCoWaves][kNbCapMax]: a wavefront's candidates
    u64 *stage = buf + kCoWaves * kNbCapMax;                 // [kCoWaves][k]: the wavefronts' finished lists
    u64 *thr = stage + kCoWaves * kSelectMaxK;               // [kCoWaves]: what a new candidate has to beat
    float *thv = reinterpret_cast<float *>(thr + kCoWaves);  // [kCoWaves]: compact_row's other output, unused here
    uint32_t *ctr = reinterpret_cast<uint32_t *>(thv + kCoWaves);   // [band]: c(q, lo + i)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, k = p.k;
    const int64_t wg = p.first + blockIdx.x;
    const int64_t r = wg / p.bands;
    const int b = (int)(wg - r * p.bands);
    const int64_t lo = (int64_t)b * p.band, hi = min(lo + p.band, p.n_items);
    const int n_ctr = (int)((hi - lo + kWave - 1) / kWave) * kWave;   // <= band: the band is a multiple of 64

    int64_t bp, be;
    const int64_t q = co_query(p, r, &bp, &be);
    if (q < 0 && b == 0 && tid == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
    const int64_t a = be - bp;
    int m = 0;
    if (a > 0) {                                             // the same for the whole workgroup
        for (int i = tid; i < n_ctr; i += kCoBlock) ctr[i] = 0u;
        if (tid < kCoWaves) {
            thr[tid] = 0ull;
            thv[tid] = -INFINITY;
        }
        __syncthreads();
        co_walk(p, bp, be, lo, hi, b == 0, b == p.bands - 1, tid, [&](int64_t j) { atomicAdd(&ctr[(int)(j - lo)], 1u); });
        __syncthreads();

        // every fourth run of 64 counters: the score of an eligible one, filtered against the wavefront's threshold
        if (w < kCoWaves) {
            const float ra = 1.0f / sqrtf((float)a);             // hipcc default: both correctly rounded, as k_build_dis
            u64 *mine = buf + w * kNbCapMax;
            u64 t = 0ull;
            int n = 0;
            for (int base = w * kWave; base < n_ctr; base += kCoWaves * kWave) {
                const uint32_t c = ctr[base + lane];
                const int64_t j = lo + base + lane;              // a counter past the catalogue is 0
                u64 e = 0ull;
                if (c >= (uint32_t)p.min_count && j != q && (!p.item_ok || p.item_ok[j] != 0)) {
                    float s = (float)c;
                    bool ok = true;
                    if (p.measure != LGC_COOCCUR_COUNT) {
                        const int64_t bj = p.buyer_ptr[j + 1] - p.buyer_ptr[j];
                        if (p.measure == LGC_COOCCUR_COSINE) {
                            const float rb = 1.0f / sqrtf((float)bj);
                            s = __fmul_rn(__fmul_rn(s, ra), rb);
                        } else {
                            const int64_t den = a + bj - (int64_t)c;
                            ok = den > 0;
                            s = ok ? s / (float)den : 0.0f;
                        }
                    }
                    if (ok) e = pack_candidate(s, (int)j);
                }
                const u64 have = __ballot(e > t);                // a candidate is never 0
                if (have == 0ull) continue;                      // the same for every lane
                if (e > t) mine[n + __popcll(have & ((1ull << lane) - 1ull))] = e;
                n += __popcll(have);
                if (n > kNbCapMax - kWave) {
                    n = compact_row(mine, n, k, lane, thr + w, thv + w);
                    t = thr[w];
                }
            }
            n = compact_row(mine, n, k, lane, nullptr, nullptr);
            if (lane < k) stage[w * k + lane] = lane < n ? mine[lane] : 0ull;
        }
        __syncthreads();
        if (w == 0) m = merge_keep(buf, stage, kCoWaves * k, k, lane);
    }
    if (w != 0 || lane >= k) return;
    const u64 e = lane < m ? buf[lane] : 0ull;
    if (p.bands > 1) {
        p.ws[wg * k + lane] = e;
        return;
    }
    write_candidate(p.out_index, p.out_value, r * k + lane, e);
    if (p.out_count) p.out_count[r * k + lane] = e ? (int32_t)ctr[(~(uint32_t)e & 0x7FFFFFFFu) - (uint32_t)lo] : 0;
}

// One workgroup per query: wavefront 0 merges the bands' lists (merge_keep) and writes the result; for out_count the
// workgroup then walks the query's buyers once more and counts the returned items alone, found by a search among them.
__global__ __launch_bounds__(kCoBlock) void k_cooccur_merge(const CoArgs p) {
    __shared__ u64 mbuf[kNbCapMax];
    __shared__ int64_t sid[kSelectMaxK];                     // the returned items ascending
    __shared__ int spos[kSelectMaxK];                        // the place of sid[i] in the result
    __shared__ uint32_t cnt[kSelectMaxK];                    // by place
    __shared__ int n_found;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, k = p.k;
    const int64_t r = p.first + blockIdx.x;
    if (w == 0) {
        const int m = merge_keep(mbuf, p.ws + r * p.bands * k, p.bands * k, k, lane);
        const u64 e = lane < m ? mbuf[lane] : 0ull;
        if (lane < k) write_candidate(p.out_index, p.out_value, r * k + lane, e);
        if (p.out_count) {
            const int64_t item = (int64_t)(~(uint32_t)e & 0x7FFFFFFFu);
            int below = 0;
            for (int i = 0; i < m; ++i) below += (int64_t)(~(uint32_t)mbuf[i] & 0x7FFFFFFFu) < item ? 1 : 0;
            if (lane < m) {                                  // the items of a row are all different
                sid[below] = item;
                spos[below] = lane;
            }
            cnt[lane] = 0u;
            if (lane == 0) n_found = m;
        }
    }
    if (!p.out_count) return;
    __syncthreads();
    const int m = n_found;
    if (m > 0) {
        int64_t bp, be;
        co_query(p, r, &bp, &be);
        co_walk(p, bp, be, sid[0], sid[m - 1] + 1, false, false, tid, [&](int64_t j) {
            const int at = lower_bound(sid, 0, m, j);
            if (at < m && sid[at] == j) atomicAdd(&cnt[spos[at]], 1u);
        });
    }
    __syncthreads();
    if (tid < k) p.out_count[r * k + tid] = tid < m ? (int32_t)cnt[tid] : 0;
}

// the counters of a band in use: what was asked for (0: the library's choice), never more than the catalogue rounded up to 64
inline int co_band(int64_t n_items, int band) {
    return (int)std::min<int64_t>((n_items + kWave - 1) / kWave * kWave, band > 0 ? band : kCoAutoBand);
}

inline int64_t co_bands(int64_t n_items, int band) {
    const int w = co_band(n_items, band);
    return (n_items + w - 1) / w;
}

inline bool co_sizes_ok(int64_t n_queries, int64_t n_items, int k, int band) {
    if (n_queries < 0 || n_items < 1 || n_queries >= INT32_MAX || n_items >= INT32_MAX || k < 1 || k > LGC_COOCCUR_MAX_K) return false;
    if (band != 0 && (band < kWave || band > LGC_COOCCUR_MAX_BAND || band % kWave != 0)) return false;
    return co_bands(n_items, band) <= kCoMaxBands;           // (query, band) pairs beyond one grid take several launches
}

unsigned long long lds_ok_cooccur;

}  // namespace

extern "C" {

size_t lgc_cooccur_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t band, void *) {   // no launch
    if (!co_sizes_ok(n_queries, n_items, k, band)) return 0;
    const int64_t bands = co_bands(n_items, band);
    return bands > 1 ? (size_t)(n_queries * bands) * (size_t)k * sizeof(u64) : 0;
}

int lgc_cooccur_topk(const int64_t *buyer_ptr, const int64_t *buyer_users, int64_t n_items, const int64_t *seen_ptr,
                     const int64_t *seen_items, int64_t n_users, const int64_t *query_ids, int64_t n_queries,
                     const uint8_t *item_ok, int32_t min_count, int32_t measure, int32_t k, int32_t band, int64_t *out_index,
                     float *out_value, int32_t *out_count, void *workspace, size_t workspace_bytes, int32_t *status,
                     void *stream_) {
    if (!buyer_ptr || !buyer_users || !seen_ptr || !seen_items || !out_index || !status || n_queries < 0 || n_users < 0 ||
        measure < LGC_COOCCUR_COUNT || measure > LGC_COOCCUR_JACCARD)
        return LGC_E_INVAL;
    if (!co_sizes_ok(n_queries, n_items, k, band) || n_users >= INT32_MAX || min_count < 1) return LGC_E_RANGE;
    if (!aligned_to(buyer_ptr, 8) || !aligned_to(buyer_users, 8) || !aligned_to(seen_ptr, 8) || !aligned_to(seen_items, 8) ||
        !aligned_to(query_ids, 8) || !aligned_to(out_index, 8) || !aligned_to(out_value, 4) || !aligned_to(out_count, 4) ||
        !aligned_to(status, 4) || !aligned_to(workspace, 8))
        return LGC_E_ALIGN;
    const size_t need = lgc_cooccur_workspace_bytes(n_queries, n_items, k, band, stream_);
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    if (n_queries == 0) return 0;

    CoArgs p{};
    p.buyer_ptr = buyer_ptr;
    p.buyer_users = buyer_users;
    p.seen_ptr = seen_ptr;
    p.seen_items = seen_items;
    p.query_ids = query_ids;
    p.item_ok = item_ok;
    p.out_index = out_index;
    p.out_value = out_value;
    p.out_count = out_count;
    p.ws = reinterpret_cast<u64 *>(workspace);
    p.status = status;
    p.n_items = n_items;
    p.n_users = n_users;
    p.min_count = min_count;
    p.measure = measure;
    p.k = k;
    p.band = co_band(n_items, band);
    p.bands = (int32_t)co_bands(n_items, band);
    const size_t lds = kCoLdsFixed + sizeof(uint32_t) * (size_t)p.band;
    int rc = allow_lds(reinterpret_cast<const void *>(k_cooccur), lds, 48 * 1024, 144 * 1024, &lds_ok_cooccur);
    if (rc != 0) return rc;
    const int64_t total = n_queries * p.bands;
    for (p.first = 0; p.first < total; p.first += kCoMaxGrid) {
        const unsigned grid = (unsigned)std::min<int64_t>(kCoMaxGrid, total - p.first);
        hipLaunchKernelGGL(k_cooccur, dim3(grid), dim3(kCoBlock), lds, as_stream(stream_), p);
        rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    if (p.bands == 1) return 0;
    for (p.first = 0; p.first < n_queries; p.first += kCoMaxGrid) {
        const unsigned grid = (unsigned)std::min<int64_t>(kCoMaxGrid, n_queries - p.first);
        hipLaunchKernelGGL(k_cooccur_merge, dim3(grid), dim3(kCoBlock), 0, as_stream(stream_), p);
        rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // extern "C"

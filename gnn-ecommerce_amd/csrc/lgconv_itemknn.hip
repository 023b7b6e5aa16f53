// lgconv_itemknn.hip -- the item-kNN recommender: per basket (a user's purchase list, a cart, a session) the rows of a
// [n_items, kn] neighbour table that the basket's items name are summed into candidate scores in LDS, in the basket's own
// order and without a float atomic, what must not be returned is removed, and the k best are selected in the same launch.
// It reads no embedding.
// C ABI: include/lgconv_hip.h
#include "lgconv_select.h"

namespace {

// Geometry.  A workgroup of kKnBlock threads owns one (query, band): `band` fp32 accumulators and
// `band` uint32 vote words of consecutive items in LDS.  Every one of its kKnWalkers wavefronts owns a run of the band and
// walks ALL rows the basket names, in list order, lane p holding place p of a row, and applies the entries that fall into
// its own run with plain LDS read-modify-writes: the valid indices of one row are distinct, so no two lanes meet, and the
// rows of one wavefront land in program order, so the sum of a candidate is taken in the basket's order.  No barrier inside
// the walk.  The top bit of a vote word marks an item that is itself an entry of the basket.  Then the first four
// wavefronts scan every fourth run of 64 items each and keep their k best (the candidate word and compact_row of
// lgconv_select.h) and wavefront 0 merges the four lists.  One band: that is the result.  Several bands: the list and the
// votes of its items go to the workspace and k_knn_merge merges the bands' lists of a query.
constexpr int kKnBlock = 1024;                               // 16 wavefronts, each with its own run of the band
constexpr int kKnWalkers = kKnBlock / kWave;
constexpr int kKnAhead = 4;                                  // neighbour rows a wavefront has requested before it applies one
constexpr int kKnWaves = 4;                                  // wavefronts that scan and select
constexpr int kKnAutoBand = 8192;                            // the fastest of 4096 / 8192 / 16384 for 10^4 users: two workgroups a CU
constexpr int64_t kKnMaxBands = 1 << 20;                     // bands * k places of one query are merged with an int count
constexpr int64_t kKnMaxGrid = 1 << 22;                      // workgroups of one launch
constexpr uint32_t kKnInBasket = 0x80000000u;                // the mark in a vote word
constexpr size_t kKnLdsFixed = sizeof(u64) * (kKnWaves * kNbCapMax + kKnWaves * kSelectMaxK + kKnWaves) + sizeof(float) * kKnWaves;
static_assert(LGC_KNN_MAX_K <= kSelectMaxK, "compact_row holds a buffer in two registers a lane");
static_assert(LGC_KNN_MAX_NEIGHBORS <= kWave, "a lane holds one place of a neighbour row");
static_assert(kKnLdsFixed % 16 == 0 && kKnLdsFixed + 2 * sizeof(uint32_t) * LGC_KNN_MAX_BAND <= 144 * 1024,
              "the largest band fits the LDS opt-in");
static_assert(LGC_KNN_MAX_BAND % kWave == 0 && kKnAutoBand % kWave == 0 && kKnAutoBand <= LGC_KNN_MAX_BAND, "bands are runs of 64");

struct KnArgs {
    const int64_t *nbr_index;
    const float *nbr_value;
    const int64_t *list_ptr;
    const int64_t *list_items;
    const float *list_weight;
    const int64_t *list_rows;
    const uint8_t *item_ok;
    int64_t *out_index;
    float *out_value;
    int32_t *out_votes;
    u64 *ws;                                                 // [n_queries * bands * k] candidate words ...
    int32_t *ws_votes;                                       // ... and behind them the votes of each
    int32_t *status;
    int64_t first;                                           // the launch's first workgroup (k_knn) or query (merge)
    int64_t nbr_stride, n_items, n_lists;
    int32_t kn, exclude_basket, min_votes, k, band, bands;
};

// One wavefront walks basket entries [lp, le) in order and applies what falls into items [mlo, mhi) of the band that begins
// at item lo.  64 entries (and weights) are read at a time, the next 64 requested before the current ones are used; of the
// rows they name, kKnAhead are requested ahead of the one that is applied.  A basket entry or a neighbour index outside
// [0, n_items) is range-checked before an address is formed from it, skipped, and flagged where `flag` (one wavefront of one
// band, so that the word is written once per fault and not sixteen times).  -1 in a row is an empty place.
template <bool WEIGHTED>
__device__ __forceinline__ void kn_walk(const KnArgs &p, int64_t lp, int64_t le, int64_t lo, int64_t mlo, int64_t mhi,
                                        float *acc, uint32_t *vot, int lane, bool flag) {
    const bool place = lane < p.kn;                          // elements at or past kn of a row are never read
    int64_t itn = lp + lane < le ? p.list_items[lp + lane] : -1;
    float wtn = WEIGHTED && lp + lane < le ? p.list_weight[lp + lane] : 1.0f;
    for (int64_t base = lp; base < le; base += kWave) {
        const int cnt = (int)min((int64_t)kWave, le - base);
        const int64_t it = itn;
        const float wt = wtn;
        const int64_t nx = base + kWave + lane;
        itn = nx < le ? p.list_items[nx] : -1;
        if (WEIGHTED) wtn = nx < le ? p.list_weight[nx] : 1.0f;
        if (flag && lane < cnt && (uint64_t)it >= (uint64_t)p.n_items) atomicOr(p.status, LGC_ST_INDEX_OOB);

        int64_t jn[kKnAhead];
        float vn[kKnAhead];
        auto request = [&](int t0) {
#pragma unroll
            for (int u = 0; u < kKnAhead; ++u) {
                const int64_t i = t0 + u < cnt ? __shfl(it, t0 + u, kWave) : -1;    // the same in every lane
                jn[u] = -1;
                vn[u] = 0.0f;
                if (place && (uint64_t)i < (uint64_t)p.n_items) {
                    jn[u] = p.nbr_index[i * p.nbr_stride + lane];
                    vn[u] = p.nbr_value[i * p.nbr_stride + lane];
                }
            }
        };
        request(0);
        for (int t0 = 0; t0 < cnt; t0 += kKnAhead) {
            int64_t j[kKnAhead];
            float v[kKnAhead];
#pragma unroll
            for (int u = 0; u < kKnAhead; ++u) {
                j[u] = jn[u];
                v[u] = vn[u];
            }
            if (t0 + kKnAhead < cnt) request(t0 + kKnAhead);
#pragma unroll
            for (int u = 0; u < kKnAhead; ++u) {
                if (t0 + u >= cnt) break;                    // the same in every lane
                const int64_t i = __shfl(it, t0 + u, kWave);
                const float w = __shfl(wt, t0 + u, kWave);
                const int64_t jj = j[u];
                if (jj != -1) {
                    if ((uint64_t)jj >= (uint64_t)p.n_items) {
                        if (flag) atomicOr(p.status, LGC_ST_INDEX_OOB);
                    } else if (jj >= mlo && jj < mhi) {
                        const int o = (int)(jj - lo);
                        const float term = WEIGHTED ? __fmul_rn(w, v[u]) : v[u];
                        acc[o] = __fadd_rn(acc[o], term);
                        vot[o] += 1u;
                    }
                }
                if (lane == 0 && i >= mlo && i < mhi) vot[(int)(i - lo)] |= kKnInBasket;   // after the row: in program order
            }
        }
    }
}

__global__ __launch_bounds__(kKnBlock) void k_knn(const KnArgs p) {
    extern __shared__ __attribute__((aligned(16))) u64 kn_lds[];
    u64 *buf = kn_lds;                                       // [kKnWaves][kNbCapMax]: a wavefront's candidates
    u64 *stage = buf + kKnWaves * kNbCapMax;                 // [kKnWaves][k]: the wavefronts' finished lists
    u64 *thr = stage + kKnWaves * kSelectMaxK;               // [kKnWaves]: what a new candidate has to beat
    float *thv = reinterpret_cast<float *>(thr + kKnWaves);  // [kKnWaves]: compact_row's other output, unused here
    float *acc = thv + kKnWaves;                             // [band]: the score of item lo + i
    uint32_t *vot = reinterpret_cast<uint32_t *>(acc + p.band);   // [band]: its votes, the top bit the basket's mark
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, k = p.k;
    const int64_t wg = p.first + blockIdx.x;
    const int64_t r = wg / p.bands;
    const int b = (int)(wg - r * p.bands);
    const int64_t lo = (int64_t)b * p.band, hi = min(lo + p.band, p.n_items);
    const int n_ctr = (int)((hi - lo + kWave - 1) / kWave) * kWave;   // <= band: the band is a multiple of 64

    const int64_t l = p.list_rows ? p.list_rows[r] : r;
    const bool inside = l >= 0 && l < p.n_lists;             // range-checked before any address is formed from it
    if (!inside && b == 0 && tid == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
    const int64_t lp = inside ? p.list_ptr[l] : 0, le = inside ? p.list_ptr[l + 1] : 0;
    int m = 0;
    if (le > lp) {                                           // the same for the whole workgroup
        for (int i = tid; i < n_ctr; i += kKnBlock) {
            acc[i] = 0.0f;
            vot[i] = 0u;
        }
        if (tid < kKnWaves) {
            thr[tid] = 0ull;
            thv[tid] = -INFINITY;
        }
        __syncthreads();
        const int run = (n_ctr / kWave + kKnWalkers - 1) / kKnWalkers * kWave;      // items of a wavefront's run
        const int64_t mlo = lo + (int64_t)w * run, mhi = min(mlo + run, hi);
        if (p.list_weight) kn_walk<true>(p, lp, le, lo, mlo, mhi, acc, vot, lane, b == 0 && w == 0);
        else kn_walk<false>(p, lp, le, lo, mlo, mhi, acc, vot, lane, b == 0 && w == 0);
        __syncthreads();

        // every fourth run of 64 items: an eligible one's score, filtered against the wavefront's threshold
        if (w < kKnWaves) {
            u64 *mine = buf + w * kNbCapMax;
            u64 t = 0ull;
            int n = 0;
            for (int base = w * kWave; base < n_ctr; base += kKnWaves * kWave) {
                const uint32_t word = vot[base + lane];
                const int64_t j = lo + base + lane;              // an item past the catalogue has no votes
                u64 e = 0ull;
                if ((word & ~kKnInBasket) >= (uint32_t)p.min_votes && !(p.exclude_basket && (word & kKnInBasket)) &&
                    (!p.item_ok || p.item_ok[j] != 0))
                    e = pack_candidate(acc[base + lane], (int)j);
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
        if (w == 0) m = merge_keep(buf, stage, kKnWaves * k, k, lane);
    }
    if (w != 0 || lane >= k) return;
    const u64 e = lane < m ? buf[lane] : 0ull;
    const int32_t votes = e ? (int32_t)(vot[(~(uint32_t)e & 0x7FFFFFFFu) - (uint32_t)lo] & ~kKnInBasket) : 0;
    if (p.bands > 1) {
        p.ws[wg * k + lane] = e;
        p.ws_votes[wg * k + lane] = votes;
        return;
    }
    write_candidate(p.out_index, p.out_value, r * k + lane, e);
    if (p.out_votes) p.out_votes[r * k + lane] = votes;
}

// One wavefront per query merges the bands' lists (merge_keep) and writes the result; the votes of a returned item lie
// beside its candidate word in the list of the item's band.
__global__ __launch_bounds__(kWave) void k_knn_merge(const KnArgs p) {
    __shared__ u64 mbuf[kNbCapMax];
    const int lane = threadIdx.x, k = p.k;
    const int64_t r = p.first + blockIdx.x;
    const int m = merge_keep(mbuf, p.ws + r * p.bands * k, p.bands * k, k, lane);
    if (lane >= k) return;
    const u64 e = lane < m ? mbuf[lane] : 0ull;
    write_candidate(p.out_index, p.out_value, r * k + lane, e);
    if (!p.out_votes) return;
    int32_t votes = 0;
    if (e) {
        const int64_t at = (r * p.bands + (int64_t)((~(uint32_t)e & 0x7FFFFFFFu) / (uint32_t)p.band)) * k;
        for (int i = 0; i < k; ++i)
            if (p.ws[at + i] == e) votes = p.ws_votes[at + i];   // the words of a query are all different
    }
    p.out_votes[r * k + lane] = votes;
}

// the items of a band in use: what was asked for (0: the library's choice), never more than the catalogue rounded up to 64
inline int kn_band(int64_t n_items, int band) {
    return (int)std::min<int64_t>((n_items + kWave - 1) / kWave * kWave, band > 0 ? band : kKnAutoBand);
}

inline int64_t kn_bands(int64_t n_items, int band) {
    const int w = kn_band(n_items, band);
    return (n_items + w - 1) / w;
}

inline bool kn_sizes_ok(int64_t n_queries, int64_t n_items, int k, int band) {
    if (n_queries < 0 || n_items < 1 || n_queries >= INT32_MAX || n_items >= INT32_MAX || k < 1 || k > LGC_KNN_MAX_K) return false;
    if (band != 0 && (band < kWave || band > LGC_KNN_MAX_BAND || band % kWave != 0)) return false;
    return kn_bands(n_items, band) <= kKnMaxBands;           // (query, band) pairs beyond one grid take several launches
}

unsigned long long lds_ok_knn;

}  // namespace

extern "C" {

size_t lgc_knn_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t band, void *) {   // no launch
    if (!kn_sizes_ok(n_queries, n_items, k, band)) return 0;
    const int64_t bands = kn_bands(n_items, band);
    return bands > 1 ? (size_t)(n_queries * bands) * (size_t)k * (sizeof(u64) + sizeof(int32_t)) : 0;
}

int lgc_knn_recommend(const int64_t *nbr_index, const float *nbr_value, int64_t nbr_stride, int64_t n_items, int32_t kn,
                      const int64_t *list_ptr, const int64_t *list_items, const float *list_weight, int64_t n_lists,
                      const int64_t *list_rows, int64_t n_queries, const uint8_t *item_ok, int32_t exclude_basket,
                      int32_t min_votes, int32_t k, int32_t band, int64_t *out_index, float *out_value, int32_t *out_votes,
                      void *workspace, size_t workspace_bytes, int32_t *status, void *stream_) {
    if (!nbr_index || !nbr_value || !list_ptr || !list_items || !out_index || !status || n_queries < 0 || n_lists < 0 ||
        nbr_stride < kn)
        return LGC_E_INVAL;
    if (!kn_sizes_ok(n_queries, n_items, k, band) || kn < 1 || kn > LGC_KNN_MAX_NEIGHBORS || min_votes < 1 ||
        n_lists >= INT32_MAX || (!list_rows && n_queries > n_lists))
        return LGC_E_RANGE;
    if (!aligned_to(nbr_index, 8) || !aligned_to(nbr_value, 4) || !aligned_to(list_ptr, 8) || !aligned_to(list_items, 8) ||
        !aligned_to(list_weight, 4) || !aligned_to(list_rows, 8) || !aligned_to(out_index, 8) || !aligned_to(out_value, 4) ||
        !aligned_to(out_votes, 4) || !aligned_to(status, 4) || !aligned_to(workspace, 8))
        return LGC_E_ALIGN;
    const size_t need = lgc_knn_workspace_bytes(n_queries, n_items, k, band, stream_);
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    if (n_queries == 0) return 0;

    KnArgs p{};
    p.nbr_index = nbr_index;
    p.nbr_value = nbr_value;
    p.list_ptr = list_ptr;
    p.list_items = list_items;
    p.list_weight = list_weight;
    p.list_rows = list_rows;
    p.item_ok = item_ok;
    p.out_index = out_index;
    p.out_value = out_value;
    p.out_votes = out_votes;
    p.status = status;
    p.nbr_stride = nbr_stride;
    p.n_items = n_items;
    p.n_lists = n_lists;
    p.kn = kn;
    p.exclude_basket = exclude_basket;
    p.min_votes = min_votes;
    p.k = k;
    p.band = kn_band(n_items, band);
    p.bands = (int32_t)kn_bands(n_items, band);
    const int64_t total = n_queries * p.bands;
    p.ws = reinterpret_cast<u64 *>(workspace);
    p.ws_votes = p.bands > 1 ? reinterpret_cast<int32_t *>(p.ws + total * k) : nullptr;
    const size_t lds = kKnLdsFixed + 2 * sizeof(uint32_t) * (size_t)p.band;
    int rc = allow_lds(reinterpret_cast<const void *>(k_knn), lds, 48 * 1024, 144 * 1024, &lds_ok_knn);
    if (rc != 0) return rc;
    for (p.first = 0; p.first < total; p.first += kKnMaxGrid) {
        const unsigned grid = (unsigned)std::min<int64_t>(kKnMaxGrid, total - p.first);
        hipLaunchKernelGGL(k_knn, dim3(grid), dim3(kKnBlock), lds, as_stream(stream_), p);
        rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    if (p.bands == 1) return 0;
    for (p.first = 0; p.first < n_queries; p.first += kKnMaxGrid) {
        const unsigned grid = (unsigned)std::min<int64_t>(kKnMaxGrid, n_queries - p.first);
        hipLaunchKernelGGL(k_knn_merge, dim3(grid), dim3(kWave), 0, as_stream(stream_), p);
        rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // extern "C"

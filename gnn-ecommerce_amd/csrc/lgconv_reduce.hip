// lgconv_reduce.hip -- middle-hop reduction of a user|item graph (include/lgconv_hip.h, lgc_reduce_*): the users with few
// entries are taken out of the CSR and their two-step paths item -> user -> item are kept as one sparse item x item
// operator  G_L = R_L^T R_L  instead.  One-time planning calls beside the tile classes and the sweep plan, not hop launches.
// lgc_reduce_concat lays both out as ONE operator [R_H^T | G_L] over a column space with gaps for the item rows.
//
// Everything is index arithmetic plus one stable radix sort and fixed-order fp64 sums: no float atomics, the same bits on
// every build.  Integer atomics only count (k_reduce_incount), which is order independent.
#include "lgconv_common.h"

#include <hipcub/hipcub.hpp>

namespace {

inline size_t r_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Workspace of lgc_reduce_count, read again by lgc_reduce_fill and lgc_reduce_gram_count.
struct ReduceWs {
    int32_t *incount;     // [split + 1]   item rows that name user u as a column
    int32_t *keep_scan;   // [split + 1]   exclusive scan of "user u is kept"; [split] = n_h
    int32_t *ent_scan;    // [E + 1]       exclusive scan of "entry e survives in the reduced CSR"; [E] = its entry count
    long long *pair_scan; // [E + 1]       exclusive scan of the pairs entry e expands into; [E] = the pair count
    void *cub;
    size_t cub_bytes;
};

size_t reduce_ws(void *base, int64_t n_nodes, int64_t n_edges, ReduceWs *ws) {
    size_t cb32 = 0, cb64 = 0;
    int32_t *n32 = nullptr;
    long long *n64 = nullptr;
    const int64_t longest = std::max<int64_t>(n_edges, n_nodes) + 1;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, cb32, n32, n32, (int)longest, (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, cb64, n64, n64, (int)longest, (hipStream_t)0);
    const size_t cb = std::max(cb32, cb64);
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += r_align_up(bytes, 256); return p + at; };
    const uintptr_t a_in = take((size_t)(n_nodes + 1) * 4), a_keep = take((size_t)(n_nodes + 1) * 4),
                    a_ent = take((size_t)(n_edges + 1) * 4), a_pair = take((size_t)(n_edges + 1) * 8), a_cub = take(cb);
    if (ws) {
        ws->incount = reinterpret_cast<int32_t *>(a_in);
        ws->keep_scan = reinterpret_cast<int32_t *>(a_keep);
        ws->ent_scan = reinterpret_cast<int32_t *>(a_ent);
        ws->pair_scan = reinterpret_cast<long long *>(a_pair);
        ws->cub = reinterpret_cast<void *>(a_cub);
        ws->cub_bytes = cb;
    }
    return off + 256;
}

// Workspace of lgc_reduce_gram_count, read again by lgc_reduce_gram_fill.
struct GramWs {
    unsigned long long *keys_in, *keys_out;   // [P]  (item row << 32) | item column
    double *vals_in, *vals_out;               // [P]  fp64 products
    int32_t *head_scan;                       // [P + 1]  exclusive scan of "position p starts a run of equal keys"
    void *cub;
    size_t cub_bytes;
};

size_t gram_ws(void *base, int64_t n_pairs, GramWs *ws) {
    size_t cb_sort = 0, cb_scan = 0;
    unsigned long long *nk = nullptr;
    double *nv = nullptr;
    int32_t *n32 = nullptr;
    const int64_t n = std::max<int64_t>(n_pairs, 1);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, cb_sort, nk, nk, nv, nv, (int)n, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, cb_scan, n32, n32, (int)(n + 1), (hipStream_t)0);
    const size_t cb = std::max(cb_sort, cb_scan);
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += r_align_up(bytes, 256); return p + at; };
    const uintptr_t a_ki = take((size_t)n * 8), a_ko = take((size_t)n * 8), a_vi = take((size_t)n * 8), a_vo = take((size_t)n * 8),
                    a_hs = take((size_t)(n + 1) * 4), a_cub = take(cb);
    if (ws) {
        ws->keys_in = reinterpret_cast<unsigned long long *>(a_ki);
        ws->keys_out = reinterpret_cast<unsigned long long *>(a_ko);
        ws->vals_in = reinterpret_cast<double *>(a_vi);
        ws->vals_out = reinterpret_cast<double *>(a_vo);
        ws->head_scan = reinterpret_cast<int32_t *>(a_hs);
        ws->cub = reinterpret_cast<void *>(a_cub);
        ws->cub_bytes = cb;
    }
    return off + 256;
}

// The row that holds entry e: the last r in [0, n_rows) with rowptr[r] <= e (rows without entries are stepped over).
__host__ __device__ inline int32_t row_of_entry(const int32_t *__restrict__ rowptr, int32_t n_rows, int32_t e) {
    int32_t lo = 0, hi = n_rows;              // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// incount[u] = entries of the item rows whose column is user u.  A column outside [0, split) in an item row is not an
// edge of a user|item graph: it is not counted here and never expanded, and its entry does not survive the reduction.
__global__ void k_reduce_incount(const int32_t *__restrict__ rowptr, const lgc_entry *__restrict__ entries, int32_t n_nodes,
                                 int32_t split, int32_t n_edges, int32_t *__restrict__ incount) {
    const int32_t e_begin = max(rowptr[split], 0), e_end = min(rowptr[n_nodes], n_edges);
    for (int64_t e = e_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e_end; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = entries[e].col;
        if (c >= 0 && c < split) atomicAdd(incount + c, 1);
    }
}

// keep[u] = 1 unless user u has at most max_deg entries in its own row AND is named by at most max_deg item rows.
__global__ void k_reduce_keep(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ incount, int32_t split,
                              int32_t max_deg, int32_t *__restrict__ keep) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > split) return;
    int32_t k = 0;
    if (u < split) k = (rowptr[u + 1] - rowptr[u] <= max_deg && incount[u] <= max_deg) ? 0 : 1;
    keep[u] = k;                              // element `split` is the scan's trailing zero
}

// user_map[u] = new id of a kept user, -1 for an eliminated one (keep_scan is the exclusive scan of the flags).
__global__ void k_reduce_user_map(const int32_t *__restrict__ keep_scan, int32_t split, int32_t *__restrict__ user_map) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= split) return;
    user_map[u] = keep_scan[u + 1] != keep_scan[u] ? keep_scan[u] : -1;
}

// Per entry: does it survive (user rows: the row is kept and the column is an item; item rows: the column is a kept
// user), and how many (item, item) pairs does it expand into (item rows: the row length of an eliminated column).
__global__ void k_reduce_entry_flags(const int32_t *__restrict__ rowptr, const lgc_entry *__restrict__ entries, int32_t n_nodes,
                                     int32_t split, const int32_t *__restrict__ user_map, int32_t *__restrict__ ent_flag,
                                     long long *__restrict__ pair_count, int32_t n_edges) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > n_edges) return;
    int32_t flag = 0;
    long long pairs = 0;
    if (e < n_edges) {
        const int32_t row = row_of_entry(rowptr, n_nodes, (int32_t)e);
        const int32_t c = entries[e].col;
        if (row < split) {
            flag = (user_map[row] >= 0 && c >= split && c < n_nodes) ? 1 : 0;
        } else if (c >= 0 && c < split) {
            if (user_map[c] >= 0) flag = 1;
            else pairs = rowptr[c + 1] - rowptr[c];
        }
    }
    ent_flag[e] = flag;                       // element n_edges is the scans' trailing zero
    pair_count[e] = pairs;
}

__global__ void k_reduce_totals(const int32_t *__restrict__ rowptr, int32_t n_edges, int32_t split,
                                const int32_t *__restrict__ keep_scan, const int32_t *__restrict__ ent_scan,
                                const long long *__restrict__ pair_scan, long long *__restrict__ totals) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    totals[0] = keep_scan[split];             // n_h
    totals[1] = ent_scan[min(max(rowptr[split], 0), n_edges)];   // entries of the kept user rows
    totals[2] = ent_scan[n_edges];            // entries of the reduced CSR
    totals[3] = pair_scan[n_edges];           // expanded pairs
}

__global__ void k_reduce_fill_rowptr(const int32_t *__restrict__ rowptr, int32_t n_nodes, int32_t split, int32_t n_h,
                                     const int32_t *__restrict__ user_map, const int32_t *__restrict__ ent_scan,
                                     int32_t n_edges, int32_t *__restrict__ rowptr_out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_nodes) return;
    if (r == n_nodes) {
        rowptr_out[n_h + (n_nodes - split)] = ent_scan[n_edges];
        return;
    }
    const int32_t nr = r < split ? user_map[r] : n_h + ((int32_t)r - split);
    if (nr >= 0 && nr < n_h + (n_nodes - split)) rowptr_out[nr] = ent_scan[min(max(rowptr[r], 0), n_edges)];
}

__global__ void k_reduce_fill_entries(const int32_t *__restrict__ rowptr, const lgc_entry *__restrict__ entries, int32_t n_nodes,
                                      int32_t split, int32_t n_h, const int32_t *__restrict__ user_map,
                                      const int32_t *__restrict__ ent_scan, int32_t n_edges, int32_t n_out,
                                      lgc_entry *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int32_t dst = ent_scan[e];
    if (ent_scan[e + 1] == dst || dst < 0 || dst >= n_out) return;
    const int32_t row = row_of_entry(rowptr, n_nodes, (int32_t)e);
    lgc_entry en = entries[e];
    en.col = row < split ? en.col - (split - n_h) : user_map[en.col];     // the flag vouches for both ranges
    out[dst] = en;                                                        // the value: a bit-identical copy
}

// Every entry (i, u) of an item row with u eliminated times every entry (u, j) of u's row: key (i, j), product in fp64.
// The pairs of one entry are consecutive and in the order of u's row; the entries are in CSR order -- with the stable
// sort that fixes the order in which equal keys are summed.
__global__ void k_gram_expand(const int32_t *__restrict__ rowptr, const lgc_entry *__restrict__ entries, int32_t n_nodes,
                              int32_t split, const long long *__restrict__ pair_scan, long long n_pairs,
                              int32_t n_edges, unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    const int64_t e = (int64_t)max(rowptr[split], 0) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const long long at = pair_scan[e], cnt = pair_scan[e + 1] - at;
    if (cnt <= 0 || at < 0 || at + cnt > n_pairs) return;
    const int32_t row = row_of_entry(rowptr, n_nodes, (int32_t)e);
    const lgc_entry a = entries[e];                                       // A[i, u]; cnt > 0 says u is a user
    const int32_t s = rowptr[a.col];
    if (s < 0 || s + cnt > n_edges) return;
    long long w = at;
    for (int32_t k = 0; k < cnt; ++k) {
        const lgc_entry b = entries[s + k];                               // A[u, j]
        if (b.col < split || b.col >= n_nodes) continue;                  // not an item: no pair (the slot keeps its filler)
        keys[w] = ((unsigned long long)(uint32_t)(row - split) << 32) | (uint32_t)(b.col - split);
        vals[w] = (double)a.val * (double)b.val;
        ++w;
    }
}

// Slots the expansion may leave unwritten (a user row naming a non-item) sort last and carry zero.
__global__ void k_gram_prefill(unsigned long long *__restrict__ keys, double *__restrict__ vals, long long n_pairs) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    keys[p] = ~0ull;
    vals[p] = 0.0;
}

__global__ void k_gram_heads(const unsigned long long *__restrict__ keys, long long n_pairs, int32_t *__restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_pairs) return;
    int32_t h = 0;
    if (p < n_pairs && keys[p] != ~0ull) h = (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
    head[p] = h;                              // element n_pairs is the scan's trailing zero
}

// One thread per run of equal keys: the run's products summed in fp64 in sorted (= expansion) order, rounded once.
__global__ void k_gram_fill_entries(const unsigned long long *__restrict__ keys, const double *__restrict__ vals,
                                    const int32_t *__restrict__ head_scan, long long n_pairs, int32_t n_h, int32_t n_out,
                                    lgc_entry *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t dst = head_scan[p];
    if (head_scan[p + 1] == dst || dst < 0 || dst >= n_out) return;
    const unsigned long long key = keys[p];
    double sum = 0.0;
    for (int64_t q = p; q < n_pairs && keys[q] == key; ++q) sum += vals[q];
    lgc_entry en;
    en.col = n_h + (int32_t)(uint32_t)(key & 0xFFFFFFFFull);
    en.val = (float)sum;
    out[dst] = en;
}

// rowptr of G_L over the compact numbering: user rows are empty, item row i starts at the first run whose key row >= i.
__global__ void k_gram_fill_rowptr(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ head_scan,
                                   long long n_pairs, int32_t n_h, int32_t n_items, int32_t *__restrict__ rowptr_out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > (int64_t)n_h + n_items) return;
    if (r <= n_h) {
        rowptr_out[r] = 0;
        return;
    }
    const unsigned long long want = (unsigned long long)(uint32_t)(r - n_h) << 32;
    long long lo = 0, hi = n_pairs;           // first position whose key >= want (fillers are ~0: beyond every row)
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    rowptr_out[r] = head_scan[lo];            // lo == n_pairs: the total
}

// ---------------------------------------------------------------------------------------------------------------------
// The concatenated operator (lgc_reduce_concat, lgc_reduce_concat_host).  Every array element is one call of a function
// below, from a kernel or from the host loop: the same arithmetic on both sides, no scan, no sort, no atomics.
// ---------------------------------------------------------------------------------------------------------------------
struct Concat {
    const int32_t *rp;          // reduced CSR, compact numbering: [n_kept + n_items + 1]
    const lgc_entry *ent;
    const int32_t *grp;         // G_L, same numbering
    const lgc_entry *gent;
    int32_t n_kept, n_items, n_gaps, gap_rows, n_phys, n_gram, n_out;
    int32_t *pos, *gap_start, *rowptr_out;
    lgc_entry *out;
};

// Band of kept user h: where the entries of the kept user rows before it fall among n_gaps equal shares (for a
// structurally symmetric graph these are the column counts of R_H^T: the sweep planner's own band rule).
__host__ __device__ inline int32_t cc_band(const Concat &c, int32_t h) {
    const int64_t ne = c.rp[c.n_kept];
    if (ne <= 0) return 0;
    const int64_t b = (int64_t)c.rp[h] * c.n_gaps / ne;
    return (int32_t)(b < c.n_gaps - 1 ? b : c.n_gaps - 1);
}

// Kept users of bands 0 .. b: the first h with rp[h] * n_gaps >= ne * (b + 1) (rp does not decrease).
__host__ __device__ inline int32_t cc_users_upto(const Concat &c, int32_t b) {
    const int64_t ne = c.rp[c.n_kept];
    if (b >= c.n_gaps - 1 || ne <= 0) return c.n_kept;
    int32_t lo = 0, hi = c.n_kept;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)c.rp[mid] * c.n_gaps < ne * (b + 1)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__host__ __device__ inline int32_t cc_min(int64_t a, int64_t b) { return (int32_t)(a < b ? a : b); }

// pos[h], h < n_kept; gap_start[b], b < n_gaps (index n_kept + b)
__host__ __device__ inline void cc_layout_at(const Concat &c, int64_t t) {
    if (t < c.n_kept) c.pos[t] = (int32_t)t + c.gap_rows * cc_band(c, (int32_t)t);
    else if (t < (int64_t)c.n_kept + c.n_gaps) {
        const int32_t b = (int32_t)(t - c.n_kept);
        c.gap_start[b] = cc_users_upto(c, b) + c.gap_rows * b;
    }
}

// rowptr_out[r], r <= n_phys + n_items.  Entries are laid out in physical row order: the kept users of band 0, the
// one-entry rows of gap 0, the users of band 1, ... then the item rows (each: its R_H^T entries, then its G_L entries).
__host__ __device__ inline void cc_rowptr_at(const Concat &c, int64_t r) {
    if (r > (int64_t)c.n_phys + c.n_items) return;
    int64_t v;
    if (r >= c.n_phys) {
        const int32_t i = (int32_t)(r - c.n_phys);
        v = (int64_t)c.rp[c.n_kept] + c.n_items + (c.rp[c.n_kept + i] - c.rp[c.n_kept]) + c.grp[c.n_kept + i];
    } else {
        int32_t before = 0;                                             // gaps that start at or before row r
        while (before < c.n_gaps && c.gap_start[before] <= r) ++before;
        if (before > 0 && r < (int64_t)c.gap_start[before - 1] + c.gap_rows) {
            const int32_t b = before - 1;
            const int64_t j = (int64_t)b * c.gap_rows + (r - c.gap_start[b]);
            v = (int64_t)c.rp[c.gap_start[b] - c.gap_rows * b] + cc_min(j, c.n_items);
        } else {
            const int32_t h = (int32_t)(r - (int64_t)c.gap_rows * before);
            v = (int64_t)c.rp[h] + cc_min((int64_t)before * c.gap_rows, c.n_items);
        }
    }
    c.rowptr_out[r] = (int32_t)v;
}

// Source element t of the four lists, in this order: the kept user rows' entries, the items (one gap row each), the
// item rows' entries on kept users, the entries of G_L.
__host__ __device__ inline void cc_entry_at(const Concat &c, int64_t t) {
    const int64_t n_user = c.rp[c.n_kept], n_all = c.rp[c.n_kept + c.n_items];
    const int64_t first_item_entry = n_user + c.n_items;                // of the output
    int64_t dst;
    lgc_entry en;
    if (t < n_user) {                                                   // (h, item): the item's row moves behind the gaps
        const int32_t h = row_of_entry(c.rp, c.n_kept, (int32_t)t);
        en = c.ent[t];
        en.col = c.n_phys + (en.col - c.n_kept);
        dst = t + cc_min((int64_t)cc_band(c, h) * c.gap_rows, c.n_items);
    } else if ((t -= n_user) < c.n_items) {                             // gap row of item t: 1.0 * the item's row
        const int32_t b = (int32_t)(t / c.gap_rows);
        en.col = c.n_phys + (int32_t)t;
        en.val = 1.0f;
        dst = (int64_t)c.rp[c.gap_start[b] - c.gap_rows * b] + t;
    } else if ((t -= c.n_items) < n_all - n_user) {                     // (item i, h)
        const int64_t e = n_user + t;
        const int32_t i = row_of_entry(c.rp + c.n_kept, c.n_items, (int32_t)e);
        en = c.ent[e];
        en.col = c.pos[en.col];
        dst = first_item_entry + t + c.grp[c.n_kept + i];
    } else if ((t -= n_all - n_user) < c.n_gram) {                      // (item i, item j): column = j's gap row
        const int32_t i = row_of_entry(c.grp + c.n_kept, c.n_items, (int32_t)t);
        en = c.gent[t];
        const int32_t j = en.col - c.n_kept;
        en.col = c.gap_start[j / c.gap_rows] + j % c.gap_rows;
        dst = first_item_entry + (c.rp[c.n_kept + i + 1] - n_user) + t;
    } else {
        return;
    }
    if (dst >= 0 && dst < c.n_out) c.out[dst] = en;
}

__global__ void k_concat_layout(Concat c) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    cc_layout_at(c, t);
}
__global__ void k_concat_rowptr(Concat c) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    cc_rowptr_at(c, r);
}
__global__ void k_concat_entries(Concat c) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < c.n_out) cc_entry_at(c, t);
}

int concat_args(const int32_t *rowptr, const lgc_entry *entries, int64_t n_entries, const int32_t *gram_rowptr,
                const lgc_entry *gram_entries, int64_t n_gram, int64_t n_kept, int64_t n_items, int32_t n_gaps,
                int32_t *user_pos, int32_t *gap_start, int32_t *rowptr_out, lgc_entry *entries_out, int64_t n_out, Concat *c) {
    if (n_entries < 0 || n_gram < 0 || n_kept < 0 || n_items < 1 || n_gaps < 1 || n_out < 0) return LGC_E_INVAL;
    if (n_gaps > LGC_REDUCE_MAX_GAPS) return LGC_E_RANGE;
    const int64_t gap_rows = (n_items + n_gaps - 1) / n_gaps, n_phys = n_kept + gap_rows * n_gaps;
    if (n_phys + n_items >= INT32_MAX || n_entries + n_items + n_gram >= INT32_MAX) return LGC_E_RANGE;
    if (!rowptr || !gram_rowptr || !gap_start || !rowptr_out || !entries_out || (n_entries > 0 && !entries) ||
        (n_gram > 0 && !gram_entries) || (n_kept > 0 && !user_pos) || n_out != n_entries + n_items + n_gram)
        return LGC_E_INVAL;
    *c = Concat{rowptr, entries, gram_rowptr, gram_entries, (int32_t)n_kept, (int32_t)n_items, n_gaps, (int32_t)gap_rows,
                (int32_t)n_phys, (int32_t)n_gram, (int32_t)n_out, user_pos, gap_start, rowptr_out, entries_out};
    return 0;
}

int reduce_args_ok(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split) {
    if (n_nodes < 0 || n_edges < 0 || split < 0) return LGC_E_INVAL;
    if (n_nodes >= INT32_MAX || n_edges >= INT32_MAX) return LGC_E_RANGE;
    if (!rowptr || split <= 0 || split >= n_nodes || (n_edges > 0 && !entries)) return LGC_E_INVAL;
    return 0;
}

}  // namespace

extern "C" {

size_t lgc_reduce_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    if (n_nodes < 0 || n_edges < 0 || n_nodes >= INT32_MAX || n_edges >= INT32_MAX) return 0;
    return reduce_ws(nullptr, n_nodes, n_edges, nullptr);
}

int lgc_reduce_count(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                     int32_t max_deg, void *workspace, size_t workspace_bytes, int32_t *user_map, int64_t *totals,
                     void *stream_) {
    if (const int rc = reduce_args_ok(rowptr, entries, n_nodes, n_edges, split)) return rc;
    if (max_deg < 0 || !workspace || !user_map || !totals) return LGC_E_INVAL;
    if (workspace_bytes < lgc_reduce_workspace_bytes(n_nodes, n_edges)) return LGC_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return LGC_E_ALIGN;
    hipStream_t st = as_stream(stream_);
    ReduceWs ws;
    reduce_ws(workspace, n_nodes, n_edges, &ws);
    const int32_t n = (int32_t)n_nodes, sp = (int32_t)split;
    hipError_t err = hipMemsetAsync(ws.incount, 0, (size_t)(split + 1) * 4, st);
    if (err != hipSuccess) return (int)err;
    if (n_edges > 0)
        hipLaunchKernelGGL(k_reduce_incount, dim3((unsigned)std::min<int64_t>(ceil_div(n_edges, kBlock), 256 * 16)), dim3(kBlock), 0,
                           st, rowptr, entries, n, sp, (int32_t)n_edges, ws.incount);
    hipLaunchKernelGGL(k_reduce_keep, dim3(ceil_div(split + 1, kBlock)), dim3(kBlock), 0, st, rowptr, ws.incount, sp, max_deg,
                       ws.keep_scan);
    err = hipcub::DeviceScan::ExclusiveSum(ws.cub, ws.cub_bytes, ws.keep_scan, ws.keep_scan, (int)(split + 1), st);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(k_reduce_user_map, dim3(ceil_div(split, kBlock)), dim3(kBlock), 0, st, ws.keep_scan, sp, user_map);
    hipLaunchKernelGGL(k_reduce_entry_flags, dim3(ceil_div(n_edges + 1, kBlock)), dim3(kBlock), 0, st, rowptr, entries, n, sp,
                       user_map, ws.ent_scan, ws.pair_scan, (int32_t)n_edges);
    err = hipcub::DeviceScan::ExclusiveSum(ws.cub, ws.cub_bytes, ws.ent_scan, ws.ent_scan, (int)(n_edges + 1), st);
    if (err != hipSuccess) return (int)err;
    err = hipcub::DeviceScan::ExclusiveSum(ws.cub, ws.cub_bytes, ws.pair_scan, ws.pair_scan, (int)(n_edges + 1), st);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(k_reduce_totals, dim3(1), dim3(64), 0, st, rowptr, (int32_t)n_edges, sp, ws.keep_scan, ws.ent_scan, ws.pair_scan,
                       reinterpret_cast<long long *>(totals));
    return (int)hipGetLastError();
}

int lgc_reduce_fill(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                    const void *workspace, const int32_t *user_map, int64_t n_kept, int64_t n_out, int32_t *rowptr_out,
                    lgc_entry *entries_out, void *stream_) {
    if (const int rc = reduce_args_ok(rowptr, entries, n_nodes, n_edges, split)) return rc;
    if (!workspace || !user_map || !rowptr_out || n_kept < 0 || n_kept > split || n_out < 0 || n_out > n_edges ||
        (n_out > 0 && !entries_out))
        return LGC_E_INVAL;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return LGC_E_ALIGN;
    hipStream_t st = as_stream(stream_);
    ReduceWs ws;
    reduce_ws(const_cast<void *>(workspace), n_nodes, n_edges, &ws);
    const int32_t n = (int32_t)n_nodes, sp = (int32_t)split;
    hipLaunchKernelGGL(k_reduce_fill_rowptr, dim3(ceil_div(n_nodes + 1, kBlock)), dim3(kBlock), 0, st, rowptr, n, sp,
                       (int32_t)n_kept, user_map, ws.ent_scan, (int32_t)n_edges, rowptr_out);
    if (n_out > 0)
        hipLaunchKernelGGL(k_reduce_fill_entries, dim3(ceil_div(n_edges, kBlock)), dim3(kBlock), 0, st, rowptr, entries, n, sp,
                           (int32_t)n_kept, user_map, ws.ent_scan, (int32_t)n_edges, (int32_t)n_out, entries_out);
    return (int)hipGetLastError();
}

size_t lgc_reduce_gram_workspace_bytes(int64_t n_pairs) {
    if (n_pairs < 0 || n_pairs >= INT32_MAX) return 0;
    return gram_ws(nullptr, n_pairs, nullptr);
}

int lgc_reduce_gram_count(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                          const void *workspace, int64_t n_pairs, void *gram_workspace, size_t gram_workspace_bytes,
                          int64_t *total, void *stream_) {
    if (const int rc = reduce_args_ok(rowptr, entries, n_nodes, n_edges, split)) return rc;
    if (n_pairs < 0 || !workspace || !total) return LGC_E_INVAL;
    if (n_pairs >= INT32_MAX) return LGC_E_RANGE;
    if (!gram_workspace) return LGC_E_INVAL;
    if (gram_workspace_bytes < lgc_reduce_gram_workspace_bytes(n_pairs)) return LGC_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0 || reinterpret_cast<uintptr_t>(gram_workspace) % 256 != 0) return LGC_E_ALIGN;
    hipStream_t st = as_stream(stream_);
    hipError_t err = hipMemsetAsync(total, 0, sizeof(int64_t), st);
    if (err != hipSuccess) return (int)err;
    if (n_pairs == 0) return 0;
    ReduceWs ws;
    reduce_ws(const_cast<void *>(workspace), n_nodes, n_edges, &ws);
    GramWs gw;
    gram_ws(gram_workspace, n_pairs, &gw);
    const int32_t n = (int32_t)n_nodes, sp = (int32_t)split;
    hipLaunchKernelGGL(k_gram_prefill, dim3(ceil_div(n_pairs, kBlock)), dim3(kBlock), 0, st, gw.keys_in, gw.vals_in,
                       (long long)n_pairs);
    // the grid covers every entry: the kernel starts at the first entry of the item rows, which only the device knows
    hipLaunchKernelGGL(k_gram_expand, dim3(ceil_div(n_edges, kBlock)), dim3(kBlock), 0, st, rowptr, entries, n, sp, ws.pair_scan,
                       (long long)n_pairs, (int32_t)n_edges, gw.keys_in, gw.vals_in);
    err = hipcub::DeviceRadixSort::SortPairs(gw.cub, gw.cub_bytes, gw.keys_in, gw.keys_out, gw.vals_in, gw.vals_out, (int)n_pairs,
                                             0, 64, st);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(k_gram_heads, dim3(ceil_div(n_pairs + 1, kBlock)), dim3(kBlock), 0, st, gw.keys_out, (long long)n_pairs,
                       gw.head_scan);
    err = hipcub::DeviceScan::ExclusiveSum(gw.cub, gw.cub_bytes, gw.head_scan, gw.head_scan, (int)(n_pairs + 1), st);
    if (err != hipSuccess) return (int)err;
    // the int32 total widened on the way out: a 4-byte copy into the zeroed 8-byte word (little endian)
    err = hipMemcpyAsync(total, gw.head_scan + n_pairs, sizeof(int32_t), hipMemcpyDeviceToDevice, st);
    if (err != hipSuccess) return (int)err;
    return (int)hipGetLastError();
}

int lgc_reduce_gram_fill(const void *gram_workspace, int64_t n_pairs, int64_t n_kept, int64_t n_items, int64_t n_out,
                         int32_t *rowptr_out, lgc_entry *entries_out, void *stream_) {
    if (n_pairs < 0 || n_kept < 0 || n_items < 1 || n_out < 0 || !rowptr_out) return LGC_E_INVAL;
    if (n_pairs >= INT32_MAX || n_kept + n_items >= INT32_MAX) return LGC_E_RANGE;
    if (n_out > n_pairs || (n_pairs > 0 && !gram_workspace) || (n_out > 0 && !entries_out)) return LGC_E_INVAL;
    if (reinterpret_cast<uintptr_t>(gram_workspace) % 256 != 0) return LGC_E_ALIGN;
    hipStream_t st = as_stream(stream_);
    const int64_t rows = n_kept + n_items;
    if (n_pairs == 0) return (int)hipMemsetAsync(rowptr_out, 0, (size_t)(rows + 1) * 4, st);
    GramWs gw;
    gram_ws(const_cast<void *>(gram_workspace), n_pairs, &gw);
    hipLaunchKernelGGL(k_gram_fill_rowptr, dim3(ceil_div(rows + 1, kBlock)), dim3(kBlock), 0, st, gw.keys_out, gw.head_scan,
                       (long long)n_pairs, (int32_t)n_kept, (int32_t)n_items, rowptr_out);
    if (n_out > 0)
        hipLaunchKernelGGL(k_gram_fill_entries, dim3(ceil_div(n_pairs, kBlock)), dim3(kBlock), 0, st, gw.keys_out, gw.vals_out,
                           gw.head_scan, (long long)n_pairs, (int32_t)n_kept, (int32_t)n_out, entries_out);
    return (int)hipGetLastError();
}

int64_t lgc_reduce_concat_rows(int64_t n_kept, int64_t n_items, int32_t n_gaps) {
    if (n_kept < 0 || n_items < 1 || n_gaps < 1 || n_gaps > LGC_REDUCE_MAX_GAPS) return -1;
    return n_kept + (n_items + n_gaps - 1) / n_gaps * n_gaps;
}

int lgc_reduce_concat(const int32_t *rowptr, const lgc_entry *entries, int64_t n_entries, const int32_t *gram_rowptr,
                      const lgc_entry *gram_entries, int64_t n_gram, int64_t n_kept, int64_t n_items, int32_t n_gaps,
                      int32_t *user_pos, int32_t *gap_start, int32_t *rowptr_out, lgc_entry *entries_out, int64_t n_out,
                      void *stream_) {
    Concat c;
    if (const int rc = concat_args(rowptr, entries, n_entries, gram_rowptr, gram_entries, n_gram, n_kept, n_items, n_gaps,
                                   user_pos, gap_start, rowptr_out, entries_out, n_out, &c))
        return rc;
    hipStream_t st = as_stream(stream_);
    hipLaunchKernelGGL(k_concat_layout, dim3(ceil_div(n_kept + n_gaps, kBlock)), dim3(kBlock), 0, st, c);
    hipLaunchKernelGGL(k_concat_rowptr, dim3(ceil_div((int64_t)c.n_phys + n_items + 1, kBlock)), dim3(kBlock), 0, st, c);
    hipLaunchKernelGGL(k_concat_entries, dim3(ceil_div(n_out, kBlock)), dim3(kBlock), 0, st, c);
    return (int)hipGetLastError();
}

int lgc_reduce_concat_host(const int32_t *rowptr, const lgc_entry *entries, int64_t n_entries, const int32_t *gram_rowptr,
                           const lgc_entry *gram_entries, int64_t n_gram, int64_t n_kept, int64_t n_items, int32_t n_gaps,
                           int32_t *user_pos, int32_t *gap_start, int32_t *rowptr_out, lgc_entry *entries_out, int64_t n_out) {
    Concat c;
    if (const int rc = concat_args(rowptr, entries, n_entries, gram_rowptr, gram_entries, n_gram, n_kept, n_items, n_gaps,
                                   user_pos, gap_start, rowptr_out, entries_out, n_out, &c))
        return rc;
    if (rowptr[n_kept + n_items] != n_entries || gram_rowptr[n_kept + n_items] != n_gram) return LGC_E_INVAL;
    for (int64_t t = 0; t < n_kept + n_gaps; ++t) cc_layout_at(c, t);
    for (int64_t r = 0; r <= (int64_t)c.n_phys + n_items; ++r) cc_rowptr_at(c, r);
    for (int64_t t = 0; t < n_out; ++t) cc_entry_at(c, t);
    return 0;
}

}  // extern "C"

// lgconv_rerank.hip -- diversified re-ranking: greedy maximal marginal relevance over a candidate list, and the intra-list
// diversity that judges it.  One wavefront per row; the N x N similarity matrix of a list never exists.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// Geometry.  Every wavefront owns one row of candidates, so the argmax of a step and the hand-out
// of the chosen row are cross-lane operations without a barrier; a workgroup is ONE wavefront, so that as many rows are
// resident on a CU as their staged candidates leave room for (five at D = 64, N = 100).  Lane l owns
// positions l, l + 64, l + 128, l + 192: their lambda * rel, their penalty and an "open" bit stay in registers.  Where the
// candidate rows fit kRrLdsPerWave they are staged once in LDS (route LDS), whole width padded with zeros to 4 columns,
// with a row stride of 4 * odd floats: 16 consecutive rows start on 16 different bank quads, so the 16-byte reads of 64
// lanes, each of its own row, do not collide, and the read of the chosen row is one broadcast.  Otherwise (route GLOBAL)
// every step reads the rows from memory again; after the first step they sit in L2.  Both routes run the same chain.
constexpr int kRrBlock = kWave;               // one wavefront a workgroup: the grid is the rows
constexpr int kRrStage = 8;                   // 16-byte loads a lane has in flight while the rows are staged
constexpr int kRrSlots = LGC_RERANK_MAX_CAND / kWave;
constexpr int kRrLdsPerWave = 36 * 1024;
static_assert(kRrSlots * kWave == LGC_RERANK_MAX_CAND, "a lane owns the same number of positions");
static_assert(kRrLdsPerWave <= 48 * 1024, "the staged rows stay inside the default LDS limit of a workgroup");

// floats between two staged rows: the width rounded up to 4, in 16-byte groups an odd number
inline __host__ __device__ int rr_row_stride(int dim) { return 4 * (((dim + 3) / 4) | 1); }
inline bool rr_staged(int n, int dim) { return (int64_t)n * rr_row_stride(dim) * (int64_t)sizeof(float) <= kRrLdsPerWave; }

struct RrCuts {
    int32_t c[LGC_RM_MAX_CUTOFFS];
    int32_t n;
};

struct RrArgs {
    const float *items;
    int64_t item_stride;
    const float *scale;
    const int64_t *cand;                      // the candidate rows (lgc_rerank_mmr) or the lists (lgc_list_diversity)
    int64_t cand_stride;
    const float *rel;
    int64_t rel_stride;
    int64_t *out_index;
    int32_t *out_pos;
    float *out_value;
    double *out_div;
    int64_t out_stride;
    int32_t *status;
    int32_t n_items, n_rows, dim, n_cand, k, ls;   // ls = rr_row_stride(dim)
    float lambda, oml;
    RrCuts cuts;
};

// What a row's wavefront keeps of its positions, and where their item rows are read from.
template <bool STAGED>
struct RrRow {
    int id[kRrSlots];                         // the item of position lane + 64 s, -1 = none
    float sc[kRrSlots];                       // scale[item], 1 without a scale
    const float *src[kRrSlots];               // the item's row: in LDS (STAGED) or in the table
    const int *ids;                           // [n] in LDS: the same ids, for every lane
    const float *scs;                         // [n] in LDS: the same scales (a step's chosen one is read from here, not from memory)
    const float *rows;                        // the wavefront's staged rows

    // Reads positions [0, n) of the list at `list`: -1 is empty, any other id outside the table is skipped and flagged, both
    // before an address is formed from it.  Contains the kernel's only barriers.
    __device__ __forceinline__ void take(const RrArgs &p, const int64_t *__restrict__ list, int n, int *ids_w,
                                         float *scs_w, float *rows_w, int lane) {
        ids = ids_w;
        scs = scs_w;
        rows = rows_w;
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s) {
            const int pos = lane + kWave * s;
            id[s] = -1;
            sc[s] = 1.0f;
            if (pos < n) {
                const int64_t v = list[pos];
                if (v >= 0 && v < p.n_items) {
                    id[s] = (int)v;
                    if (p.scale) sc[s] = p.scale[v];
                } else if (v != -1) {
                    atomicOr(p.status, LGC_ST_INDEX_OOB);
                }
                ids_w[pos] = id[s];
                scs_w[pos] = sc[s];
            }
            src[s] = STAGED ? rows_w + (size_t)pos * p.ls : p.items + (int64_t)max(id[s], 0) * p.item_stride;
        }
        __syncthreads();
        if (STAGED) {
            // 16 lanes fetch a row of 64 floats; kRrStage loads are issued before the first is stored, so the
            // latency of a gather from memory is paid once per kRrStage KiB and not once per KiB
            const int groups = (p.dim + 3) / 4, total = n * groups;
            for (int e0 = lane; e0 < total; e0 += kWave * kRrStage) {
                f4 v[kRrStage];
                int dst[kRrStage];
#pragma unroll
                for (int i = 0; i < kRrStage; ++i) {
                    const int e = e0 + kWave * i;
                    dst[i] = -1;
                    v[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (e < total) {
                        const int row = e / groups, g = e - row * groups;
                        const int it = ids_w[row];
                        if (it >= 0) {
                            dst[i] = row * p.ls + 4 * g;
                            v[i] = load4<false>(p.items + (int64_t)it * p.item_stride, 4 * g, p.dim);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kRrStage; ++i)
                    if (dst[i] >= 0) *reinterpret_cast<f4 *>(rows_w + dst[i]) = v[i];
            }
            __syncthreads();
        }
    }

    __device__ __forceinline__ const float *row_of(const RrArgs &p, int pos) const {
        return STAGED ? rows + (size_t)pos * p.ls : p.items + (int64_t)ids[pos] * p.item_stride;
    }

    // acc[s] = dot(row of position lane + 64 s, rc) for the slots of `live`, the others are left at +0: lgc_score_rows' chain
    // (score_chain).  The slots' chains are independent of each other.
    __device__ __forceinline__ void dots(const RrArgs &p, const float *rc, uint32_t live, int nslots, float (&acc)[kRrSlots]) const {
        const float *rp[kRrSlots];
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s) {
            rp[s] = (live >> s) & 1u ? src[s] : rc;
            acc[s] = 0.0f;
        }
#pragma unroll 4
        for (int d = 0; d < p.dim; d += 4) {
            const f4 cv = STAGED ? *reinterpret_cast<const f4 *>(rc + d) : load4<false>(rc, d, p.dim);
#pragma unroll
            for (int s = 0; s < kRrSlots; ++s) {
                if (s < nslots) {
                    const f4 a = STAGED ? *reinterpret_cast<const f4 *>(rp[s] + d) : load4<false>(rp[s], d, p.dim);
                    acc[s] = score_chain(a, cv, acc[s]);
                }
            }
        }
    }
};

template <bool STAGED>
__global__ __launch_bounds__(kRrBlock) void k_rerank_mmr(const RrArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rr_lds[];
    __shared__ int rr_ids[LGC_RERANK_MAX_CAND];
    __shared__ float rr_scs[LGC_RERANK_MAX_CAND];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int n = p.n_cand, k = p.k, nslots = (n + kWave - 1) / kWave;
    RrRow<STAGED> row;
    row.take(p, p.cand + r * p.cand_stride, n, rr_ids, rr_scs, rr_lds, lane);

    float lrel[kRrSlots], pen[kRrSlots];
    uint32_t open = 0u;                                      // bit s: position lane + 64 s is valid and not yet chosen
#pragma unroll
    for (int s = 0; s < kRrSlots; ++s) {
        pen[s] = 0.0f;
        lrel[s] = 0.0f;
        if (row.id[s] >= 0) {
            open |= 1u << s;
            lrel[s] = __fmul_rn(p.lambda, p.rel[r * p.rel_stride + lane + kWave * s]);
        }
    }
    for (int t = 0; t < k; ++t) {
        // the choice: one 64-bit word per open position, the order key of the objective above the complemented position
        u64 best = 0ull;
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s) {
            if ((open >> s) & 1u) {
                const float obj = t == 0 ? lrel[s] : __fsub_rn(lrel[s], __fmul_rn(p.oml, pen[s]));
                const u64 key = ((u64)order_key(obj) << 32) | (uint32_t)~(uint32_t)(lane + kWave * s);
                best = key > best ? key : best;
            }
        }
        best = wave_max(best);
        const int c = best ? (int)~(uint32_t)best : -1;      // the same for every lane
        if (lane == 0) {
            const int64_t o = r * k + t;
            p.out_index[o] = c >= 0 ? (int64_t)row.ids[c] : -1;
            if (p.out_pos) p.out_pos[o] = c;
            if (p.out_value) p.out_value[o] = c >= 0 ? key_value((uint32_t)(best >> 32)) : -INFINITY;
        }
        if (c < 0 || t + 1 == k) continue;                   // nothing left to choose from: the tail is -1 / -1 / -inf
        if ((c & (kWave - 1)) == lane) open &= ~(1u << (c >> 6));
        const float sj = row.scs[c];
        float acc[kRrSlots];
        row.dots(p, row.row_of(p, c), open, nslots, acc);
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s) {
            if ((open >> s) & 1u) {
                const float sim = p.scale ? __fmul_rn(__fmul_rn(acc[s], row.sc[s]), sj) : acc[s];
                pen[s] = t == 0 ? sim : ((sim != sim || sim > pen[s]) ? sim : pen[s]);
            }
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(kRrBlock) void k_list_diversity(const RrArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rr_lds[];
    __shared__ int rr_ids[LGC_RERANK_MAX_CAND];
    __shared__ float rr_scs[LGC_RERANK_MAX_CAND];
    __shared__ double rr_t[LGC_RERANK_MAX_CAND];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int n = p.cuts.c[p.cuts.n - 1];                    // positions at and past the last cutoff are never read
    const int nslots = (n + kWave - 1) / kWave;
    RrRow<STAGED> row;
    row.take(p, p.cand + r * p.cand_stride, n, rr_ids, rr_scs, rr_lds, lane);

    {
        double tb[kRrSlots];
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s) tb[s] = 0.0;
        for (int a = 0; a + 1 < n; ++a) {
            const int j = row.ids[a];                        // the same for every lane
            if (j < 0) continue;
            const float sa = row.scs[a];
            uint32_t live = 0u;                              // bit s: position lane + 64 s is valid and lies after a
#pragma unroll
            for (int s = 0; s < kRrSlots; ++s)
                if (row.id[s] >= 0 && lane + kWave * s > a) live |= 1u << s;
            float acc[kRrSlots];
            row.dots(p, row.row_of(p, a), live, nslots, acc);
#pragma unroll
            for (int s = 0; s < kRrSlots; ++s) {
                if ((live >> s) & 1u) {
                    const float sim = p.scale ? __fmul_rn(__fmul_rn(acc[s], sa), row.sc[s]) : acc[s];
                    tb[s] = __dadd_rn(tb[s], __dsub_rn(1.0, (double)sim));
                }
            }
        }
#pragma unroll
        for (int s = 0; s < kRrSlots; ++s)
            if (lane + kWave * s < n) rr_t[lane + kWave * s] = tb[s];
    }
    __syncthreads();
    if (lane == 0) {                               // the prefix over b ascending; a cutoff is a snapshot of it
        double sum = 0.0;
        int64_t valid = 0;
        int ci = 0;
        for (int b = 0; b < n; ++b) {
            sum = __dadd_rn(sum, rr_t[b]);
            valid += rr_ids[b] >= 0 ? 1 : 0;
            if (b + 1 == p.cuts.c[ci]) {
                p.out_div[r * p.out_stride + ci] = valid < 2 ? (double)NAN : __ddiv_rn(sum, (double)(valid * (valid - 1) / 2));
                ++ci;
            }
        }
    }
}

template <typename K>
int rr_launch(K staged, K global, const RrArgs &p, int n_staged, void *stream_) {
    const unsigned grid = (unsigned)p.n_rows;
    if (!rr_staged(n_staged, p.dim)) {
        hipLaunchKernelGGL(global, dim3(grid), dim3(kRrBlock), 0, as_stream(stream_), p);
        return (int)hipGetLastError();
    }
    const size_t lds = sizeof(float) * (size_t)n_staged * p.ls;   // at most kRrLdsPerWave: no opt-in
    hipLaunchKernelGGL(staged, dim3(grid), dim3(kRrBlock), lds, as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int lgc_rerank_route(int32_t n_cand, int32_t dim) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (n_cand < 1 || n_cand > LGC_RERANK_MAX_CAND) return LGC_E_RANGE;
    return rr_staged(n_cand, dim) ? LGC_RERANK_ROUTE_LDS : LGC_RERANK_ROUTE_GLOBAL;
}

int lgc_rerank_mmr(const float *items, int64_t item_stride, int64_t n_items, int32_t dim, const float *scale,
                   const int64_t *cand, int64_t cand_stride, const float *rel, int64_t rel_stride, int64_t n_rows,
                   int32_t n_cand, int32_t k, float lambda, int64_t *out_index, int32_t *out_pos, float *out_value,
                   int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!items || !cand || !rel || !out_index || !status || n_rows < 0 || item_stride < dim || lambda != lambda)
        return LGC_E_INVAL;
    if (n_cand < 1 || n_cand > LGC_RERANK_MAX_CAND || k < 1 || k > n_cand || lambda < 0.0f || lambda > 1.0f || n_items < 1 ||
        n_items >= INT32_MAX || n_rows >= INT32_MAX)
        return LGC_E_RANGE;
    if (cand_stride < n_cand || rel_stride < n_cand) return LGC_E_INVAL;
    if (!aligned_to(items, 4) || !aligned_to(scale, 4) || !aligned_to(rel, 4) || !aligned_to(out_value, 4) ||
        !aligned_to(out_pos, 4) || !aligned_to(status, 4) || !aligned_to(cand, 8) || !aligned_to(out_index, 8))
        return LGC_E_ALIGN;
    if (n_rows == 0) return 0;

    RrArgs p{};
    p.items = items;
    p.item_stride = item_stride;
    p.scale = scale;
    p.cand = cand;
    p.cand_stride = cand_stride;
    p.rel = rel;
    p.rel_stride = rel_stride;
    p.out_index = out_index;
    p.out_pos = out_pos;
    p.out_value = out_value;
    p.status = status;
    p.n_items = (int32_t)n_items;
    p.n_rows = (int32_t)n_rows;
    p.dim = dim;
    p.n_cand = n_cand;
    p.k = k;
    p.ls = rr_row_stride(dim);
    p.lambda = lambda;
    p.oml = 1.0f - lambda;
    return rr_launch(k_rerank_mmr<true>, k_rerank_mmr<false>, p, n_cand, stream_);
}

int lgc_list_diversity(const float *items, int64_t item_stride, int64_t n_items, int32_t dim, const float *scale,
                       const int64_t *lists, int64_t list_stride, int64_t n_rows, int32_t k, const int32_t *cutoffs,
                       int32_t n_cutoffs, double *out, int64_t out_stride, int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!items || !lists || !cutoffs || !out || !status || n_rows < 0 || item_stride < dim || n_cutoffs < 1 ||
        out_stride < n_cutoffs)
        return LGC_E_INVAL;
    if (k < 1 || k > LGC_RERANK_MAX_CAND || n_cutoffs > LGC_RM_MAX_CUTOFFS || n_items < 1 || n_items >= INT32_MAX ||
        n_rows >= INT32_MAX)
        return LGC_E_RANGE;
    for (int i = 0; i < n_cutoffs; ++i)
        if (cutoffs[i] < 1 || cutoffs[i] > k || (i > 0 && cutoffs[i] <= cutoffs[i - 1])) return LGC_E_RANGE;
    if (list_stride < k) return LGC_E_INVAL;
    if (!aligned_to(items, 4) || !aligned_to(scale, 4) || !aligned_to(status, 4) || !aligned_to(lists, 8) || !aligned_to(out, 8))
        return LGC_E_ALIGN;
    if (n_rows == 0) return 0;

    RrArgs p{};
    p.items = items;
    p.item_stride = item_stride;
    p.scale = scale;
    p.cand = lists;
    p.cand_stride = list_stride;
    p.out_div = out;
    p.out_stride = out_stride;
    p.status = status;
    p.n_items = (int32_t)n_items;
    p.n_rows = (int32_t)n_rows;
    p.dim = dim;
    p.n_cand = k;
    p.k = k;
    p.ls = rr_row_stride(dim);
    p.cuts.n = n_cutoffs;
    for (int i = 0; i < n_cutoffs; ++i) p.cuts.c[i] = cutoffs[i];
    return rr_launch(k_list_diversity<true>, k_list_diversity<false>, p, k, stream_);
}

}  // extern "C"

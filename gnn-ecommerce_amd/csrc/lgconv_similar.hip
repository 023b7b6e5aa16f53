// lgconv_similar.hip -- similar items: the k nearest rows of the item table by dot product or cosine, scored on the fp32
// matrix cores and selected in the same launch; no score is ever written to memory.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

typedef unsigned long long u64;

// Geometry.  A workgroup owns kNbBM query rows: gathered through query_ids and staged once in LDS,
// whole width, zero-padded to 16 columns.  Its slice of the catalogue passes through LDS in tiles of kNbBN items, each in
// chunks of kNbKC columns (the next chunk is already in registers while the current one is multiplied).  Wavefront w
// scores all kNbBM rows against items [32 w, 32 w + 32) of the tile: 4 x 2 accumulators of v_mfma_f32_16x16x4_f32, all
// independent.  Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][item l & 15]; one instruction adds k = 0, 1, 2, 3
// in that order to the chain, so a 16-column group is four instructions and the chain runs over d ascending from +0 --
// lgc_score_rows' chain.  Inside a group the LDS images hold column 4 j + q at position 4 q + j, so that the four
// operands lane quarter q needs (steps j = 0 .. 3) are ONE 16-byte read.
constexpr int kNbBM = 64, kNbBN = 128, kNbKC = 32;
constexpr int kNbBS = kNbKC + 4;              // floats; (stride / 4) odd: 16 consecutive rows hit 16 different bank quads
constexpr int kNbStage = kNbBN * (kNbKC / 4) / kBlock;   // float4 groups of a chunk a thread holds
constexpr int kNbCapMax = 128;                // a candidate buffer is compacted by one wavefront, two entries a lane
constexpr int kNbRowsPerWave = kNbBM / (kBlock / kWave);
static_assert(kNbStage * kBlock == kNbBN * (kNbKC / 4), "a chunk is dealt evenly over the workgroup");
static_assert(LGC_NEIGHBORS_MAX_K <= 64 && kNbCapMax == 2 * kWave, "compact_row holds a buffer in two registers a lane");

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// lgc_mask_topk's total order (lgconv_serve.hip): ascending with the value, every NaN the one top key, -0 = +0
__device__ __forceinline__ uint32_t order_key(float v) {
    const float w = __fadd_rn(v, 0.0f);
    const uint32_t u = __float_as_uint(w);
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return w != w ? 0xFFFFFFFFu : key;
}

// the value a key stands for (the NaN key gives the positive quiet NaN 0x7FFFFFFF)
__device__ __forceinline__ float key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// A candidate is ONE 64-bit word: the order key above the complemented item index, so that a larger word is a better
// candidate (greater value, or equal value and smaller index) and no two candidates of a row are equal.  0 = no candidate
// (the smallest real key is -inf's 0x007FFFFF).
__device__ __forceinline__ u64 pack_candidate(float v, int item) { return ((u64)order_key(v) << 32) | (uint32_t)~item; }

// Four floats of a table row starting at column d; columns >= dim read as 0 and are never touched.
__device__ __forceinline__ f4 nb_load4(const float *__restrict__ row, int d, int dim, bool live) {
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (live) {
        if (d + 4 <= dim) {
            v = *reinterpret_cast<const f4u *>(row + d);
        } else {
            if (d + 0 < dim) v.x = row[d + 0];
            if (d + 1 < dim) v.y = row[d + 1];
            if (d + 2 < dim) v.z = row[d + 2];
        }
    }
    return v;
}

// columns c0 .. c0 + 3 (c0 % 4 == 0) of a row image whose 16-column groups are permuted as above
__device__ __forceinline__ void nb_store4(float *row, int c0, f4 v) {
    float *g = row + (c0 & ~15) + ((c0 & 15) >> 2);
    g[0] = v.x;
    g[4] = v.y;
    g[8] = v.z;
    g[12] = v.w;
}

// One wavefront sorts the n <= kNbCapMax candidates of buf in descending order and keeps the first k: every lane holds two
// of them and counts how many are greater (they are all different), which is the place it writes its own to.  Reads and
// writes of one wavefront reach LDS in program order and every write depends on all the reads, so it works in place.
// Returns the new count; *thr (if given) becomes the k-th candidate once there are k, and *thv the value it stands for.
__device__ __forceinline__ int compact_row(u64 *buf, int n, int k, int lane, u64 *thr, float *thv) {
    const u64 e0 = lane < n ? buf[lane] : 0ull, e1 = lane + kWave < n ? buf[lane + kWave] : 0ull;
    int r0 = 0, r1 = 0;
    for (int t0 = 0; t0 < n; t0 += 8) {                      // eight reads in flight; the buffers are multiples of 8 long
        u64 x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = buf[t0 + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u64 v = t0 + i < n ? x[i] : 0ull;          // what lies past n is stale
            r0 += v > e0 ? 1 : 0;
            if (n > kWave) r1 += v > e1 ? 1 : 0;             // the same for every lane: a short buffer has no second entry
        }
    }
    if (lane < n && r0 < k) buf[r0] = e0;
    if (lane + kWave < n && r1 < k) buf[r1] = e1;
    if (thr && n >= k) {
        if (lane < n && r0 == k - 1) {
            *thr = e0;
            *thv = key_value((uint32_t)(e0 >> 32));
        }
        if (lane + kWave < n && r1 == k - 1) {
            *thr = e1;
            *thv = key_value((uint32_t)(e1 >> 32));
        }
    }
    return min(n, k);
}

// place j of a finished row: candidate e (0 = none)
__device__ __forceinline__ void nb_write_out(const NbArgs &p, int64_t o, u64 e) {
    p.out_index[o] = e ? (int64_t)(~(uint32_t)e & 0x7FFFFFFFu) : -1;
    if (p.out_value) p.out_value[o] = e ? key_value((uint32_t)(e >> 32)) : -INFINITY;
}

__global__ __launch_bounds__(kBlock) void k_item_neighbors(const NbArgs p) {
    extern __shared__ __attribute__((aligned(16))) float nb_lds[];
    const int sq = p.dp + 4, cap = p.cap, k = p.k, dim = p.dim;
    float *Qs = nb_lds;                                      // [kNbBM][sq]: the query rows
    float *Bs = Qs + kNbBM * sq;                             // [kNbBN][kNbBS]: a chunk of the item tile
    u64 *buf = reinterpret_cast<u64 *>(Bs + kNbBN * kNbBS);  // [kNbBM][cap]: the candidates of a row
    u64 *thr = buf + kNbBM * cap;                            // [kNbBM]: what a new candidate has to beat
    int *cnt = reinterpret_cast<int *>(thr + kNbBM);         // [kNbBM]
    int *qid = cnt + kNbBM;                                  // [kNbBM]: the item a row asks about, -1 = no row
    float *qsc = reinterpret_cast<float *>(qid + kNbBM);     // [kNbBM]: scale[query]
    float *thv = qsc + kNbBM;                                // [kNbBM]: the value of thr's key (-inf while there is none)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kNbBM;

    if (tid < kNbBM) {
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
    const int qgroups = p.dp / 4;
    for (int e = tid; e < kNbBM * qgroups; e += kBlock) {
        const int row = e / qgroups, g = e - row * qgroups;
        const int id = qid[row];
        nb_store4(Qs + row * sq, 4 * g, nb_load4(p.items + (int64_t)max(id, 0) * p.item_stride, 4 * g, dim, id >= 0));
    }

    // this slice's item tiles, and the steps (tile, chunk) over them
    const int t_lo = (int)((int64_t)p.item_tiles * blockIdx.y / p.slices);
    const int t_hi = (int)((int64_t)p.item_tiles * (blockIdx.y + 1) / p.slices);
    const int nch = (p.dp + kNbKC - 1) / kNbKC;
    const int n_steps = (t_hi - t_lo) * nch;

    f4 stage[kNbStage];
    auto load_chunk = [&](int step) {
        const int tile = t_lo + step / nch, ch = step % nch;
#pragma unroll
        for (int i = 0; i < kNbStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            const int item = tile * kNbBN + it, d = ch * kNbKC + 4 * g;
            const bool live = (uint32_t)item < (uint32_t)p.n_items && d < dim;   // below 2^31 + 128: compared unsigned
            stage[i] = nb_load4(p.items + (int64_t)(live ? item : 0) * p.item_stride, d, dim, live);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < kNbStage; ++i) {
            const int e = tid + kBlock * i, it = e >> 3, g = e & 7;
            nb_store4(Bs + it * kNbBS, 4 * g, stage[i]);
        }
    };

    f32x4 acc[4][2];
    int item[2];
    bool iok[2];
    float isc[2];
    if (n_steps > 0) load_chunk(0);
    for (int step = 0; step < n_steps; ++step) {
        const int tile = t_lo + step / nch, ch = step % nch;
        if (ch == 0) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            // what the epilogue needs of this lane's two items, requested a whole tile of products ahead
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                item[nj] = tile * kNbBN + 32 * w + 16 * nj + c;
                const bool inside = (uint32_t)item[nj] < (uint32_t)p.n_items;   // below 2^31 + 128: compared unsigned
                iok[nj] = inside && (!p.item_ok || p.item_ok[item[nj]] != 0);
                isc[nj] = (p.scale && inside) ? p.scale[item[nj]] : 1.0f;
            }
        }
        __syncthreads();                                     // the previous chunk is consumed
        store_chunk();
        __syncthreads();                                     // also orders the query rows before their first use
        if (step + 1 < n_steps) load_chunk(step + 1);        // in flight during this chunk's products
        const int groups = min(kNbKC / 16, p.dp / 16 - ch * (kNbKC / 16));
        for (int g = 0; g < groups; ++g) {
            f4 a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                a[mi] = *reinterpret_cast<const f4 *>(Qs + (16 * mi + c) * sq + ch * kNbKC + 16 * g + 4 * q);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
                b[nj] = *reinterpret_cast<const f4 *>(Bs + (32 * w + 16 * nj + c) * kNbBS + 16 * g + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], acc[mi][nj], 0, 0, 0);
        }
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
                    float s = acc[mi][nj][r];
                    if (p.scale) s = __fmul_rn(__fmul_rn(s, rs), isc[nj]);
                    acc[mi][nj][r] = s;
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
                            const u64 e = pack_candidate(acc[mi][nj][r], item[nj]);
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
            if (p.slices == 1) nb_write_out(p, r * k + lane, e);
            else p.ws[(r * p.slices + blockIdx.y) * k + lane] = e;
        }
    }
}

// One wavefront per query row merges the slices' candidates: 64 at a time are appended to the row's buffer (empty places
// skipped), which is compacted to the k best whenever another 64 might not fit.
__global__ __launch_bounds__(kBlock) void k_neighbors_merge(const NbArgs p) {
    __shared__ u64 mbuf[kBlock / kWave][kNbCapMax];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, k = p.k;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + w;
    if (r >= p.n_queries) return;
    u64 *buf = mbuf[w];
    const u64 *src = p.ws + r * p.slices * k;
    const int total = p.slices * k;
    int n = 0;
    for (int base = 0; base < total; base += kWave) {
        const u64 e = base + lane < total ? src[base + lane] : 0ull;
        const u64 have = __ballot(e != 0ull);
        if (e != 0ull) buf[n + __popcll(have & ((1ull << lane) - 1ull))] = e;
        n += __popcll(have);
        if (n > kNbCapMax - kWave) n = compact_row(buf, n, k, lane, nullptr, nullptr);
    }
    n = compact_row(buf, n, k, lane, nullptr, nullptr);
    if (lane < k) nb_write_out(p, r * k + lane, lane < n ? buf[lane] : 0ull);
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

bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

inline int nb_cap(int k) { return k <= 32 ? 64 : 96; }

// The slice count in use: the one asked for, or with 0 the smallest that gives about 512 workgroups (two for every CU);
// never more than there are item tiles.
inline int nb_slices(int64_t n_queries, int64_t n_items, int slices) {
    const int64_t item_tiles = (n_items + kNbBN - 1) / kNbBN, row_tiles = std::max<int64_t>(1, (n_queries + kNbBM - 1) / kNbBM);
    int64_t s = slices > 0 ? slices : (512 + row_tiles - 1) / row_tiles;
    s = std::min<int64_t>(s, 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, item_tiles));
}

inline bool nb_sizes_ok(int64_t n_queries, int64_t n_items, int k, int slices) {
    return n_queries >= 0 && n_items >= 1 && n_queries < INT32_MAX && n_items < INT32_MAX && k >= 1 &&
           k <= LGC_NEIGHBORS_MAX_K && slices >= 0 && slices <= 64;
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
    const int64_t item_tiles = (n_items + kNbBN - 1) / kNbBN;
    int64_t places;                                          // candidate lists of k places
    if (slices > 0) {
        const int64_t s = std::min<int64_t>(slices, item_tiles);
        places = s > 1 ? n_queries * s : 0;
    } else {
        // what the chosen count needs is not monotonic in n_queries (more row tiles, fewer slices); its two bounds are
        const int64_t s_max = std::min<int64_t>(64, item_tiles);
        places = s_max > 1 ? std::min<int64_t>(n_queries * s_max, n_queries + 512 * (int64_t)kNbBM) : 0;
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
    const int s = nb_slices(n_queries, n_items, slices);
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
    p.dp = (dim + 15) & ~15;
    p.exclude_self = exclude_self;
    p.k = k;
    p.slices = s;
    p.cap = nb_cap(k);
    p.item_tiles = (int32_t)((n_items + kNbBN - 1) / kNbBN);
    const size_t lds = sizeof(float) * ((size_t)kNbBM * (p.dp + 4) + (size_t)kNbBN * kNbBS) +
                       sizeof(u64) * ((size_t)kNbBM * p.cap + kNbBM) + (sizeof(int) * 2 + sizeof(float) * 2) * kNbBM;
    if (lds > 48 * 1024) {
        const int rc_attr = allow_big_lds(reinterpret_cast<const void *>(k_item_neighbors), 144 * 1024, &lds_ok_neighbors);
        if (rc_attr != 0) return rc_attr;
    }
    const int64_t row_tiles = (n_queries + kNbBM - 1) / kNbBM;
    hipLaunchKernelGGL(k_item_neighbors, dim3((unsigned)row_tiles, (unsigned)s), dim3(kBlock), lds, as_stream(stream_), p);
    int rc = (int)hipGetLastError();
    if (rc != 0 || s == 1) return rc;
    hipLaunchKernelGGL(k_neighbors_merge, dim3((unsigned)ceil_div(n_queries, kBlock / kWave)), dim3(kBlock), 0,
                       as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

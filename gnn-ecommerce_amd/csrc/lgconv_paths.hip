// lgconv_paths.hip -- hop distances and shortest paths over the forward CSR: bit-parallel multi-source BFS (up to 64
// sources per batch, one bit each in a 64-bit word per node) and the walk back along the stored levels.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// One adjacency entry as the CSR stores it, an 8-byte (column, value) pair.  The value is never read (the compiler
// loads the column's four bytes only): an edge of weight 0 or of negative weight is an edge (nx.Graph(edges) ignores
// weights).
typedef int e2 __attribute__((ext_vector_type(2)));

constexpr int kBfsGroup = 8;                     // lanes per short row: eight 8-byte entries = one 64-byte line per step
constexpr int kBfsRowsPerBlock = kBlock / kBfsGroup;

// What a wavefront reports for a level: nodes newly reached (counters[0]: `newly` is set by the lane that speaks for
// such a node) and the OR of the bits published (counters[2] = the sources whose frontier is not empty).  At most one
// atomic per counter word and wavefront.
__device__ __forceinline__ void report_level(bool newly, uint64_t bits, unsigned long long *counters) {
    if (__ballot(bits != 0) == 0) return;                         // wave-uniform
    const unsigned long long bal = __ballot(newly);
    bits = wave_or(bits);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (bal) atomicAdd(&counters[0], (unsigned long long)__popcll(bal));
        atomicOr(&counters[2], (unsigned long long)bits);
    }
}

__global__ __launch_bounds__(kBlock) void k_bfs_zero(uint64_t *__restrict__ seen, uint64_t *__restrict__ frontier,
                                                    int64_t n_nodes) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kBlock)
        seen[v] = frontier[v] = 0;
}

// One thread per source.  Two sources on one node set two bits of the same word: atomic OR.
__global__ void k_bfs_seed(const int64_t *__restrict__ sources, int32_t n_sources, int64_t n_nodes,
                           unsigned long long *__restrict__ seen, unsigned long long *__restrict__ frontier,
                           int32_t *__restrict__ status) {
    const int b = threadIdx.x;
    if (b >= n_sources) return;
    const int64_t s = sources[b];
    if (s < 0 || s >= n_nodes) {
        atomicOr(status, LGC_ST_INDEX_OOB);
        return;
    }
    atomicOr(&seen[s], 1ull << b);
    atomicOr(&frontier[s], 1ull << b);
}

// Rows of at most short_max entries: a group of eight lanes per row.  Longer rows get frontier_out[v] = 0 here -- the
// chunk kernel, launched after this one, ORs into it.  A row every active source has already reached is finished
// without reading one entry.
__global__ __launch_bounds__(kBlock) void k_bfs_rows(const int32_t *__restrict__ rowptr, const e2 *__restrict__ entries,
                                                    int32_t row_begin, int32_t row_end, int32_t short_max,
                                                    uint64_t active, const uint64_t *__restrict__ frontier_in,
                                                    uint64_t *__restrict__ frontier_out, uint64_t *__restrict__ seen,
                                                    unsigned long long *__restrict__ counters) {
    const int sub = threadIdx.x & (kBfsGroup - 1);
    const int64_t v = (int64_t)row_begin + (int64_t)blockIdx.x * kBfsRowsPerBlock + threadIdx.x / kBfsGroup;
    const bool live = v < row_end;
    int32_t begin = 0, end = 0;
    uint64_t was = ~0ull;
    if (live) {
        begin = rowptr[v];
        end = rowptr[v + 1];
        was = seen[v];
    }
    const bool is_short = end - begin <= short_max;
    const bool scan = live && is_short && (~was & active) != 0;
    uint64_t acc = 0;
    if (scan)
        for (int32_t e = begin + sub; e < end; e += kBfsGroup) acc |= frontier_in[entries[e].x];
#pragma unroll
    for (int off = 1; off < kBfsGroup; off <<= 1) acc |= __shfl_xor(acc, off);
    const uint64_t fresh = (live && sub == 0) ? acc & ~was : 0;
    if (live && sub == 0) {
        frontier_out[v] = fresh;                                  // 0 for a long row and for a skipped one
        if (fresh) seen[v] = was | fresh;
    }
    report_level(fresh != 0, fresh, counters);
}

// Rows longer than short_max: one wavefront per chunk of the graph's row plan, a cross-lane OR, lane 0 publishes.
// A row cut into several chunks (slot >= 0) combines through a 64-bit integer atomic OR on frontier_out[v] and on
// seen[v].  Integer OR is associative, commutative and idempotent, so whatever order the chunks arrive in the words
// end with the same bits: the result is the same on every run.  A chunk masks its partial with the seen[v] it happens
// to read; if that already holds a bit another chunk of this level published, the bit is in frontier_out[v] already.
// The node counts as newly reached for the one chunk whose OR found frontier_out[v] still 0.
__global__ __launch_bounds__(kBlock) void k_bfs_chunks(const e2 *__restrict__ entries, const lgc_chunk *__restrict__ chunks,
                                                      int32_t n_chunks, uint64_t active,
                                                      const uint64_t *__restrict__ frontier_in,
                                                      uint64_t *__restrict__ frontier_out, uint64_t *__restrict__ seen,
                                                      unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    uint64_t fresh = 0;
    bool newly = false;
    if (c < n_chunks) {                                           // wave-uniform
        const lgc_chunk ch = chunks[c];
        const uint64_t was = seen[ch.row];
        if ((~was & active) != 0) {                               // wave-uniform: every lane read the same word
            uint64_t acc = 0;
            for (int32_t e = ch.begin + lane; e < ch.end; e += kWave) acc |= frontier_in[entries[e].x];
            acc = wave_or(acc) & ~was;
            if (lane == 0 && acc) {
                fresh = acc;
                if (ch.slot < 0) {                                // the row's only chunk: plain stores
                    frontier_out[ch.row] = acc;
                    seen[ch.row] = was | acc;
                    newly = true;
                } else {
                    newly = atomicOr(reinterpret_cast<unsigned long long *>(&frontier_out[ch.row]), (unsigned long long)acc) == 0;
                    atomicOr(reinterpret_cast<unsigned long long *>(&seen[ch.row]), (unsigned long long)acc);
                }
            }
        }
    }
    report_level(newly, fresh, counters);
}

// One thread per (source, target) pair still unset.
__global__ __launch_bounds__(kBlock) void k_bfs_resolve(const int64_t *__restrict__ sources,
                                                       const int64_t *__restrict__ targets, int32_t n_sources,
                                                       int32_t n_targets, int64_t n_nodes,
                                                       const uint64_t *__restrict__ frontier, int32_t level,
                                                       int32_t *__restrict__ dist, unsigned long long *__restrict__ counters,
                                                       int32_t *__restrict__ status) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool done = false;
    if (p < (int64_t)n_sources * n_targets && dist[p] == LGC_BFS_UNSET) {
        const int b = (int)(p / n_targets);
        const int64_t s = sources[b], t = targets[p];
        if (s < 0 || s >= n_nodes || t < 0 || t >= n_nodes) {
            atomicOr(status, LGC_ST_INDEX_OOB);
            dist[p] = -1;
            done = true;
        } else if ((frontier[t] >> b) & 1ull) {
            dist[p] = level;
            done = true;
        }
    }
    const unsigned long long bal = __ballot(done);
    if (bal != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&counters[1], (unsigned long long)__popcll(bal));
}

// One wavefront per pair.  From the target, for l = d - 1 ... 0: the first column of the current node's row, in stored
// entry order, that source b reached at level l (lowest lane of the first 64-entry step that has one).
__global__ __launch_bounds__(kBlock) void k_bfs_backtrack(const int32_t *__restrict__ rowptr, const e2 *__restrict__ entries,
                                                         const uint64_t *__restrict__ levels, int32_t n_levels,
                                                         int64_t n_nodes, const int64_t *__restrict__ targets,
                                                         const int32_t *__restrict__ dist, int64_t n_pairs,
                                                         int32_t n_targets, int64_t *__restrict__ paths,
                                                         int32_t path_len) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t p = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (p >= n_pairs) return;                                     // wave-uniform
    int64_t *row = paths + p * path_len;
    const int32_t d = dist[p];
    int64_t cur = targets[p];
    const bool walk = d >= 0 && d < n_levels && d < path_len && cur >= 0 && cur < n_nodes;
    for (int i = lane; i < path_len; i += kWave)
        if (!walk || i > d) row[i] = -1;
    if (!walk) return;
    const int b = (int)(p / n_targets);
    if (lane == 0) row[d] = cur;
    for (int32_t l = d - 1; l >= 0; --l) {
        const uint64_t *reached = levels + (int64_t)l * n_nodes;
        const int32_t begin = rowptr[cur], end = rowptr[cur + 1];
        int64_t next = -1;
        for (int32_t e0 = begin; e0 < end && next < 0; e0 += kWave) {
            const int32_t e = e0 + lane;
            int32_t col = -1;
            bool hit = false;
            if (e < end) {
                col = entries[e].x;
                hit = (reached[col] >> b) & 1ull;
            }
            const unsigned long long bal = __ballot(hit);
            if (bal != 0) next = __shfl(col, __ffsll((long long)bal) - 1);
        }
        if (lane == 0) row[l] = next;
        if (next < 0) {                                           // levels and dist disagree: leave the rest unset
            for (int i = lane; i < l; i += kWave) row[i] = -1;
            return;
        }
        cur = next;
    }
}

}  // namespace

extern "C" {

int lgc_bfs_init(const int64_t *sources, int32_t n_sources, int64_t n_nodes, uint64_t *seen, uint64_t *frontier,
                 int32_t *status, void *stream_) {
    if (!sources || !seen || !frontier || !status || n_sources < 0 || n_nodes < 0) return LGC_E_INVAL;
    if (n_sources > LGC_BFS_MAX_SOURCES || n_nodes >= INT32_MAX) return LGC_E_RANGE;
    if (n_sources == 0 || n_nodes == 0) return 0;
    const int64_t blocks = std::min<int64_t>(ceil_div(n_nodes, kBlock), 4096);
    hipLaunchKernelGGL(k_bfs_zero, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream_), seen, frontier, n_nodes);
    hipLaunchKernelGGL(k_bfs_seed, dim3(1), dim3(LGC_BFS_MAX_SOURCES), 0, as_stream(stream_), sources, n_sources, n_nodes,
                       reinterpret_cast<unsigned long long *>(seen), reinterpret_cast<unsigned long long *>(frontier), status);
    return (int)hipGetLastError();
}

int lgc_bfs_level(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, int32_t short_max,
                  const lgc_chunk *chunks, int32_t n_chunks, uint64_t active, const uint64_t *frontier_in,
                  uint64_t *frontier_out, uint64_t *seen, uint64_t *counters, void *stream_) {
    if (!rowptr || !entries || !frontier_in || !frontier_out || !seen || !counters || row_begin < 0 || row_end < row_begin ||
        short_max < 0 || n_chunks < 0 || (n_chunks > 0 && !chunks) || frontier_in == frontier_out)
        return LGC_E_INVAL;
    if (row_end == INT32_MAX) return LGC_E_RANGE;
    if (active == 0 || row_end == row_begin) return 0;
    const e2 *ent = reinterpret_cast<const e2 *>(entries);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counters);
    hipLaunchKernelGGL(k_bfs_rows, dim3(ceil_div((int64_t)row_end - row_begin, kBfsRowsPerBlock)), dim3(kBlock), 0,
                       as_stream(stream_), rowptr, ent, row_begin, row_end, short_max, active, frontier_in, frontier_out, seen,
                       cnt);
    if (n_chunks > 0)
        hipLaunchKernelGGL(k_bfs_chunks, dim3(ceil_div(n_chunks, kBlock / kWave)), dim3(kBlock), 0, as_stream(stream_), ent,
                           chunks, n_chunks, active, frontier_in, frontier_out, seen, cnt);
    return (int)hipGetLastError();
}

int lgc_bfs_resolve(const int64_t *sources, const int64_t *targets, int32_t n_sources, int64_t n_targets, int64_t n_nodes,
                    const uint64_t *frontier, int32_t level, int32_t *dist, uint64_t *counters, int32_t *status,
                    void *stream_) {
    if (!sources || !targets || !frontier || !dist || !counters || !status || n_sources < 0 || n_targets < 0 || n_nodes < 0 ||
        level < 0)
        return LGC_E_INVAL;
    if (n_sources > LGC_BFS_MAX_SOURCES || n_nodes >= INT32_MAX || n_targets >= INT32_MAX) return LGC_E_RANGE;
    if (n_sources == 0 || n_targets == 0) return 0;
    hipLaunchKernelGGL(k_bfs_resolve, dim3(ceil_div((int64_t)n_sources * n_targets, kBlock)), dim3(kBlock), 0,
                       as_stream(stream_), sources, targets, n_sources, (int32_t)n_targets, n_nodes, frontier, level, dist,
                       reinterpret_cast<unsigned long long *>(counters), status);
    return (int)hipGetLastError();
}

int lgc_bfs_backtrack(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, const uint64_t *levels,
                      int32_t n_levels, const int64_t *targets, const int32_t *dist, int32_t n_sources, int64_t n_targets,
                      int64_t *paths, int32_t path_len, void *stream_) {
    if (!rowptr || !entries || !levels || !targets || !dist || !paths || n_nodes < 0 || n_levels < 1 || n_sources < 0 ||
        n_targets < 0 || path_len < 1)
        return LGC_E_INVAL;
    if (n_sources > LGC_BFS_MAX_SOURCES || n_nodes >= INT32_MAX || n_targets >= INT32_MAX) return LGC_E_RANGE;
    if (n_sources == 0 || n_targets == 0) return 0;
    const int64_t n_pairs = (int64_t)n_sources * n_targets;
    hipLaunchKernelGGL(k_bfs_backtrack, dim3(ceil_div(n_pairs, kBlock / kWave)), dim3(kBlock), 0, as_stream(stream_), rowptr,
                       reinterpret_cast<const e2 *>(entries), levels, n_levels, n_nodes, targets, dist, n_pairs,
                       (int32_t)n_targets, paths, path_len);
    return (int)hipGetLastError();
}

}  // extern "C"

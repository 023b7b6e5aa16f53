// lgconv_select.h -- the selection of the fused score-and-select units (lgconv_similar.hip, lgconv_retrieve.hip; DESIGN.md
// sections 19 and 26): the candidate word, the in-place compaction of a row's buffer by one wavefront, the rule by which a
// finished place is written out, and the merge of the slices' lists of one row.  One definition each; the scoring kernels
// and their prologues are the units' own.
#pragma once
#include "lgconv_common.h"

namespace {

constexpr int kNbCapMax = 128;                // a candidate buffer is compacted by one wavefront, two entries a lane
constexpr int kSelectMaxK = 64;               // compact_row holds a buffer in two registers a lane
static_assert(kNbCapMax == 2 * kWave, "compact_row holds a buffer in two registers a lane");

// A candidate is ONE 64-bit word: the order key (order_key) above the complemented item index, so that a larger word is a better
// candidate (greater value, or equal value and smaller index) and no two candidates of a row are equal.  0 = no candidate
// (the smallest real key is -inf's 0x007FFFFF).
__device__ __forceinline__ u64 pack_candidate(float v, int item) { return ((u64)order_key(v) << 32) | (uint32_t)~item; }

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

// place o of a finished result: candidate e (0 = none: -1 / -inf); out_value may be null
__device__ __forceinline__ void write_candidate(int64_t *out_index, float *out_value, int64_t o, u64 e) {
    out_index[o] = e ? (int64_t)(~(uint32_t)e & 0x7FFFFFFFu) : -1;
    if (out_value) out_value[o] = e ? key_value((uint32_t)(e >> 32)) : -INFINITY;
}

// One wavefront merges the `total` places the slices left for one row at src: 64 at a time are appended to buf
// ([kNbCapMax], the wavefront's own; empty places skipped), which is compacted to the k best whenever another 64 might not
// fit.  merge_keep leaves the best in buf[0, n), best first, and returns n <= k; merge_row writes them to places
// o .. o + k - 1 of the result.
__device__ __forceinline__ int merge_keep(u64 *buf, const u64 *src, int total, int k, int lane) {
    int n = 0;
    for (int base = 0; base < total; base += kWave) {
        const u64 e = base + lane < total ? src[base + lane] : 0ull;
        const u64 have = __ballot(e != 0ull);
        if (e != 0ull) buf[n + __popcll(have & ((1ull << lane) - 1ull))] = e;
        n += __popcll(have);
        if (n > kNbCapMax - kWave) n = compact_row(buf, n, k, lane, nullptr, nullptr);
    }
    return compact_row(buf, n, k, lane, nullptr, nullptr);
}

__device__ __forceinline__ void merge_row(u64 *buf, const u64 *src, int total, int k, int lane, int64_t *out_index,
                                          float *out_value, int64_t o) {
    const int n = merge_keep(buf, src, total, k, lane);
    if (lane < k) write_candidate(out_index, out_value, o + lane, lane < n ? buf[lane] : 0ull);
}

// the buffer of a row: room for k kept candidates and at least 32 new ones, a multiple of 8
inline int select_cap(int k) { return k <= 32 ? 64 : 96; }

}  // namespace

// lgconv_hardneg.hip -- hard negatives for the mini-batch sampler: the first n_cand admissible draws of lgc_sample_triples'
// stream are scored against the user's row and the highest-scored one is the negative.  One launch, one wavefront per
// sample, lane = attempt; a candidate's dot product is ONE lane's chain, so no sum crosses lanes.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// Geometry.  A workgroup is four wavefronts, each with a sample of its own; they share nothing but
// the one barrier behind the staging of their user rows.  Round r of a sample gives attempt 64 r + lane + 1 to every lane:
// the lane draws its node, binary-searches the user's ignore set, and a ballot with a prefix popcount keeps the first
// admissible lanes up to the number still wanted.  A kept lane walks its own item row against the user row, which every
// lane reads from LDS at the same address (a broadcast): lgc_score_rows' chain in one lane.
constexpr int kHnRows = kBlock / kWave;       // samples of a workgroup
constexpr int kHnAttempts = 256;              // lgc_sample_triples' limit
constexpr int kHnRounds = kHnAttempts / kWave;
constexpr int kHnBatch = 8;                   // 16-byte loads of its row a lane has in flight
constexpr int kHnRowMax = 256;                // floats of a staged user row: lgc_dim_ok's widest, a multiple of 4
static_assert(kHnRounds * kWave == kHnAttempts, "whole rounds");

struct HnArgs {
    const int64_t *users;
    const int32_t *pos_ptr;
    const int64_t *pos_items;
    const int32_t *ign_ptr;
    const int64_t *ign_items;
    const float *user_table;
    const float *item_table;
    int64_t user_stride, item_stride;
    int64_t *pos_out;
    int64_t *neg_out;
    float *neg_score;
    int32_t *neg_attempt;
    int32_t *n_admissible;
    int32_t *status;
    u64 seed, step;
    int32_t n, n_users, n_items, n_cand, dim;
};

// dot(user row, item row) of a live lane, +0 in the others: lgc_score_rows' chain (score_chain), the user's value the first
// factor.  `ur` is the staged user row in LDS, zero-filled to a multiple of 4; kHnBatch loads of the lane's row are issued
// before the first is consumed.
template <bool VEC>
__device__ __forceinline__ float hn_dot(const float *ur, const float *__restrict__ row, int dim, int groups, bool live) {
    float acc = 0.0f;
    if (live) {
        for (int g0 = 0; g0 < groups; g0 += kHnBatch) {
            f4 b[kHnBatch];
#pragma unroll
            for (int j = 0; j < kHnBatch; ++j)
                if (g0 + j < groups) b[j] = load4<VEC>(row, 4 * (g0 + j), dim);
#pragma unroll
            for (int j = 0; j < kHnBatch; ++j) {
                if (g0 + j < groups) {
                    const f4 a = *reinterpret_cast<const f4 *>(ur + 4 * (g0 + j));
                    acc = score_chain(a, b[j], acc);
                }
            }
        }
    }
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_sample_hard(const HnArgs p) {
    __shared__ __attribute__((aligned(16))) float hn_user[kHnRows][kHnRowMax];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t i = (int64_t)blockIdx.x * kHnRows + wv;    // the wavefront's sample
    const bool in_batch = i < p.n;
    const int groups = (p.dim + 3) / 4;

    // the user, range-checked before any address is formed from it; its row goes to LDS, zeros past dim
    int64_t u = -1;
    bool ok = false;
    if (in_batch) {
        u = p.users[i];
        ok = u >= 0 && u < p.n_users;
        if (ok) ok = p.pos_ptr[u + 1] != p.pos_ptr[u];
    }
    {
        const float *urow = p.user_table + (ok ? u : 0) * p.user_stride;
        for (int d = lane; d < 4 * groups; d += kWave) hn_user[wv][d] = (ok && d < p.dim) ? urow[d] : 0.0f;
    }
    __syncthreads();                                         // the kernel's only barrier: every wavefront reaches it
    if (!in_batch) return;
    if (!ok) {
        if (lane == 0) {
            atomicOr(p.status, LGC_ST_INDEX_OOB);
            p.pos_out[i] = p.neg_out[i] = p.n_users;
            if (p.neg_score) p.neg_score[i] = 0.0f;
            if (p.neg_attempt) p.neg_attempt[i] = 0;
            if (p.n_admissible) p.n_admissible[i] = 0;
        }
        return;
    }
    const float *ur = hn_user[wv];
    const u64 key = mix64(mix64(p.seed) ^ mix64(p.step * 0xD1B54A32D192ED03ull + (u64)i));
    if (lane == 0) {
        const int32_t pb = p.pos_ptr[u], pc = p.pos_ptr[u + 1] - pb;
        p.pos_out[i] = p.pos_items[pb + (int64_t)bounded(mix64(key), (u64)pc)];
    }
    const int32_t ib = p.ign_ptr[u], ie = p.ign_ptr[u + 1];

    // best: the order key of the score above the complemented attempt, so that the larger word is the better score and,
    // among equal scores, the earlier attempt -- in a round and across rounds alike
    u64 best = 0ull;
    float best_score = 0.0f;
    int best_item = 0, taken = 0, item = 0;
    for (int r = 0; r < kHnRounds && taken < p.n_cand; ++r) {
        const int attempt = r * kWave + lane + 1;
        item = (int)bounded(mix64(key + 0x632BE59BD9B4E019ull * (u64)attempt), (u64)p.n_items);
        const int64_t node = (int64_t)p.n_users + item;
        const bool admissible = !in_sorted(p.ign_items, ib, ie, node);
        const u64 mask = __ballot(admissible);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        const bool keep = admissible && taken + before < p.n_cand;
        taken = min(p.n_cand, taken + __popcll(mask));
        const float score = hn_dot<VEC>(ur, p.item_table + (int64_t)item * p.item_stride, p.dim, groups, keep);
        const u64 mine = keep ? ((u64)order_key(score) << 32) | (uint32_t)~(uint32_t)attempt : 0ull;
        const u64 top = wave_max(mine);
        if (top > best) {                                    // the same for every lane
            const int src = (int)(~(uint32_t)top - 1u) & (kWave - 1);
            best = top;
            best_score = __shfl(score, src, kWave);          // the chain's own bits: the key has folded -0 and the NaNs
            best_item = __shfl(item, src, kWave);
        }
    }
    int best_attempt = (int)~(uint32_t)best;
    if (taken == 0) {
        // all 256 draws are ignored: the last one is kept, as lgc_sample_triples does, with its score
        const float score = hn_dot<VEC>(ur, p.item_table + (int64_t)item * p.item_stride, p.dim, groups, lane == kWave - 1);
        best_score = __shfl(score, kWave - 1, kWave);
        best_item = __shfl(item, kWave - 1, kWave);
        best_attempt = kHnAttempts;
    }
    if (lane == 0) {
        if (taken == 0) atomicOr(p.status, LGC_ST_SAMPLER_EXHAUSTED);
        p.neg_out[i] = (int64_t)p.n_users + best_item;
        if (p.neg_score) p.neg_score[i] = best_score;
        if (p.neg_attempt) p.neg_attempt[i] = best_attempt;
        if (p.n_admissible) p.n_admissible[i] = taken;
    }
}

}  // namespace

extern "C" {

int lgc_sample_hard_triples(const int64_t *users, int64_t n, const int32_t *pos_ptr, const int64_t *pos_items,
                            const int32_t *ign_ptr, const int64_t *ign_items, int64_t n_users, int64_t n_items, uint64_t seed,
                            uint64_t step, int32_t n_cand, const float *user_table, int64_t user_stride,
                            const float *item_table, int64_t item_stride, int32_t dim, int64_t *pos_out, int64_t *neg_out,
                            float *neg_score, int32_t *neg_attempt, int32_t *n_admissible, int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!users || !pos_ptr || !pos_items || !ign_ptr || !user_table || !item_table || !pos_out || !neg_out || !status ||
        n < 0 || n_users < 0 || n_items < 1 || user_stride < dim || item_stride < dim)
        return LGC_E_INVAL;
    if (n_cand < 1 || n_cand > LGC_HARDNEG_MAX_CAND || n >= INT32_MAX || n_users >= INT32_MAX || n_items >= INT32_MAX ||
        n_users + n_items >= INT32_MAX)
        return LGC_E_RANGE;
    if (n == 0) return 0;
    HnArgs p;
    p.users = users;
    p.pos_ptr = pos_ptr;
    p.pos_items = pos_items;
    p.ign_ptr = ign_ptr;
    p.ign_items = ign_items;
    p.user_table = user_table;
    p.item_table = item_table;
    p.user_stride = user_stride;
    p.item_stride = item_stride;
    p.pos_out = pos_out;
    p.neg_out = neg_out;
    p.neg_score = neg_score;
    p.neg_attempt = neg_attempt;
    p.n_admissible = n_admissible;
    p.status = status;
    p.seed = seed;
    p.step = step;
    p.n = (int32_t)n;
    p.n_users = (int32_t)n_users;
    p.n_items = (int32_t)n_items;
    p.n_cand = n_cand;
    p.dim = dim;
    const bool vec = dim % 4 == 0 && item_stride % 4 == 0 && aligned_to(item_table, 16);
    hipLaunchKernelGGL(vec ? k_sample_hard<true> : k_sample_hard<false>, dim3(ceil_div(n, kHnRows)), dim3(kBlock), 0,
                       as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

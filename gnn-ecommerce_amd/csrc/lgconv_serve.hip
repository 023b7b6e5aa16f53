// lgconv_serve.hip -- the serving tail (seen-mask + top-k per row), the mini-batch sampler and the epoch evaluation
// (score panels, hits per row, metric sums).
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// Serving tail: multiplicative seen-mask + top-k per row, on the device
// ----------------------------------------------------------------------------------------
// masked[i] = score[i] * (1 - seen[i])  (src/lightgcn.py:175 -- seen items become 0, they are not removed), then the
// k largest by (value descending, index ascending); every NaN, of either sign bit, ranks above +inf as in torch.topk,
// and -0 equals +0 (order_key).  One workgroup per row.  Rows of up to 65,536 columns are read
// ONCE: each thread keeps its 64 order-preserving keys in registers.  Short cut: the k-th largest of the 1,024
// per-thread maxima bounds the k-th largest element from below; the few elements in or above its 11-bit bin go to a
// list in LDS and each counts the entries ahead of it (= its output position).  Heavily tied or flat rows (list
// longer than 512) and wider rows take the general path: three radix passes (11 + 11 + 10 bits, histograms in LDS)
// find the k-th largest key T, one pass collects everything above T plus as many elements equal to T as are still
// needed -- lowest indices first -- and a bitonic sort orders the k winners.  Nothing but [rows, k] leaves the device.
constexpr int kTopkMax = 256;
constexpr int kTopkBlock = 1024;   // 16 wavefronts on one row: a single-row request is latency-bound on one CU

constexpr int kTopkRegs = 64;      // keys a thread can hold: rows up to kTopkRegs * kTopkBlock columns are read once
constexpr int kTopkCopies = 4;     // histogram copies (lane & 3), one bank apart: scores crowd into a few exponent bins
constexpr int kTopkHistStride = 2049;
constexpr int kTopkShort = 512;    // longest candidate list the short cut ranks by counting

// REGS: the row's masked keys live in registers (one read of the row, all passes on registers); otherwise every pass
// streams the row again (rows wider than kTopkRegs * kTopkBlock columns).
#ifdef LGC_TOPK_TRACE   // debug builds (tools/topk_trace.py): phase time stamps of block 0
__device__ unsigned long long g_topk_trace[16];
#define LGC_TOPK_STAMP(slot) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_topk_trace[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define LGC_TOPK_STAMP(slot) do { } while (0)
#endif

// MASK: 0 none, 1 dense [rows, n_cols] floats, 2 per-user item lists.
template <bool REGS, int MASK>
__global__ __launch_bounds__(kTopkBlock) void k_mask_topk(const float *__restrict__ scores, int64_t score_stride,
                                                         const float *__restrict__ seen, int64_t seen_stride,
                                                         const int64_t *__restrict__ list_ptr,
                                                         const int64_t *__restrict__ list_items,
                                                         const int64_t *__restrict__ list_rows, int32_t n_cols,
                                                         int32_t k, int64_t *__restrict__ out_index,
                                                         float *__restrict__ out_value) {
    extern __shared__ uint32_t seen_bits[];     // list form of the mask: one bit per column, built here
    __shared__ uint32_t hist[kTopkCopies * kTopkHistStride];
    __shared__ uint32_t cand_key[kTopkMax], cand_inv[kTopkMax];   // candidates: key, then ~index (lowest index wins ties)
    __shared__ uint32_t sh_bin, sh_need, sh_count, sh_short, sh_wave[kTopkBlock / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const float *srow = scores + (int64_t)blockIdx.x * score_stride;
    const float *mrow = MASK == 1 ? seen + (int64_t)blockIdx.x * seen_stride : nullptr;
    LGC_TOPK_STAMP(0);
    if (MASK == 2) {   // seen items of this row's user as a bitmask in LDS: the dense [rows, n_cols] mask never exists
        for (int b = tid; b < (n_cols + 31) / 32; b += kTopkBlock) seen_bits[b] = 0u;
        __syncthreads();
        const int64_t u = list_rows ? list_rows[blockIdx.x] : (int64_t)blockIdx.x;
        for (int64_t e = list_ptr[u] + tid; e < list_ptr[u + 1]; e += kTopkBlock) {
            const int64_t it = list_items[e];
            if (it >= 0 && it < n_cols) atomicOr(&seen_bits[it >> 5], 1u << (it & 31));
        }
        __syncthreads();
    }
    // score * (1 - seen) in upstream's arithmetic; the list form has seen = 1 for listed columns, 0 elsewhere
    auto masked_at = [&](float s, float m, int i) {
        if (MASK == 2) return (seen_bits[i >> 5] >> (i & 31)) & 1u ? __fmul_rn(s, 0.0f) : s;
        return MASK == 1 ? __fmul_rn(s, __fsub_rn(1.0f, m)) : s;
    };
    // slots past the row end hold key 0, below every real key (real keys are lifted to >= 1; the smallest one a value
    // has is -inf's 0x007FFFFF, so the lift moves nothing), so the passes need no bounds test.  Loads are clamped, not
    // predicated: no divergent control flow around them.
    auto key_of = [&](float s, float m, int i) {
        const uint32_t key = max(order_key(masked_at(s, m, min(i, n_cols - 1))), 1u);
        return i < n_cols ? key : 0u;
    };
    uint32_t keys[REGS ? kTopkRegs : 1];
    if (REGS) {
        constexpr int G = 16;                         // independent loads per thread in flight: one CU, latency-bound
#pragma unroll
        for (int j0 = 0; j0 < kTopkRegs; j0 += G) {
            if (j0 * kTopkBlock < n_cols) {           // block-uniform
                float sv[G], mv[G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int i = min((j0 + j) * kTopkBlock + tid, n_cols - 1);
                    sv[j] = srow[i];
                    mv[j] = MASK == 1 ? mrow[i] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < G; ++j) keys[j0 + j] = key_of(sv[j], mv[j], (j0 + j) * kTopkBlock + tid);
            } else {
#pragma unroll
                for (int j = 0; j < G; ++j) keys[j0 + j] = 0u;
            }
        }
    }
    LGC_TOPK_STAMP(1);
    uint32_t *my_hist = hist + (lane & (kTopkCopies - 1)) * kTopkHistStride;
    // Walk the nb bins of hist[] down from the top until `want` elements are covered: sh_bin = the bin that crosses,
    // sh_need = elements still wanted from it, sh_count = its population.  Thread t owns nb / 1024 bins (block scan).
    auto find_bin = [&](int nb, uint32_t want) {
        const int per = nb / kTopkBlock;                     // 2 or 1
        uint32_t mine = 0;
        for (int j = 0; j < per; ++j) mine += hist[nb - 1 - (tid * per + j)];
        uint32_t incl = mine;                                // inclusive scan, thread 0 = highest bins
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == kWave - 1) sh_wave[wv] = incl;
        __syncthreads();
        for (int q = 0; q < wv; ++q) incl += sh_wave[q];
        const uint32_t before = incl - mine;
        if (before < want && incl >= want) {                 // exactly one thread
            uint32_t acc = before;
            for (int j = 0; j < per; ++j) {
                const int b = nb - 1 - (tid * per + j);
                if (acc + hist[b] >= want) { sh_bin = (uint32_t)b; sh_need = want - acc; sh_count = hist[b]; break; }
                acc += hist[b];
            }
        }
        __syncthreads();
    };
    auto fold_copies = [&](int nb) {
        for (int b = tid; b < nb; b += kTopkBlock) {
            uint32_t c = hist[b];
#pragma unroll
            for (int q = 1; q < kTopkCopies; ++q) c += hist[q * kTopkHistStride + b];
            hist[b] = c;
        }
        __syncthreads();
    };
    // Short cut (keys in registers): the k-th largest of the 1024 per-thread maxima is a lower bound of the k-th
    // largest element, and on anything but heavily tied rows only a few dozen elements reach its 11-bit bin.  Those
    // go to a short list in LDS and every entry counts the entries ahead of it: its count is its output position.
    // More than kTopkShort entries (ties, flat rows): the general radix passes below do the row.
    if (REGS) {
        uint32_t mx = 0;
#pragma unroll
        for (int j = 0; j < kTopkRegs; ++j) mx = max(mx, keys[j]);
        for (int b = tid; b < kTopkCopies * kTopkHistStride; b += kTopkBlock) hist[b] = 0;
        if (tid == 0) sh_short = 0;
        __syncthreads();
        atomicAdd(&my_hist[mx >> 21], 1u);                   // a thread without a column has mx = 0: bin 0, never needed
        __syncthreads();
        fold_copies(2048);
        find_bin(2048, (uint32_t)k);
        const uint32_t low = max(sh_bin << 21, 1u);
        uint32_t *short_key = hist, *short_inv = hist + kTopkShort;   // the histogram is free again
#pragma unroll
        for (int j = 0; j < kTopkRegs; ++j)
            if (j * kTopkBlock < n_cols && keys[j] >= low) {
                const uint32_t pos = atomicAdd(&sh_short, 1u);
                if (pos < kTopkShort) {
                    short_key[pos] = keys[j];
                    short_inv[pos] = 0xFFFFFFFFu - (uint32_t)(j * kTopkBlock + tid);
                }
            }
        __syncthreads();
        LGC_TOPK_STAMP(2);
        const uint32_t n_short = sh_short;
        if (n_short <= kTopkShort) {
            if (wv * kWave < (int)n_short) {                 // whole wavefronts past the list have nothing to rank
                const uint32_t kt = tid < (int)n_short ? short_key[tid] : 0u, it = tid < (int)n_short ? short_inv[tid] : 0u;
                uint32_t ahead = 0;
                for (uint32_t c0 = 0; c0 < n_short; c0 += 8) {   // broadcast reads, eight entries in flight; slots past
                    uint32_t kc[8], ic[8];                       // the list end read as 0 = behind every entry
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const bool in = c0 + q < n_short;
                        kc[q] = in ? short_key[c0 + q] : 0u;
                        ic[q] = in ? short_inv[c0 + q] : 0u;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) ahead += (kc[q] > kt || (kc[q] == kt && ic[q] > it)) ? 1u : 0u;
                }
                if (tid < (int)n_short && ahead < (uint32_t)k) {
                    const uint32_t idx = 0xFFFFFFFFu - it;
                    out_index[(int64_t)blockIdx.x * k + ahead] = (int64_t)idx;
                    if (out_value)
                        out_value[(int64_t)blockIdx.x * k + ahead] =
                            masked_at(srow[idx], MASK == 1 ? mrow[idx] : 0.0f, (int)idx);
                }
            }
            LGC_TOPK_STAMP(12);
            return;
        }
        __syncthreads();
    }
    uint32_t prefix = 0, mask = 0, need = (uint32_t)k, eq_total = 0;
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = shifts[pass], nb = 1 << bits[pass];
        for (int b = tid; b < kTopkCopies * kTopkHistStride; b += kTopkBlock) hist[b] = 0;
        __syncthreads();
        if (REGS) {
#pragma unroll
            for (int j = 0; j < kTopkRegs; ++j)
                if (j * kTopkBlock < n_cols && (keys[j] & mask) == prefix)
                    atomicAdd(&my_hist[(keys[j] >> shift) & (nb - 1)], 1u);
        } else {
            for (int base = 0; base < n_cols; base += 4 * kTopkBlock) {   // four independent loads per thread in flight
                float sv[4], mv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = min(base + j * kTopkBlock + tid, n_cols - 1);
                    sv[j] = srow[i];
                    mv[j] = MASK == 1 ? mrow[i] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = base + j * kTopkBlock + tid;
                    const uint32_t key = key_of(sv[j], mv[j], i);
                    if (i < n_cols && (key & mask) == prefix) atomicAdd(&my_hist[(key >> shift) & (nb - 1)], 1u);
                }
            }
        }
        __syncthreads();
        LGC_TOPK_STAMP(2 + 3 * pass);
        fold_copies(nb);                               // into copy 0
        LGC_TOPK_STAMP(3 + 3 * pass);
        find_bin(nb, need);
        prefix |= sh_bin << shift;
        mask |= (uint32_t)(nb - 1) << shift;
        need = sh_need;
        eq_total = sh_count;
        __syncthreads();
        LGC_TOPK_STAMP(4 + 3 * pass);
    }
    const uint32_t T = prefix, n_gt = (uint32_t)k - need;   // take all keys > T (n_gt of them) and `need` keys == T
    if (tid == 0) sh_count = 0;
    for (int i = tid; i < kTopkMax; i += kTopkBlock) cand_key[i] = cand_inv[i] = 0u;
    __syncthreads();
    const bool ties_cut = eq_total > need;                  // more elements equal T than fit: lowest indices win
    uint32_t eq_taken = 0;                                  // block-uniform, only used when ties_cut
    auto collect = [&](int i, uint32_t key) {   // key 0 marks a slot past the row end (T >= 1 whenever k <= n_cols)
        const bool gt = key > T, eq = key == T;
        if (gt || (eq && !ties_cut)) {
            const uint32_t pos = atomicAdd(&sh_count, 1u);
            cand_key[pos] = key;
            cand_inv[pos] = 0xFFFFFFFFu - (uint32_t)i;
        }
        if (ties_cut && eq_taken < need) {   // ordered by index: ballots + per-wave offsets (rare: exact ties at the cut)
            const unsigned long long bal = __ballot(eq);
            if (lane == 0) sh_wave[wv] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t off = eq_taken, tot = 0;
            for (int q = 0; q < kTopkBlock / kWave; ++q) { if (q < wv) off += sh_wave[q]; tot += sh_wave[q]; }
            const uint32_t rank = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (eq && rank < need) {
                cand_key[n_gt + rank] = key;
                cand_inv[n_gt + rank] = 0xFFFFFFFFu - (uint32_t)i;
            }
            eq_taken += tot;
            __syncthreads();
        }
    };
    if (REGS) {
#pragma unroll
        for (int j = 0; j < kTopkRegs; ++j)
            if (j * kTopkBlock < n_cols) collect(j * kTopkBlock + tid, keys[j]);   // block-uniform condition
    } else {
        for (int base = 0; base < n_cols; base += kTopkBlock) {
            const int i = base + tid;
            const int ic = min(i, n_cols - 1);
            collect(i, key_of(srow[ic], MASK == 1 ? mrow[ic] : 0.0f, i));
        }
    }
    __syncthreads();
    LGC_TOPK_STAMP(11);
    // bitonic sort, descending, of the first n_sort >= k candidate slots (unused slots are 0 = below every real key)
    int n_sort = 2;
    while (n_sort < k) n_sort <<= 1;
    for (int size = 2; size <= n_sort; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int a = tid, b = tid ^ stride;
            if (a < n_sort && b > a) {
                const bool desc = (a & size) == 0;
                const uint32_t xk = cand_key[a], yk = cand_key[b], xi = cand_inv[a], yi = cand_inv[b];
                const bool x_lt_y = xk < yk || (xk == yk && xi < yi);
                const bool differ = xk != yk || xi != yi;
                if (differ && (desc ? x_lt_y : !x_lt_y)) {
                    cand_key[a] = yk; cand_inv[a] = yi;
                    cand_key[b] = xk; cand_inv[b] = xi;
                }
            }
            __syncthreads();
        }
    }
    LGC_TOPK_STAMP(12);
    if (tid < k) {
        const uint32_t idx = 0xFFFFFFFFu - cand_inv[tid];
        out_index[(int64_t)blockIdx.x * k + tid] = (int64_t)idx;
        if (out_value)
            out_value[(int64_t)blockIdx.x * k + tid] = masked_at(srow[idx], MASK == 1 ? mrow[idx] : 0.0f, (int)idx);
    }
}

// ----------------------------------------------------------------------------------------
// Mini-batch sampler
// ----------------------------------------------------------------------------------------
// the stream is mix64 / bounded of lgconv_common.h, which lgc_sample_hard_triples draws from as well
__global__ void k_sample_triples(const int64_t *__restrict__ users, int64_t n, const int32_t *__restrict__ pos_ptr,
                                 const int64_t *__restrict__ pos_items, const int32_t *__restrict__ ign_ptr,
                                 const int64_t *__restrict__ ign_items, int64_t n_users, int64_t n_items,
                                 uint64_t seed, uint64_t step, int64_t *__restrict__ pos_out,
                                 int64_t *__restrict__ neg_out, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t u = users[i];
    const uint64_t key = mix64(mix64(seed) ^ mix64(step * 0xD1B54A32D192ED03ull + (uint64_t)i));
    if (u < 0 || u >= n_users || pos_ptr[u + 1] == pos_ptr[u]) {
        atomicOr(status, LGC_ST_INDEX_OOB);
        pos_out[i] = neg_out[i] = n_users;
        return;
    }
    const int32_t pb = pos_ptr[u], pc = pos_ptr[u + 1] - pb;
    pos_out[i] = pos_items[pb + (int64_t)bounded(mix64(key), (uint64_t)pc)];
    const int32_t ib = ign_ptr[u], ie = ign_ptr[u + 1];
    int64_t cand = n_users;
    bool ok = false;
    for (int attempt = 0; attempt < 256 && !ok; ++attempt) {
        cand = n_users + (int64_t)bounded(mix64(key + 0x632BE59BD9B4E019ull * (uint64_t)(attempt + 1)), (uint64_t)n_items);
        const int32_t lo = lower_bound(ign_items, ib, ie, cand);   // in_sorted, spelled out
        ok = !(lo < ie && ign_items[lo] == cand);
    }
    if (!ok) atomicOr(status, LGC_ST_SAMPLER_EXHAUSTED);
    neg_out[i] = cand;
}

// ----------------------------------------------------------------------------------------
// Epoch evaluation: score panels, hits per row, metric sums
// ----------------------------------------------------------------------------------------
// out[r, i] = sum_d users[row_ids[r], d] * items[i, d]: an fp32 GEMM whose A operand is gathered.  One workgroup owns
// kScoreBN items: their rows are staged in LDS ONCE, for the whole width, and the workgroup then walks row tiles of
// kScoreBM panel rows, whose user rows pass through LDS in chunks of kScoreKC columns (the next chunk is already in
// registers while the current one is multiplied).  A thread keeps a 4 x 8 tile of sums in registers.
// Position independence: every out[r, i] is ONE chain of v_fma_f32 over d = 0, 1, ... round_up(dim, 4) - 1 in
// ascending order, starting from +0, with zeros in the columns past dim -- the same instructions on the same values
// wherever the pair sits.  Tile edges only clamp or predicate LOADS (a clamped row computes a sum nobody stores).
constexpr int kScoreBM = 64, kScoreBN = 128, kScoreKC = 32;
constexpr int kScoreAStride = kScoreKC + 4;   // floats; (stride / 4) odd: 16 consecutive rows hit 16 different bank quads

// LDS row stride (floats) of the item tile: whole float4 groups, (stride / 4) odd
__host__ __device__ inline int score_b_stride(int dim) {
    const int g = (dim + 3) / 4;
    return 4 * (g | 1);
}

__global__ __launch_bounds__(kBlock) void k_score_rows(const float *__restrict__ users, int64_t user_stride,
                                                      int64_t n_user_rows, const int64_t *__restrict__ row_ids,
                                                      int64_t n_rows, const float *__restrict__ items,
                                                      int64_t item_stride, int32_t n_items, int32_t dim,
                                                      float *__restrict__ out, int64_t out_stride,
                                                      int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float score_lds[];
    const int bs = score_b_stride(dim), dim4 = (dim + 3) & ~3, groups = dim4 / 4;
    float *Bs = score_lds;                                   // [kScoreBN][bs]
    float *As = Bs + kScoreBN * bs;                          // [kScoreBM][kScoreAStride]
    int *row_ok = reinterpret_cast<int *>(As + kScoreBM * kScoreAStride);   // [kScoreBM]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int item0 = blockIdx.x * kScoreBN;

    // the item tile, whole width, once per workgroup; items past the end are clamped to the last one (never stored)
    for (int e = tid; e < kScoreBN * groups; e += kBlock) {
        const int it = e / groups, g = e - it * groups;
        const int64_t gi = min(item0 + it, n_items - 1);
        *reinterpret_cast<f4 *>(Bs + it * bs + 4 * g) = load4<false>(items + gi * item_stride, 4 * g, dim);
    }

    // staging of the user chunk: thread -> (row ar + 32 q, columns 4 ag ..) for q = 0, 1
    const int ar = tid >> 3, ag = tid & 7;
    const int64_t n_tiles = (n_rows + kScoreBM - 1) / kScoreBM;
    for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int64_t row0 = tile * kScoreBM;
        const float *arow[2];
        bool alive[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t r = min(row0 + ar + 32 * q, n_rows - 1);
            const int64_t id = row_ids ? row_ids[r] : r;
            alive[q] = id >= 0 && id < n_user_rows;
            arow[q] = users + (alive[q] ? id : 0) * user_stride;
            if (ag == 0) {
                row_ok[ar + 32 * q] = alive[q] ? 1 : 0;
                if (!alive[q]) atomicOr(status, LGC_ST_INDEX_OOB);
            }
        }
        float acc[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
        f4 stage[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) stage[q] = load4_if(arow[q], 4 * ag, dim, alive[q] && 4 * ag < dim4);
        for (int k0 = 0; k0 < dim4; k0 += kScoreKC) {
            __syncthreads();                                 // the previous chunk (and, first time, nothing) is consumed
#pragma unroll
            for (int q = 0; q < 2; ++q)
                *reinterpret_cast<f4 *>(As + (ar + 32 * q) * kScoreAStride + 4 * ag) = stage[q];
            __syncthreads();                                 // also orders the item tile and row_ok before their first use
            const int kn = k0 + kScoreKC;
            if (kn < dim4) {
#pragma unroll
                for (int q = 0; q < 2; ++q) stage[q] = load4_if(arow[q], kn + 4 * ag, dim, alive[q] && kn + 4 * ag < dim4);
            }
            const int steps = min(kScoreKC, dim4 - k0) / 4;  // block-uniform
            for (int s = 0; s < steps; ++s) {
                f4 a[4], b[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f4 *>(As + (ty * 4 + i) * kScoreAStride + 4 * s);
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = *reinterpret_cast<const f4 *>(Bs + (tx + 16 * j) * bs + k0 + 4 * s);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = score_chain(a[i], b[j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = row0 + ty * 4 + i;
            if (r < n_rows) {
                const bool ok = row_ok[ty * 4 + i] != 0;     // a row whose id was out of range is zero-filled
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int it = item0 + tx + 16 * j;
                    if (it < n_items) out[r * out_stride + it] = ok ? acc[i][j] : 0.0f;
                }
            }
        }
        __syncthreads();                                     // row_ok is rewritten by the next tile
    }
}

// hits[r] = how many of topk[r, 0..k) occur in the positive list of the row's user; recall[r] = hits / list length.
// One wavefront per row: the top-k entries sit in LDS, the lanes stride over the list and flag the entries they
// meet (a flag, not a count: a positive listed twice still hits once, as set(a).intersection(b) upstream), the flags
// are counted.  The list length counts duplicates (upstream's len(item_id_idx_list)); an empty list gives NaN.
constexpr int kHitsRows = kBlock / kWave;

__global__ __launch_bounds__(kBlock) void k_topk_hits(const int64_t *__restrict__ topk, int64_t topk_stride, int32_t k,
                                                     const int64_t *__restrict__ pos_ptr,
                                                     const int64_t *__restrict__ pos_items,
                                                     const int64_t *__restrict__ list_rows, int64_t n_rows,
                                                     int64_t n_users, int32_t *__restrict__ hits,
                                                     double *__restrict__ recall, int32_t *__restrict__ status) {
    __shared__ int64_t sh_top[kHitsRows][kTopkMax];
    __shared__ int sh_flag[kHitsRows][kTopkMax];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = (int64_t)blockIdx.x * kHitsRows + wv;
    const bool live = r < n_rows;
    int64_t u = 0;
    bool ok = false;
    if (live) {
        u = list_rows ? list_rows[r] : r;
        ok = u >= 0 && u < n_users;
        for (int e = lane; e < k; e += kWave) {
            sh_top[wv][e] = topk[r * topk_stride + e];
            sh_flag[wv][e] = 0;
        }
    }
    __syncthreads();
    int64_t len = 0;
    if (live && ok) {
        const int64_t lo = pos_ptr[u], hi = pos_ptr[u + 1];
        len = hi - lo;
        for (int64_t p = lo + lane; p < hi; p += kWave) {
            const int64_t it = pos_items[p];
            for (int e = 0; e < k; ++e)
                if (sh_top[wv][e] == it) sh_flag[wv][e] = 1;
        }
    }
    __syncthreads();
    if (live) {
        int n = 0;
        for (int e = lane; e < k; e += kWave) n += sh_flag[wv][e];
        for (int off = kWave / 2; off > 0; off >>= 1) n += __shfl_down(n, off);
        if (lane == 0) {
            if (!ok) atomicOr(status, LGC_ST_INDEX_OOB);
            hits[r] = ok ? n : 0;
            recall[r] = ok ? (double)n / (double)len : 0.0;
        }
    }
}

// Sum of hits (int64) and of recall (double) in ONE workgroup and a fixed order: thread t adds elements t, t + 1024,
// ... in that order, then a binary tree over the threads.  No atomics: the same bits on every run.
constexpr int kSumBlock = 1024;

__global__ __launch_bounds__(kSumBlock) void k_metric_sums(const int32_t *__restrict__ hits,
                                                          const double *__restrict__ recall, int64_t n,
                                                          int64_t *__restrict__ hits_sum, double *__restrict__ recall_sum) {
    __shared__ int64_t sh_h[kSumBlock];
    __shared__ double sh_r[kSumBlock];
    const int tid = threadIdx.x;
    int64_t h = 0;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += kSumBlock) {
        if (hits) h += hits[i];
        if (recall) s += recall[i];
    }
    sh_h[tid] = h;
    sh_r[tid] = s;
    __syncthreads();
    for (int half = kSumBlock / 2; half > 0; half >>= 1) {
        if (tid < half) {
            sh_h[tid] += sh_h[tid + half];
            sh_r[tid] += sh_r[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (hits_sum) *hits_sum = sh_h[0];
        if (recall_sum) *recall_sum = sh_r[0];
    }
}

// ----------------------------------------------------------------------------------------
// Ranking metrics per row at several cutoffs, column sums, catalogue coverage
// ----------------------------------------------------------------------------------------
// The cutoffs and the discount table d_j = 1 / log2(j + 2) travel by value with the launch: the host computes the table
// once, in double, and the kernel never calls log2.
struct RankCuts {
    int32_t n;
    int32_t c[LGC_RM_MAX_CUTOFFS];
};
struct RankDiscounts {
    double d[kTopkMax];
};

// k_topk_hits' shape -- one wavefront per row, the row's top-k in LDS, the lanes striding over the positive list and
// flagging the entries they meet -- and then: four ballots turn the flags into the row's hit_bits words, and lane 0
// walks the bits in ascending j with every sum a running sum, of which a cutoff is a snapshot.  The value at a cutoff c
// is therefore the same chain of operations whatever k, n_cut and the other cutoffs are.  len = the list's length with
// duplicates (recall's denominator), nd = its number of distinct items (what IDCG and AP can at most reach).
__global__ __launch_bounds__(kBlock) void k_rank_metrics(const int64_t *__restrict__ topk, int64_t topk_stride, int32_t k,
                                                        const int64_t *__restrict__ pos_ptr,
                                                        const int64_t *__restrict__ pos_items,
                                                        const int64_t *__restrict__ pos_distinct,
                                                        const int64_t *__restrict__ list_rows, int64_t n_rows,
                                                        int64_t n_users, const RankCuts cuts, const RankDiscounts disc,
                                                        uint64_t *__restrict__ hit_bits, int32_t *__restrict__ hits,
                                                        double *__restrict__ metrics, int32_t *__restrict__ status) {
    __shared__ int64_t sh_top[kHitsRows][kTopkMax];
    __shared__ int sh_flag[kHitsRows][kTopkMax];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = (int64_t)blockIdx.x * kHitsRows + wv;
    const bool live = r < n_rows;
    int64_t u = 0;
    bool ok = false;
    if (live) {
        u = list_rows ? list_rows[r] : r;
        ok = u >= 0 && u < n_users;
        for (int e = lane; e < k; e += kWave) {
            sh_top[wv][e] = topk[r * topk_stride + e];
            sh_flag[wv][e] = 0;
        }
    }
    __syncthreads();
    int64_t len = 0;
    if (live && ok) {
        const int64_t lo = pos_ptr[u], hi = pos_ptr[u + 1];
        len = hi - lo;
        for (int64_t p = lo + lane; p < hi; p += kWave) {
            const int64_t it = pos_items[p];
            for (int e = 0; e < k; ++e)
                if (sh_top[wv][e] == it) sh_flag[wv][e] = 1;
        }
    }
    __syncthreads();
    if (!live) return;                                       // whole wavefronts: no barrier follows
    unsigned long long word[kTopkMax / kWave];
#pragma unroll
    for (int q = 0; q < kTopkMax / kWave; ++q) {
        const int e = q * kWave + lane;
        word[q] = __ballot(ok && e < k && sh_flag[wv][e] != 0);   // entries past k are no bits
    }
    if (lane != 0) return;
    if (!ok) atomicOr(status, LGC_ST_INDEX_OOB);
    if (hit_bits) {
#pragma unroll
        for (int q = 0; q < kTopkMax / kWave; ++q) hit_bits[r * (kTopkMax / kWave) + q] = word[q];
    }
    int32_t *hrow = hits + r * cuts.n;
    double *mrow = metrics + r * cuts.n * LGC_RM_COUNT;
    if (!ok) {
        for (int ci = 0; ci < cuts.n; ++ci) {
            hrow[ci] = 0;
            for (int m = 0; m < LGC_RM_COUNT; ++m) mrow[ci * LGC_RM_COUNT + m] = 0.0;
        }
        return;
    }
    const int64_t nd = pos_distinct ? pos_distinct[u] : len;
    int h = 0, ci = 0;
    double dcg = 0.0, idcg = 0.0, ap = 0.0, rr = 0.0;
#pragma unroll
    for (int q = 0; q < kTopkMax / kWave; ++q) {
        const unsigned long long w = word[q];
        for (int jj = 0; jj < kWave && ci < cuts.n; ++jj) {
            const int j = q * kWave + jj;                    // j < the last cutoff <= k while ci < cuts.n
            const double dj = disc.d[j];
            if ((w >> jj) & 1ull) {
                ++h;
                dcg += dj;
                ap += (double)h / (double)(j + 1);
                if (h == 1) rr = 1.0 / (double)(j + 1);
            }
            if (j < nd) idcg += dj;
            if (j + 1 == cuts.c[ci]) {
                const int c = j + 1;
                double *m = mrow + ci * LGC_RM_COUNT;
                hrow[ci] = h;
                m[LGC_RM_PRECISION] = (double)h / (double)c;
                m[LGC_RM_RECALL] = (double)h / (double)len;
                m[LGC_RM_NDCG] = dcg / idcg;
                m[LGC_RM_AP] = ap / (double)(c < nd ? (int64_t)c : nd);
                m[LGC_RM_RR] = rr;
                m[LGC_RM_HIT] = h > 0 ? 1.0 : 0.0;
                ++ci;
            }
        }
    }
}

// out[c] = sum over r of in[r, c]: one workgroup per column, each adding in k_metric_sums' order (thread t adds rows
// t, t + 1024, ... in that order, then the binary tree over the threads).  No atomics.
__global__ __launch_bounds__(kSumBlock) void k_column_sums(const double *__restrict__ in, int64_t in_stride, int64_t n_rows,
                                                          double *__restrict__ out) {
    __shared__ double sh_c[kSumBlock];
    const int tid = threadIdx.x;
    const double *col = in + blockIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n_rows; i += kSumBlock) s += col[i * in_stride];
    sh_c[tid] = s;
    __syncthreads();
    for (int half = kSumBlock / 2; half > 0; half >>= 1) {
        if (tid < half) sh_c[tid] += sh_c[tid + half];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = sh_c[0];
}

// bitmap[ci, item] |= 1 for every item among the first cuts.c[ci] entries of every row: one thread per (row, j) with
// j below the last cutoff; integer atomic OR.  An entry is range-checked before anything is addressed with it.
__global__ __launch_bounds__(kBlock) void k_coverage_mark(const int64_t *__restrict__ topk, int64_t topk_stride,
                                                         int64_t n_rows, const RankCuts cuts, int64_t n_items,
                                                         int64_t words, uint32_t *__restrict__ bitmap,
                                                         int32_t *__restrict__ status) {
    const int64_t width = cuts.c[cuts.n - 1], total = n_rows * width;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t r = t / width;
        const int j = (int)(t - r * width);
        const int64_t it = topk[r * topk_stride + j];
        if (it < 0 || it >= n_items) {
            atomicOr(status, LGC_ST_INDEX_OOB);
            continue;
        }
        for (int ci = 0; ci < cuts.n; ++ci)
            if (j < cuts.c[ci]) atomicOr(&bitmap[ci * words + (it >> 5)], 1u << (it & 31));
    }
}

// counts[ci] = set bits of bitmap row ci: one workgroup per cutoff, integer sums in a fixed order.
__global__ __launch_bounds__(kSumBlock) void k_coverage_count(const uint32_t *__restrict__ bitmap, int64_t words,
                                                             int64_t *__restrict__ counts) {
    __shared__ int64_t sh_n[kSumBlock];
    const int tid = threadIdx.x;
    const uint32_t *row = bitmap + (int64_t)blockIdx.x * words;
    int64_t n = 0;
    for (int64_t i = tid; i < words; i += kSumBlock) n += __popc(row[i]);
    sh_n[tid] = n;
    __syncthreads();
    for (int half = kSumBlock / 2; half > 0; half >>= 1) {
        if (tid < half) sh_n[tid] += sh_n[tid + half];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = sh_n[0];
}

// The cutoffs of lgc_rank_metrics / lgc_topk_coverage: 1..8 of them, each >= 1, strictly ascending, the last <= k.
int take_cutoffs(const int32_t *cutoffs, int32_t n_cut, int32_t k, RankCuts *out) {
    if (!cutoffs || n_cut < 1 || n_cut > LGC_RM_MAX_CUTOFFS || k < 1) return LGC_E_INVAL;
    if (k > kTopkMax) return LGC_E_RANGE;
    for (int i = 0; i < n_cut; ++i) {
        if (cutoffs[i] > kTopkMax) return LGC_E_RANGE;
        if (cutoffs[i] < 1 || (i > 0 && cutoffs[i] <= cutoffs[i - 1])) return LGC_E_INVAL;
    }
    if (cutoffs[n_cut - 1] > k) return LGC_E_INVAL;
    *out = RankCuts{};
    out->n = n_cut;
    for (int i = 0; i < n_cut; ++i) out->c[i] = cutoffs[i];
    return 0;
}

const RankDiscounts &rank_discounts() {
    static const RankDiscounts table = [] {
        RankDiscounts t;
        for (int j = 0; j < kTopkMax; ++j) t.d[j] = 1.0 / std::log2((double)(j + 2));
        return t;
    }();
    return table;
}

}  // namespace

extern "C" {

int lgc_mask_topk(const float *scores, int64_t score_stride, const float *seen, int64_t seen_stride, const int64_t *list_ptr,
                  const int64_t *list_items, const int64_t *list_rows, int64_t n_rows, int32_t n_cols, int32_t k,
                  int64_t *out_index, float *out_value, void *stream_) {
    if (!scores || !out_index || n_rows < 0 || n_cols < 1 || k < 1 || k > n_cols || score_stride < n_cols ||
        (seen && seen_stride < n_cols) || n_rows >= INT32_MAX || (seen && list_ptr) || (list_ptr && !list_items))
        return LGC_E_INVAL;
    if (k > kTopkMax) return LGC_E_RANGE;
    const size_t lds = list_ptr ? (size_t)((n_cols + 31) / 32) * 4 : 0;
    if (lds > 120 * 1024) return LGC_E_RANGE;             // the bitmask form holds up to 983,040 columns
    if (n_rows == 0) return 0;
    const bool regs = n_cols <= kTopkRegs * kTopkBlock;
    const int mode = list_ptr ? 2 : seen ? 1 : 0;
    using topk_fn = void (*)(const float *, int64_t, const float *, int64_t, const int64_t *, const int64_t *,
                             const int64_t *, int32_t, int32_t, int64_t *, float *);
    static const topk_fn kerns[2][3] = {{k_mask_topk<false, 0>, k_mask_topk<false, 1>, k_mask_topk<false, 2>},
                                        {k_mask_topk<true, 0>, k_mask_topk<true, 1>, k_mask_topk<true, 2>}};
    const topk_fn kern = kerns[regs][mode];
    static unsigned long long lds_ok_topk[2][3] = {};
    // above 16 KiB: static LDS (histogram copies, candidates) + the bitmask can pass the 64 KiB default
    const int rc_attr = allow_lds(reinterpret_cast<const void *>(kern), lds, 16 * 1024, 120 * 1024, &lds_ok_topk[regs][mode]);
    if (rc_attr != 0) return rc_attr;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_rows), dim3(kTopkBlock), lds, as_stream(stream_), scores, score_stride, seen,
                       seen_stride, list_ptr, list_items, list_rows, n_cols, k, out_index, out_value);
    return (int)hipGetLastError();
}

int lgc_sample_triples(const int64_t *users, int64_t n, const int32_t *pos_ptr, const int64_t *pos_items,
                       const int32_t *ign_ptr, const int64_t *ign_items, int64_t n_users, int64_t n_items, uint64_t seed,
                       uint64_t step, int64_t *pos_out, int64_t *neg_out, int32_t *status, void *stream_) {
    if (n < 0 || n_users < 0 || n_items < 1 || !status) return LGC_E_INVAL;
    if (n == 0) return 0;
    if (!users || !pos_ptr || !pos_items || !ign_ptr || !pos_out || !neg_out) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_sample_triples, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, as_stream(stream_), users, n,
                       pos_ptr, pos_items, ign_ptr, ign_items, n_users, n_items, seed, step, pos_out, neg_out, status);
    return (int)hipGetLastError();
}

int lgc_score_rows(const float *users, int64_t user_stride, int64_t n_user_rows, const int64_t *row_ids, int64_t n_rows,
                   const float *items, int64_t item_stride, int32_t n_items, int32_t dim, float *out, int64_t out_stride,
                   int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!users || !items || !out || !status || n_rows < 0 || n_user_rows < 0 || n_items < 1 || user_stride < dim ||
        item_stride < dim || out_stride < n_items)
        return LGC_E_INVAL;
    if (n_rows >= INT32_MAX || n_user_rows >= INT32_MAX) return LGC_E_RANGE;
    if (n_rows == 0) return 0;
    const size_t lds = (size_t)(kScoreBN * score_b_stride(dim) + kScoreBM * kScoreAStride) * 4 + kScoreBM * sizeof(int);
    static unsigned long long lds_ok_score = 0;
    const int rc_attr = allow_lds(reinterpret_cast<const void *>(k_score_rows), lds, 48 * 1024, 144 * 1024, &lds_ok_score);
    if (rc_attr != 0) return rc_attr;
    // enough workgroups for every CU twice over: the row tiles of a panel are split only when the item tiles are few
    const int64_t item_tiles = ceil_div(n_items, kScoreBN), row_tiles = ceil_div(n_rows, kScoreBM);
    const int64_t split = std::min<int64_t>(row_tiles, std::max<int64_t>(1, 512 / item_tiles));
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned)item_tiles, (unsigned)split), dim3(kBlock), lds, as_stream(stream_),
                       users, user_stride, n_user_rows, row_ids, n_rows, items, item_stride, n_items, dim, out, out_stride,
                       status);
    return (int)hipGetLastError();
}

int lgc_topk_hits(const int64_t *topk, int64_t topk_stride, int32_t k, const int64_t *pos_ptr, const int64_t *pos_items,
                  const int64_t *list_rows, int64_t n_rows, int64_t n_users, int32_t *hits, double *recall,
                  int32_t *status, void *stream_) {
    if (!topk || !pos_ptr || !hits || !recall || !status || n_rows < 0 || n_users < 0 || k < 1 || topk_stride < k)
        return LGC_E_INVAL;
    if (k > kTopkMax || n_rows >= INT32_MAX) return LGC_E_RANGE;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_topk_hits, dim3(ceil_div(n_rows, kHitsRows)), dim3(kBlock), 0, as_stream(stream_), topk,
                       topk_stride, k, pos_ptr, pos_items, list_rows, n_rows, n_users, hits, recall, status);
    return (int)hipGetLastError();
}

int lgc_metric_sums(const int32_t *hits, const double *recall, int64_t n_rows, int64_t *hits_sum, double *recall_sum,
                    void *stream_) {
    if (n_rows < 0 || (!hits_sum && !recall_sum) || (hits_sum && n_rows > 0 && !hits) ||
        (recall_sum && n_rows > 0 && !recall))
        return LGC_E_INVAL;
    if (n_rows == 0) return 0;                             // nothing to add: the sums are left as they are
    hipLaunchKernelGGL(k_metric_sums, dim3(1), dim3(kSumBlock), 0, as_stream(stream_), hits_sum ? hits : nullptr,
                       recall_sum ? recall : nullptr, n_rows, hits_sum, recall_sum);
    return (int)hipGetLastError();
}

int lgc_rank_metrics(const int64_t *topk, int64_t topk_stride, int32_t k, const int64_t *pos_ptr, const int64_t *pos_items,
                     const int64_t *pos_distinct, const int64_t *list_rows, int64_t n_rows, int64_t n_users,
                     const int32_t *cutoffs, int32_t n_cut, uint64_t *hit_bits, int32_t *hits, double *metrics,
                     int32_t *status, void *stream_) {
    if (!topk || !pos_ptr || !hits || !metrics || !status || n_rows < 0 || n_users < 0 || k < 1 || topk_stride < k)
        return LGC_E_INVAL;
    RankCuts cuts;
    const int rc = take_cutoffs(cutoffs, n_cut, k, &cuts);
    if (rc != 0) return rc;
    if (n_rows >= INT32_MAX) return LGC_E_RANGE;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_rank_metrics, dim3(ceil_div(n_rows, kHitsRows)), dim3(kBlock), 0, as_stream(stream_), topk,
                       topk_stride, k, pos_ptr, pos_items, pos_distinct, list_rows, n_rows, n_users, cuts, rank_discounts(),
                       hit_bits, hits, metrics, status);
    return (int)hipGetLastError();
}

int lgc_column_sums(const double *in, int64_t in_stride, int64_t n_rows, int32_t n_cols, double *out, void *stream_) {
    if (!out || n_rows < 0 || n_cols < 1 || in_stride < n_cols || (n_rows > 0 && !in)) return LGC_E_INVAL;
    if (n_cols > LGC_COLUMN_SUMS_MAX) return LGC_E_RANGE;
    if (n_rows == 0) return 0;                             // nothing to add: the sums are left as they are
    hipLaunchKernelGGL(k_column_sums, dim3((unsigned)n_cols), dim3(kSumBlock), 0, as_stream(stream_), in, in_stride, n_rows,
                       out);
    return (int)hipGetLastError();
}

int lgc_topk_coverage(const int64_t *topk, int64_t topk_stride, int32_t k, int64_t n_rows, const int32_t *cutoffs,
                      int32_t n_cut, int64_t n_items, uint32_t *bitmap, int64_t *counts, int32_t *status, void *stream_) {
    if (!bitmap || !counts || !status || n_rows < 0 || n_items < 1 || k < 1 || topk_stride < k || (n_rows > 0 && !topk))
        return LGC_E_INVAL;
    RankCuts cuts;
    const int rc = take_cutoffs(cutoffs, n_cut, k, &cuts);
    if (rc != 0) return rc;
    if (n_rows >= INT32_MAX || n_items >= INT32_MAX) return LGC_E_RANGE;
    const int64_t words = (n_items + 31) / 32;
    if (n_rows > 0) {
        const int64_t blocks = std::min<int64_t>(ceil_div(n_rows * cuts.c[cuts.n - 1], kBlock), 65536);
        hipLaunchKernelGGL(k_coverage_mark, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream_), topk, topk_stride,
                           n_rows, cuts, n_items, words, bitmap, status);
        const int rc_mark = (int)hipGetLastError();
        if (rc_mark != 0) return rc_mark;
    }
    hipLaunchKernelGGL(k_coverage_count, dim3((unsigned)cuts.n), dim3(kSumBlock), 0, as_stream(stream_), bitmap, words, counts);
    return (int)hipGetLastError();
}

#ifdef LGC_TOPK_TRACE
int lgc_debug_topk_trace(unsigned long long *out16) {
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_topk_trace), sizeof(unsigned long long) * 16);
}
#endif

}  // extern "C"

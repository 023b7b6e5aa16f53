// lgconv_softmax.hip -- in-batch softmax (InfoNCE / sampled-softmax) loss over a shared candidate list: every user row of a
// batch is scored against every listed item on the fp32 matrix cores, a user's own other positives are masked out through
// the sampler's ignore lists, and the loss, the gradient of the logits and the two gradient products with respect to the
// propagated rows come out of five launches in stream order.  No float atomics: the same bits on every run.
// C ABI: include/lgconv_hip.h
#include "lgconv_tile.h"

namespace {

// Geometry.
//   k_sm_logits   the tile of lgconv_tile.h: a workgroup owns kTileBM batch rows and ONE tile of kTileBN candidates, whose
//                 table rows go through citem[].  The epilogue turns the score into the logit, decides admissibility (a
//                 search in the user's ignore list) and writes the panel Z: the logit of an admissible pair (any NaN as
//                 the one quiet NaN), the word kSmMark for every other pair.  There are no slices: a row's statistics are
//                 taken from Z by ONE wavefront.
//   k_sm_rows     one wavefront per batch row over its row of Z: maximum, sum of exponentials, loss, and G in place of Z.
//   k_sm_loss     one workgroup: the row losses summed in a fixed order, divided by size.
//   k_sm_product  out = G . E_c (grad_users) and out = G^T . E_u (grad_cands): a workgroup owns 16 output rows and 64
//                 output columns, wavefront w columns [16 w, 16 w + 16); the inner extent passes through LDS in chunks of
//                 kSmPK and ONE accumulator per output element takes it in ascending order.
constexpr int kSmRows = kBlock / kWave;       // batch rows of a k_sm_rows workgroup
constexpr int kSmPM = 16, kSmPN = 64, kSmPK = 64;        // k_sm_product: output rows, output columns, inner chunk
constexpr int kSmPAS = kSmPK + 4;             // A rows: lane (c, q) reads c * 68 + q, 64 different banks
constexpr int kSmPBS = kSmPN + 16;            // B rows: lane (c, q) reads q * 80 + c, 64 different banks
constexpr uint32_t kSmMark = 0xFFFFFFFFu;     // Z: the pair is not admissible (a NaN bit pattern no admissible logit keeps)
constexpr uint32_t kSmNan = 0x7FC00000u;      // Z: an admissible logit that is a NaN

struct SmArgs {
    const float *table;
    const int64_t *row_users, *cand_items, *ign_items;
    const int32_t *target, *ign_ptr;
    const float *cand_bias;
    float *loss, *rl, *g, *grad_users, *grad_cands;   // rl: the row losses (row_loss, or the workspace)
    int32_t *n_adm, *status;
    int64_t stride, g_stride, grad_stride, size;
    float inv_tau;
    int32_t table_rows, split, n_rows, n_cand, dim, dp;   // dp = dim rounded up to 16
};

// ----------------------------------------------------------------------------------------
// the logits panel
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sm_logits(const SmArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm_lds[];
    const int dim = p.dim;
    Tile tl(sm_lds, p.dp);                                   // Qs: the user rows; Bs: a chunk of the candidate tile
    float *cbias = tl.lds_end();                             // [kTileBN]: the bias of a column
    int *citem = reinterpret_cast<int *>(cbias + kTileBN);   // [kTileBN]: the node of a column, -1 = none or not an item
    int *uid = citem + kTileBN;                              // [kTileBM]: the user of a row, -1 = no valid row
    int *tcol = uid + kTileBM;                               // [kTileBM]: its target column, -1 = no valid row
    int *titem = tcol + kTileBM;                             // [kTileBM]: the node of the target column
    int *ibeg = titem + kTileBM;                             // [kTileBM]: the user's ignore list, [ibeg, iend)
    int *iend = ibeg + kTileBM;
    const int tid = tl.tid, w = tl.w, c = tl.c, q = tl.q;
    const int64_t row0 = (int64_t)blockIdx.x * kTileBM;
    const uint32_t col0 = blockIdx.y * (uint32_t)kTileBN;    // below 2^31 + 128: unsigned, no overflow

    // every id is range-checked here, before an address is formed from it
    if (tid < kTileBM) {
        const int64_t r = row0 + tid;
        int u = -1, t = -1, ti = -1, ib = 0, ie = 0;
        if (r < p.n_rows) {
            const int64_t uu = p.row_users[r];
            const int32_t tt = p.target[r];
            bool ok = uu >= 0 && uu < p.split && tt >= 0 && tt < p.n_cand;
            if (ok) {
                const int64_t node = p.cand_items[tt];
                ok = node >= p.split && node < p.table_rows;
                if (ok) {
                    u = (int)uu;
                    t = tt;
                    ti = (int)node;
                    if (p.ign_ptr) {
                        ib = p.ign_ptr[uu];
                        ie = p.ign_ptr[uu + 1];
                    }
                }
            }
            if (!ok && blockIdx.y == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
        }
        uid[tid] = u;
        tcol[tid] = t;
        titem[tid] = ti;
        ibeg[tid] = ib;
        iend[tid] = ie;
    }
    if (tid < kTileBN) {
        const uint32_t col = col0 + tid;
        int node = -1;
        float bias = 0.0f;
        if (col < (uint32_t)p.n_cand) {
            const int64_t id = p.cand_items[col];
            if (id >= p.split && id < p.table_rows) node = (int)id;
            else if (blockIdx.x == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
            if (p.cand_bias) bias = p.cand_bias[col];
        }
        citem[tid] = node;
        cbias[tid] = bias;
    }
    __syncthreads();
    tl.stage_rows(p.table, p.stride, dim, [&](int row) { return uid[row]; });

    const int nch = (p.dp + kTileKC - 1) / kTileKC;
    auto load_chunk = [&](int ch) { tl.load_chunk(p.table, p.stride, dim, ch, [&](int it) { return citem[it]; }); };
    tl.reset();
    load_chunk(0);
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                     // the previous chunk is consumed
        tl.store_chunk();
        __syncthreads();                                     // also orders the user rows before their first use
        if (ch + 1 < nch) load_chunk(ch + 1);                // in flight during this chunk's products
        // Tile::product (lgconv_tile.h), restated: as a call it costs this kernel 8 VGPRs and with them one of its five
        // wavefronts per SIMD
        const int groups = min(kTileKC / 16, p.dp / 16 - ch * (kTileKC / 16));
        for (int g = 0; g < groups; ++g) {
            f4 a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                a[mi] = *reinterpret_cast<const f4 *>(tl.Qs + (16 * mi + c) * tl.sq + ch * kTileKC + 16 * g + 4 * q);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
                b[nj] = *reinterpret_cast<const f4 *>(tl.Bs + (32 * w + 16 * nj + c) * kTileBS + 16 * g + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        tl.acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], tl.acc[mi][nj], 0, 0, 0);
        }
    }

    // lane (c, q) holds rows 16 mi + 4 q + r of candidates 32 w + 16 nj + c
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int row = 16 * (x >> 2) + 4 * q + (x & 3);
        const int64_t gr = row0 + row;
        if (gr >= p.n_rows) continue;
        const int t = tcol[row], ti = titem[row], ib = ibeg[row], ie = iend[row];
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) {
            const int cl = 32 * w + 16 * nj + c;
            const uint32_t gc = col0 + cl;
            if (gc >= (uint32_t)p.n_cand) continue;
            float z = __fmul_rn(tl.acc[x >> 2][nj][x & 3], p.inv_tau);
            if (p.cand_bias) z = __fadd_rn(z, cbias[cl]);
            bool adm = false;
            if (t >= 0) {
                const int node = citem[cl];
                if ((int)gc == t) {
                    adm = true;
                } else if (node >= 0 && node != ti) {
                    adm = !in_sorted(p.ign_items, ib, ie, (int64_t)node);
                }
            }
            const uint32_t bits = adm ? (z != z ? kSmNan : __float_as_uint(z)) : kSmMark;
            p.g[gr * p.g_stride + gc] = __uint_as_float(bits);
        }
    }
}

// ----------------------------------------------------------------------------------------
// a row of Z -> its loss and its row of G: wavefront = row, lane = column in rounds of 64
// ----------------------------------------------------------------------------------------
// A float butterfly from distance 1 up, the sum in every lane: the order is part of the result (the tests restate it), so
// this is not the shared wave_sum, which runs from distance 32 down.
__device__ __forceinline__ float sm_wave_sum(float v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v = __fadd_rn(v, __shfl_xor(v, m, kWave));
    return v;
}

__global__ __launch_bounds__(kBlock) void k_sm_rows(const SmArgs p) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = (int64_t)blockIdx.x * kSmRows + wv;
    if (r >= p.n_rows) return;                               // no barrier in this kernel
    float *z_row = p.g + r * p.g_stride;
    const int n = p.n_cand;
    const int32_t t = p.target[r];
    // k_sm_logits marks the whole row of an invalid batch row, its target column too; a valid row's target is admissible
    const bool valid = t >= 0 && t < n && __float_as_uint(z_row[t]) != kSmMark;
    if (!valid) {
        for (int j = lane; j < n; j += kWave) z_row[j] = 0.0f;
        if (lane == 0) {
            p.rl[r] = 0.0f;
            if (p.n_adm) p.n_adm[r] = 0;
        }
        return;
    }
    const float zt = z_row[t];
    float m = -INFINITY;
    int cnt = 0, bad = 0;
    for (int j = lane; j < n; j += kWave) {
        const float z = z_row[j];
        if (__float_as_uint(z) == kSmMark) continue;
        cnt += 1;
        bad |= (z != z || z == INFINITY) ? 1 : 0;
        m = fmaxf(m, z);
    }
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) {
        m = fmaxf(m, __shfl_xor(m, k, kWave));
        cnt += __shfl_xor(cnt, k, kWave);
        bad |= __shfl_xor(bad, k, kWave);
    }
    float s = 0.0f;
    if (!bad) {
        for (int j = lane; j < n; j += kWave) {
            const float z = z_row[j];
            if (__float_as_uint(z) == kSmMark) continue;
            s = __fadd_rn(s, expf(__fsub_rn(z, m)));
        }
        s = sm_wave_sum(s);
    }
    // G = (p - [j = t]) * inv_tau / size in place of Z; exactly +0 where the pair is not admissible
    const float scale = __fdiv_rn(p.inv_tau, (float)p.size);
    for (int j = lane; j < n; j += kWave) {
        const float z = z_row[j];
        float gv = 0.0f;
        if (__float_as_uint(z) != kSmMark) {
            if (bad) {
                gv = __uint_as_float(kSmNan);
            } else {
                const float pj = __fdiv_rn(expf(__fsub_rn(z, m)), s);
                gv = __fmul_rn(__fsub_rn(pj, j == t ? 1.0f : 0.0f), scale);
            }
        }
        z_row[j] = gv;
    }
    if (lane == 0) {
        p.rl[r] = bad ? __uint_as_float(kSmNan) : __fadd_rn(__fsub_rn(m, zt), logf(s));
        if (p.n_adm) p.n_adm[r] = cnt - 1;
    }
}

// ----------------------------------------------------------------------------------------
// *loss = (sum of the row losses) / size: one workgroup, thread i takes rows i, i + 256, ... ascending, then a tree in LDS
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sm_loss(const SmArgs p) {
    __shared__ float part[kBlock];
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < p.n_rows; i += kBlock) s = __fadd_rn(s, p.rl[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] = __fadd_rn(part[threadIdx.x], part[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) p.loss[0] = __fdiv_rn(part[0], (float)p.size);
}

// ----------------------------------------------------------------------------------------
// the two gradient products.  TRANS false: out[i] = sum_j G[i, j] table[cand_items[j]]; true: out[j] = sum_i G[i, j]
// table[row_users[i]].  A table row whose id is out of range counts as zeros and is never addressed.
// ----------------------------------------------------------------------------------------
template <bool TRANS>
__global__ __launch_bounds__(kBlock) void k_sm_product(const SmArgs p) {
    __shared__ __attribute__((aligned(16))) float As[kSmPM * kSmPAS];
    __shared__ __attribute__((aligned(16))) float Bs[kSmPK * kSmPBS];
    __shared__ int kid[kSmPK];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int M = TRANS ? p.n_cand : p.n_rows, K = TRANS ? p.n_rows : p.n_cand;
    const int64_t lo = TRANS ? 0 : p.split, hi = TRANS ? p.split : p.table_rows;
    const int64_t *ids = TRANS ? p.row_users : p.cand_items;
    float *out = TRANS ? p.grad_cands : p.grad_users;
    const uint32_t m0 = blockIdx.x * (uint32_t)kSmPM;        // below 2^31 + 16: unsigned
    const int d0 = blockIdx.y * kSmPN;

    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t k0 = 0; k0 < K; k0 += kSmPK) {
        __syncthreads();                                     // the previous chunk is consumed
        if (tid < kSmPK) {
            int node = -1;
            if (k0 + tid < K) {
                const int64_t id = ids[k0 + tid];
                if (id >= lo && id < hi) node = (int)id;     // range-checked before an address is formed
            }
            kid[tid] = node;
        }
#pragma unroll
        for (int i = 0; i < kSmPM * kSmPK / kBlock; ++i) {   // G: zeros past either extent
            const int e = tid + kBlock * i;
            const int mm = TRANS ? (e & (kSmPM - 1)) : (e / kSmPK), kk = TRANS ? (e / kSmPM) : (e & (kSmPK - 1));
            const uint32_t gm = m0 + mm;
            const int64_t gk = k0 + kk;
            float v = 0.0f;
            if (gm < (uint32_t)M && gk < K) v = TRANS ? p.g[gk * p.g_stride + gm] : p.g[(int64_t)gm * p.g_stride + gk];
            As[mm * kSmPAS + kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSmPK * kSmPN / kBlock; ++i) {   // table rows: zeros past dim, never read there
            const int e = tid + kBlock * i, kk = e / kSmPN, col = e & (kSmPN - 1);
            const int node = kid[kk], d = d0 + col;
            float v = 0.0f;
            if (node >= 0 && d < p.dim) v = p.table[(int64_t)node * p.stride + d];
            Bs[kk * kSmPBS + col] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kSmPK / 4; ++kk)               // one instruction adds k = 4 kk .. 4 kk + 3 in order
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[c * kSmPAS + 4 * kk + q], Bs[(4 * kk + q) * kSmPBS + 16 * w + c], acc, 0,
                                                       0, 0);
    }
    // lane (c, q) holds output rows 4 q + r of column 16 w + c
    const int d = d0 + 16 * w + c;
    if (d < p.dim) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t gm = m0 + 4 * q + r;
            if (gm < (uint32_t)M) out[(int64_t)gm * p.grad_stride + d] = acc[r];
        }
    }
}

inline bool sm_sizes_ok(int64_t n_rows, int64_t n_cand) {
    if (n_rows < 0 || n_cand < 0 || n_rows > INT32_MAX || n_cand > INT32_MAX) return false;
    return n_cand <= (int64_t)65535 * kTileBN;                 // candidate tiles are the grid's second extent; with it the
                                                             // panel stays below 2^54 floats: its bytes fit 64 bits
}

// the row losses first, padded to 16 bytes, then the panel
inline size_t sm_rl_floats(int64_t n_rows) { return (size_t)((n_rows + 3) & ~(int64_t)3); }

unsigned long long lds_ok_sm_logits;

}  // namespace

extern "C" {

size_t lgc_softmax_workspace_bytes(int64_t n_rows, int64_t n_cand) {
    if (!sm_sizes_ok(n_rows, n_cand)) return 0;
    return sizeof(float) * (sm_rl_floats(n_rows) + (size_t)n_rows * (size_t)n_cand);
}

int lgc_softmax_batch(const float *table, int64_t stride, int64_t table_rows, int64_t split, int32_t dim,
                      const int64_t *row_users, int64_t n_rows, const int64_t *cand_items, int64_t n_cand, const int32_t *target,
                      const int32_t *ign_ptr, const int64_t *ign_items, const float *cand_bias, float inv_tau, int64_t size,
                      float *loss, float *row_loss, int32_t *n_adm, float *grad_logits, int64_t g_stride, float *grad_users,
                      float *grad_cands, int64_t grad_stride, void *workspace, size_t workspace_bytes, int32_t *status,
                      void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!table || !row_users || !cand_items || !target || !loss || !grad_users || !grad_cands || !status ||
        (ign_ptr == nullptr) != (ign_items == nullptr) || n_rows < 0 || n_cand < 0 || table_rows < 0 || size < 1 || stride < dim ||
        grad_stride < dim || (grad_logits && g_stride < n_cand) || !std::isfinite(inv_tau) || !(inv_tau > 0.0f) || split < 0 ||
        split > table_rows)
        return LGC_E_INVAL;
    if (table_rows > INT32_MAX || !sm_sizes_ok(n_rows, n_cand)) return LGC_E_RANGE;
    if (!aligned_to(table, 4) || !aligned_to(target, 4) || !aligned_to(ign_ptr, 4) || !aligned_to(cand_bias, 4) ||
        !aligned_to(loss, 4) || !aligned_to(row_loss, 4) || !aligned_to(n_adm, 4) || !aligned_to(grad_logits, 4) ||
        !aligned_to(grad_users, 4) || !aligned_to(grad_cands, 4) || !aligned_to(workspace, 4) || !aligned_to(status, 4) ||
        !aligned_to(row_users, 8) || !aligned_to(cand_items, 8) || !aligned_to(ign_items, 8))
        return LGC_E_ALIGN;
    const size_t need = lgc_softmax_workspace_bytes(n_rows, n_cand);
    if (need > 0 && (!workspace || workspace_bytes < need)) return LGC_E_WORKSPACE;
    hipStream_t stream = as_stream(stream_);
    if (n_rows == 0 || n_cand == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), stream);

    SmArgs p{};
    p.table = table;
    p.row_users = row_users;
    p.cand_items = cand_items;
    p.ign_items = ign_items;
    p.target = target;
    p.ign_ptr = ign_ptr;
    p.cand_bias = cand_bias;
    p.loss = loss;
    p.rl = row_loss ? row_loss : reinterpret_cast<float *>(workspace);
    p.g = grad_logits ? grad_logits : reinterpret_cast<float *>(workspace) + sm_rl_floats(n_rows);
    p.grad_users = grad_users;
    p.grad_cands = grad_cands;
    p.n_adm = n_adm;
    p.status = status;
    p.stride = stride;
    p.g_stride = grad_logits ? g_stride : n_cand;
    p.grad_stride = grad_stride;
    p.size = size;
    p.inv_tau = inv_tau;
    p.table_rows = (int32_t)table_rows;
    p.split = (int32_t)split;
    p.n_rows = (int32_t)n_rows;
    p.n_cand = (int32_t)n_cand;
    p.dim = dim;
    p.dp = tile_dp(dim);

    const size_t lds = sizeof(float) * (tile_lds_floats(p.dp) + kTileBN) + sizeof(int) * (kTileBN + 5 * kTileBM);
    int rc = allow_lds(reinterpret_cast<const void *>(k_sm_logits), lds, 48 * 1024, 96 * 1024, &lds_ok_sm_logits);
    if (rc != 0) return rc;
    const unsigned row_tiles = (unsigned)((n_rows + kTileBM - 1) / kTileBM), cand_tiles = (unsigned)((n_cand + kTileBN - 1) / kTileBN);
    hipLaunchKernelGGL(k_sm_logits, dim3(row_tiles, cand_tiles), dim3(kBlock), lds, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_sm_rows, dim3(ceil_div(n_rows, kSmRows)), dim3(kBlock), 0, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_sm_loss, dim3(1), dim3(kBlock), 0, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    const unsigned col_tiles = (unsigned)((dim + kSmPN - 1) / kSmPN);
    hipLaunchKernelGGL(k_sm_product<false>, dim3(ceil_div(n_rows, kSmPM), col_tiles), dim3(kBlock), 0, stream, p);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_sm_product<true>, dim3(ceil_div(n_cand, kSmPM), col_tiles), dim3(kBlock), 0, stream, p);
    return (int)hipGetLastError();
}

}  // extern "C"

// lgconv_train.hip -- what a training step runs around the hops: segment sums and seed preparation of the sparse
// backward pass, pair scoring, BPR loss, the regulariser and the Adam step.  C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// Fixed-order sum of runs: `key` is sorted; position t is a HEAD when key[t] != key[t - 1].  The lane group of a head adds
// vals[t], vals[t + 1], ... of its run in that order (fp32, sequential) and writes y[dest[t]] = (accumulate ? y[dest[t]]
// : 0) + scale * sum; positions that are not heads, and heads with dest < 0, write nothing.  Every destination row is
// owned by one lane group: no atomics, the same bits on every run -- the gradient of a scoring step has a few thousand
// non-zero rows (src/lightgcn.py:123-125 scores 2B pairs), repeated nodes are summed here instead of by float atomics.
__global__ __launch_bounds__(kBlock) void k_segment_sum(const int64_t *__restrict__ key, const int64_t *__restrict__ dest,
                                                       const float *__restrict__ vals, const int32_t *__restrict__ vals_index,
                                                       int64_t n, float scale,
                                                       float *__restrict__ y, int64_t y_stride, int64_t y_rows, int32_t dim,
                                                       int32_t accumulate) {
    const int lane = threadIdx.x & (kWave - 1);
    const int lpr = (dim + 3) / 4, groups = kWave / lpr;
    const int g = lane / lpr, l = lane - g * lpr;
    const int64_t t = ((int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave)) * groups + g;
    if (g >= groups || t >= n) return;
    const int64_t k = key[t];
    if (t > 0 && key[t - 1] == k) return;
    const int64_t d = dest[t];
    if (d < 0 || d >= y_rows) return;
    const int c0 = l * 4;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t u = t; u < n && key[u] == k; ++u) {
        const int64_t v = vals_index ? (int64_t)vals_index[u] : u;   // the sorted position's row of an UNSORTED value table
        for (int i = 0; i < 4; ++i)
            if (c0 + i < dim) acc[i] = __fadd_rn(acc[i], vals[v * dim + c0 + i]);
    }
    float *out = y + d * y_stride + c0;
    for (int i = 0; i < 4; ++i)
        if (c0 + i < dim) out[i] = __fadd_rn(accumulate ? out[i] : 0.0f, __fmul_rn(scale, acc[i]));
}

// ----------------------------------------------------------------------------------------
// Seed preparation of the sparse backward pass (lgc_seed_prepare): ONE workgroup sorts up to kSeedMax row ids and
// derives everything the segment sums and the seeded pull need -- what the host code did with ~25 small launches
// (sort, gathers, compares, index_puts) per training step.
// ----------------------------------------------------------------------------------------
constexpr int kSeedMax = 8192;
constexpr int kSeedBlock = 1024;

// Pass 1 (m / 8 workgroups): every workgroup keeps all m keys -- row + 1, ids outside the table as "no row" = 0; the
// position is the tie-break -- in LDS and RANKS eight of them by counting the smaller ones, 32 threads per key, each
// scanning 1/32 of the array (LDS reads: a wavefront reads two addresses, both broadcasts); (key, position) pairs are
// distinct, so the ranks are a permutation and sorted[rank] = key is a stable sort by row.  The scan is a dependent chain of
// LDS reads, so its time falls with the threads per key: 4 -> 36.7 us, 8 -> 19.5 us at m = 4096.  A one-workgroup bitonic sort of
// the same keys took 38-51 us (78 barrier stages of LDS-bound 64-bit compare-exchanges); 1024 keys per workgroup with
// one thread per key 69 us (four workgroups on the whole chip).
constexpr int kRankKeys = 8;      // keys ranked per workgroup of 256 threads: 32 threads per key (19.5 us with 8, 36.7 with 4)

__global__ __launch_bounds__(kBlock) void k_seed_rank(const int64_t *__restrict__ rows, int32_t m, int64_t n_nodes,
                                                     unsigned long long *__restrict__ sorted) {
    __shared__ __attribute__((aligned(16))) uint32_t key[kSeedMax];   // row + 1 (0 = "no row"); position = array index: 32 KiB
    __shared__ int part[kBlock];
    for (int i = threadIdx.x; i < m; i += kBlock) {
        int64_t r = rows[i];
        if (r < 0 || r >= n_nodes) r = -1;
        key[i] = (uint32_t)(r + 1);
    }
    __syncthreads();
    constexpr int kParts = kBlock / kRankKeys;
    const int k = threadIdx.x & (kRankKeys - 1), q = threadIdx.x / kRankKeys;     // key k of this workgroup, slice q of the array
    const int i = blockIdx.x * kRankKeys + k;
    const uint32_t mine = i < m ? key[i] : 0u;
    const int per = ((m + 4 * kParts - 1) / (4 * kParts)) * 4, lo = min(m, q * per), hi = min(m, lo + per);   // whole uint4s
    // (row, position) order: everything with a smaller row, and the equal rows in front of me; branch-free, four keys per
    // LDS read, two reads in flight
    int rank = 0;
    int j = lo;
    auto count4 = [&](const u4 o, int at) {
        return (int)(o.x < mine) + (int)((o.x == mine) & (at < i)) + (int)(o.y < mine) + (int)((o.y == mine) & (at + 1 < i)) +
               (int)(o.z < mine) + (int)((o.z == mine) & (at + 2 < i)) + (int)(o.w < mine) + (int)((o.w == mine) & (at + 3 < i));
    };
    for (; j + 8 <= hi; j += 8) {
        const u4 o0 = *reinterpret_cast<const u4 *>(key + j), o1 = *reinterpret_cast<const u4 *>(key + j + 4);
        rank += count4(o0, j) + count4(o1, j + 4);
    }
    for (; j < hi; ++j) {
        const uint32_t o = key[j];
        rank += (int)(o < mine) + (int)((o == mine) & (j < i));
    }
    part[threadIdx.x] = rank;
    __syncthreads();
    if (q == 0 && i < m) {
        int total = 0;
#pragma unroll
        for (int p = 0; p < kParts; ++p) total += part[p * kRankKeys + k];
        sorted[total] = ((unsigned long long)mine << 13) | (unsigned)i;
    }
}

// Pass 2: one thread per sorted position -- run heads, destination lists, the pull's column map.
__global__ void k_seed_finish(const unsigned long long *__restrict__ key, int32_t m, int64_t split,
                              int64_t *__restrict__ rows_sorted, int32_t *__restrict__ perm, int64_t *__restrict__ dest_item,
                              int64_t *__restrict__ dest_slot, int64_t *__restrict__ dest_user,
                              uint8_t *__restrict__ col_flag, int32_t *__restrict__ col_slot) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const unsigned long long k = key[t];
    const int64_t row = (int64_t)(k >> 13) - 1;
    const bool head = t == 0 || (int64_t)(key[t - 1] >> 13) - 1 != row;
    const bool user = row >= 0 && row < split, item = row >= split;
    rows_sorted[t] = row;
    perm[t] = (int32_t)(k & 0x1FFF);
    dest_item[t] = (head && item) ? row : -1;
    dest_slot[t] = (head && user) ? t : -1;
    dest_user[t] = (head && user) ? row : -1;
    if (head && user && col_flag) {
        col_flag[row] = 1;
        col_slot[row] = t;
    }
}

// flag[row] = value for the user rows (0 <= row < split) of a sorted row list: takes the flags of a step's seeds back
__global__ void k_seed_flags(const int64_t *__restrict__ rows_sorted, int64_t m, int64_t split, uint8_t *__restrict__ flag,
                             uint8_t value) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int64_t row = rows_sorted[t];
    if (row >= 0 && row < split) flag[row] = value;
}

// Pair scoring that keeps what the backward pass needs (lgc_pair_dot_rows): scores as k_pair_dot, plus the two gathered
// rows of every pair and a validity byte -- instead of four compares, three ands, two clamps and two row gathers on the
// host side.  An out-of-range pair scores NaN, keeps zero rows, ok = 0, and raises the status bit.
__global__ __launch_bounds__(kBlock) void k_pair_dot_rows(const float *__restrict__ emb, int64_t stride, int32_t dim,
                                                         int64_t n_nodes, const int64_t *__restrict__ idx0,
                                                         const int64_t *__restrict__ idx1, int64_t n_pairs,
                                                         float *__restrict__ scores, float *__restrict__ rows0,
                                                         float *__restrict__ rows1, uint8_t *__restrict__ ok,
                                                         int32_t *__restrict__ status) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t m = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);
    if (m >= n_pairs) return;
    const int64_t a = idx0[m], b = idx1[m];
    const bool valid = a >= 0 && a < n_nodes && b >= 0 && b < n_nodes;   // wave-uniform
    if (!valid && lane == 0) {
        atomicOr(status, LGC_ST_INDEX_OOB);
        scores[m] = NAN;
    }
    if (lane == 0 && ok) ok[m] = valid ? 1 : 0;
    const float *pa = emb + a * stride, *pb = emb + b * stride;
    float s = 0.0f;
    for (int c = lane; c < dim; c += kWave) {
        const float va = valid ? pa[c] : 0.0f, vb = valid ? pb[c] : 0.0f;
        s += va * vb;
        if (rows0) rows0[m * dim + c] = va;
        if (rows1) rows1[m * dim + c] = vb;
    }
    if (!valid) return;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) scores[m] = s;
}

// The seed of the backward pass from the gradient of the scores (lgc_pair_seed_vals):
//   vals[m]           = g[m] * rows1[m]      d score_m / d out[idx0[m]] = out[idx1[m]]
//   vals[n_pairs + m] = g[m] * rows0[m]      d score_m / d out[idx1[m]] = out[idx0[m]]
// with g[m] = mask[m] ? grad_scores[m] * (*grad_scale) : 0.  grad_scale: an optional DEVICE scalar (the upstream
// gradient of a loss this node computed itself), so that no host sync is needed to read it.
__global__ __launch_bounds__(kBlock) void k_pair_seed_vals(const float *__restrict__ grad_scores, const uint8_t *__restrict__ mask,
                                                          const float *__restrict__ grad_scale, const float *__restrict__ rows0,
                                                          const float *__restrict__ rows1, int64_t n_pairs, int32_t dim,
                                                          float *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs * dim) return;
    const int64_t m = i / dim;
    float g = (mask == nullptr || mask[m]) ? grad_scores[m] : 0.0f;
    if (grad_scale) g = __fmul_rn(g, *grad_scale);
    vals[i] = __fmul_rn(g, rows1[i]);
    vals[n_pairs * dim + i] = __fmul_rn(g, rows0[i]);
}

// BPR loss of one batch of triples and its gradient with respect to the scores (lgc_bpr_loss): what
// `recommendation_loss(out[:B], out[B:], 0) * B` of src/train_lightgcn.py:141 (src/lightgcn.py:262-286 with lambda_reg = 0)
// and its autograd compute with ~15 launches:  loss = -sum_{t: mask[t]} log sigmoid(s[t] - s[B + t]) / size,
// grad[t] = -sigmoid(-(s[t] - s[B + t])) / size, grad[B + t] = -grad[t] (0 where the mask is off).  One workgroup, a fixed
// reduction tree: the same bits on every run.  logsigmoid(d) = min(d, 0) - log1p(exp(-|d|)), torch's formula.
__global__ __launch_bounds__(kSeedBlock) void k_bpr_loss(const float *__restrict__ scores, const uint8_t *__restrict__ mask,
                                                        int64_t n_triples, float inv_size, float *__restrict__ loss,
                                                        float *__restrict__ grad) {
    __shared__ float part[kSeedBlock];
    float acc = 0.0f;
    for (int64_t t = threadIdx.x; t < n_triples; t += kSeedBlock) {
        const bool on = mask == nullptr || mask[t] != 0;
        const float d = on ? scores[t] - scores[n_triples + t] : 0.0f;
        const float ls = fminf(d, 0.0f) - log1pf(expf(-fabsf(d)));
        const float sg = 1.0f / (1.0f + expf(d));                  // sigmoid(-d)
        if (on) acc += ls;
        grad[t] = on ? -sg * inv_size : 0.0f;
        grad[n_triples + t] = on ? sg * inv_size : 0.0f;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kSeedBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = -part[0] * inv_size;
}

// The regulariser of src/utils_v2.py:193-211 on three id lists of one table (lgc_reg_rows): what
//   (1/2) * (w[u].norm().pow(2) + w[p].norm().pow(2) + w[n].norm().pow(2)) / size * decay
// costs as 13 torch launches (three gathers into [B, D] copies, three norms, pows, adds, scalings) plus nine more that
// normalise the ids for the gradient's row list -- in ONE workgroup: a thread per row (columns in order), per-list sums of
// squares added up in a fixed order (the same bits on every run),
// value = scale * ((sqrt S_u)^2 + (sqrt S_p)^2 + (sqrt S_n)^2) like the expression above.  rows_out (int64 [m0 + m1 + m2],
// optional): the ids as row numbers, negative ids wrapped (torch's indexing), an id outside [-n_rows, n_rows) as -1 = "no
// row" -- such an id contributes nothing and sets LGC_ST_INDEX_OOB (upstream's gather raises).
__global__ __launch_bounds__(kSeedBlock) void k_reg_rows(const float *__restrict__ w, int64_t stride, int32_t dim, int64_t n_rows,
                                                        const int64_t *__restrict__ ids0, int64_t m0,
                                                        const int64_t *__restrict__ ids1, int64_t m1,
                                                        const int64_t *__restrict__ ids2, int64_t m2, float scale,
                                                        float *__restrict__ value, int64_t *__restrict__ rows_out,
                                                        int32_t *__restrict__ status) {
    constexpr int kWaves = kSeedBlock / kWave;
    __shared__ float part[3][kWaves];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t total = m0 + m1 + m2;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    // a THREAD per row (a wavefront per row made one workgroup walk 3 B rows through two dependent loads each: 200 us): the
    // dim / 4 loads of a row are independent, a thread has all of them in flight
    for (int64_t t = threadIdx.x; t < total; t += kSeedBlock) {
        const int which = t < m0 ? 0 : (t < m0 + m1 ? 1 : 2);
        int64_t id = which == 0 ? ids0[t] : (which == 1 ? ids1[t - m0] : ids2[t - m0 - m1]);
        if (id < 0) id += n_rows;
        const bool ok = id >= 0 && id < n_rows;
        if (rows_out != nullptr) rows_out[t] = ok ? id : -1;
        if (!ok) {
            atomicOr(status, LGC_ST_INDEX_OOB);
            continue;
        }
        const float *row = w + id * stride;
        float sq = 0.0f;
        int c = 0;
        for (; c + 4 <= dim; c += 4) {
            const f4 v = *reinterpret_cast<const f4u *>(row + c);
            sq += v.x * v.x;
            sq += v.y * v.y;
            sq += v.z * v.z;
            sq += v.w * v.w;
        }
        for (; c < dim; ++c) sq += row[c] * row[c];
        acc[which] += sq;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float v = acc[j];
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) part[j][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float out = 0.0f;
        for (int j = 0; j < 3; ++j) {
            float sum = 0.0f;
            for (int i = 0; i < kWaves; ++i) sum += part[j][i];
            const float nrm = sqrtf(sum);
            out += nrm * nrm;
        }
        value[0] = out * scale;
    }
}

// ----------------------------------------------------------------------------------------
// Dense Adam step over the embedding table (the caller's optimizer.step(), src/train_lightgcn.py:58,147)
// ----------------------------------------------------------------------------------------
// One pass: w, g, m, v read once, w, m, v written once (7 x 434 MB at 1.7 M x 64): torch.optim.Adam's arithmetic for
// amsgrad=False, weight_decay=0, maximize=False --
//   m <- m + (g - m) (1 - beta1);  v <- beta2 v + (1 - beta2) g g;  w <- w - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t computed by the host in double and handed over as step_size, bc2_sqrt.
// (1 - beta1) and (1 - beta2) come from the host, rounded from double like torch's scalars: 1.0f - 0.999f is 4.7e-5 off.
constexpr int kAdamU = 2;
__global__ __launch_bounds__(kBlock) void k_adam(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                                float *__restrict__ v, int64_t n4, int64_t n, float beta2, float omb1, float omb2,
                                                float eps, float step_size, float bc2_sqrt, const float *__restrict__ hyper) {
    if (hyper != nullptr) {   // lgc_adam_step_hp: the step's scalars live in device memory (a captured launch is replayed with
        omb1 = hyper[0]; beta2 = hyper[1]; omb2 = hyper[2]; eps = hyper[3]; step_size = hyper[4]; bc2_sqrt = hyper[5];   // new values)
    }
    auto one = [&](float &wi, float gi, float &mi, float &vi) {
        mi = mi + (gi - mi) * omb1;
        vi = beta2 * vi + omb2 * gi * gi;
        wi = wi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    };
    constexpr int U = kAdamU;                 // float4s per thread and array: 8 loads in flight per thread (1 / 4: the same time)
    const int64_t base = ((int64_t)blockIdx.x * blockDim.x) * U + threadIdx.x;
    f4 w4[U], g4[U], m4[U], v4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * blockDim.x;
        if (i < n4) {
            w4[u] = reinterpret_cast<f4 *>(w)[i];
            g4[u] = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(g) + i);   // read once: 566 -> 546 us for 108 M elements
            m4[u] = reinterpret_cast<f4 *>(m)[i];
            v4[u] = reinterpret_cast<f4 *>(v)[i];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * blockDim.x;
        if (i < n4) {
            float wv[4] = {w4[u].x, w4[u].y, w4[u].z, w4[u].w}, gv[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w};
            float mv[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w}, vv[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) one(wv[j], gv[j], mv[j], vv[j]);
            reinterpret_cast<f4 *>(w)[i] = f4{wv[0], wv[1], wv[2], wv[3]};
            reinterpret_cast<f4 *>(m)[i] = f4{mv[0], mv[1], mv[2], mv[3]};
            reinterpret_cast<f4 *>(v)[i] = f4{vv[0], vv[1], vv[2], vv[3]};
        }
    }
    // tail (n not a multiple of 4): the first threads of block 0
    const int64_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) one(w[t], g[t], m[t], v[t]);
}

// ----------------------------------------------------------------------------------------
// Pair scoring
// ----------------------------------------------------------------------------------------
// One wavefront per pair; lanes stride the feature axis, butterfly reduce over 64 lanes.
__global__ __launch_bounds__(kBlock) void k_pair_dot(const float *__restrict__ emb, int64_t stride, int32_t dim,
                                                    int64_t n_nodes, const int64_t *__restrict__ idx0,
                                                    const int64_t *__restrict__ idx1, int64_t n_pairs,
                                                    float *__restrict__ scores, int32_t *__restrict__ status) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t m = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);
    if (m >= n_pairs) return;
    const int64_t a = idx0[m], b = idx1[m];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) {  // wave-uniform
        if (lane == 0) {
            atomicOr(status, LGC_ST_INDEX_OOB);
            scores[m] = NAN;
        }
        return;
    }
    const float *pa = emb + a * stride, *pb = emb + b * stride;
    float s = 0.0f;
    for (int c = lane; c < dim; c += kWave) s += pa[c] * pb[c];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) scores[m] = s;
}

}  // namespace

extern "C" {

int lgc_segment_sum(const int64_t *key_sorted, const int64_t *dest, const float *vals, const int32_t *vals_index, int64_t n,
                    float scale, float *y, int64_t y_stride, int64_t y_rows, int32_t dim, int32_t accumulate, void *stream_) {
    if (!y || n < 0 || y_rows < 0 || dim < 1 || dim > 256 || y_stride < dim) return LGC_E_INVAL;
    if (n == 0) return 0;
    if (!key_sorted || !dest || !vals) return LGC_E_INVAL;
    const int groups = kWave / ((dim + 3) / 4);
    hipLaunchKernelGGL(k_segment_sum, dim3(ceil_div(n, (int64_t)(kBlock / kWave) * groups)), dim3(kBlock), 0, as_stream(stream_),
                       key_sorted, dest, vals, vals_index, n, scale, y, y_stride, y_rows, dim, accumulate);
    return (int)hipGetLastError();
}

int lgc_seed_prepare(const int64_t *rows, int64_t m, int64_t split, int64_t n_nodes, int64_t *rows_sorted, int32_t *perm,
                     int64_t *dest_item, int64_t *dest_slot, int64_t *dest_user, uint8_t *col_flag, int32_t *col_slot,
                     uint64_t *scratch, void *stream_) {
    if (m < 0 || m > LGC_SEED_MAX) return LGC_E_RANGE;
    if (split < 0 || n_nodes < split || (col_flag != nullptr) != (col_slot != nullptr)) return LGC_E_INVAL;
    if (m == 0) return 0;
    if (!rows || !rows_sorted || !perm || !dest_item || !dest_slot || !dest_user || !scratch) return LGC_E_INVAL;
    hipStream_t st = as_stream(stream_);
    hipLaunchKernelGGL(k_seed_rank, dim3(ceil_div(m, kRankKeys)), dim3(kBlock), 0, st, rows, (int32_t)m, n_nodes,
                       reinterpret_cast<unsigned long long *>(scratch));
    hipLaunchKernelGGL(k_seed_finish, dim3(ceil_div(m, kBlock)), dim3(kBlock), 0, st,
                       reinterpret_cast<const unsigned long long *>(scratch), (int32_t)m, split, rows_sorted, perm, dest_item,
                       dest_slot, dest_user, col_flag, col_slot);
    return (int)hipGetLastError();
}

int lgc_seed_flags(const int64_t *rows_sorted, int64_t m, int64_t split, uint8_t *col_flag, int32_t value, void *stream_) {
    if (m < 0 || split < 0 || value < 0 || value > 255) return LGC_E_INVAL;
    if (m == 0) return 0;
    if (!rows_sorted || !col_flag) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_seed_flags, dim3(ceil_div(m, kBlock)), dim3(kBlock), 0, as_stream(stream_), rows_sorted, m, split,
                       col_flag, (uint8_t)value);
    return (int)hipGetLastError();
}

int lgc_pair_dot_rows(const float *emb, int64_t stride, int32_t dim, int64_t n_nodes, const int64_t *idx0, const int64_t *idx1,
                      int64_t n_pairs, float *scores, float *rows0, float *rows1, uint8_t *ok, int32_t *status, void *stream_) {
    if (!emb || !status || dim < 1 || stride < dim || n_nodes < 0 || n_pairs < 0) return LGC_E_INVAL;
    if (n_pairs == 0) return 0;
    if (!idx0 || !idx1 || !scores) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_pair_dot_rows, dim3(ceil_div(n_pairs, kBlock / kWave)), dim3(kBlock), 0, as_stream(stream_), emb, stride,
                       dim, n_nodes, idx0, idx1, n_pairs, scores, rows0, rows1, ok, status);
    return (int)hipGetLastError();
}

int lgc_pair_seed_vals(const float *grad_scores, const uint8_t *mask, const float *grad_scale, const float *rows0,
                       const float *rows1, int64_t n_pairs, int32_t dim, float *vals, void *stream_) {
    if (n_pairs < 0 || dim < 1) return LGC_E_INVAL;
    if (n_pairs == 0) return 0;
    if (!grad_scores || !rows0 || !rows1 || !vals) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_pair_seed_vals, dim3(ceil_div(n_pairs * dim, kBlock)), dim3(kBlock), 0, as_stream(stream_), grad_scores,
                       mask, grad_scale, rows0, rows1, n_pairs, dim, vals);
    return (int)hipGetLastError();
}

int lgc_bpr_loss(const float *scores, const uint8_t *mask, int64_t n_triples, int64_t size, float *loss, float *grad,
                 void *stream_) {
    if (!loss || n_triples < 0 || size <= 0) return LGC_E_INVAL;
    if (n_triples > 0 && (!scores || !grad)) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_bpr_loss, dim3(1), dim3(kSeedBlock), 0, as_stream(stream_), scores, mask, n_triples,
                       1.0f / (float)size, loss, grad);
    return (int)hipGetLastError();
}

int lgc_reg_rows(const float *w, int64_t stride, int32_t dim, int64_t n_rows, const int64_t *ids0, int64_t m0, const int64_t *ids1,
                 int64_t m1, const int64_t *ids2, int64_t m2, float scale, float *value, int64_t *rows_out, int32_t *status,
                 void *stream_) {
    if (!w || !value || !status || dim < 1 || stride < dim || n_rows < 0 || m0 < 0 || m1 < 0 || m2 < 0) return LGC_E_INVAL;
    if ((m0 > 0 && !ids0) || (m1 > 0 && !ids1) || (m2 > 0 && !ids2)) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_reg_rows, dim3(1), dim3(kSeedBlock), 0, as_stream(stream_), w, stride, dim, n_rows, ids0, m0, ids1, m1, ids2,
                       m2, scale, value, rows_out, status);
    return (int)hipGetLastError();
}

static int adam_launch(float *w, const float *g, float *m, float *v, int64_t n, float one_minus_beta1, float beta2,
                       float one_minus_beta2, float eps, float step_size, float bias_correction2_sqrt, const float *hyper,
                       void *stream_) {
    if (!w || !g || !m || !v || n < 0) return LGC_E_INVAL;
    // dword-aligned, and all four at the same offset inside a 16-byte line (a row range of same-shaped tables whose rows
    // are not whole float4s, e.g. rows [lo, hi) of a [N, 90] table): the first elements up to the line are done one by one
    const uintptr_t mis = reinterpret_cast<uintptr_t>(w) & 15;
    if ((mis & 3) != 0 || (reinterpret_cast<uintptr_t>(g) & 15) != mis || (reinterpret_cast<uintptr_t>(m) & 15) != mis ||
        (reinterpret_cast<uintptr_t>(v) & 15) != mis)
        return LGC_E_ALIGN;
    if (n == 0) return 0;
    hipStream_t stream = as_stream(stream_);
    const int64_t head = std::min<int64_t>(n, (int64_t)((16 - mis) & 15) / 4);
    if (head > 0)
        hipLaunchKernelGGL(k_adam, dim3(1), dim3(kBlock), 0, stream, w, g, m, v, (int64_t)0, head, beta2, one_minus_beta1,
                           one_minus_beta2, eps, step_size, bias_correction2_sqrt, hyper);
    w += head; g += head; m += head; v += head; n -= head;
    if (n == 0) return (int)hipGetLastError();
    const int64_t n4 = n / 4;
    const int64_t blocks = std::max<int64_t>(ceil_div(n4, (int64_t)kBlock * kAdamU), 1);
    if (blocks >= INT32_MAX) return LGC_E_RANGE;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(kBlock), 0, stream, w, g, m, v, n4, n, beta2,
                       one_minus_beta1, one_minus_beta2, eps, step_size, bias_correction2_sqrt, hyper);
    return (int)hipGetLastError();
}

int lgc_adam_step(float *w, const float *g, float *m, float *v, int64_t n, float one_minus_beta1, float beta2,
                  float one_minus_beta2, float eps, float step_size, float bias_correction2_sqrt, void *stream_) {
    if (!(bias_correction2_sqrt > 0.0f)) return LGC_E_INVAL;
    return adam_launch(w, g, m, v, n, one_minus_beta1, beta2, one_minus_beta2, eps, step_size, bias_correction2_sqrt, nullptr,
                       stream_);
}

int lgc_adam_step_hp(float *w, const float *g, float *m, float *v, int64_t n, const float *hyper, void *stream_) {
    if (!hyper) return LGC_E_INVAL;
    return adam_launch(w, g, m, v, n, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, hyper, stream_);
}

int lgc_pair_dot(const float *emb, int64_t stride, int32_t dim, int64_t n_nodes, const int64_t *idx0,
                 const int64_t *idx1, int64_t n_pairs, float *scores, int32_t *status, void *stream_) {
    if (!emb || !status || dim < 1 || stride < dim || n_nodes < 0 || n_pairs < 0) return LGC_E_INVAL;
    if (n_pairs == 0) return 0;
    if (!idx0 || !idx1 || !scores) return LGC_E_INVAL;
    hipLaunchKernelGGL(k_pair_dot, dim3(ceil_div(n_pairs, kBlock / kWave)), dim3(kBlock), 0, as_stream(stream_), emb,
                       stride, dim, n_nodes, idx0, idx1, n_pairs, scores, status);
    return (int)hipGetLastError();
}

}  // extern "C"

// lgconv_explain.hip -- score attribution: every score <e_u, E[t]> of a request row split additively over the row's own
// interaction list, the full split and the m largest contributions per target.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// score(u, t) = a0 <z, E[t]> + sum_k c_k <F[i_k], E[t]>   (DESIGN.md section 18): fold-in's line dotted with a served item row.
//
// One workgroup per request row.  The row's target rows of E and its layer-0 row z are staged once in LDS, row stride
// 4 * (groups | 1) floats as lgc_score_rows' item tile (lanes on different targets read different bank quads).  The list
// is walked in batches of kAttrBatch entries:
//   phase A  every thread owns (entry, target) pairs of the batch: one chain of fused multiply-adds over d ascending from
//            +0 with zeros past dim -- lgc_score_rows' chain, so dot(F[i], E[t]) has the bits that entry point writes for
//            the two rows -- then ONE rounded product with c_k, into an LDS tile [batch, n_targets] and into `contrib`;
//   phase B  thread t < n_targets walks the tile in list order: adds into its running total (__fadd_rn from +0) and
//            inserts into its sorted list of the best (order_key of lgc_mask_topk, ties by list position) in
//            registers -- only when its key beats the one in place top_m - 1.
// The list entries of batch b + 2 and the F rows of batch b + 1 are requested before batch b is worked on.
// Session form: c_k with lgc_fold_in's arithmetic (sequential fp32 degree in list order by wavefront 0, correctly rounded
// 1 / sqrt, inf -> 0, (item_dis * w) * d left to right).  Graph form: c_k = the CSR value.  A skipped entry (item or
// column out of range) takes no part: +0 in `contrib`, nothing in total and top.  No float atomics, plain vector stores.
constexpr int kAttrBatch = 32;
constexpr int kAttrTop = LGC_ATTR_MAX_TOP;
constexpr int kAttrStage = kAttrBatch * 64 / kBlock;   // float4 groups of the next batch's F rows a thread holds (dim <= 256)
static_assert(kAttrStage * kBlock == kAttrBatch * 64, "a batch of 256-column rows is dealt evenly over the workgroup");

struct AttrArgs {
    lgc_attr_args a;
    int32_t groups, es;             // float4 groups of a row (ceil(dim / 4)); LDS row stride in floats
};

// Four floats of a table row from column d; columns >= dim read as 0 and are never touched: what load4 of lgconv_common.h
// gives, but dword by dword where the rows are not 16-byte aligned.  Kept: load4<false>'s one overlapping 16-byte load is
// other code for k_attribute<false>, and that has not been timed.
template <bool VEC>
__device__ __forceinline__ f4 attr_load4(const float *__restrict__ row, int d, int dim) {
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (VEC) {
        v = *reinterpret_cast<const f4 *>(row + d);          // dim % 4 == 0, rows 16-byte aligned
    } else {
        if (d + 0 < dim) v.x = row[d + 0];
        if (d + 1 < dim) v.y = row[d + 1];
        if (d + 2 < dim) v.z = row[d + 2];
        if (d + 3 < dim) v.w = row[d + 3];
    }
    return v;
}

// lgc_score_rows' chain (score_chain) over the whole staged rows, `a` the user-side row, `b` the item row
__device__ __forceinline__ float attr_dot(const float *a, const float *b, int groups) {
    float acc = 0.0f;
    for (int g = 0; g < groups; ++g) {
        const f4 x = *reinterpret_cast<const f4 *>(a + 4 * g), y = *reinterpret_cast<const f4 *>(b + 4 * g);
        acc = score_chain(x, y, acc);
    }
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_attribute(const AttrArgs p) {
    extern __shared__ __attribute__((aligned(16))) float attr_lds[];
    const lgc_attr_args &a = p.a;
    const int T = a.n_targets, groups = p.groups, es = p.es, dim = a.dim, m = a.top_m;
    float *Es = attr_lds;                                    // [T + 1][es]: the target rows of E, then z
    float *Fs = Es + (T + 1) * es;                           // [kAttrBatch][es]: the F rows of the current batch
    float *tile = Fs + kAttrBatch * es;                      // [kAttrBatch][T]: the batch's contributions
    int *s_tgt = reinterpret_cast<int *>(tile + kAttrBatch * T);   // [64]: target item, -1 = nothing
    int *m_item = s_tgt + 64;                                // [3][kAttrBatch]: item of an entry, -1 = skipped / past the end
    float *m_c = reinterpret_cast<float *>(m_item + 3 * kAttrBatch);   // [3][kAttrBatch]: c_k
    float *s_d = m_c + 3 * kAttrBatch;                       // [1]: d of the session form
    int *s_init = reinterpret_cast<int *>(s_d + 1);          // [1]: the init row, -1 = none
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t r = blockIdx.x;
    const bool session = a.list_ptr != nullptr;

    // the row's list [lo, lo + n) and its span of `contrib`
    int64_t lo = 0, n = 0;
    bool bad_row = false;
    if (session) {
        lo = a.list_ptr[r];
        n = a.list_ptr[r + 1] - lo;
    } else {
        const int64_t rid = a.row_ids[r];
        bad_row = rid < 0 || rid >= a.n_graph_rows;          // range-checked before rowptr is indexed
        if (!bad_row) {
            lo = a.rowptr[rid];
            n = a.rowptr[rid + 1] - lo;
        }
    }
    if (n < 0) n = 0;
    int64_t c_lo = 0, span = 0;
    if (a.contrib) {
        c_lo = a.contrib_ptr[r];
        span = a.contrib_ptr[r + 1] - c_lo;
    }
    if (bad_row) {                                           // block-uniform: every output of the row is "nothing"
        if (tid == 0) atomicOr(a.status, LGC_ST_INDEX_OOB);
        for (int64_t e = tid; e < span * T; e += kBlock) a.contrib[c_lo * T + e] = 0.0f;
        if (tid < T) {
            const int64_t o = r * T + tid;
            if (a.base) a.base[o] = 0.0f;
            if (a.total) a.total[o] = 0.0f;
            for (int q = 0; q < m; ++q) {
                a.top_pos[o * m + q] = -1;
                a.top_item[o * m + q] = -1;
                a.top_value[o * m + q] = 0.0f;
            }
        }
        return;
    }

    // targets and the init row: range-checked here, before any address is formed from them
    if (tid < T) {
        const int64_t t = a.targets[r * a.target_stride + tid];
        const bool ok = t >= 0 && t < a.n_items;
        if (!ok && t != -1) atomicOr(a.status, LGC_ST_INDEX_OOB);
        s_tgt[tid] = ok ? (int)t : -1;
    } else if (tid == kWave) {
        const int64_t id = a.init_rows ? a.init_rows[r] : -1;
        const bool ok = id >= 0 && id < a.n_init_rows;
        if (!ok && id != -1) atomicOr(a.status, LGC_ST_INDEX_OOB);
        s_init[0] = ok ? (int)id : -1;
    }

    // entry `pos` of the list: its item (-1: past the end or out of range) and c_k
    auto load_entry = [&](int64_t pos, float d, int &item, float &c) {
        item = -1;
        c = 0.0f;
        if (pos >= n) return;
        const int64_t e = lo + pos;
        if (session) {
            const int64_t it = a.list_items[e];
            if (it >= 0 && it < a.n_items) {
                item = (int)it;
                const float w = a.list_weight ? a.list_weight[e] : 1.0f;
                c = a.normalize ? __fmul_rn(__fmul_rn(a.item_dis[it], w), d) : w;
            } else {
                atomicOr(a.status, LGC_ST_INDEX_OOB);
            }
        } else {
            const lgc_entry en = a.entries[e];
            const int64_t it = (int64_t)en.col - a.col_base;
            if (it >= 0 && it < a.n_items) {
                item = (int)it;
                c = en.val;
            } else {
                atomicOr(a.status, LGC_ST_INDEX_OOB);
            }
        }
    };

    // d = deg^-1/2 with lgc_fold_in's arithmetic: the fp32 sum of the weights sequentially in list order (an entry out of
    // range enters as +0), 1 / sqrt correctly rounded, inf -> 0.  Wavefront 0 walks the list 64 entries at a time.
    if (tid < kWave && session && a.normalize) {
        auto load_w = [&](int64_t base) {
            const int64_t pos = base + lane;
            float w = 0.0f;
            if (pos < n) {
                const int64_t it = a.list_items[lo + pos];
                if (it >= 0 && it < a.n_items) w = a.list_weight ? a.list_weight[lo + pos] : 1.0f;
            }
            return w;
        };
        float deg = 0.0f, w = load_w(0);
        for (int64_t base = 0; base < n; base += kWave) {
            float w_next = 0.0f;
            if (base + kWave < n) w_next = load_w(base + kWave);         // in flight during this batch's adds
            const int nb = (int)min((int64_t)kWave, n - base);
            for (int i = 0; i < nb; ++i)
                deg = __fadd_rn(deg, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), i)));
            w = w_next;
        }
        float d = 1.0f / sqrtf(deg);
        if (d == INFINITY) d = 0.0f;
        if (lane == 0) s_d[0] = d;
    }
    __syncthreads();                                         // s_tgt, s_init, s_d

    // the target rows of E and z, whole width, once; a column or row that is "nothing" is zeros and never multiplied
    const int init_id = s_init[0];
    for (int e = tid; e < (T + 1) * groups; e += kBlock) {
        const int row = e / groups, g = e - row * groups;
        f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row < T) {
            const int t = s_tgt[row];
            if (t >= 0) v = attr_load4<VEC>(a.items + (int64_t)t * a.item_stride, 4 * g, dim);
        } else if (init_id >= 0) {
            v = attr_load4<VEC>(a.init + (int64_t)init_id * a.init_stride, 4 * g, dim);
        }
        *reinterpret_cast<f4 *>(Es + row * es + 4 * g) = v;
    }
    // the entries of batches 0 and 1
    const float d = (session && a.normalize) ? s_d[0] : 1.0f;
    if (tid < 2 * kAttrBatch) {
        int item;
        float c;
        load_entry(tid, d, item, c);
        m_item[tid] = item;                                  // buffers 0 and 1 are adjacent
        m_c[tid] = c;
    }
    __syncthreads();

    // the F rows of one batch: thread -> float4 group e = tid + kBlock * q of the [kAttrBatch, groups] block
    f4 stage[kAttrStage];
    auto load_rows = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kAttrStage; ++q) {
            const int e = tid + kBlock * q;
            f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (e < kAttrBatch * groups) {
                const int j = e / groups, g = e - j * groups;
                const int it = m_item[buf * kAttrBatch + j];
                if (it >= 0) v = attr_load4<VEC>(a.fold + (int64_t)it * a.fold_stride, 4 * g, dim);
            }
            stage[q] = v;
        }
    };
    auto store_rows = [&]() {
#pragma unroll
        for (int q = 0; q < kAttrStage; ++q) {
            const int e = tid + kBlock * q;
            if (e < kAttrBatch * groups) {
                const int j = e / groups, g = e - j * groups;
                *reinterpret_cast<f4 *>(Fs + j * es + 4 * g) = stage[q];
            }
        }
    };
    if (n > 0) {
        load_rows(0);
        store_rows();
    }
    __syncthreads();

    // phase B's state: thread t < T owns target t
    const int my_tgt = tid < T ? s_tgt[tid] : -1;
    float total = 0.0f;
    uint32_t tkey[kAttrTop];
    int tpos[kAttrTop], titem[kAttrTop];
    float tval[kAttrTop];
    uint32_t thr = 0u;                                       // the key in place m - 1: what a new entry has to beat
#pragma unroll
    for (int q = 0; q < kAttrTop; ++q) {
        tkey[q] = 0u;                                        // below every real key (-inf has key 0x007FFFFF)
        tpos[q] = -1;
        titem[q] = -1;
        tval[q] = 0.0f;
    }

    const int64_t n_batches = (n + kAttrBatch - 1) / kAttrBatch;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int cur = (int)(b % 3), nxt = (int)((b + 1) % 3), nxt2 = (int)((b + 2) % 3);
        const int64_t base = b * kAttrBatch;
        const int nb = (int)min((int64_t)kAttrBatch, n - base);
        // requested before this batch is worked on: the entries of batch b + 2, the F rows of batch b + 1
        int item2 = -1;
        float c2 = 0.0f;
        if (tid < kAttrBatch) load_entry(base + 2 * kAttrBatch + tid, d, item2, c2);
        const bool more = b + 1 < n_batches;                 // block-uniform
        if (more) load_rows(nxt);

        // phase A
        for (int pr = tid; pr < nb * T; pr += kBlock) {
            const int j = pr / T, t = pr - j * T;
            const int it = m_item[cur * kAttrBatch + j];
            float v = 0.0f;
            if (it >= 0 && s_tgt[t] >= 0) v = __fmul_rn(m_c[cur * kAttrBatch + j], attr_dot(Fs + j * es, Es + t * es, groups));
            tile[pr] = v;
            if (a.contrib && base + j < span) a.contrib[(c_lo + base + j) * T + t] = v;
        }
        __syncthreads();                                     // the tile is whole; Fs is consumed

        // phase B, in list order
        if (my_tgt >= 0) {
            for (int j = 0; j < nb; ++j) {
                const int it = m_item[cur * kAttrBatch + j];
                if (it < 0) continue;                        // a skipped entry takes no part (the same for every lane)
                const float v = tile[j * T + tid];
                total = __fadd_rn(total, v);
                if (m > 0) {
                    // only a key above the one in place m - 1 enters the list (an equal key stays behind the earlier
                    // entry: ascending list position among ties); on a long list that is soon a rare event
                    uint32_t k = order_key(v);
                    if (k > thr) {
                        int kp = (int)(base + j), ki = it;
                        float kv = v;
                        bool up = false;
#pragma unroll
                        for (int q = 0; q < kAttrTop; ++q) { // once placed, every later place moves down by one
                            up = up || k > tkey[q];
                            const uint32_t ok_ = tkey[q];
                            const int op = tpos[q], oi = titem[q];
                            const float ov = tval[q];
                            tkey[q] = up ? k : ok_;
                            tpos[q] = up ? kp : op;
                            titem[q] = up ? ki : oi;
                            tval[q] = up ? kv : ov;
                            k = up ? ok_ : k;
                            kp = up ? op : kp;
                            ki = up ? oi : ki;
                            kv = up ? ov : kv;
                        }
#pragma unroll
                        for (int q = 0; q < kAttrTop; ++q) thr = q == m - 1 ? tkey[q] : thr;
                    }
                }
            }
        }
        if (more) store_rows();
        if (tid < kAttrBatch) {
            m_item[nxt2 * kAttrBatch + tid] = item2;
            m_c[nxt2 * kAttrBatch + tid] = c2;
        }
        __syncthreads();                                     // Fs and the entries of batch b + 2 are in place; the tile is consumed
    }

    // base = a0 * dot(z, E[t]); added to the total last (fold-in's "a0 * z term last")
    if (tid < T) {
        const int64_t o = r * T + tid;
        float bs = 0.0f;
        if (my_tgt >= 0 && init_id >= 0) bs = __fmul_rn(a.a0, attr_dot(Es + T * es, Es + tid * es, groups));
        if (my_tgt >= 0) total = __fadd_rn(total, bs);
        if (a.base) a.base[o] = bs;
        if (a.total) a.total[o] = total;
#pragma unroll
        for (int q = 0; q < kAttrTop; ++q) {
            if (q < m) {
                a.top_pos[o * m + q] = tpos[q];
                a.top_item[o * m + q] = titem[q];
                a.top_value[o * m + q] = tval[q];
            }
        }
    }
}

unsigned long long lds_ok_attr[2];

}  // namespace

extern "C" {

int lgc_attribute(const lgc_attr_args *args, void *stream_) {
    if (!args) return LGC_E_INVAL;
    const lgc_attr_args &a = *args;
    if (!lgc_dim_ok(a.dim)) return LGC_E_DIM;
    const bool session = a.list_ptr || a.list_items, graph = a.rowptr || a.entries || a.row_ids;
    if (session == graph) return LGC_E_INVAL;                // exactly one form of the lists
    if (session && (!a.list_ptr || !a.list_items || (a.normalize != 0 && a.normalize != 1) || (a.normalize == 1 && !a.item_dis)))
        return LGC_E_INVAL;
    if (graph && (!a.rowptr || !a.entries || !a.row_ids || a.n_graph_rows < 0)) return LGC_E_INVAL;
    if (!a.fold || !a.items || !a.targets || !a.status || a.n_rows < 0 || a.n_items < 1 || a.n_init_rows < 0 ||
        a.fold_stride < a.dim || a.item_stride < a.dim || (a.init_rows && !a.init) || (a.init_rows && a.init_stride < a.dim))
        return LGC_E_INVAL;
    if (a.n_targets < 1 || a.n_targets > LGC_ATTR_MAX_TARGETS || a.top_m < 0 || a.top_m > LGC_ATTR_MAX_TOP) return LGC_E_RANGE;
    if (a.target_stride < a.n_targets || (a.contrib && !a.contrib_ptr) ||
        (a.top_m > 0 && (!a.top_pos || !a.top_item || !a.top_value)))
        return LGC_E_INVAL;
    if (!a.contrib && !a.base && !a.total && a.top_m == 0) return LGC_E_INVAL;   // no output at all
    if (a.n_rows >= INT32_MAX || a.n_items >= INT32_MAX || (graph && a.n_graph_rows >= INT32_MAX)) return LGC_E_RANGE;
    if (!aligned_to(a.fold, 4) || !aligned_to(a.items, 4) || (a.init_rows && !aligned_to(a.init, 4)) || !aligned_to(a.contrib, 4) ||
        !aligned_to(a.base, 4) || !aligned_to(a.total, 4) || !aligned_to(a.top_value, 4))
        return LGC_E_ALIGN;
    if (a.n_rows == 0) return 0;
    AttrArgs p{};
    p.a = a;
    if (!a.init_rows) { p.a.init = nullptr; p.a.init_stride = 0; p.a.n_init_rows = 0; }
    if (!a.contrib) p.a.contrib_ptr = nullptr;
    if (a.top_m == 0) { p.a.top_pos = nullptr; p.a.top_item = nullptr; p.a.top_value = nullptr; }
    p.groups = (a.dim + 3) / 4;
    p.es = 4 * (p.groups | 1);
    // 16-byte loads where every row starts on a 16-byte boundary; dword loads otherwise (lgc_spmm's rule)
    const bool vec = a.dim % 4 == 0 && aligned_to(a.fold, 16) && a.fold_stride % 4 == 0 && aligned_to(a.items, 16) &&
                     a.item_stride % 4 == 0 && (!a.init_rows || (aligned_to(a.init, 16) && a.init_stride % 4 == 0));
    void (*kern)(const AttrArgs) = vec ? k_attribute<true> : k_attribute<false>;
    const size_t lds = sizeof(float) * ((size_t)(a.n_targets + 1 + kAttrBatch) * p.es + (size_t)kAttrBatch * a.n_targets) +
                       sizeof(int32_t) * (64 + 6 * kAttrBatch + 4);
    const int rc_attr = allow_lds(reinterpret_cast<const void *>(kern), lds, 64 * 1024, 112 * 1024, &lds_ok_attr[vec ? 1 : 0]);
    if (rc_attr != 0) return rc_attr;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.n_rows), dim3(kBlock), lds, as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

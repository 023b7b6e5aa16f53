// lgconv_foldin.hip -- fold-in: the embedding of a node that is not a row of the trained table (a new visitor, or a known
// user whose list changed), from its interaction list and the per-model item table F.
// C ABI: include/lgconv_hip.h
#include "lgconv_common.h"

namespace {

// e = a0 * z + sum_k c_k * F[i_k],  c_k = item_dis[i_k] * w_k * d,  d = (sum_k w_k)^-1/2  (inf -> 0): the row
// `get_embedding` gives a node appended to the trained graph with one-way edges i_k -> node.
//
// One wavefront per request row.  The list is read 64 entries at a time, one entry per lane (coalesced); an entry then
// reaches the lanes that need it through a cross-lane read, so the walk over the list is wave-uniform; the next 64
// entries are requested before the current ones are worked on.  Two passes:
//   1. deg = the fp32 sum of the weights SEQUENTIALLY IN LIST ORDER (lgc_build_csr's degree), entries whose item is out
//      of range left out (their weight enters as +0, which changes no bit of a sum that started at +0);
//   2. c_k per lane -- (item_dis * w) * d left to right, each product rounded, k_build_entries' expression -- and the
//      gathers of F: kInFlight independent row loads are issued, then their products are added in list order.
// Lanes run over columns.  VEC = 4: 16-byte loads, one float4 accumulator per lane, a lane group of 16 / 32 / 64 lanes per
// row; lists of up to 32 entries are summed in list order by every group alike (group 0 stores), longer ones are dealt over
// the 64 / lanes_per_row groups by position and the groups' sums added in group order -- a fixed order, no atomics.
// VEC = 1: dword loads, NACC = ceil(dim / 64) accumulators per lane (columns lane, lane + 64, ...), list order throughout.
// No LDS, no scratch; every store is a plain vector store.
constexpr int kFoldInFlight = 8;
constexpr int kFoldShort = 32;      // lists up to here: list order, the short-row contract of lgc_spmm / lgc_spmm_tiles

struct FoldArgs {
    const int64_t *list_ptr, *list_items;
    const float *list_weight;
    int64_t n_rows;
    const float *item_dis, *fold;
    int64_t fold_stride, n_items;
    const int64_t *init_rows;
    const float *init;
    int64_t init_stride, n_init_rows;
    float a0;
    int32_t normalize, dim, lpr;    // lpr: lanes per row (VEC = 4: 16, 32 or 64; VEC = 1: 64)
    float *out;
    int64_t out_stride;
    int32_t *status;
};

template <int VEC, int NACC>
__global__ __launch_bounds__(kBlock) void k_fold_in(const FoldArgs p) {
    static_assert(VEC == 1 || NACC == 1, "the float4 form holds one accumulator group per lane");
    constexpr int W = VEC * NACC;                            // floats a lane holds per row
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (r >= p.n_rows) return;                               // wave-uniform
    const int64_t lo = p.list_ptr[r], hi = p.list_ptr[r + 1];
    const int64_t n = hi - lo;
    const int g = lane / p.lpr, l = lane - g * p.lpr;
    const int groups = (VEC == 4 && n > kFoldShort) ? kWave / p.lpr : 1;     // wave-uniform
    const int gi = groups > 1 ? g : 0;                       // which share of the list this lane's group sums

    // columns of this lane: VEC = 4 -> [4 l, 4 l + 4); VEC = 1 -> lane + 64 a
    bool live[NACC];
    int col[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        col[a] = VEC == 4 ? 4 * l : lane + kWave * a;
        live[a] = col[a] < p.dim;
    }

    // entry lo + base + lane: its item (-1: past the list's end or out of range) and weight (+0 then)
    auto load_batch = [&](int64_t base, int64_t &item, float &w) {
        const int64_t e = lo + base + lane;
        item = -1;
        w = 0.0f;
        if (e < hi) {
            const int64_t it = p.list_items[e];
            if (it >= 0 && it < p.n_items) {                 // range-checked before any address is formed from it
                item = it;
                w = p.list_weight ? p.list_weight[e] : 1.0f;
            } else {
                atomicOr(p.status, LGC_ST_INDEX_OOB);
            }
        }
    };
    int64_t item0;
    float w0;
    load_batch(0, item0, w0);                                // most requests are one batch: loaded once for both passes

    float d = 1.0f;
    if (p.normalize) {
        float deg = 0.0f, w = w0;
        for (int64_t base = 0; base < n; base += kWave) {
            int64_t item_next = -1;
            float w_next = 0.0f;
            if (base + kWave < n) load_batch(base + kWave, item_next, w_next);   // in flight during this batch's adds
            const int nb = (int)min((int64_t)kWave, n - base);
            for (int i = 0; i < nb; ++i)
                deg = __fadd_rn(deg, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), i)));
            w = w_next;
        }
        d = 1.0f / sqrtf(deg);                               // both steps correctly rounded, as k_build_dis
        if (d == INFINITY) d = 0.0f;
    }

    float acc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = 0.0f;
    int64_t item = item0;
    float w = w0;
    for (int64_t base = 0; base < n; base += kWave) {
        int64_t item_next = -1;
        float w_next = 0.0f;
        if (base + kWave < n) load_batch(base + kWave, item_next, w_next);       // in flight during this batch's gathers
        float c = w;
        if (p.normalize) c = __fmul_rn(__fmul_rn(item >= 0 ? p.item_dis[item] : 0.0f, w), d);
        const int it32 = (int)item;                          // n_items < 2^31
        const int nb = (int)min((int64_t)kWave, n - base);
        for (int t = 0; t < nb; t += kFoldInFlight * groups) {
            float x[kFoldInFlight][W], cq[kFoldInFlight];
            bool ok[kFoldInFlight];
#pragma unroll
            for (int q = 0; q < kFoldInFlight; ++q) {        // the loads first ...
                const int idx = t + q * groups + gi;
                const int src = min(idx, kWave - 1);
                const int it = __shfl(it32, src);
                cq[q] = __shfl(c, src);
                ok[q] = idx < nb && it >= 0;
                const float *row = p.fold + (int64_t)(ok[q] ? it : 0) * p.fold_stride;
#pragma unroll
                for (int a = 0; a < NACC; ++a) {
                    if constexpr (VEC == 4) {
                        f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (live[a]) v = *reinterpret_cast<const f4 *>(row + col[a]);
                        x[q][0] = v.x; x[q][1] = v.y; x[q][2] = v.z; x[q][3] = v.w;
                    } else {
                        x[q][a] = live[a] ? row[col[a]] : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < kFoldInFlight; ++q) {        // ... then the adds, in list order
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float s = __fadd_rn(acc[i], __fmul_rn(cq[q], x[q][i]));
                    acc[i] = ok[q] ? s : acc[i];             // a skipped entry adds nothing (not 0 * F: F may hold inf)
                }
            }
        }
        item = item_next;
        w = w_next;
    }
    if (groups > 1) {                                        // the groups' sums in group order, into group 0
        float part[W];
#pragma unroll
        for (int i = 0; i < W; ++i) part[i] = acc[i];
        for (int q = 1; q < groups; ++q) {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[i] = __fadd_rn(acc[i], __shfl(part[i], l + q * p.lpr));
        }
    }

    // the a0 * z term last; an id that is neither a row nor -1 is flagged and adds nothing
    const int64_t id = p.init_rows ? p.init_rows[r] : -1;
    const bool has_init = id >= 0 && id < p.n_init_rows;
    if (id != -1 && !has_init && lane == 0) atomicOr(p.status, LGC_ST_INDEX_OOB);
    if (g != 0) return;
    float *orow = p.out + r * p.out_stride;
    const float *zrow = p.init + (has_init ? id : 0) * p.init_stride;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        if (!live[a]) continue;
        if constexpr (VEC == 4) {
            if (has_init) {
                const f4 z = *reinterpret_cast<const f4 *>(zrow + col[a]);
                acc[0] = __fadd_rn(acc[0], __fmul_rn(p.a0, z.x));
                acc[1] = __fadd_rn(acc[1], __fmul_rn(p.a0, z.y));
                acc[2] = __fadd_rn(acc[2], __fmul_rn(p.a0, z.z));
                acc[3] = __fadd_rn(acc[3], __fmul_rn(p.a0, z.w));
            }
            const f4 o = {acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f4 *>(orow + col[a]) = o;
        } else {
            if (has_init) acc[a] = __fadd_rn(acc[a], __fmul_rn(p.a0, zrow[col[a]]));
            orow[col[a]] = acc[a];
        }
    }
}

}  // namespace

extern "C" {

int lgc_fold_in(const int64_t *list_ptr, const int64_t *list_items, const float *list_weight, int64_t n_rows,
                const float *item_dis, const float *fold, int64_t fold_stride, int64_t n_items, const int64_t *init_rows,
                const float *init, int64_t init_stride, int64_t n_init_rows, float a0, int32_t normalize, int32_t dim,
                float *out, int64_t out_stride, int32_t *status, void *stream_) {
    if (!lgc_dim_ok(dim)) return LGC_E_DIM;
    if (!list_ptr || !list_items || !fold || !out || !status || n_rows < 0 || n_items < 1 || n_init_rows < 0 ||
        fold_stride < dim || out_stride < dim || (normalize != 0 && normalize != 1) || (normalize == 1 && !item_dis) ||
        (init_rows && !init) || (init_rows && init_stride < dim))
        return LGC_E_INVAL;
    if (n_rows >= INT32_MAX || n_items >= INT32_MAX) return LGC_E_RANGE;
    if (!aligned_to(fold, 4) || !aligned_to(out, 4) || (init_rows && !aligned_to(init, 4))) return LGC_E_ALIGN;
    if (n_rows == 0) return 0;
    FoldArgs p{};
    p.list_ptr = list_ptr; p.list_items = list_items; p.list_weight = list_weight; p.n_rows = n_rows;
    p.item_dis = item_dis; p.fold = fold; p.fold_stride = fold_stride; p.n_items = n_items;
    p.init_rows = init_rows; p.init = init_rows ? init : nullptr; p.init_stride = init_rows ? init_stride : 0;
    p.n_init_rows = init_rows ? n_init_rows : 0;
    p.a0 = a0; p.normalize = normalize; p.dim = dim; p.out = out; p.out_stride = out_stride; p.status = status;
    // 16-byte loads where every row starts on a 16-byte boundary; dword loads otherwise (lgc_spmm's rule)
    const bool vec = dim % 4 == 0 && aligned_to(fold, 16) && fold_stride % 4 == 0 && aligned_to(out, 16) &&
                     out_stride % 4 == 0 && (!init_rows || (aligned_to(init, 16) && init_stride % 4 == 0));
    p.lpr = !vec ? kWave : dim <= 64 ? 16 : dim <= 128 ? 32 : 64;
    void (*kern)(const FoldArgs) = k_fold_in<4, 1>;
    if (!vec) {
        const int nacc = (dim + kWave - 1) / kWave;
        kern = nacc == 1 ? k_fold_in<1, 1> : nacc == 2 ? k_fold_in<1, 2> : nacc == 3 ? k_fold_in<1, 3> : k_fold_in<1, 4>;
    }
    hipLaunchKernelGGL(kern, dim3(ceil_div(n_rows, kBlock / kWave)), dim3(kBlock), 0, as_stream(stream_), p);
    return (int)hipGetLastError();
}

}  // extern "C"

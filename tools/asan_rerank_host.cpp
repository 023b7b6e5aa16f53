// The argument checks of lgc_rerank_route, lgc_rerank_mmr and lgc_list_diversity (include/lgconv_hip.h) as a stand-alone
// host program, for tools/asan_rerank_host.sh: every call below must return its code before anything is launched, so the
// device pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "lgconv_hip.h"

static int failures = 0;

static void expect(const char *what, long long got, long long want) {
    if (got != want) {
        std::fprintf(stderr, "%s: returned %lld, expected %lld\n", what, got, want);
        ++failures;
    }
}

// addresses of host words: valid, 16-byte aligned, and never read or written by a call that returns before its launch
alignas(16) static int64_t i64[4];
alignas(16) static float f32[4];
alignas(16) static int32_t i32[4];
alignas(16) static double f64[4];

template <typename T>
static T *off_by(T *p, int bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + bytes); }

struct Mmr {
    const float *items = f32;
    int64_t item_stride = 64, n_items = 300;
    int32_t dim = 64;
    const float *scale = f32;
    const int64_t *cand = i64;
    int64_t cand_stride = 256;
    const float *rel = f32;
    int64_t rel_stride = 256, n_rows = 4;
    int32_t n_cand = 100, k = 20;
    float lambda = 0.7f;
    int64_t *out_index = i64;
    int32_t *out_pos = i32;
    float *out_value = f32;
    int32_t *status = i32;
    int run() const {
        return lgc_rerank_mmr(items, item_stride, n_items, dim, scale, cand, cand_stride, rel, rel_stride, n_rows, n_cand, k,
                              lambda, out_index, out_pos, out_value, status, nullptr);
    }
};

static const int32_t cuts_ok[3] = {5, 10, 20};

struct Div {
    const float *items = f32;
    int64_t item_stride = 64, n_items = 300;
    int32_t dim = 64;
    const float *scale = f32;
    const int64_t *lists = i64;
    int64_t list_stride = 256, n_rows = 4;
    int32_t k = 20;
    const int32_t *cutoffs = cuts_ok;
    int32_t n_cutoffs = 3;
    double *out = f64;
    int64_t out_stride = 8;
    int32_t *status = i32;
    int run() const {
        return lgc_list_diversity(items, item_stride, n_items, dim, scale, lists, list_stride, n_rows, k, cutoffs, n_cutoffs, out,
                                  out_stride, status, nullptr);
    }
};

int main() {
    // lgc_rerank_route
    expect("route staged", lgc_rerank_route(100, 64), LGC_RERANK_ROUTE_LDS);
    expect("route staged, D = 90", lgc_rerank_route(100, 90), LGC_RERANK_ROUTE_LDS);
    expect("route edge", lgc_rerank_route(135, 64), LGC_RERANK_ROUTE_LDS);
    expect("route past the edge", lgc_rerank_route(136, 64), LGC_RERANK_ROUTE_GLOBAL);
    expect("route widest", lgc_rerank_route(256, 256), LGC_RERANK_ROUTE_GLOBAL);
    expect("route no candidates", lgc_rerank_route(0, 64), LGC_E_RANGE);
    expect("route 257 candidates", lgc_rerank_route(257, 64), LGC_E_RANGE);
    expect("route dim 0", lgc_rerank_route(100, 0), LGC_E_DIM);

    // lgc_rerank_mmr
    Mmr c;
    { Mmr b = c; b.items = nullptr; expect("null items", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.cand = nullptr; expect("null cand", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.rel = nullptr; expect("null rel", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.out_index = nullptr; expect("null out_index", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.n_rows = -1; expect("negative n_rows", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.item_stride = 63; expect("short item stride", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.cand_stride = 99; expect("short cand stride", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.rel_stride = 99; expect("short rel stride", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.lambda = NAN; expect("lambda NaN", b.run(), LGC_E_INVAL); }
    { Mmr b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Mmr b = c; b.dim = 257; b.item_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Mmr b = c; b.n_cand = 0; expect("n_cand 0", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.n_cand = LGC_RERANK_MAX_CAND + 1; expect("n_cand 257", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.k = 0; expect("k 0", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.k = 101; expect("k above n_cand", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.lambda = -0.5f; expect("lambda below 0", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.lambda = 1.5f; expect("lambda above 1", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.lambda = INFINITY; expect("lambda inf", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.n_items = (int64_t)1 << 31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.n_rows = (int64_t)1 << 31; expect("2^31 rows", b.run(), LGC_E_RANGE); }
    { Mmr b = c; b.items = off_by(f32, 2); expect("misaligned items", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.scale = off_by(f32, 2); expect("misaligned scale", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.rel = off_by(f32, 2); expect("misaligned rel", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.out_value = off_by(f32, 2); expect("misaligned out_value", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.out_pos = off_by(i32, 2); expect("misaligned out_pos", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.cand = off_by(i64, 4); expect("misaligned cand", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.out_index = off_by(i64, 4); expect("misaligned out_index", b.run(), LGC_E_ALIGN); }
    { Mmr b = c; b.n_rows = 0; expect("no rows", b.run(), 0); }
    { Mmr b = c; b.n_rows = 0; b.scale = nullptr; b.out_pos = nullptr; b.out_value = nullptr; expect("no rows, no options", b.run(), 0); }
    { Mmr b = c; b.n_rows = 0; b.n_cand = 256; b.k = 256; b.dim = 256; b.item_stride = 259; b.lambda = 1.0f; expect("no rows, limits", b.run(), 0); }
    { Mmr b = c; b.n_rows = 0; b.n_cand = 1; b.k = 1; b.cand_stride = 1; b.rel_stride = 1; b.lambda = 0.0f; expect("no rows, smallest", b.run(), 0); }
    { Mmr b = c; b.n_rows = 0; b.item_stride = 63; expect("no rows, still validated", b.run(), LGC_E_INVAL); }

    // lgc_list_diversity
    Div d;
    static const int32_t not_ascending[2] = {10, 5}, twice[2] = {5, 5}, zero[2] = {0, 5}, past_k[2] = {5, 21}, nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    static const int32_t eight[8] = {1, 2, 3, 4, 5, 6, 7, 8}, widest[3] = {1, 2, 256};
    { Div b = d; b.items = nullptr; expect("diversity null items", b.run(), LGC_E_INVAL); }
    { Div b = d; b.lists = nullptr; expect("diversity null lists", b.run(), LGC_E_INVAL); }
    { Div b = d; b.cutoffs = nullptr; expect("diversity null cutoffs", b.run(), LGC_E_INVAL); }
    { Div b = d; b.out = nullptr; expect("diversity null out", b.run(), LGC_E_INVAL); }
    { Div b = d; b.status = nullptr; expect("diversity null status", b.run(), LGC_E_INVAL); }
    { Div b = d; b.n_rows = -1; expect("diversity negative n_rows", b.run(), LGC_E_INVAL); }
    { Div b = d; b.item_stride = 63; expect("diversity short item stride", b.run(), LGC_E_INVAL); }
    { Div b = d; b.list_stride = 19; expect("diversity short list stride", b.run(), LGC_E_INVAL); }
    { Div b = d; b.out_stride = 2; expect("diversity short out stride", b.run(), LGC_E_INVAL); }
    { Div b = d; b.n_cutoffs = 0; expect("diversity no cutoffs", b.run(), LGC_E_INVAL); }
    { Div b = d; b.dim = 0; expect("diversity dim 0", b.run(), LGC_E_DIM); }
    { Div b = d; b.k = 0; expect("diversity k 0", b.run(), LGC_E_RANGE); }
    { Div b = d; b.k = 257; b.list_stride = 300; expect("diversity k 257", b.run(), LGC_E_RANGE); }
    { Div b = d; b.n_items = 0; expect("diversity no items", b.run(), LGC_E_RANGE); }
    { Div b = d; b.n_items = (int64_t)1 << 31; expect("diversity 2^31 items", b.run(), LGC_E_RANGE); }
    { Div b = d; b.n_rows = (int64_t)1 << 31; expect("diversity 2^31 rows", b.run(), LGC_E_RANGE); }
    { Div b = d; b.cutoffs = not_ascending; b.n_cutoffs = 2; expect("cutoffs descending", b.run(), LGC_E_RANGE); }
    { Div b = d; b.cutoffs = twice; b.n_cutoffs = 2; expect("cutoffs repeated", b.run(), LGC_E_RANGE); }
    { Div b = d; b.cutoffs = zero; b.n_cutoffs = 2; expect("cutoff 0", b.run(), LGC_E_RANGE); }
    { Div b = d; b.cutoffs = past_k; b.n_cutoffs = 2; expect("cutoff past k", b.run(), LGC_E_RANGE); }
    { Div b = d; b.cutoffs = nine; b.n_cutoffs = 9; b.out_stride = 9; expect("nine cutoffs", b.run(), LGC_E_RANGE); }
    { Div b = d; b.items = off_by(f32, 2); expect("diversity misaligned items", b.run(), LGC_E_ALIGN); }
    { Div b = d; b.scale = off_by(f32, 2); expect("diversity misaligned scale", b.run(), LGC_E_ALIGN); }
    { Div b = d; b.lists = off_by(i64, 4); expect("diversity misaligned lists", b.run(), LGC_E_ALIGN); }
    { Div b = d; b.out = off_by(f64, 4); expect("diversity misaligned out", b.run(), LGC_E_ALIGN); }
    { Div b = d; b.n_rows = 0; expect("diversity no rows", b.run(), 0); }
    { Div b = d; b.n_rows = 0; b.scale = nullptr; b.cutoffs = eight; b.n_cutoffs = 8; expect("diversity no rows, eight cutoffs", b.run(), 0); }
    { Div b = d; b.n_rows = 0; b.k = 256; b.cutoffs = widest; b.dim = 256; b.item_stride = 259; expect("diversity no rows, limits", b.run(), 0); }
    { Div b = d; b.n_rows = 0; b.cutoffs = past_k; b.n_cutoffs = 2; expect("diversity no rows, still validated", b.run(), LGC_E_RANGE); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_rerank_host: every argument check returned its code before any launch");
    return 0;
}

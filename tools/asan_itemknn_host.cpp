// The argument checks of lgc_knn_workspace_bytes and lgc_knn_recommend (include/lgconv_hip.h) as a stand-alone host
// program, for tools/asan_itemknn_host.sh: every call below must return its code before anything is launched, so the device
// pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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
alignas(16) static int32_t cnt[4];
alignas(16) static uint8_t u8[16];

template <typename T>
static T *off_by(T *p, int bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + bytes); }

struct Call {
    const int64_t *nbr_index = i64;
    const float *nbr_value = f32;
    int64_t nbr_stride = 64, n_items = 300;
    int32_t kn = 64;
    const int64_t *list_ptr = i64, *list_items = i64;
    const float *list_weight = f32;
    int64_t n_lists = 50;
    const int64_t *list_rows = i64;
    int64_t n_queries = 4;
    const uint8_t *item_ok = u8;
    int32_t exclude_basket = 1, min_votes = 1, k = 20, band = 0;
    int64_t *out_index = i64;
    float *out_value = f32;
    int32_t *out_votes = cnt;
    void *workspace = i64;
    size_t workspace_bytes = (size_t)1 << 40;
    int32_t *status = i32;
    int run() const {
        return lgc_knn_recommend(nbr_index, nbr_value, nbr_stride, n_items, kn, list_ptr, list_items, list_weight, n_lists,
                                 list_rows, n_queries, item_ok, exclude_basket, min_votes, k, band, out_index, out_value, out_votes,
                                 workspace, workspace_bytes, status, nullptr);
    }
};

static long long size(int64_t n_queries, int64_t n_items, int32_t k, int32_t band) {
    return (long long)lgc_knn_workspace_bytes(n_queries, n_items, k, band, nullptr);
}

int main() {
    // the workspace size: what the call refuses is 0
    expect("size refuses k 0", size(4, 300, 0, 64), 0);
    expect("size refuses k 65", size(4, 300, 65, 64), 0);
    expect("size refuses band 63", size(4, 300, 20, 63), 0);
    expect("size refuses band -64", size(4, 300, 20, -64), 0);
    expect("size refuses a band past the LDS budget", size(4, 300, 20, LGC_KNN_MAX_BAND + 64), 0);
    expect("size refuses no items", size(4, 0, 20, 64), 0);
    expect("size refuses 2^31 items", size(4, (int64_t)1 << 31, 20, 0), 0);
    expect("size refuses negative queries", size(-1, 300, 20, 64), 0);
    expect("size refuses more than 2^20 bands", size(4, ((int64_t)1 << 26) + 1, 20, 64), 0);
    expect("size of 5 bands", size(4, 300, 20, 64), 4 * 5 * 20 * 12);
    expect("size of one band", size(4, 300, 20, 320), 0);
    expect("size, band chosen", size(4, 54571, 20, 0), 4 * 7 * 20 * 12);
    expect("size of 2^20 bands", size(4, (int64_t)1 << 26, 20, 64), 4LL * (1 << 20) * 20 * 12);
    expect("size at the limits", size(INT32_MAX - 1, (int64_t)1 << 26, 64, 64), (long long)(INT32_MAX - 1) * (1 << 20) * 64 * 12);
    expect("size, band chosen, at the limits", size(INT32_MAX - 1, INT32_MAX - 1, 64, 0), (long long)(INT32_MAX - 1) * 262144 * 64 * 12);
    // ... and it grows with each of its three sizes, at every band
    const int64_t queries[] = {0, 1, 63, 64, 65, 1000, 54571, 1000000, INT32_MAX - 1};
    const int64_t items[] = {1, 64, 65, 128, 129, 200, 1000, 8192, 8193, 16384, 16385, 54571, 1640000, (int64_t)1 << 26};
    const int32_t ks[] = {1, 5, 20, 64};
    const int32_t bands[] = {0, 64, 128, 192, 256, 8192, LGC_KNN_MAX_BAND};
    for (int32_t band : bands)
        for (size_t a = 0; a < sizeof(queries) / sizeof(*queries); ++a)
            for (size_t b = 0; b < sizeof(items) / sizeof(*items); ++b)
                for (size_t c = 0; c < sizeof(ks) / sizeof(*ks); ++c) {
                    const long long here = size(queries[a], items[b], ks[c], band);
                    if (a > 0) expect("size grows with n_queries", size(queries[a - 1], items[b], ks[c], band) <= here, 1);
                    if (b > 0) expect("size grows with n_items", size(queries[a], items[b - 1], ks[c], band) <= here, 1);
                    if (c > 0) expect("size grows with k", size(queries[a], items[b], ks[c - 1], band) <= here, 1);
                }

    // lgc_knn_recommend
    Call c;
    { Call b = c; b.nbr_index = nullptr; expect("null nbr_index", b.run(), LGC_E_INVAL); }
    { Call b = c; b.nbr_value = nullptr; expect("null nbr_value", b.run(), LGC_E_INVAL); }
    { Call b = c; b.list_ptr = nullptr; expect("null list_ptr", b.run(), LGC_E_INVAL); }
    { Call b = c; b.list_items = nullptr; expect("null list_items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.out_index = nullptr; expect("null out_index", b.run(), LGC_E_INVAL); }
    { Call b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_queries = -1; expect("negative n_queries", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_lists = -1; expect("negative n_lists", b.run(), LGC_E_INVAL); }
    { Call b = c; b.nbr_stride = 63; expect("a stride below kn", b.run(), LGC_E_INVAL); }
    { Call b = c; b.nbr_stride = INT64_MIN; b.kn = 1; expect("stride -2^63", b.run(), LGC_E_INVAL); }
    { Call b = c; b.k = 0; expect("k 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.k = LGC_KNN_MAX_K + 1; expect("k 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.kn = 0; expect("kn 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.kn = INT32_MIN; expect("kn -2^31", b.run(), LGC_E_RANGE); }
    { Call b = c; b.kn = LGC_KNN_MAX_NEIGHBORS + 1; b.nbr_stride = 65; expect("kn 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = 32; expect("band 32", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = 100; expect("band 100", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = -64; expect("band -64", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = LGC_KNN_MAX_BAND + 64; expect("band past the LDS budget", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = INT32_MAX; expect("band 2^31 - 1", b.run(), LGC_E_RANGE); }
    { Call b = c; b.min_votes = 0; expect("min_votes 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.min_votes = INT32_MIN; expect("min_votes -2^31", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = (int64_t)1 << 31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = INT64_MAX; expect("2^63 - 1 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = ((int64_t)1 << 26) + 1; b.band = 64; expect("more than 2^20 bands", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_lists = INT32_MAX; expect("2^31 - 1 lists", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT32_MAX; expect("2^31 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT64_MAX; expect("2^63 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.list_rows = nullptr; b.n_queries = 51; expect("more queries than lists without list_rows", b.run(), LGC_E_RANGE); }
    { Call b = c; b.nbr_index = off_by(i64, 4); expect("misaligned nbr_index", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.nbr_value = off_by(f32, 2); expect("misaligned nbr_value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_ptr = off_by(i64, 4); expect("misaligned list_ptr", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_items = off_by(i64, 4); expect("misaligned list_items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_weight = off_by(f32, 2); expect("misaligned list_weight", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_rows = off_by(i64, 4); expect("misaligned list_rows", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_index = off_by(i64, 4); expect("misaligned out_index", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_value = off_by(f32, 2); expect("misaligned out_value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_votes = off_by(cnt, 2); expect("misaligned out_votes", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.status = off_by(i32, 2); expect("misaligned status", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace = off_by(i64, 4); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.band = 64; b.workspace_bytes = 4 * 5 * 20 * 12 - 1; expect("workspace one byte short", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.band = 64; b.workspace = nullptr; expect("workspace missing", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_items = 54571; b.workspace_bytes = 0; expect("workspace missing, band chosen", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_queries = 0; expect("no queries", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.list_weight = nullptr; b.list_rows = nullptr; b.item_ok = nullptr; b.out_value = nullptr;
      b.out_votes = nullptr; b.workspace = nullptr; b.workspace_bytes = 0; expect("no queries, no options", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.k = 64; b.kn = 1; b.nbr_stride = 1; b.band = LGC_KNN_MAX_BAND; b.min_votes = INT32_MAX;
      b.n_lists = 0; b.list_rows = nullptr; b.n_items = 1; b.exclude_basket = 0; expect("no queries, limits", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.nbr_stride = 63; expect("no queries, still validated", b.run(), LGC_E_INVAL); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_itemknn_host: every argument check returned its code before any launch");
    return 0;
}

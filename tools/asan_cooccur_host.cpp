// The argument checks of lgc_cooccur_workspace_bytes and lgc_cooccur_topk (include/lgconv_hip.h) as a stand-alone host
// program, for tools/asan_cooccur_host.sh: every call below must return its code before anything is launched, so the device
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
    const int64_t *buyer_ptr = i64, *buyer_users = i64;
    int64_t n_items = 300;
    const int64_t *seen_ptr = i64, *seen_items = i64;
    int64_t n_users = 50;
    const int64_t *query_ids = i64;
    int64_t n_queries = 4;
    const uint8_t *item_ok = u8;
    int32_t min_count = 1, measure = LGC_COOCCUR_COSINE, k = 20, band = 0;
    int64_t *out_index = i64;
    float *out_value = f32;
    int32_t *out_count = cnt;
    void *workspace = i64;
    size_t workspace_bytes = (size_t)1 << 40;
    int32_t *status = i32;
    int run() const {
        return lgc_cooccur_topk(buyer_ptr, buyer_users, n_items, seen_ptr, seen_items, n_users, query_ids, n_queries, item_ok,
                                min_count, measure, k, band, out_index, out_value, out_count, workspace, workspace_bytes, status,
                                nullptr);
    }
};

int main() {
    // the workspace size
    expect("size refuses k 0", (long long)lgc_cooccur_workspace_bytes(4, 300, 0, 64, nullptr), 0);
    expect("size refuses k 65", (long long)lgc_cooccur_workspace_bytes(4, 300, 65, 64, nullptr), 0);
    expect("size refuses band 63", (long long)lgc_cooccur_workspace_bytes(4, 300, 20, 63, nullptr), 0);
    expect("size refuses band -64", (long long)lgc_cooccur_workspace_bytes(4, 300, 20, -64, nullptr), 0);
    expect("size refuses a band past the LDS budget", (long long)lgc_cooccur_workspace_bytes(4, 300, 20, LGC_COOCCUR_MAX_BAND + 64, nullptr), 0);
    expect("size refuses no items", (long long)lgc_cooccur_workspace_bytes(4, 0, 20, 64, nullptr), 0);
    expect("size refuses 2^31 items", (long long)lgc_cooccur_workspace_bytes(4, (int64_t)1 << 31, 20, 0, nullptr), 0);
    expect("size refuses negative queries", (long long)lgc_cooccur_workspace_bytes(-1, 300, 20, 64, nullptr), 0);
    expect("size refuses more than 2^20 bands", (long long)lgc_cooccur_workspace_bytes(4, ((int64_t)1 << 26) + 1, 20, 64, nullptr), 0);
    expect("size of 5 bands", (long long)lgc_cooccur_workspace_bytes(4, 300, 20, 64, nullptr), 4 * 5 * 20 * 8);
    expect("size of one band", (long long)lgc_cooccur_workspace_bytes(4, 300, 20, 320, nullptr), 0);
    expect("size, band chosen", (long long)lgc_cooccur_workspace_bytes(4, 54571, 20, 0, nullptr), 4 * 4 * 20 * 8);
    expect("size of 2^20 bands", (long long)lgc_cooccur_workspace_bytes(4, (int64_t)1 << 26, 20, 64, nullptr), 4LL * (1 << 20) * 20 * 8);
    expect("size at the limits", (long long)lgc_cooccur_workspace_bytes(INT32_MAX - 1, (int64_t)1 << 26, 64, 64, nullptr),
           (long long)(INT32_MAX - 1) * (1 << 20) * 64 * 8);
    expect("size, band chosen, at the limits", (long long)lgc_cooccur_workspace_bytes(INT32_MAX - 1, INT32_MAX - 1, 64, 0, nullptr),
           (long long)(INT32_MAX - 1) * 131072 * 64 * 8);

    // lgc_cooccur_topk
    Call c;
    { Call b = c; b.buyer_ptr = nullptr; expect("null buyer_ptr", b.run(), LGC_E_INVAL); }
    { Call b = c; b.buyer_users = nullptr; expect("null buyer_users", b.run(), LGC_E_INVAL); }
    { Call b = c; b.seen_ptr = nullptr; expect("null seen_ptr", b.run(), LGC_E_INVAL); }
    { Call b = c; b.seen_items = nullptr; expect("null seen_items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.out_index = nullptr; expect("null out_index", b.run(), LGC_E_INVAL); }
    { Call b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_queries = -1; expect("negative n_queries", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_users = -1; expect("negative n_users", b.run(), LGC_E_INVAL); }
    { Call b = c; b.measure = -1; expect("measure -1", b.run(), LGC_E_INVAL); }
    { Call b = c; b.measure = 3; expect("measure 3", b.run(), LGC_E_INVAL); }
    { Call b = c; b.k = 0; expect("k 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.k = LGC_COOCCUR_MAX_K + 1; expect("k 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = 32; expect("band 32", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = 100; expect("band 100", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = -64; expect("band -64", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = LGC_COOCCUR_MAX_BAND + 64; expect("band past the LDS budget", b.run(), LGC_E_RANGE); }
    { Call b = c; b.band = INT32_MAX; expect("band 2^31 - 1", b.run(), LGC_E_RANGE); }
    { Call b = c; b.min_count = 0; expect("min_count 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.min_count = INT32_MIN; expect("min_count -2^31", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = (int64_t)1 << 31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = INT64_MAX; expect("2^63 - 1 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = ((int64_t)1 << 26) + 1; b.band = 64; expect("more than 2^20 bands", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_users = INT32_MAX; expect("2^31 - 1 users", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT32_MAX; expect("2^31 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT64_MAX; expect("2^63 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.buyer_ptr = off_by(i64, 4); expect("misaligned buyer_ptr", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.buyer_users = off_by(i64, 4); expect("misaligned buyer_users", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.seen_ptr = off_by(i64, 4); expect("misaligned seen_ptr", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.seen_items = off_by(i64, 4); expect("misaligned seen_items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.query_ids = off_by(i64, 4); expect("misaligned query_ids", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_index = off_by(i64, 4); expect("misaligned out_index", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_value = off_by(f32, 2); expect("misaligned out_value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_count = off_by(cnt, 2); expect("misaligned out_count", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.status = off_by(i32, 2); expect("misaligned status", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace = off_by(i64, 4); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.band = 64; b.workspace_bytes = 4 * 5 * 20 * 8 - 1; expect("workspace one byte short", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.band = 64; b.workspace = nullptr; expect("workspace missing", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_items = 54571; b.workspace_bytes = 0; expect("workspace missing, band chosen", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_queries = 0; expect("no queries", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.query_ids = nullptr; b.item_ok = nullptr; b.out_value = nullptr; b.out_count = nullptr;
      b.workspace = nullptr; b.workspace_bytes = 0; expect("no queries, no options", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.k = 64; b.band = LGC_COOCCUR_MAX_BAND; b.min_count = INT32_MAX; b.n_users = 0; b.n_items = 1;
      b.measure = LGC_COOCCUR_JACCARD; expect("no queries, limits", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.measure = 3; expect("no queries, still validated", b.run(), LGC_E_INVAL); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_cooccur_host: every argument check returned its code before any launch");
    return 0;
}

// The argument checks of lgc_row_rnorm, lgc_item_neighbors_workspace_bytes and lgc_item_neighbors (include/lgconv_hip.h) as
// a stand-alone host program, for tools/asan_similar_host.sh: every call below must return its code before anything is
// launched, so the device pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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
alignas(16) static uint8_t u8[16];

template <typename T>
static T *off_by(T *p, int bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + bytes); }

struct Call {
    const float *items = f32;
    int64_t item_stride = 64, n_items = 300;
    int32_t dim = 64;
    const int64_t *query_ids = i64;
    int64_t n_queries = 4;
    const float *scale = f32;
    const uint8_t *item_ok = u8;
    int32_t exclude_self = 1, k = 20, slices = 0;
    int64_t *out_index = i64;
    float *out_value = f32;
    void *workspace = i64;
    size_t workspace_bytes = (size_t)1 << 40;
    int32_t *status = i32;
    int run() const {
        return lgc_item_neighbors(items, item_stride, n_items, dim, query_ids, n_queries, scale, item_ok, exclude_self, k, slices,
                                  out_index, out_value, workspace, workspace_bytes, status, nullptr);
    }
};

int main() {
    // lgc_row_rnorm
    expect("rnorm null table", lgc_row_rnorm(nullptr, 64, 10, 64, f32, nullptr), LGC_E_INVAL);
    expect("rnorm null out", lgc_row_rnorm(f32, 64, 10, 64, nullptr, nullptr), LGC_E_INVAL);
    expect("rnorm negative rows", lgc_row_rnorm(f32, 64, -1, 64, f32, nullptr), LGC_E_INVAL);
    expect("rnorm short stride", lgc_row_rnorm(f32, 63, 10, 64, f32, nullptr), LGC_E_INVAL);
    expect("rnorm dim 0", lgc_row_rnorm(f32, 64, 10, 0, f32, nullptr), LGC_E_DIM);
    expect("rnorm dim 257", lgc_row_rnorm(f32, 300, 10, 257, f32, nullptr), LGC_E_DIM);
    expect("rnorm 2^31 rows", lgc_row_rnorm(f32, 64, (int64_t)1 << 31, 64, f32, nullptr), LGC_E_RANGE);
    expect("rnorm 2^31 - 1 rows", lgc_row_rnorm(f32, 64, INT32_MAX, 64, f32, nullptr), LGC_E_RANGE);
    expect("rnorm misaligned table", lgc_row_rnorm(off_by(f32, 2), 64, 10, 64, f32, nullptr), LGC_E_ALIGN);
    expect("rnorm misaligned out", lgc_row_rnorm(f32, 64, 10, 64, off_by(f32, 2), nullptr), LGC_E_ALIGN);
    expect("rnorm no rows", lgc_row_rnorm(f32, 64, 0, 64, f32, nullptr), 0);
    expect("rnorm no rows, widest", lgc_row_rnorm(f32, 259, 0, 256, f32, nullptr), 0);

    // the workspace size
    expect("size refuses k 0", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 0, 2), 0);
    expect("size refuses k 65", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 65, 2), 0);
    expect("size refuses slices 65", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 20, 65), 0);
    expect("size refuses slices -1", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 20, -1), 0);
    expect("size refuses no items", (long long)lgc_item_neighbors_workspace_bytes(4, 0, 20, 2), 0);
    expect("size refuses 2^31 items", (long long)lgc_item_neighbors_workspace_bytes(4, (int64_t)1 << 31, 20, 2), 0);
    expect("size refuses negative queries", (long long)lgc_item_neighbors_workspace_bytes(-1, 300, 20, 2), 0);
    expect("size of 2 ranges", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 20, 2), 4 * 2 * 20 * 8);
    expect("size of one range", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 20, 1), 0);
    expect("size clamps to the item tiles", (long long)lgc_item_neighbors_workspace_bytes(4, 300, 20, 64), 4 * 3 * 20 * 8);
    expect("size at the limits", (long long)lgc_item_neighbors_workspace_bytes(INT32_MAX - 1, INT32_MAX - 1, 64, 64),
           (long long)(INT32_MAX - 1) * 64 * 64 * 8);

    // lgc_item_neighbors
    Call c;
    { Call b = c; b.items = nullptr; expect("null items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.out_index = nullptr; expect("null out_index", b.run(), LGC_E_INVAL); }
    { Call b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_queries = -1; expect("negative n_queries", b.run(), LGC_E_INVAL); }
    { Call b = c; b.item_stride = 63; expect("short stride", b.run(), LGC_E_INVAL); }
    { Call b = c; b.exclude_self = 2; expect("exclude_self 2", b.run(), LGC_E_INVAL); }
    { Call b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Call b = c; b.dim = 257; b.item_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Call b = c; b.k = 0; expect("k 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.k = LGC_NEIGHBORS_MAX_K + 1; expect("k 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.slices = -1; expect("slices -1", b.run(), LGC_E_RANGE); }
    { Call b = c; b.slices = 65; expect("slices 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = (int64_t)1 << 31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT32_MAX; expect("2^31 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.items = off_by(f32, 2); expect("misaligned items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.scale = off_by(f32, 2); expect("misaligned scale", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_value = off_by(f32, 2); expect("misaligned out_value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_index = off_by(i64, 4); expect("misaligned out_index", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace = off_by(i64, 4); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.slices = 2; b.workspace_bytes = 4 * 2 * 20 * 8 - 1; expect("workspace one byte short", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.slices = 2; b.workspace = nullptr; expect("workspace missing", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.workspace_bytes = 0; expect("workspace missing, ranges chosen", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_queries = 0; expect("no queries", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.query_ids = nullptr; b.scale = nullptr; b.item_ok = nullptr; b.out_value = nullptr;
      b.exclude_self = 0; b.workspace = nullptr; b.workspace_bytes = 0; b.slices = 1; expect("no queries, no options", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.k = 64; b.slices = 64; b.dim = 256; b.item_stride = 259; expect("no queries, limits", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.item_stride = 63; expect("no queries, still validated", b.run(), LGC_E_INVAL); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_similar_host: every argument check returned its code before any launch");
    return 0;
}

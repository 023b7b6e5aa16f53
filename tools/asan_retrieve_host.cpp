// The argument checks of lgc_retrieve_workspace_bytes and lgc_retrieve_topk (include/lgconv_hip.h) as a stand-alone host
// program, for tools/asan_retrieve_host.sh: every call below must return its code before anything is launched, so the device
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
alignas(16) static uint8_t u8[16];

template <typename T>
static T *off_by(T *p, int bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + bytes); }

struct Call {
    const float *queries = f32;
    int64_t query_stride = 64, n_query_rows = 50;
    const float *cands = f32;
    int64_t cand_stride = 64, n_cand = 300;
    int32_t dim = 64;
    const int64_t *query_ids = i64;
    int64_t n_queries = 4;
    const float *query_scale = f32, *cand_scale = f32;
    const uint8_t *cand_ok = u8;
    const int64_t *list_ptr = i64, *list_items = i64, *list_rows = i64;
    int64_t n_lists = 50;
    const int64_t *skip_id = i64;
    int32_t k = 20, slices = 0;
    int64_t *out_index = i64;
    float *out_value = f32;
    void *workspace = i64;
    size_t workspace_bytes = (size_t)1 << 40;
    int32_t *status = i32;
    int run() const {
        return lgc_retrieve_topk(queries, query_stride, n_query_rows, cands, cand_stride, n_cand, dim, query_ids, n_queries,
                                 query_scale, cand_scale, cand_ok, list_ptr, list_items, list_rows, n_lists, skip_id, k, slices,
                                 out_index, out_value, workspace, workspace_bytes, status, nullptr);
    }
};

int main() {
    // the workspace size
    expect("size refuses k 0", (long long)lgc_retrieve_workspace_bytes(4, 300, 0, 2), 0);
    expect("size refuses k 65", (long long)lgc_retrieve_workspace_bytes(4, 300, 65, 2), 0);
    expect("size refuses slices 1025", (long long)lgc_retrieve_workspace_bytes(4, 300, 20, 1025), 0);
    expect("size refuses slices -1", (long long)lgc_retrieve_workspace_bytes(4, 300, 20, -1), 0);
    expect("size refuses no candidates", (long long)lgc_retrieve_workspace_bytes(4, 0, 20, 2), 0);
    expect("size refuses 2^31 candidates", (long long)lgc_retrieve_workspace_bytes(4, (int64_t)1 << 31, 20, 2), 0);
    expect("size refuses negative queries", (long long)lgc_retrieve_workspace_bytes(-1, 300, 20, 2), 0);
    expect("size of 2 ranges", (long long)lgc_retrieve_workspace_bytes(4, 300, 20, 2), 4 * 2 * 20 * 8);
    expect("size of one range", (long long)lgc_retrieve_workspace_bytes(4, 300, 20, 1), 0);
    expect("size clamps to the candidate tiles", (long long)lgc_retrieve_workspace_bytes(4, 300, 20, 1024), 4 * 3 * 20 * 8);
    expect("size at the limits", (long long)lgc_retrieve_workspace_bytes(INT32_MAX - 1, INT32_MAX - 1, 64, 1024),
           (long long)(INT32_MAX - 1) * 1024 * 64 * 8);
    expect("size, ranges chosen, at the limits", (long long)lgc_retrieve_workspace_bytes(INT32_MAX - 1, INT32_MAX - 1, 64, 0),
           ((long long)(INT32_MAX - 1) + 512 * 64) * 64 * 8);

    // lgc_retrieve_topk
    Call c;
    { Call b = c; b.queries = nullptr; expect("null queries", b.run(), LGC_E_INVAL); }
    { Call b = c; b.cands = nullptr; expect("null cands", b.run(), LGC_E_INVAL); }
    { Call b = c; b.out_index = nullptr; expect("null out_index", b.run(), LGC_E_INVAL); }
    { Call b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_queries = -1; expect("negative n_queries", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_query_rows = -1; expect("negative n_query_rows", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_lists = -1; expect("negative n_lists", b.run(), LGC_E_INVAL); }
    { Call b = c; b.query_stride = 63; expect("short query stride", b.run(), LGC_E_INVAL); }
    { Call b = c; b.cand_stride = 63; expect("short cand stride", b.run(), LGC_E_INVAL); }
    { Call b = c; b.query_scale = nullptr; expect("cand_scale alone", b.run(), LGC_E_INVAL); }
    { Call b = c; b.cand_scale = nullptr; expect("query_scale alone", b.run(), LGC_E_INVAL); }
    { Call b = c; b.list_items = nullptr; expect("list_ptr without list_items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Call b = c; b.dim = 257; b.query_stride = b.cand_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Call b = c; b.k = 0; expect("k 0", b.run(), LGC_E_RANGE); }
    { Call b = c; b.k = LGC_RETRIEVE_MAX_K + 1; expect("k 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.slices = -1; expect("slices -1", b.run(), LGC_E_RANGE); }
    { Call b = c; b.slices = LGC_RETRIEVE_MAX_SLICES + 1; expect("slices 1025", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_cand = 0; expect("no candidates", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_cand = (int64_t)1 << 31; expect("2^31 candidates", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_queries = INT32_MAX; expect("2^31 - 1 queries", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_query_rows = INT32_MAX; expect("2^31 - 1 query rows", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_lists = INT32_MAX; expect("2^31 - 1 lists", b.run(), LGC_E_RANGE); }
    { Call b = c; b.queries = off_by(f32, 2); expect("misaligned queries", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.cands = off_by(f32, 2); expect("misaligned cands", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.query_scale = off_by(f32, 2); expect("misaligned query_scale", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.cand_scale = off_by(f32, 2); expect("misaligned cand_scale", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_value = off_by(f32, 2); expect("misaligned out_value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.query_ids = off_by(i64, 4); expect("misaligned query_ids", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_ptr = off_by(i64, 4); expect("misaligned list_ptr", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_items = off_by(i64, 4); expect("misaligned list_items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.list_rows = off_by(i64, 4); expect("misaligned list_rows", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.skip_id = off_by(i64, 4); expect("misaligned skip_id", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.out_index = off_by(i64, 4); expect("misaligned out_index", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace = off_by(i64, 4); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.slices = 2; b.workspace_bytes = 4 * 2 * 20 * 8 - 1; expect("workspace one byte short", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.slices = 2; b.workspace = nullptr; expect("workspace missing", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.workspace_bytes = 0; expect("workspace missing, ranges chosen", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_queries = 0; expect("no queries", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.query_ids = nullptr; b.query_scale = b.cand_scale = nullptr; b.cand_ok = nullptr;
      b.list_ptr = b.list_items = b.list_rows = nullptr; b.skip_id = nullptr; b.out_value = nullptr; b.workspace = nullptr;
      b.workspace_bytes = 0; b.slices = 1; expect("no queries, no options", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.k = 64; b.slices = 1024; b.dim = 256; b.query_stride = 259; b.cand_stride = 256;
      expect("no queries, limits", b.run(), 0); }
    { Call b = c; b.n_queries = 0; b.cand_stride = 63; expect("no queries, still validated", b.run(), LGC_E_INVAL); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_retrieve_host: every argument check returned its code before any launch");
    return 0;
}

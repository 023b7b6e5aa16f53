// The argument checks of lgc_softmax_batch and lgc_softmax_workspace_bytes (include/lgconv_hip.h) as a stand-alone host
// program, for tools/asan_softmax_host.sh: every call below must return its code before anything is launched, so the device
// pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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

struct Soft {
    const float *table = f32;
    int64_t stride = 64, table_rows = 400, split = 100;
    int32_t dim = 64;
    const int64_t *row_users = i64;
    int64_t n_rows = 8;
    const int64_t *cand_items = i64;
    int64_t n_cand = 16;
    const int32_t *target = i32;
    const int32_t *ign_ptr = i32;
    const int64_t *ign_items = i64;
    const float *cand_bias = f32;
    float inv_tau = 1.0f;
    int64_t size = 8;
    float *loss = f32, *row_loss = f32;
    int32_t *n_adm = i32;
    float *grad_logits = f32;
    int64_t g_stride = 16;
    float *grad_users = f32, *grad_cands = f32;
    int64_t grad_stride = 64;
    void *workspace = f32;
    size_t workspace_bytes = (size_t)1 << 20;
    int32_t *status = i32;
    int run() const {
        return lgc_softmax_batch(table, stride, table_rows, split, dim, row_users, n_rows, cand_items, n_cand, target, ign_ptr,
                                 ign_items, cand_bias, inv_tau, size, loss, row_loss, n_adm, grad_logits, g_stride, grad_users,
                                 grad_cands, grad_stride, workspace, workspace_bytes, status, nullptr);
    }
};

static const void *off(const void *p, int bytes) { return static_cast<const char *>(p) + bytes; }

int main() {
    const int64_t two31 = (int64_t)1 << 31;
    Soft c;
    { Soft b = c; b.table = nullptr; expect("null table", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.row_users = nullptr; expect("null row_users", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.cand_items = nullptr; expect("null cand_items", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.target = nullptr; expect("null target", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.loss = nullptr; expect("null loss", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.grad_users = nullptr; expect("null grad_users", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.grad_cands = nullptr; expect("null grad_cands", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.ign_ptr = nullptr; expect("ign_items without ign_ptr", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.ign_items = nullptr; expect("ign_ptr without ign_items", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.n_rows = -1; expect("negative n_rows", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.n_cand = -1; expect("negative n_cand", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.table_rows = -1; expect("negative table_rows", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.size = 0; expect("size 0", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.size = INT64_MIN; expect("size most negative", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.stride = 63; expect("short stride", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.grad_stride = 63; expect("short grad_stride", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.g_stride = 15; expect("short g_stride", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.inv_tau = 0.0f; expect("inv_tau 0", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.inv_tau = -2.0f; expect("inv_tau negative", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.inv_tau = INFINITY; expect("inv_tau inf", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.inv_tau = NAN; expect("inv_tau nan", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.split = -1; expect("split -1", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.split = 401; expect("split past the table", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Soft b = c; b.dim = 257; b.stride = b.grad_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Soft b = c; b.dim = 0; b.table = nullptr; expect("the width is judged first", b.run(), LGC_E_DIM); }
    { Soft b = c; b.n_rows = two31; expect("2^31 rows", b.run(), LGC_E_RANGE); }
    { Soft b = c; b.n_cand = two31; b.g_stride = two31; expect("2^31 candidates", b.run(), LGC_E_RANGE); }
    { Soft b = c; b.table_rows = two31; expect("2^31 table rows", b.run(), LGC_E_RANGE); }
    { Soft b = c; b.n_cand = 65535 * 128 + 1; b.g_stride = b.n_cand; expect("too many candidate tiles", b.run(), LGC_E_RANGE); }
    { Soft b = c; b.n_rows = INT64_MAX; b.n_cand = INT64_MAX; b.g_stride = INT64_MAX; expect("counts whose product overflows", b.run(), LGC_E_RANGE); }
    { Soft b = c; b.table = static_cast<const float *>(off(f32, 2)); expect("misaligned table", b.run(), LGC_E_ALIGN); }
    { Soft b = c; b.row_users = static_cast<const int64_t *>(off(i64, 4)); expect("misaligned row_users", b.run(), LGC_E_ALIGN); }
    { Soft b = c; b.ign_items = static_cast<const int64_t *>(off(i64, 4)); expect("misaligned ign_items", b.run(), LGC_E_ALIGN); }
    { Soft b = c; b.workspace = const_cast<void *>(off(f32, 1)); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Soft b = c; b.workspace_bytes = lgc_softmax_workspace_bytes(8, 16) - 1; expect("short workspace", b.run(), LGC_E_WORKSPACE); }
    { Soft b = c; b.workspace = nullptr; expect("no workspace", b.run(), LGC_E_WORKSPACE); }
    { Soft b = c; b.n_rows = two31 - 1; b.n_cand = 65535 * 128; b.g_stride = b.n_cand; b.table_rows = two31 - 1;
      expect("the largest sizes: refused for the workspace alone", b.run(), LGC_E_WORKSPACE); }
    { Soft b = c; b.n_rows = 0; b.stride = 63; expect("no rows, still validated", b.run(), LGC_E_INVAL); }
    { Soft b = c; b.n_cand = 0; b.g_stride = 0; b.dim = 300; expect("no candidates, still validated", b.run(), LGC_E_DIM); }

    expect("workspace(0, 0)", (long long)lgc_softmax_workspace_bytes(0, 0), 0);
    expect("workspace(-1, 4)", (long long)lgc_softmax_workspace_bytes(-1, 4), 0);
    expect("workspace(4, 2^31)", (long long)lgc_softmax_workspace_bytes(4, two31), 0);
    expect("workspace(INT64_MAX, INT64_MAX)", (long long)lgc_softmax_workspace_bytes(INT64_MAX, INT64_MAX), 0);
    size_t last = 0;
    for (int64_t n = 0; n < 300; n += 7) {                   // monotonic in both
        size_t row_last = 0;
        for (int64_t m = 0; m < 300; m += 5) {
            const size_t s = lgc_softmax_workspace_bytes(n, m);
            if (s < row_last || s < (size_t)(4 * (n * m + n))) expect("workspace monotonic in n_cand", 1, 0);
            row_last = s;
        }
        if (row_last < last) expect("workspace monotonic in n_rows", 1, 0);
        last = row_last;
    }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_softmax_host: every argument check returned its code before any launch");
    return 0;
}

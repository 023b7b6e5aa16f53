// The argument checks of lgc_fold_in (include/lgconv_hip.h) as a stand-alone host program, for tools/asan_foldin_host.sh:
// every call below must return its code before anything is launched, so the device pointers are never dereferenced and no
// GPU is needed.  Exit status 0 = every code as expected.
#include <cstdint>
#include <cstdio>

#include "lgconv_hip.h"

static int failures = 0;

static void expect(const char *what, int got, int want) {
    if (got != want) {
        std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
        ++failures;
    }
}

// addresses of host words: valid, 16-byte aligned, and never read or written by a call that returns before its launch
alignas(16) static int64_t i64[4];
alignas(16) static float f32[4];
alignas(16) static int32_t i32[4];

struct Args {
    const int64_t *ptr = i64, *items = i64;
    const float *weight = f32;
    int64_t n_rows = 4;
    const float *dis = f32, *fold = f32;
    int64_t fold_stride = 64, n_items = 300;
    const int64_t *init_rows = i64;
    const float *init = f32;
    int64_t init_stride = 64, n_init_rows = 10;
    float a0 = 0.25f;
    int32_t normalize = 1, dim = 64;
    float *out = f32;
    int64_t out_stride = 64;
    int32_t *status = i32;
};

static int fold(const Args &a) {
    return lgc_fold_in(a.ptr, a.items, a.weight, a.n_rows, a.dis, a.fold, a.fold_stride, a.n_items, a.init_rows, a.init,
                       a.init_stride, a.n_init_rows, a.a0, a.normalize, a.dim, a.out, a.out_stride, a.status, nullptr);
}

int main() {
    const int64_t big = INT32_MAX;
    Args a;
    a = Args{}; a.ptr = nullptr; expect("null list_ptr", fold(a), LGC_E_INVAL);
    a = Args{}; a.items = nullptr; expect("null list_items", fold(a), LGC_E_INVAL);
    a = Args{}; a.fold = nullptr; expect("null fold", fold(a), LGC_E_INVAL);
    a = Args{}; a.out = nullptr; expect("null out", fold(a), LGC_E_INVAL);
    a = Args{}; a.status = nullptr; expect("null status", fold(a), LGC_E_INVAL);
    a = Args{}; a.n_rows = -1; expect("negative rows", fold(a), LGC_E_INVAL);
    a = Args{}; a.n_items = -1; expect("negative items", fold(a), LGC_E_INVAL);
    a = Args{}; a.n_items = 0; expect("no items", fold(a), LGC_E_INVAL);
    a = Args{}; a.n_init_rows = -1; expect("negative init rows", fold(a), LGC_E_INVAL);
    a = Args{}; a.fold_stride = 63; expect("fold stride below dim", fold(a), LGC_E_INVAL);
    a = Args{}; a.out_stride = 63; expect("out stride below dim", fold(a), LGC_E_INVAL);
    a = Args{}; a.init_stride = 63; expect("init stride below dim", fold(a), LGC_E_INVAL);
    a = Args{}; a.normalize = 2; expect("normalize = 2", fold(a), LGC_E_INVAL);
    a = Args{}; a.normalize = -1; expect("normalize = -1", fold(a), LGC_E_INVAL);
    a = Args{}; a.dis = nullptr; expect("normalize without item_dis", fold(a), LGC_E_INVAL);
    a = Args{}; a.init = nullptr; expect("init_rows without init", fold(a), LGC_E_INVAL);
    a = Args{}; a.dim = 0; expect("dim 0", fold(a), LGC_E_DIM);
    a = Args{}; a.dim = -1; expect("dim -1", fold(a), LGC_E_DIM);
    a = Args{}; a.dim = 257; a.fold_stride = a.out_stride = a.init_stride = 300; expect("dim 257", fold(a), LGC_E_DIM);
    a = Args{}; a.n_rows = big; expect("2^31 - 1 rows", fold(a), LGC_E_RANGE);
    a = Args{}; a.n_rows = big + 1; expect("2^31 rows", fold(a), LGC_E_RANGE);
    a = Args{}; a.n_items = big; expect("2^31 - 1 items", fold(a), LGC_E_RANGE);
    a = Args{}; a.fold = reinterpret_cast<const float *>(reinterpret_cast<const char *>(f32) + 2);
    expect("fold not dword aligned", fold(a), LGC_E_ALIGN);
    // no rows: validated, nothing launched
    a = Args{}; a.n_rows = 0; expect("no rows", fold(a), 0);
    a = Args{}; a.n_rows = 0; a.weight = nullptr; a.init_rows = nullptr; a.init = nullptr; a.init_stride = 0; a.n_init_rows = 0;
    expect("no rows, no weights, no init", fold(a), 0);
    a = Args{}; a.n_rows = 0; a.normalize = 0; a.dis = nullptr; expect("no rows, raw weights", fold(a), 0);
    a = Args{}; a.n_rows = 0; a.dim = 1; a.fold_stride = a.out_stride = a.init_stride = 1; expect("no rows, dim 1", fold(a), 0);
    a = Args{}; a.n_rows = 0; a.dim = 256; a.fold_stride = a.init_stride = 256; a.out_stride = 259; expect("no rows, dim 256", fold(a), 0);
    a = Args{}; a.n_rows = 0; a.fold_stride = 63; expect("no rows, still validated", fold(a), LGC_E_INVAL);

    std::printf("fold-in argument checks: %d failure(s)\n", failures);
    return failures != 0;
}

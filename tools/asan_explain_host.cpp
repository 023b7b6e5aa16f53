// The argument checks of lgc_attribute (include/lgconv_hip.h) as a stand-alone host program, for tools/asan_explain_host.sh:
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
alignas(16) static lgc_entry ent[2];

static lgc_attr_args common() {
    lgc_attr_args a{};
    a.n_rows = 4;
    a.fold = f32; a.items = f32; a.fold_stride = 64; a.item_stride = 64; a.n_items = 300;
    a.init_rows = i64; a.init = f32; a.init_stride = 64; a.n_init_rows = 10; a.a0 = 0.25f;
    a.targets = i64; a.target_stride = 20; a.n_targets = 20; a.top_m = 3; a.dim = 64;
    a.contrib_ptr = i64; a.contrib = f32; a.base = f32; a.total = f32;
    a.top_pos = i32; a.top_item = i64; a.top_value = f32; a.status = i32;
    return a;
}

static lgc_attr_args session() {
    lgc_attr_args a = common();
    a.list_ptr = i64; a.list_items = i64; a.list_weight = f32; a.item_dis = f32; a.normalize = 1;
    return a;
}

static lgc_attr_args graph() {
    lgc_attr_args a = common();
    a.rowptr = i32; a.entries = ent; a.row_ids = i64; a.n_graph_rows = 10; a.col_base = 10;
    return a;
}

static int run(const lgc_attr_args &a) { return lgc_attribute(&a, nullptr); }

template <typename T>
static const T *off_by_two(const T *p) { return reinterpret_cast<const T *>(reinterpret_cast<const char *>(p) + 2); }

int main() {
    const int64_t big = INT32_MAX;
    expect("null args", lgc_attribute(nullptr, nullptr), LGC_E_INVAL);
    for (int form = 0; form < 2; ++form) {
        auto make = form ? graph : session;
        lgc_attr_args a;
        a = make(); a.fold = nullptr; expect("null fold", run(a), LGC_E_INVAL);
        a = make(); a.items = nullptr; expect("null items", run(a), LGC_E_INVAL);
        a = make(); a.targets = nullptr; expect("null targets", run(a), LGC_E_INVAL);
        a = make(); a.status = nullptr; expect("null status", run(a), LGC_E_INVAL);
        a = make(); a.n_rows = -1; expect("negative rows", run(a), LGC_E_INVAL);
        a = make(); a.n_items = -1; expect("negative items", run(a), LGC_E_INVAL);
        a = make(); a.n_items = 0; expect("no items", run(a), LGC_E_INVAL);
        a = make(); a.n_init_rows = -1; expect("negative init rows", run(a), LGC_E_INVAL);
        a = make(); a.fold_stride = 63; expect("fold stride below dim", run(a), LGC_E_INVAL);
        a = make(); a.item_stride = 63; expect("item stride below dim", run(a), LGC_E_INVAL);
        a = make(); a.init_stride = 63; expect("init stride below dim", run(a), LGC_E_INVAL);
        a = make(); a.target_stride = 19; expect("target stride below n_targets", run(a), LGC_E_INVAL);
        a = make(); a.init = nullptr; expect("init_rows without init", run(a), LGC_E_INVAL);
        a = make(); a.contrib_ptr = nullptr; expect("contrib without contrib_ptr", run(a), LGC_E_INVAL);
        a = make(); a.top_pos = nullptr; expect("top_m without top_pos", run(a), LGC_E_INVAL);
        a = make(); a.top_item = nullptr; expect("top_m without top_item", run(a), LGC_E_INVAL);
        a = make(); a.top_value = nullptr; expect("top_m without top_value", run(a), LGC_E_INVAL);
        a = make(); a.contrib = nullptr; a.base = nullptr; a.total = nullptr; a.top_m = 0; expect("no output", run(a), LGC_E_INVAL);
        a = make(); a.dim = 0; expect("dim 0", run(a), LGC_E_DIM);
        a = make(); a.dim = -1; expect("dim -1", run(a), LGC_E_DIM);
        a = make(); a.dim = 257; a.fold_stride = a.item_stride = a.init_stride = 300; expect("dim 257", run(a), LGC_E_DIM);
        a = make(); a.n_targets = 0; expect("no targets", run(a), LGC_E_RANGE);
        a = make(); a.n_targets = 65; a.target_stride = 65; expect("65 targets", run(a), LGC_E_RANGE);
        a = make(); a.top_m = 9; expect("top_m 9", run(a), LGC_E_RANGE);
        a = make(); a.top_m = -1; expect("top_m -1", run(a), LGC_E_RANGE);
        a = make(); a.n_rows = big; expect("2^31 - 1 rows", run(a), LGC_E_RANGE);
        a = make(); a.n_rows = big + 1; expect("2^31 rows", run(a), LGC_E_RANGE);
        a = make(); a.n_items = big; expect("2^31 - 1 items", run(a), LGC_E_RANGE);
        a = make(); a.fold = off_by_two(f32); expect("fold not dword aligned", run(a), LGC_E_ALIGN);
        a = make(); a.items = off_by_two(f32); expect("items not dword aligned", run(a), LGC_E_ALIGN);
        a = make(); a.init = off_by_two(f32); expect("init not dword aligned", run(a), LGC_E_ALIGN);
        a = make(); a.total = const_cast<float *>(off_by_two(f32)); expect("total not dword aligned", run(a), LGC_E_ALIGN);
        // no rows: validated, nothing launched
        a = make(); a.n_rows = 0; expect("no rows", run(a), 0);
        a = make(); a.n_rows = 0; a.init_rows = nullptr; a.init = nullptr; a.init_stride = 0; a.n_init_rows = 0;
        expect("no rows, no init", run(a), 0);
        a = make(); a.n_rows = 0; a.contrib = nullptr; a.contrib_ptr = nullptr; a.base = nullptr; a.total = nullptr;
        expect("no rows, top-m alone", run(a), 0);
        a = make(); a.n_rows = 0; a.n_targets = 64; a.target_stride = 64; a.top_m = 8; expect("no rows, the limits", run(a), 0);
        a = make(); a.n_rows = 0; a.dim = 1; a.fold_stride = a.item_stride = a.init_stride = 1; expect("no rows, dim 1", run(a), 0);
        a = make(); a.n_rows = 0; a.dim = 256; a.fold_stride = a.init_stride = 256; a.item_stride = 259; expect("no rows, dim 256", run(a), 0);
        a = make(); a.n_rows = 0; a.fold_stride = 63; expect("no rows, still validated", run(a), LGC_E_INVAL);
    }
    lgc_attr_args a;
    a = session(); a.rowptr = i32; a.entries = ent; a.row_ids = i64; expect("both list forms", run(a), LGC_E_INVAL);
    a = common(); expect("neither list form", run(a), LGC_E_INVAL);
    a = session(); a.list_ptr = nullptr; expect("null list_ptr", run(a), LGC_E_INVAL);
    a = session(); a.list_items = nullptr; expect("null list_items", run(a), LGC_E_INVAL);
    a = session(); a.normalize = 2; expect("normalize = 2", run(a), LGC_E_INVAL);
    a = session(); a.normalize = -1; expect("normalize = -1", run(a), LGC_E_INVAL);
    a = session(); a.item_dis = nullptr; expect("normalize without item_dis", run(a), LGC_E_INVAL);
    a = session(); a.n_rows = 0; a.normalize = 0; a.item_dis = nullptr; a.list_weight = nullptr; expect("no rows, raw weights", run(a), 0);
    a = graph(); a.rowptr = nullptr; expect("null rowptr", run(a), LGC_E_INVAL);
    a = graph(); a.entries = nullptr; expect("null entries", run(a), LGC_E_INVAL);
    a = graph(); a.row_ids = nullptr; expect("null row_ids", run(a), LGC_E_INVAL);
    a = graph(); a.n_graph_rows = -1; expect("negative graph rows", run(a), LGC_E_INVAL);
    a = graph(); a.n_graph_rows = big + 1; expect("2^31 graph rows", run(a), LGC_E_RANGE);

    std::printf("attribution argument checks: %d failure(s)\n", failures);
    return failures != 0;
}

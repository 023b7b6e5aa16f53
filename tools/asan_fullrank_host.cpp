// The argument checks of lgc_rank_positions_workspace_bytes and lgc_rank_positions (include/lgconv_hip.h) as a stand-alone
// host program, for tools/asan_fullrank_host.sh: every call below must return its code before anything is launched, so the
// device pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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

template <typename T>
static T *off_by(T *p, int bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + bytes); }

struct Call {
    const float *users = f32, *items = f32;
    int64_t user_stride = 64, n_user_rows = 50, item_stride = 64, n_items = 300;
    int32_t dim = 64;
    const int64_t *pair_users = i64, *pair_items = i64;
    int64_t n_pairs = 4;
    const int64_t *seen_ptr = i64, *seen_items = i64;
    int32_t seen_mode = LGC_RANK_SEEN_ZERO, slices = 0;
    int32_t *rank = i32, *n_equal = i32, *n_cand = i32;
    float *value = f32;
    void *workspace = i64;
    size_t workspace_bytes = (size_t)1 << 40;
    int32_t *status = i32;
    int run() const {
        return lgc_rank_positions(users, user_stride, n_user_rows, items, item_stride, n_items, dim, pair_users, pair_items,
                                  n_pairs, seen_ptr, seen_items, seen_mode, slices, rank, n_equal, n_cand, value, workspace,
                                  workspace_bytes, status, nullptr);
    }
};

int main() {
    // the workspace size
    expect("size refuses slices 65", (long long)lgc_rank_positions_workspace_bytes(4, 300, 65), 0);
    expect("size refuses slices -1", (long long)lgc_rank_positions_workspace_bytes(4, 300, -1), 0);
    expect("size refuses no items", (long long)lgc_rank_positions_workspace_bytes(4, 0, 2), 0);
    expect("size refuses 2^31 items", (long long)lgc_rank_positions_workspace_bytes(4, (int64_t)1 << 31, 2), 0);
    expect("size refuses negative pairs", (long long)lgc_rank_positions_workspace_bytes(-1, 300, 2), 0);
    expect("size refuses 2^31 - 1 pairs", (long long)lgc_rank_positions_workspace_bytes(INT32_MAX, 300, 2), 0);
    expect("size of no pairs", (long long)lgc_rank_positions_workspace_bytes(0, 300, 2), 0);
    expect("size of 4 pairs", (long long)lgc_rank_positions_workspace_bytes(4, 300, 2), 16);
    expect("size at the limits", (long long)lgc_rank_positions_workspace_bytes(INT32_MAX - 1, INT32_MAX - 1, 64),
           (long long)(INT32_MAX - 1) * 4);

    // lgc_rank_positions
    Call c;
    { Call b = c; b.users = nullptr; expect("null users", b.run(), LGC_E_INVAL); }
    { Call b = c; b.items = nullptr; expect("null items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.pair_users = nullptr; expect("null pair_users", b.run(), LGC_E_INVAL); }
    { Call b = c; b.pair_items = nullptr; expect("null pair_items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.rank = nullptr; expect("null rank", b.run(), LGC_E_INVAL); }
    { Call b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_pairs = -1; expect("negative n_pairs", b.run(), LGC_E_INVAL); }
    { Call b = c; b.n_user_rows = -1; expect("negative n_user_rows", b.run(), LGC_E_INVAL); }
    { Call b = c; b.user_stride = 63; expect("short user stride", b.run(), LGC_E_INVAL); }
    { Call b = c; b.item_stride = 63; expect("short item stride", b.run(), LGC_E_INVAL); }
    { Call b = c; b.seen_mode = 2; expect("seen_mode 2", b.run(), LGC_E_INVAL); }
    { Call b = c; b.seen_mode = -1; expect("seen_mode -1", b.run(), LGC_E_INVAL); }
    { Call b = c; b.seen_items = nullptr; expect("seen_ptr without seen_items", b.run(), LGC_E_INVAL); }
    { Call b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Call b = c; b.dim = 257; b.user_stride = b.item_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Call b = c; b.slices = -1; expect("slices -1", b.run(), LGC_E_RANGE); }
    { Call b = c; b.slices = 65; expect("slices 65", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_items = (int64_t)1 << 31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_pairs = INT32_MAX; expect("2^31 - 1 pairs", b.run(), LGC_E_RANGE); }
    { Call b = c; b.n_user_rows = INT32_MAX; expect("2^31 - 1 user rows", b.run(), LGC_E_RANGE); }
    { Call b = c; b.users = off_by(f32, 2); expect("misaligned users", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.items = off_by(f32, 2); expect("misaligned items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.value = off_by(f32, 2); expect("misaligned value", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.rank = off_by(i32, 2); expect("misaligned rank", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.n_equal = off_by(i32, 2); expect("misaligned n_equal", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.n_cand = off_by(i32, 2); expect("misaligned n_cand", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.pair_users = off_by(i64, 4); expect("misaligned pair_users", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.pair_items = off_by(i64, 4); expect("misaligned pair_items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.seen_ptr = off_by(i64, 4); expect("misaligned seen_ptr", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.seen_items = off_by(i64, 4); expect("misaligned seen_items", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace = off_by(i64, 2); expect("misaligned workspace", b.run(), LGC_E_ALIGN); }
    { Call b = c; b.workspace_bytes = 15; expect("workspace one byte short", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.workspace = nullptr; expect("workspace missing", b.run(), LGC_E_WORKSPACE); }
    { Call b = c; b.n_pairs = 0; expect("no pairs", b.run(), 0); }
    { Call b = c; b.n_pairs = 0; b.seen_ptr = b.seen_items = nullptr; b.n_equal = b.n_cand = nullptr; b.value = nullptr;
      b.workspace = nullptr; b.workspace_bytes = 0; b.seen_mode = LGC_RANK_SEEN_REMOVE; expect("no pairs, no options", b.run(), 0); }
    { Call b = c; b.n_pairs = 0; b.seen_ptr = nullptr; b.seen_items = off_by(i64, 4); expect("no lists, seen_items ignored", b.run(), 0); }
    { Call b = c; b.n_pairs = 0; b.slices = 64; b.dim = 256; b.user_stride = b.item_stride = 259; expect("no pairs, limits", b.run(), 0); }
    { Call b = c; b.n_pairs = 0; b.n_user_rows = 0; b.n_items = 1; expect("no pairs, smallest tables", b.run(), 0); }
    { Call b = c; b.n_pairs = 0; b.item_stride = 63; expect("no pairs, still validated", b.run(), LGC_E_INVAL); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_fullrank_host: every argument check returned its code before any launch");
    return 0;
}

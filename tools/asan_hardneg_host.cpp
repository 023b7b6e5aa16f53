// The argument checks of lgc_sample_hard_triples (include/lgconv_hip.h) as a stand-alone host program, for
// tools/asan_hardneg_host.sh: every call below must return its code before anything is launched, so the device pointers are
// never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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

struct Hard {
    const int64_t *users = i64;
    int64_t n = 4;
    const int32_t *pos_ptr = i32;
    const int64_t *pos_items = i64;
    const int32_t *ign_ptr = i32;
    const int64_t *ign_items = i64;
    int64_t n_users = 100, n_items = 300;
    uint64_t seed = 1, step = 2;
    int32_t n_cand = 8;
    const float *user_table = f32;
    int64_t user_stride = 64;
    const float *item_table = f32;
    int64_t item_stride = 64;
    int32_t dim = 64;
    int64_t *pos_out = i64, *neg_out = i64;
    float *neg_score = f32;
    int32_t *neg_attempt = i32, *n_admissible = i32, *status = i32;
    int run() const {
        return lgc_sample_hard_triples(users, n, pos_ptr, pos_items, ign_ptr, ign_items, n_users, n_items, seed, step, n_cand,
                                       user_table, user_stride, item_table, item_stride, dim, pos_out, neg_out, neg_score,
                                       neg_attempt, n_admissible, status, nullptr);
    }
};

int main() {
    const int64_t two31 = (int64_t)1 << 31;
    Hard c;
    { Hard b = c; b.users = nullptr; expect("null users", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.pos_ptr = nullptr; expect("null pos_ptr", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.pos_items = nullptr; expect("null pos_items", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.ign_ptr = nullptr; expect("null ign_ptr", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.user_table = nullptr; expect("null user_table", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.item_table = nullptr; expect("null item_table", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.pos_out = nullptr; expect("null pos_out", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.neg_out = nullptr; expect("null neg_out", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.status = nullptr; expect("null status", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.n = -1; expect("negative n", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.n_users = -1; expect("negative n_users", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.n_items = 0; expect("no items", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.n_items = -5; expect("negative n_items", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.user_stride = 63; expect("short user stride", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.item_stride = 63; expect("short item stride", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.dim = 0; expect("dim 0", b.run(), LGC_E_DIM); }
    { Hard b = c; b.dim = -1; expect("dim -1", b.run(), LGC_E_DIM); }
    { Hard b = c; b.dim = 257; b.user_stride = b.item_stride = 300; expect("dim 257", b.run(), LGC_E_DIM); }
    { Hard b = c; b.dim = 0; b.users = nullptr; b.n_cand = 0; expect("the width is judged first", b.run(), LGC_E_DIM); }
    { Hard b = c; b.n_cand = 0; expect("n_cand 0", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_cand = -1; expect("n_cand -1", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_cand = LGC_HARDNEG_MAX_CAND + 1; expect("n_cand 257", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n = two31; expect("2^31 samples", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_users = two31; expect("2^31 users", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_items = two31; expect("2^31 items", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_users = two31 / 2; b.n_items = two31 / 2; expect("2^31 nodes", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n_users = INT64_MAX; b.n_items = INT64_MAX; expect("node counts whose sum overflows", b.run(), LGC_E_RANGE); }
    { Hard b = c; b.n = 0; expect("no samples", b.run(), 0); }
    { Hard b = c; b.n = 0; b.neg_score = nullptr; b.neg_attempt = nullptr; b.n_admissible = nullptr; b.ign_items = nullptr;
      expect("no samples, no options", b.run(), 0); }
    { Hard b = c; b.n = 0; b.n_cand = LGC_HARDNEG_MAX_CAND; b.dim = 256; b.user_stride = 259; b.item_stride = 256;
      b.seed = b.step = UINT64_MAX; expect("no samples, limits", b.run(), 0); }
    { Hard b = c; b.n = 0; b.n_cand = 1; b.dim = 1; b.user_stride = b.item_stride = 1; b.n_users = 0; b.n_items = 1;
      expect("no samples, smallest", b.run(), 0); }
    { Hard b = c; b.n = 0; b.n_users = two31 / 2; b.n_items = two31 / 2 - 2; expect("no samples, most nodes", b.run(), 0); }
    { Hard b = c; b.n = 0; b.item_stride = 63; expect("no samples, still validated", b.run(), LGC_E_INVAL); }
    { Hard b = c; b.n = 0; b.n_cand = 257; expect("no samples, n_cand still validated", b.run(), LGC_E_RANGE); }

    if (failures) {
        std::fprintf(stderr, "%d unexpected return codes\n", failures);
        return 1;
    }
    std::puts("asan_hardneg_host: every argument check returned its code before any launch");
    return 0;
}

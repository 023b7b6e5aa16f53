// The argument checks of lgc_rank_metrics / lgc_column_sums / lgc_topk_coverage (include/lgconv_hip.h) as a stand-alone
// host program, for tools/asan_metrics_host.sh: every call below must return its code before anything is launched, so
// the device pointers are never dereferenced and no GPU is needed.  The cutoffs ARE read, on the host: they are real
// arrays of exactly n_cut entries, so a read past them is the sanitizer's to report.  Exit status 0 = every code as expected.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lgconv_hip.h"

static int failures = 0;

static void expect(const char *what, int got, int want) {
    if (got != want) {
        std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
        ++failures;
    }
}

int main() {
    // addresses of host words: valid, aligned, and never read or written by a call that returns before its launch
    static int64_t i64[4];
    static uint64_t u64[4];
    static uint32_t u32[4];
    static int32_t i32[4];
    static double f64[4];
    const int64_t big = INT32_MAX;
    // heap arrays of exactly n_cut entries
    const std::vector<int32_t> c3{5, 10, 20}, c1{20}, eight{1, 2, 63, 64, 65, 128, 192, 256}, nine{1, 2, 3, 4, 5, 6, 7, 8, 9};
    const std::vector<int32_t> same{5, 5, 20}, down{10, 5, 20}, zero{0, 5, 20}, over_k{5, 10, 21}, over_max{5, 10, 257}, neg{-4, 5};

    auto rank = [&](const int64_t *topk, int64_t stride, int32_t k, const int64_t *ptr, int64_t n, int64_t nu,
                    const std::vector<int32_t> *cuts, int32_t nc, int32_t *hits, double *metrics, int32_t *status) {
        return lgc_rank_metrics(topk, stride, k, ptr, i64, i64, i64, n, nu, cuts ? cuts->data() : nullptr, nc, u64, hits, metrics,
                                status, nullptr);
    };
    expect("rank null topk", rank(nullptr, 20, 20, i64, 4, 10, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank null pos_ptr", rank(i64, 20, 20, nullptr, 4, 10, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank null hits", rank(i64, 20, 20, i64, 4, 10, &c3, 3, nullptr, f64, i32), LGC_E_INVAL);
    expect("rank null metrics", rank(i64, 20, 20, i64, 4, 10, &c3, 3, i32, nullptr, i32), LGC_E_INVAL);
    expect("rank null status", rank(i64, 20, 20, i64, 4, 10, &c3, 3, i32, f64, nullptr), LGC_E_INVAL);
    expect("rank null cutoffs", rank(i64, 20, 20, i64, 4, 10, nullptr, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank negative rows", rank(i64, 20, 20, i64, -1, 10, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank negative users", rank(i64, 20, 20, i64, 4, -1, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank k = 0", rank(i64, 20, 0, i64, 4, 10, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank stride below k", rank(i64, 19, 20, i64, 4, 10, &c3, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank no cutoffs", rank(i64, 20, 20, i64, 4, 10, &c3, 0, i32, f64, i32), LGC_E_INVAL);
    expect("rank nine cutoffs", rank(i64, 20, 20, i64, 4, 10, &nine, 9, i32, f64, i32), LGC_E_INVAL);
    expect("rank equal cutoffs", rank(i64, 20, 20, i64, 4, 10, &same, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank descending cutoffs", rank(i64, 20, 20, i64, 4, 10, &down, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank cutoff 0", rank(i64, 20, 20, i64, 4, 10, &zero, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank negative cutoff", rank(i64, 20, 20, i64, 4, 10, &neg, 2, i32, f64, i32), LGC_E_INVAL);
    expect("rank cutoff above k", rank(i64, 20, 20, i64, 4, 10, &over_k, 3, i32, f64, i32), LGC_E_INVAL);
    expect("rank k = 257", rank(i64, 257, 257, i64, 4, 10, &c3, 3, i32, f64, i32), LGC_E_RANGE);
    expect("rank cutoff 257", rank(i64, 256, 256, i64, 4, 10, &over_max, 3, i32, f64, i32), LGC_E_RANGE);
    expect("rank 2^31 rows", rank(i64, 20, 20, i64, big, 10, &c3, 3, i32, f64, i32), LGC_E_RANGE);
    expect("rank no rows", rank(i64, 20, 20, i64, 0, 10, &c3, 3, i32, f64, i32), 0);
    expect("rank no rows, one cutoff", rank(i64, 20, 20, i64, 0, 10, &c1, 1, i32, f64, i32), 0);
    expect("rank no rows, eight cutoffs", rank(i64, 256, 256, i64, 0, 10, &eight, 8, i32, f64, i32), 0);

    expect("sums null out", lgc_column_sums(f64, 6, 5, 6, nullptr, nullptr), LGC_E_INVAL);
    expect("sums null in", lgc_column_sums(nullptr, 6, 5, 6, f64, nullptr), LGC_E_INVAL);
    expect("sums negative rows", lgc_column_sums(f64, 6, -1, 6, f64, nullptr), LGC_E_INVAL);
    expect("sums no columns", lgc_column_sums(f64, 6, 5, 0, f64, nullptr), LGC_E_INVAL);
    expect("sums stride below width", lgc_column_sums(f64, 5, 5, 6, f64, nullptr), LGC_E_INVAL);
    expect("sums 65 columns", lgc_column_sums(f64, 65, 5, LGC_COLUMN_SUMS_MAX + 1, f64, nullptr), LGC_E_RANGE);
    expect("sums no rows", lgc_column_sums(f64, 64, 0, LGC_COLUMN_SUMS_MAX, f64, nullptr), 0);
    expect("sums no rows, no input", lgc_column_sums(nullptr, 6, 0, 6, f64, nullptr), 0);

    auto cover = [&](const int64_t *topk, int64_t stride, int32_t k, int64_t n, const std::vector<int32_t> *cuts, int32_t nc,
                     int64_t n_items, uint32_t *bitmap, int64_t *counts, int32_t *status) {
        return lgc_topk_coverage(topk, stride, k, n, cuts ? cuts->data() : nullptr, nc, n_items, bitmap, counts, status, nullptr);
    };
    expect("cover null topk", cover(nullptr, 20, 20, 4, &c3, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover null bitmap", cover(i64, 20, 20, 4, &c3, 3, 300, nullptr, i64, i32), LGC_E_INVAL);
    expect("cover null counts", cover(i64, 20, 20, 4, &c3, 3, 300, u32, nullptr, i32), LGC_E_INVAL);
    expect("cover null status", cover(i64, 20, 20, 4, &c3, 3, 300, u32, i64, nullptr), LGC_E_INVAL);
    expect("cover null cutoffs", cover(i64, 20, 20, 4, nullptr, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover negative rows", cover(i64, 20, 20, -1, &c3, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover no items", cover(i64, 20, 20, 4, &c3, 3, 0, u32, i64, i32), LGC_E_INVAL);
    expect("cover negative items", cover(i64, 20, 20, 4, &c3, 3, -5, u32, i64, i32), LGC_E_INVAL);
    expect("cover k = 0", cover(i64, 20, 0, 4, &c3, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover stride below k", cover(i64, 19, 20, 4, &c3, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover no cutoffs", cover(i64, 20, 20, 4, &c3, 0, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover nine cutoffs", cover(i64, 20, 20, 4, &nine, 9, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover equal cutoffs", cover(i64, 20, 20, 4, &same, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover cutoff above k", cover(i64, 20, 20, 4, &over_k, 3, 300, u32, i64, i32), LGC_E_INVAL);
    expect("cover k = 257", cover(i64, 257, 257, 4, &c3, 3, 300, u32, i64, i32), LGC_E_RANGE);
    expect("cover cutoff 257", cover(i64, 256, 256, 4, &over_max, 3, 300, u32, i64, i32), LGC_E_RANGE);
    expect("cover 2^31 rows", cover(i64, 20, 20, big, &c3, 3, 300, u32, i64, i32), LGC_E_RANGE);
    expect("cover 2^31 items", cover(i64, 20, 20, 4, &c3, 3, big, u32, i64, i32), LGC_E_RANGE);

    std::printf("ranking-metric argument checks: %d failure(s)\n", failures);
    return failures != 0;
}

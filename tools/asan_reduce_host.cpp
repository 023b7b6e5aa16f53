// lgc_reduce_concat_host (include/lgconv_hip.h: the builder of the concatenated operator [R_H^T | G_L], the code the
// kernels of lgc_reduce_concat call element by element) as a stand-alone host program, for tools/asan_reduce_host.sh.
// Random reduced CSRs in heap buffers of exactly the documented sizes, so that any read or write past an end is an
// AddressSanitizer report; the outputs are checked against the layout's own invariants.  No GPU is needed: the device
// entry point is only called with arguments it rejects before its first launch.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "lgconv_hip.h"

static int failures = 0;

static void expect(const char *what, long long got, long long want) {
    if (got != want) {
        std::fprintf(stderr, "%s: got %lld, expected %lld\n", what, got, want);
        ++failures;
    }
}

// One random case: n_kept users of random row lengths (zero allowed), item rows on kept users, a random G_L.
static void run_case(std::mt19937 &rng, int n_kept, int n_items, int n_gaps, int max_len) {
    auto below = [&](int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)n); };
    const int n_rows = n_kept + n_items;
    std::vector<int32_t> rp(n_rows + 1, 0), grp(n_rows + 1, 0);
    std::vector<lgc_entry> ent, gent;
    for (int r = 0; r < n_rows; ++r) {
        const int len = (r < n_kept || n_kept > 0) ? below(max_len + 1) : 0;
        for (int k = 0; k < len; ++k) ent.push_back({r < n_kept ? n_kept + below(n_items) : below(n_kept), 0.5f + (float)k});
        rp[r + 1] = (int32_t)ent.size();
        if (r >= n_kept) {
            const int glen = below(max_len + 1);
            for (int k = 0; k < glen; ++k) gent.push_back({n_kept + below(n_items), 0.25f});
        }
        grp[r + 1] = (int32_t)gent.size();
    }
    const int64_t n_phys = lgc_reduce_concat_rows(n_kept, n_items, n_gaps);
    const int gap_rows = (n_items + n_gaps - 1) / n_gaps;
    expect("n_phys", n_phys, n_kept + (int64_t)gap_rows * n_gaps);
    const int64_t n_out = (int64_t)ent.size() + n_items + (int64_t)gent.size();
    // exact sizes: new[] of zero elements is a valid, unreadable pointer
    std::vector<int32_t> pos(n_kept), gap_start(n_gaps), rp_out(n_phys + n_items + 1, -1);
    std::vector<lgc_entry> out(n_out, lgc_entry{-1, 0.0f});
    const int rc = lgc_reduce_concat_host(rp.data(), ent.empty() ? nullptr : ent.data(), (int64_t)ent.size(), grp.data(),
                                          gent.empty() ? nullptr : gent.data(), (int64_t)gent.size(), n_kept, n_items, n_gaps,
                                          n_kept ? pos.data() : nullptr, gap_start.data(), rp_out.data(), out.data(), n_out);
    expect("lgc_reduce_concat_host", rc, 0);
    if (rc != 0) return;
    expect("rowptr_out[0]", rp_out[0], 0);
    expect("rowptr_out[last]", rp_out[n_phys + n_items], n_out);
    for (int64_t r = 0; r < n_phys + n_items; ++r)
        if (rp_out[r + 1] < rp_out[r]) { expect("rowptr_out ascends", rp_out[r + 1], rp_out[r]); break; }
    std::vector<char> owned(n_phys, 0);
    for (int h = 0; h < n_kept; ++h) {
        if (pos[h] < 0 || pos[h] >= n_phys || owned[pos[h]]++) { expect("user_pos in range, once", pos[h], -1); break; }
        expect("a user's row keeps its length", rp_out[pos[h] + 1] - rp_out[pos[h]], rp[h + 1] - rp[h]);
    }
    for (int j = 0; j < n_items; ++j) {
        const int64_t row = (int64_t)gap_start[j / gap_rows] + j % gap_rows;
        if (row < 0 || row >= n_phys || owned[row]++) { expect("gap row in range, once", row, -1); break; }
        expect("a gap row holds one entry", rp_out[row + 1] - rp_out[row], 1);
        expect("... its item", out[rp_out[row]].col, n_phys + j);
        const int r = n_kept + j;
        expect("an item row keeps both lengths", rp_out[n_phys + j + 1] - rp_out[n_phys + j], (rp[r + 1] - rp[r]) + (grp[r + 1] - grp[r]));
    }
    for (int64_t r = 0; r < n_phys + n_items; ++r)
        for (int32_t e = rp_out[r]; e < rp_out[r + 1]; ++e) {
            const bool ok = r < n_phys ? (out[e].col >= n_phys && out[e].col < n_phys + n_items) : (out[e].col >= 0 && out[e].col < n_phys && owned[out[e].col]);
            if (!ok) { expect("every entry written, column on the other side and owned", out[e].col, -2); return; }
        }
}

int main() {
    std::mt19937 rng(20240611);
    const int shapes[][4] = {{0, 30, 8, 12}, {200, 30, 8, 9}, {37, 9, 8, 6}, {60, 6, 8, 5}, {1, 1, 1, 3}, {5, 70, 64, 4}, {300, 40, 3, 0},
                             {17, 33, 8, 40}, {1000, 257, 8, 7}};
    for (const auto &s : shapes)
        for (int rep = 0; rep < 3; ++rep) run_case(rng, s[0], s[1], s[2], s[3]);

    alignas(16) static int32_t word[4];
    lgc_entry *ents = reinterpret_cast<lgc_entry *>(word);
    expect("host: null rowptr", lgc_reduce_concat_host(nullptr, ents, 2, word, ents, 1, 1, 1, 1, word, word, word, ents, 4), LGC_E_INVAL);
    expect("host: n_out", lgc_reduce_concat_host(word, ents, 2, word, ents, 1, 1, 1, 1, word, word, word, ents, 5), LGC_E_INVAL);
    expect("host: n_gaps 65", lgc_reduce_concat_host(word, ents, 2, word, ents, 1, 1, 1, 65, word, word, word, ents, 4), LGC_E_RANGE);
    expect("host: rowptr disagrees with n_entries", lgc_reduce_concat_host(word, ents, 2, word, ents, 0, 1, 1, 1, word, word, word, ents, 3),
           LGC_E_INVAL);
    expect("device: null outputs", lgc_reduce_concat(word, ents, 2, word, ents, 1, 1, 1, 1, word, word, nullptr, ents, 4, nullptr), LGC_E_INVAL);
    expect("device: no items", lgc_reduce_concat(word, ents, 2, word, ents, 1, 1, 0, 1, word, word, word, ents, 3, nullptr), LGC_E_INVAL);
    expect("device: too many rows", lgc_reduce_concat(word, ents, 2, word, ents, 1, (int64_t)1 << 31, 1, 1, word, word, word, ents, 4, nullptr),
           LGC_E_RANGE);
    expect("rows: bad gaps", lgc_reduce_concat_rows(4, 6, 0), -1);

    if (failures) {
        std::fprintf(stderr, "%d unexpected results\n", failures);
        return 1;
    }
    std::puts("asan_reduce_host: the host builder stayed inside its buffers and every invariant held");
    return 0;
}

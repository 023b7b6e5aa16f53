// The argument checks of lgc_bfs_init / _level / _resolve / _backtrack (include/lgconv_hip.h) as a stand-alone host
// program, for tools/asan_paths_host.sh: every call below must return its code before anything is launched, so the
// pointers are never dereferenced and no GPU is needed.  Exit status 0 = every code as expected.
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

int main() {
    // addresses of host words: valid, aligned, and never read or written by a call that returns before its launch
    static int64_t i64[4];
    static uint64_t u64[4], u64b[4];
    static int32_t i32[4];
    static lgc_entry ent[1];
    static lgc_chunk chk[1];
    const int64_t big = INT32_MAX;

    expect("init null sources", lgc_bfs_init(nullptr, 1, 8, u64, u64b, i32, nullptr), LGC_E_INVAL);
    expect("init null seen", lgc_bfs_init(i64, 1, 8, nullptr, u64b, i32, nullptr), LGC_E_INVAL);
    expect("init null frontier", lgc_bfs_init(i64, 1, 8, u64, nullptr, i32, nullptr), LGC_E_INVAL);
    expect("init null status", lgc_bfs_init(i64, 1, 8, u64, u64b, nullptr, nullptr), LGC_E_INVAL);
    expect("init negative sources", lgc_bfs_init(i64, -1, 8, u64, u64b, i32, nullptr), LGC_E_INVAL);
    expect("init negative nodes", lgc_bfs_init(i64, 1, -8, u64, u64b, i32, nullptr), LGC_E_INVAL);
    expect("init 65 sources", lgc_bfs_init(i64, LGC_BFS_MAX_SOURCES + 1, 8, u64, u64b, i32, nullptr), LGC_E_RANGE);
    expect("init 2^31 nodes", lgc_bfs_init(i64, 1, big, u64, u64b, i32, nullptr), LGC_E_RANGE);
    expect("init no sources", lgc_bfs_init(i64, 0, 8, u64, u64b, i32, nullptr), 0);

    expect("level null rowptr", lgc_bfs_level(nullptr, ent, 0, 8, 32, chk, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level null entries", lgc_bfs_level(i32, nullptr, 0, 8, 32, chk, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level null frontier_in", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 1, nullptr, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level null frontier_out", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 1, u64, nullptr, u64, u64, nullptr), LGC_E_INVAL);
    expect("level null seen", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 1, u64, u64b, nullptr, u64, nullptr), LGC_E_INVAL);
    expect("level null counters", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 1, u64, u64b, u64, nullptr, nullptr), LGC_E_INVAL);
    expect("level chunks missing", lgc_bfs_level(i32, ent, 0, 8, 32, nullptr, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level negative chunks", lgc_bfs_level(i32, ent, 0, 8, 32, chk, -1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level negative short_max", lgc_bfs_level(i32, ent, 0, 8, -1, chk, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level rows reversed", lgc_bfs_level(i32, ent, 8, 0, 32, chk, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_INVAL);
    expect("level in == out", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 1, u64, u64, u64, u64, nullptr), LGC_E_INVAL);
    expect("level 2^31 rows", lgc_bfs_level(i32, ent, 0, INT32_MAX, 32, chk, 1, 1, u64, u64b, u64, u64, nullptr), LGC_E_RANGE);
    expect("level no rows", lgc_bfs_level(i32, ent, 4, 4, 32, chk, 1, 1, u64, u64b, u64, u64, nullptr), 0);
    expect("level no active source", lgc_bfs_level(i32, ent, 0, 8, 32, chk, 1, 0, u64, u64b, u64, u64, nullptr), 0);

    expect("resolve null sources", lgc_bfs_resolve(nullptr, i64, 1, 1, 8, u64, 0, i32, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve null targets", lgc_bfs_resolve(i64, nullptr, 1, 1, 8, u64, 0, i32, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve null frontier", lgc_bfs_resolve(i64, i64, 1, 1, 8, nullptr, 0, i32, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve null dist", lgc_bfs_resolve(i64, i64, 1, 1, 8, u64, 0, nullptr, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve null counters", lgc_bfs_resolve(i64, i64, 1, 1, 8, u64, 0, i32, nullptr, i32, nullptr), LGC_E_INVAL);
    expect("resolve null status", lgc_bfs_resolve(i64, i64, 1, 1, 8, u64, 0, i32, u64b, nullptr, nullptr), LGC_E_INVAL);
    expect("resolve negative level", lgc_bfs_resolve(i64, i64, 1, 1, 8, u64, -1, i32, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve negative targets", lgc_bfs_resolve(i64, i64, 1, -1, 8, u64, 0, i32, u64b, i32, nullptr), LGC_E_INVAL);
    expect("resolve 65 sources", lgc_bfs_resolve(i64, i64, 65, 1, 8, u64, 0, i32, u64b, i32, nullptr), LGC_E_RANGE);
    expect("resolve 2^31 nodes", lgc_bfs_resolve(i64, i64, 1, 1, big, u64, 0, i32, u64b, i32, nullptr), LGC_E_RANGE);
    expect("resolve 2^31 targets", lgc_bfs_resolve(i64, i64, 1, big, 8, u64, 0, i32, u64b, i32, nullptr), LGC_E_RANGE);
    expect("resolve no sources", lgc_bfs_resolve(i64, i64, 0, 1, 8, u64, 0, i32, u64b, i32, nullptr), 0);
    expect("resolve no targets", lgc_bfs_resolve(i64, i64, 1, 0, 8, u64, 0, i32, u64b, i32, nullptr), 0);

    expect("backtrack null rowptr", lgc_bfs_backtrack(nullptr, ent, 8, u64, 1, i64, i32, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack null entries", lgc_bfs_backtrack(i32, nullptr, 8, u64, 1, i64, i32, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack null levels", lgc_bfs_backtrack(i32, ent, 8, nullptr, 1, i64, i32, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack null targets", lgc_bfs_backtrack(i32, ent, 8, u64, 1, nullptr, i32, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack null dist", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, nullptr, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack null paths", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 1, 1, nullptr, 1, nullptr), LGC_E_INVAL);
    expect("backtrack no levels", lgc_bfs_backtrack(i32, ent, 8, u64, 0, i64, i32, 1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack no path_len", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 1, 1, i64, 0, nullptr), LGC_E_INVAL);
    expect("backtrack negative sources", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, -1, 1, i64, 1, nullptr), LGC_E_INVAL);
    expect("backtrack 65 sources", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 65, 1, i64, 1, nullptr), LGC_E_RANGE);
    expect("backtrack 2^31 nodes", lgc_bfs_backtrack(i32, ent, big, u64, 1, i64, i32, 1, 1, i64, 1, nullptr), LGC_E_RANGE);
    expect("backtrack 2^31 targets", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 1, big, i64, 1, nullptr), LGC_E_RANGE);
    expect("backtrack no sources", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 0, 1, i64, 1, nullptr), 0);
    expect("backtrack no targets", lgc_bfs_backtrack(i32, ent, 8, u64, 1, i64, i32, 1, 0, i64, 1, nullptr), 0);

    std::printf("lgc_bfs_* argument checks: %d failure(s)\n", failures);
    return failures != 0;
}

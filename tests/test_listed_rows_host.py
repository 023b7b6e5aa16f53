"""The listed-rows hop's small operators, row lists and references hold what they promise (tests/listed_rows_support.py);
nothing here needs a device.

1. every operator and every named list has the property it exists for;
2. the plan arithmetic never asks for more chunks than the partial table holds -- the cap ``k_rows_chunks`` relies on when it
   writes slot w -- for every list and every ``partial_rows`` the device tests use;
3. the fp32 emulation stays inside the running-sum bound of tests/test_tiles_host.py against fp64 for every row of every
   operator, at every width and epilogue, for the whole-row spans and for rows cut at 256, 320 and 4096 entries;
4. hand-worked roundings in which the grouped order and the stored order give different bits;
5. ``lgc_spmm_rows_split`` refuses a ``partials`` pointer that is not dword aligned.
"""
import ctypes

import numpy as np
import pytest

import listed_rows_support as S
import tiles_support as T

OPS = S.operators()
LISTS = S.lists()
ROOMS = S.TIGHT_ROOMS + (S.DEFAULT_ROOM,)


def longest_foreign_run_between_long_rows(op, ids):
    """The longest run of consecutive foreign ids whose two neighbours are rows of more than 32 entries."""
    foreign = S.is_foreign(op, ids)
    best, m = 0, 0
    while m < len(ids):
        if not foreign[m]:
            m += 1
            continue
        end = m
        while end < len(ids) and foreign[end]:
            end += 1
        if m > 0 and end < len(ids) and op.lengths[ids[m - 1]] > S.SHORT_MAX and op.lengths[ids[end]] > S.SHORT_MAX:
            best = max(best, end - m)
        m = end
    return best


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def test_names_sizes_and_value_ranges():
    assert tuple(OPS) == S.OP_NAMES and tuple(LISTS) == S.LIST_NAMES
    for op in OPS.values():
        assert op.rowptr.size == op.table_rows + 1 and op.cols.dtype == np.int32 and op.vals.dtype == np.float32
        assert 0 < op.row_begin < op.row_end < op.table_rows                     # ids below and above the range exist
        assert op.cols.min() >= 0 and op.cols.max() < S.COLUMN_ROWS <= op.table_rows
        assert np.unique(op.cols).size < op.cols.size                            # drawn with repeats
        assert np.all(np.abs(op.vals) >= 2.0 ** -6) and np.all(np.abs(op.vals) < 2.0 ** 6)
        assert op.lengths[:op.row_begin].max() > S.CHUNK_LEN and op.lengths[op.row_end:].max() > S.CHUNK_LEN   # foreign rows have entries
    assert {S.groups_of(d) for d in S.DIMS} == {64, 21, 16, 32, 4, 3, 2, 1} == {S.groups_of(d) for d in S.ONE_DIM_PER_GROUPS}
    assert {S.groups_of(d) for d in S.NARROW_DIMS} == {64}
    assert set((1, 3, 4, 7, 64, 65, 90, 128, 129, 256)) <= set(S.DIMS)
    assert [S.lanes_per_row(d) for d in (1, 3, 4, 7, 90, 129, 256)] == [1, 3, 1, 2, 23, 33, 64]
    assert 64 % S.lanes_per_row(3) != 0 and 4 * S.lanes_per_row(7) > 7 and 4 * S.lanes_per_row(90) > 90   # idle lane, overlaps


def test_lengths_holds_every_length_twice():
    op = OPS["lengths"]
    deg = sorted(op.lengths[op.row_begin:op.row_end].tolist())
    assert deg == sorted((S.SWITCH_LENGTHS + S.ONE_CHUNK_LENGTHS + S.BOUNDARY_LENGTHS + S.HUB_LENGTHS) * 2)
    for n in (0, 1, 3, 4, 5, 31, 32, 33, 34, 63, 64, 65, 192, 193, 255, 256, 257, 511, 512, 513, 768):
        assert len(S.rows_of_length(op, n)) == 2, n
    assert op.lengths[op.row_begin:op.row_end].tolist() != deg                  # shuffled row order


@pytest.mark.parametrize("dim", S.DIMS)
def test_a_hub_runs_the_four_slot_loop_of_the_combine_and_leaves_a_tail(dim):
    """``combine_core``: lane group g takes slots g, g + G, ..: four per trip while s + 3 G < slots, then one by one."""
    groups = S.groups_of(dim)
    name = "wide_hub" if groups == 64 else "lengths"
    length = S.hub_length(groups)
    assert len(S.rows_of_length(OPS[name], length)) >= 1
    slots = -(-length // S.CHUNK_LEN)
    assert slots == S.hub_chunks(groups) > 4 * groups and length % S.CHUNK_LEN != 0
    trips = [0] * groups
    tails = [0] * groups
    for g in range(groups):
        s = g
        while s + 3 * groups < slots:
            trips[g] += 1
            s += 4 * groups
        while s < slots:
            tails[g] += 1
            s += groups
    assert min(trips) >= 1 and max(tails) >= 1
    if groups > 2:
        assert min(tails) == 0                                   # and some groups end with the loop


def test_many_short_holds_more_than_8192_rows_of_at_most_8_entries():
    op = OPS["many_short"]
    deg = op.lengths[op.row_begin:op.row_end]
    assert (deg <= 8).sum() > S.GRID_WAVES and set(deg[deg <= 8].tolist()) == set(range(9))
    assert sorted(deg[deg > 8].tolist()) == sorted(S.MANY_SHORT_LONG) and min(S.MANY_SHORT_LONG) > S.CHUNK_LEN


# ---------------------------------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------------------------------
def test_each_once_and_reversed():
    op = OPS["lengths"]
    assert LISTS["each_once"].ids.tolist() == list(op.range_rows())
    assert LISTS["reversed"].ids.tolist() == list(op.range_rows())[::-1]
    wide = OPS["wide_hub"]
    assert LISTS["wide_each_once"].ids.tolist() == list(wide.range_rows())


@pytest.mark.parametrize("name", ("repeats", "wide_repeats"))
def test_repeats_names_a_hub_a_257_row_and_a_5_row_three_times_each_adjacent_and_apart(name):
    rl = LISTS[name]
    op = OPS[rl.op]
    ids = rl.ids.tolist()
    deg = op.lengths
    hub = max(ids, key=lambda r: deg[r] if not S.is_foreign(op, [r])[0] else -1)
    assert deg[hub] == (S.WIDE_HUB_LENGTH if rl.op == "wide_hub" else max(S.HUB_LENGTHS))
    for row in (hub, S.rows_of_length(op, 257)[0], S.rows_of_length(op, 5)[0]):
        at = [m for m, r in enumerate(ids) if r == row]
        assert len(at) == 3, row
    for row in (hub, S.rows_of_length(op, 5)[0]):
        at = [m for m, r in enumerate(ids) if r == row]
        gaps = np.diff(at)
        assert gaps.min() == 1 and gaps.max() > 1, row
    at = [m for m, r in enumerate(ids) if r == S.rows_of_length(op, 257)[0]]
    assert np.diff(at).min() > 1


def test_foreign_lists_hold_every_kind_at_the_ends_and_in_long_runs():
    op = OPS["lengths"]
    head, tail, runs = (LISTS[n].ids for n in ("foreign_head", "foreign_tail", "foreign_runs"))
    for ids in (head, tail, runs, LISTS["all_foreign"].ids):
        f = ids[S.is_foreign(op, ids)]
        assert (f < 0).any() and ((f >= 0) & (f < op.row_begin)).any() and ((f >= op.row_end) & (f < op.table_rows)).any()
        assert (f >= op.table_rows).any() and (f >= 2 ** 31).any() and (f < -2 ** 31).any()
    assert S.is_foreign(op, head[:66]).all() and not S.is_foreign(op, head[66:]).any()
    assert S.is_foreign(op, tail[-66:]).all() and not S.is_foreign(op, tail[:-66]).any()
    assert S.is_foreign(op, runs[[0, -1]]).all()
    assert longest_foreign_run_between_long_rows(op, runs) >= 130
    foreign = S.is_foreign(op, runs)
    run_lengths = [len(run) for run in "".join("f" if f else "r" for f in foreign).split("r") if run]
    assert sorted(run_lengths)[-4:] == [64, 65, 70, 130]          # one probe step of the search is at most 64 positions wide
    assert S.is_foreign(op, LISTS["all_foreign"].ids).all() and LISTS["all_foreign"].n_ids == 70
    assert S.plan(op, LISTS["all_foreign"].ids, 70 + S.DEFAULT_ROOM).tolist() == [0] * 71 + [S.CHUNK_LEN]
    wide = OPS["wide_hub"]
    assert S.is_foreign(wide, LISTS["wide_repeats"].ids).sum() == 3


def test_single_position_lists():
    op = OPS["lengths"]
    for name, length, chunks in (("one_0", 0, 1), ("one_32", 32, 1), ("one_33", 33, 1), ("one_hub", max(S.HUB_LENGTHS), S.hub_chunks(32))):
        rl = LISTS[name]
        assert rl.n_ids == 1 and op.lengths[rl.ids[0]] == length
        assert S.plan(op, rl.ids, 1 + S.DEFAULT_ROOM).tolist() == [0, chunks, S.CHUNK_LEN]
    rl = LISTS["one_wide_hub"]
    assert rl.n_ids == 1 and S.plan(OPS["wide_hub"], rl.ids, 1 + S.DEFAULT_ROOM).tolist() == [0, S.hub_chunks(64), S.CHUNK_LEN]


def test_only_short_is_one_chunk_per_position():
    rl = LISTS["only_short"]
    op = OPS[rl.op]
    assert (op.lengths[rl.ids] <= S.SHORT_MAX).all() and set(op.lengths[rl.ids].tolist()) == {0, 1, 3, 4, 5, 31, 32}
    for room in ROOMS:
        assert S.plan(op, rl.ids, rl.n_ids + room)[:rl.n_ids + 1].tolist() == list(range(rl.n_ids + 1))


@pytest.mark.parametrize("n", S.SIZES)
def test_sized_lists_mix_chunk_counts_and_put_cut_rows_around_every_scan_tile_boundary(n):
    rl = LISTS[f"sized_{n}"]
    op = OPS[rl.op]
    assert rl.n_ids == n
    c = S.chunk_counts(op, rl.ids, S.CHUNK_LEN)
    assert (c > 1).any() and (c == 0).any()
    if n > 2:
        assert (c == 1).any()
    for edge in range(S.SCAN_TILE, n + 1, S.SCAN_TILE):
        assert c[edge - 1] > 1
        if edge < n:
            assert c[edge] > 1
        if edge + 1 < n:
            assert c[edge + 1] == 0
    assert S.chunk_length(op, rl.ids, n + S.DEFAULT_ROOM) == S.CHUNK_LEN
    # rounds of the 64-ary search over [0, n): the range shrinks to ceil(range / 64) per round
    rounds, span = 0, n
    while span > 1:
        span, rounds = -(-span // S.WAVE), rounds + 1
    assert rounds == (1 if n <= 64 else 2 if n <= 4096 else 3)


def test_sized_lists_cover_one_two_and_three_search_rounds_and_up_to_five_scan_tiles():
    assert {n <= 64 for n in S.SIZES} == {True, False} and max(S.SIZES) > 4096 >= sorted(S.SIZES)[-2]
    assert {-(-n // S.SCAN_TILE) for n in S.SIZES} == {1, 2, 3, 5}


def test_beyond_the_grid_sends_wavefronts_on_a_second_trip_that_writes_slots():
    rl = LISTS["beyond_the_grid"]
    op = OPS[rl.op]
    assert rl.n_ids > S.GRID_WAVES and not S.is_foreign(op, rl.ids).any()
    partial_rows = S.partial_rows_of(rl)
    work = S.plan(op, rl.ids, partial_rows)
    assert work[-1] == S.CHUNK_LEN and work[rl.n_ids] > S.GRID_WAVES
    assert min(partial_rows, 8192) == S.GRID_WAVES               # the fixed grid: 8192 wavefronts
    own = S.owners(work, rl.n_ids)
    second_trip = np.arange(S.GRID_WAVES, int(work[rl.n_ids]))
    counts = np.diff(work[:rl.n_ids + 1])
    assert (counts[own[second_trip]] > 1).any() and (counts[own[second_trip]] == 1).any()
    assert (op.lengths[rl.ids[:S.GRID_WAVES + 1]] <= 8).all()


def test_every_list_runs_at_one_width_per_lane_group_count():
    for name in S.LIST_NAMES:
        dims = S.dims_of(name)
        if LISTS[name].op == "wide_hub":
            assert {S.groups_of(d) for d in dims} == {64}
        else:
            assert {S.groups_of(d) for d in dims} == set(S.ALL_GROUPS)
    for name in S.EVERY_WIDTH_LISTS:
        assert S.dims_of(name) == S.DIMS


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_on_a_list_worked_by_hand():
    op = OPS["lengths"]
    r0, r32, r33, r256, r257, r768 = (S.rows_of_length(op, n)[0] for n in (0, 32, 33, 256, 257, 768))
    ids = np.array([r257, -1, r0, r768, op.row_end, r33, r32, 2, r256], np.int64)
    #                2     0   1    3        0        1    1   0    1
    assert S.plan(op, ids, 9 + S.DEFAULT_ROOM).tolist() == [0, 2, 2, 3, 6, 6, 7, 8, 8, 9, 256]
    assert S.owners(S.plan(op, ids, 9 + S.DEFAULT_ROOM), 9).tolist() == [0, 0, 2, 3, 3, 3, 5, 6, 8]
    # 1346 entries: room 5 holds 1346 // 256 = 5, room 4 does not: ceil(1346 / 4) = 337 -> 384
    assert sum((257, 0, 768, 33, 32, 256)) == 1346
    assert S.plan(op, ids, 9 + 5)[-1] == 256
    assert S.plan(op, ids, 9 + 4).tolist() == [0, 1, 1, 2, 4, 4, 5, 6, 6, 7, 384]
    assert S.plan(op, ids, 9 + 1).tolist() == [0, 1, 1, 2, 3, 3, 4, 5, 5, 6, 1408]


@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_the_plan_never_exceeds_the_partial_table(name):
    """sum ceil(len / L) <= total / L + n_ids: with L = 256 and total // 256 <= room that is below room + 1 + n_ids, with
    L >= total / room at most room + n_ids -- the partial table's rows either way."""
    rl = LISTS[name]
    op = OPS[rl.op]
    for room in ROOMS:
        partial_rows = rl.n_ids + room
        work = S.plan(op, rl.ids, partial_rows)
        L = int(work[-1])
        assert L >= S.CHUNK_LEN and L % S.WAVE == 0
        assert 0 <= work[rl.n_ids] <= partial_rows, (room, L)
        assert (np.diff(work[:rl.n_ids + 1]) >= 0).all()
        own = S.owners(work, rl.n_ids)
        assert not S.is_foreign(op, rl.ids[own]).any()                            # no chunk belongs to a foreign id
        brute = [max(m for m in range(rl.n_ids) if work[m] <= w) for w in range(0, int(work[rl.n_ids]), 97)]
        assert own[::97].tolist() == brute


def test_tight_tables_lengthen_the_chunks_and_still_cut_rows():
    """What test_tight_tables on the device runs: lists whose chunk length grows at room 1, 2 or 8, some of them with rows
    that are still cut."""
    lengthened, still_cut = set(), set()
    for name in S.LIST_NAMES:
        rl = LISTS[name]
        op = OPS[rl.op]
        for room in S.TIGHT_ROOMS:
            work = S.plan(op, rl.ids, rl.n_ids + room)
            if work[-1] > S.CHUNK_LEN:
                lengthened.add((name, room))
                if (np.diff(work[:rl.n_ids + 1]) > 1).any():
                    still_cut.add((name, room))
    assert {"each_once", "repeats", "one_hub", "foreign_runs", "sized_1025", "beyond_the_grid", "one_wide_hub"} <= {n for n, _ in lengthened}
    assert {r for _, r in still_cut} >= {2, 8} and len({n for n, _ in still_cut}) >= 6
    assert S.plan(OPS["lengths"], LISTS["one_hub"].ids, 1 + 8)[1] == 8 and S.plan(OPS["lengths"], LISTS["one_hub"].ids, 1 + 1)[1] == 1


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("name", S.OP_NAMES)
def test_emulation_is_within_the_running_sum_bound(name, dim):
    """Per element  |emulation - fp64| <= (n + 2) * 2^-24 * (|a| * sum |val * x| + |b * r|)  for a row of n entries -- the
    bound test_tiles_host.py derives for the stored order.  It holds for the grouped order too: there a product passes
    through the additions of its lane group (at most ceil(n / groups) - 1 that round, the first is to +0), of the group
    sums (at most groups - 1), and for a cut row of the chunk sums in their group and of those groups -- never more than
    n - 1 roundings, since every addition that rounds merges two non-empty sets of the row's entries, and n entries can be merged
    n - 1 times."""
    op = OPS[name]
    rows = np.arange(op.row_begin, op.row_end)
    worst = 0.0
    for L in (None,) + S.CUT_LENS:
        if L is not None and not S.cut_rows(name, dim, L):
            continue
        for epilogue in S.EPILOGUES:
            got = S.finished(name, dim, L, rows, epilogue)
            want, mag, n = S.evaluate_fp64(name, dim, epilogue)
            assert got.dtype == np.float32 and got.shape == want.shape
            bound = (n[:, None] + 2) * 2.0 ** -24 * mag
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (name, dim, L, epilogue)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert 0.0 < worst <= 1.0                    # the emulation rounds: it is not the fp64 value
    assert S.cut_rows(name, dim, 256) and (name == "many_short" or S.cut_rows(name, dim, 4096))


@pytest.mark.parametrize("dim", (1, 7, 90, 256))
def test_rows_of_up_to_32_entries_follow_the_rule_of_the_tile_path(dim):
    """The bits of ``tiles_support.emulate``, which ``lgc_spmm_tiles`` is held to: the three entry points agree on them."""
    op = OPS["lengths"]
    rows = [r for r in op.range_rows() if op.lengths[r] <= S.SHORT_MAX]
    x, r = S.table_values("lengths", dim, "x"), S.table_values("lengths", dim, "r")
    for L in (None, 256, 320):
        for epilogue in S.EPILOGUES:
            a, with_r, b = epilogue
            want = T.emulate(op, x, rows, a, r if with_r else None, b)
            assert np.array_equal(T.bits(S.finished("lengths", dim, L, rows, epilogue)), T.bits(want))


def test_rows_of_one_chunk_do_not_depend_on_the_chunk_length():
    op = OPS["lengths"]
    rows = np.array([r for r in op.range_rows() if op.lengths[r] <= 256])
    assert {33, 34, 255, 256} <= set(op.lengths[rows].tolist())
    for dim in (4, 65):
        whole = S.accumulated("lengths", dim, None)
        assert np.array_equal(T.bits(S.accumulated("lengths", dim, 256)[rows - op.row_begin]), T.bits(whole[rows - op.row_begin]))
        cut = np.array(sorted(S.cut_rows("lengths", dim, 256)))
        assert (op.lengths[cut] > 256).all() and cut.size == 2 * (5 + len(S.HUB_LENGTHS))
        if S.groups_of(dim) > 1:        # another association: other bits in nearly every element
            differ = T.bits(S.accumulated("lengths", dim, 256)[cut - op.row_begin]) != T.bits(whole[cut - op.row_begin])
            assert differ.mean() > 0.25


def _hand_op(n, table_rows=None):
    """One row of ``n`` entries, entry k naming table row k with value 1."""
    table_rows = table_rows or n
    rowptr = np.array([0] + [n] * table_rows, np.int64)
    return T.TileOp("hand", rowptr, np.arange(n, dtype=np.int32), np.ones(n, np.float32), 0, 1, table_rows)


def test_hand_worked_grouped_and_stored_order_give_different_bits():
    """Terms 1, 2^-24, 2^-24, ..: in stored order every addition is a tie that rounds back to the even 1.  Two lane groups:
    group 0 holds 1 and every second small term and stays 1 the same way, group 1 adds its small terms exactly, and
    1 + 17 * 2^-24 is 8.5 ulps above 1: a tie that rounds to the even 1 + 8 * 2^-23."""
    tiny = np.float32(2.0 ** -24)
    terms = np.full((4, 1), tiny, np.float32)
    terms[0] = 1.0
    assert T.bits(S.sequential(terms)).tolist() == [0x3F800000]
    assert T.bits(S.grouped(terms, 2)).tolist() == [0x3F800001]                 # 1 and 2^-24 | 2^-24 + 2^-24 = one ulp
    assert T.bits(S.grouped(terms, 1)).tolist() == [0x3F800000] and T.bits(S.grouped(terms, 64)).tolist() == [0x3F800000]
    # the switch at 32 entries, through the row functions: 128 columns are two lane groups
    dim = 128
    assert S.groups_of(dim) == 2
    x = np.full((34, dim), tiny, np.float32)
    x[0] = 1.0
    assert T.bits(S.whole_row(_hand_op(32, 34), x, 0, 2)).tolist() == [0x3F800000] * dim       # 32 entries: stored order
    assert T.bits(S.whole_row(_hand_op(33, 34), x, 0, 2)).tolist() == [0x3F800008] * dim       # group 1: 16 terms, 1 + 2^-20
    assert T.bits(S.whole_row(_hand_op(34), x, 0, 2)).tolist() == [0x3F800008] * dim           # 17 terms: the tie above
    assert T.bits(S.whole_row(_hand_op(34), x, 0, 1)).tolist() == [0x3F800000] * dim           # one group: stored order again
    assert T.bits(T.accumulate(_hand_op(34), x, [0])[0]).tolist() == [0x3F800000] * dim


def test_hand_worked_cut_row():
    """130 entries cut at 64 with one lane group: chunk 0 is 1 (63 ties), chunk 1 is 64 * 2^-24 = 2^-18, chunk 2 is 2^-23;
    their sum 1 + 2^-18 + 2^-23 is exact, while the whole row in stored order stays 1.  With two lane groups the last
    chunk goes to group 0 with the first: (1 + 2^-23) + 2^-18."""
    x = np.full((130, 4), np.float32(2.0 ** -24), np.float32)
    x[0] = 1.0
    op = _hand_op(130)
    assert S.chunk_bounds(op, 0, 64) == [(0, 64), (64, 128), (128, 130)]
    sums, combined = S.cut_row(op, x, 0, 64, 1)
    assert T.bits(sums[:, 0]).tolist() == T.bits(np.array([1.0, 2.0 ** -18, 2.0 ** -23], np.float32)).tolist()
    assert T.bits(combined).tolist() == [0x3F800021] * 4
    assert T.bits(S.whole_row(op, x, 0, 1)).tolist() == [0x3F800000] * 4
    sums2, combined2 = S.cut_row(op, x, 0, 64, 2)
    # two groups inside a chunk: chunk 0 = 1 + 32 * 2^-24 = 1 + 2^-19
    assert T.bits(sums2[:, 0]).tolist() == T.bits(np.array([1.0 + 2.0 ** -19, 2.0 ** -18, 2.0 ** -23], np.float32)).tolist()
    assert T.bits(combined2).tolist() == [0x3F800000 + 16 + 1 + 32] * 4
    # a chunk length that ends the row exactly: no empty last chunk
    assert S.chunk_bounds(op, 0, 65) == [(0, 65), (65, 130)]


def test_expected_tables_mark_what_is_written():
    rl = LISTS["foreign_runs"]
    op = OPS[rl.op]
    dim = 7
    _, y_stride, _ = S.strides_of("padded", dim)
    inside = S.listed_range_rows(rl)
    y = S.expected_y(rl, dim, y_stride, 256, S.EPILOGUES[1])
    written = np.unique(inside)
    assert y.shape == (op.table_rows + S.GUARD_ROWS, y_stride)
    assert (y[written, :dim] != S.SENTINEL).all() and (y[:, dim:] == S.SENTINEL).all()
    assert (np.delete(y, written, axis=0) == S.SENTINEL).all()
    yc = S.expected_y(rl, dim, y_stride, 256, S.EPILOGUES[1], compact=True)
    at = np.flatnonzero(~S.is_foreign(op, rl.ids))
    assert yc.shape == (rl.n_ids + S.GUARD_ROWS, y_stride) and np.array_equal(yc[at, :dim], y[rl.ids[at], :dim])
    assert (np.delete(yc, at, axis=0) == S.SENTINEL).all() and (yc[:, dim:] == S.SENTINEL).all()
    partial_rows = S.partial_rows_of(rl)
    slots, want, total = S.expected_partials(rl, dim, partial_rows)
    work = S.plan(op, rl.ids, partial_rows)
    counts = np.diff(work[:rl.n_ids + 1])
    assert total == work[rl.n_ids] and slots.size == counts[counts > 1].sum() == want.shape[0] and want.shape[1] == dim
    assert slots.tolist() == [w for m in np.flatnonzero(counts > 1) for w in range(work[m], work[m + 1])]
    assert S.expected_work(rl, partial_rows)[:rl.n_ids + 2].tolist() == work.tolist()
    for layout in S.LAYOUTS:
        for d in S.DIMS:
            xs, ys, rs = S.strides_of(layout, d)
            assert min(xs, ys, rs) >= d
            if layout == "padded":
                assert len({xs, ys, rs}) == 3 and min(xs, ys, rs) > d
            if layout == "odd":
                assert ys % 2 == 1 and rs % 2 == 1 and ys > d
    t = S.input_table("lengths", dim, "r", 11, keep=written)
    assert np.isnan(t[:, dim:]).all() and not np.isnan(t[written, :dim]).any() and np.isnan(t).sum() == t.size - written.size * dim


# ---------------------------------------------------------------------------------------------------------------------
# argument check
# ---------------------------------------------------------------------------------------------------------------------
def test_a_partial_table_that_is_not_dword_aligned_is_refused():
    from gnn_ecommerce_amd import _native
    lib = _native.load()
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(512)        # never dereferenced: validation comes first
    split = lambda part, compact=0: lib.lgc_spmm_rows_split(one, one, 0, 4, one, 3, 8, one, 64, two, 64, 8, None, 0, 1.0, 0.0, 64,
                                                            compact, one, part, 100, None)
    for address in (1026, 1025, 1027):
        assert split(ctypes.c_void_p(address)) == -5 and split(ctypes.c_void_p(address), 1) == -5

"""The tile path's small operators, references and case table hold what they promise (tests/tiles_support.py); nothing
here needs a device.

1. every named operator has the property it exists for;
2. the GPU case table reaches every (kernel body, class width) pair and every tiles_per_wave, computed from the table
   and the route rule;
3. ``graph.plan_tile_classes`` keeps its invariants on every operator, order and ``max_len``;
4. the fp32 emulation stays inside the running-sum bound against fp64 (``test_emulation_is_within_the_running_sum_bound``
   derives it) and reproduces two cases worked by hand.
"""
import numpy as np
import pytest

import tiles_support as S

OPS = S.operators()


def classes_by_width(op):
    return {w: (order, meta) for w, order, meta in S.kernel_classes(op)}


def test_names_and_sizes():
    assert tuple(OPS) == S.NAMES
    for op in OPS.values():
        assert op.rowptr.size == op.table_rows + 1 and op.cols.dtype == np.int32 and op.vals.dtype == np.float32
        assert 0 <= op.row_begin <= op.row_end <= op.table_rows
        if not op.name.startswith("many_tiles"):
            assert op.row_end - op.row_begin <= 64, op.name
        assert np.all(np.abs(op.vals) >= 2.0 ** -6) and np.all(np.abs(op.vals) < 2.0 ** 6)
    x = S.table_values("one_over", 20, "x")
    assert np.all(np.abs(x) >= 2.0 ** -6) and np.all(np.abs(x) < 2.0 ** 6) and {-1.0, 1.0} == set(np.sign(x).ravel())


def test_one_row_is_one_tile_with_15_padding_slots():
    op = OPS["one_row"]
    (w, order, meta), = S.kernel_classes(op)
    assert w == 8 and order.size == 16 and S.padding_slots(order) == 15 and meta.tolist() == [1]
    assert S.owned_rows(order).tolist() == [0]


def test_all_empty_takes_the_no_entries_branch_and_is_still_planned():
    op = OPS["all_empty"]
    assert op.rowptr[op.row_end] == op.rowptr[op.row_begin] and op.cols.size == 0
    for mode in S.ORDERS:
        (w, order, meta), = S.planned_classes(op, mode)
        assert w == 8 and meta.tolist() == [0, 0] and S.padding_slots(order) == 12
        assert S.owned_rows(order).tolist() == list(range(20))           # the output of an empty row is still written


def test_exact_tiles_has_no_padding_slot_and_one_over_a_second_tile_of_one_row():
    exact, over = classes_by_width(OPS["exact_tiles"]), classes_by_width(OPS["one_over"])
    for w in S.WIDTHS:
        R = S.geometry(w)[1]
        order, meta = exact[w]
        assert order.size == R and S.padding_slots(order) == 0 and meta.size == 1
        order, meta = over[w]
        assert order.size == 2 * R and meta.size == 2
        assert (order[:R] >= 0).all() and (order[R:] >= 0).sum() == 1


def test_only_wide_has_no_class_8_and_no_class_16():
    op = OPS["only_wide"]
    for mode in S.ORDERS:
        assert [w for w, _, _ in S.planned_classes(op, mode)] == [32]
    assert op.lengths[:op.row_end].min() >= 17


def test_length_edges_holds_every_length_twice_and_three_chunk_plan_rows():
    op = OPS["length_edges"]
    deg = op.lengths[op.row_begin:op.row_end]
    assert sorted(deg.tolist()) == sorted(S.EDGE_LENGTHS * 2 + S.LONG_LENGTHS)
    assert sorted(n for _, n in S.chunk_rows(op)) == [1, 1, 2]            # 33 and 64 in one chunk, 300 in two
    owned = np.concatenate([S.owned_rows(order) for _, order, _ in S.kernel_classes(op)])
    assert sorted(owned.tolist()) == S.tiled_rows(op).tolist() and len(owned) == 42
    for other in S.NAMES:
        if other != "length_edges":
            assert S.chunk_rows(OPS[other]) == [], other


def test_lopsided_batches_have_a_meta_byte_far_above_three_of_four_rows():
    op = OPS["lopsided_batches"]
    deg = op.lengths
    got = classes_by_width(op)
    assert sorted(got) == list(S.WIDTHS)
    for w, (order, meta) in got.items():
        _, R, _, _, B = S.geometry(w)
        by = S.meta_bytes(meta, w)
        assert meta.size == 2 and S.padding_slots(order) == 0
        for t in range(2):
            batch0 = sorted(int(deg[order[t * R + g * B]]) for g in range(4))       # slot g * B + bt, bt = 0
            assert batch0 == [1, 1, 1, w] and by[t, 0] == w
            assert by[t, 1:].max() <= 1
    # the planner itself sees the same rows class by class: (W, 1, 1, 1) in one batch only for W = 8
    assert [w for w, _, _ in S.planned_classes(op, "natural")] == list(S.WIDTHS)


def test_item_half_starts_inside_the_table_and_reads_below_its_range():
    op = OPS["item_half"]
    assert op.row_begin > 0 and op.row_begin % 16 != 0 and op.row_end < op.table_rows
    lo, hi = int(op.rowptr[op.row_begin]), int(op.rowptr[op.row_end])
    assert op.cols[lo:hi].max() < op.row_begin
    assert lo > 0 and hi < op.cols.size                                   # rows outside the range have entries too
    assert sorted(w for w, _, _ in S.kernel_classes(op)) == list(S.WIDTHS)
    owned = np.concatenate([S.owned_rows(order) for _, order, _ in S.kernel_classes(op)])
    assert sorted(owned.tolist()) == list(op.range_rows())


def test_edge_columns_names_the_first_and_the_last_table_row_only():
    op = OPS["edge_columns"]
    assert set(op.cols.tolist()) == {0, op.table_rows - 1}
    assert any(len(op.row(r)[0]) > 2 for r in op.range_rows())            # hence repeats inside a row
    assert sorted(w for w, _, _ in S.kernel_classes(op)) == list(S.WIDTHS)


def test_unread_rows_are_unreferenced():
    op = OPS["unread_rows"]
    assert op.unread == (0, op.table_rows // 2, op.table_rows - 1)
    assert not set(op.cols.tolist()) & set(op.unread)
    for _, order, _ in S.kernel_classes(op):
        a, stride, lead = S.input_arena(op, 20, "dense", "x", S.owned_rows(order))
        x = a.reshape(op.table_rows, 20)
        assert np.isnan(x[list(op.unread)]).all()


@pytest.mark.parametrize("n", S.MANY_TILES)
def test_many_tiles_has_n_tiles_in_every_class(n):
    got = classes_by_width(OPS[f"many_tiles_{n}"])
    assert sorted(got) == list(S.WIDTHS)
    for w, (order, meta) in got.items():
        assert meta.size == n and 0 < S.padding_slots(order) < S.geometry(w)[1]


def test_many_tiles_leaves_wavefronts_without_a_tile_with_a_short_stretch_and_with_one_full_stretch():
    """A workgroup holds four wavefronts of tiles_per_wave tiles each."""
    seen = set()
    for n in S.MANY_TILES:
        for tpw in S.TILES_PER_WAVE:
            waves = -(-n // tpw)
            if waves % 4:
                seen.add("idle wavefront")
            if n % tpw:
                seen.add("short last stretch")
            if n == tpw:
                seen.add("exactly one full stretch")
            if waves > 4:
                seen.add("second workgroup")
    assert seen == {"idle wavefront", "short last stretch", "exactly one full stretch", "second workgroup"}


def test_the_gpu_table_reaches_every_body_at_every_width_and_every_stretch():
    reached, stretch = set(), set()
    for case in S.cases():
        body = case.body()
        for w, _, _ in S.kernel_classes(OPS[case.op]):
            reached.add((body, w))
            stretch.add((body, w, case.tiles_per_wave))
    assert reached == {(b, w) for b in S.BODIES for w in S.WIDTHS}
    assert stretch == {(b, w, t) for b in S.BODIES for w in S.WIDTHS for t in S.TILES_PER_WAVE}
    # the generic body runs the DPP widths too (meta = NULL), and every listed width is in the table for every operator
    for name in S.NAMES:
        dims = {(c.dim, c.meta) for c in S.cases_of("widths", name)}
        assert dims == {(d, True) for d in S.GENERIC_DIMS + S.DPP_DIMS + S.WIDE_DIMS} | {(d, False) for d in S.DPP_DIMS + S.WIDE_DIMS}
        assert {c.body() for c in S.cases_of("widths", name, meta=False)} == {"generic"}
        assert {(c.dim, c.layout) for c in S.cases_of("layouts", name)} == {(d, l) for d in S.ONE_DIM_OF.values() for l in S.LAYOUTS}
    for dims, body in ((S.GENERIC_DIMS, "generic"), (S.DPP_DIMS, "dpp"), (S.WIDE_DIMS, "dpp_wide")):
        for dim in dims:
            for layout in S.LAYOUTS:
                assert S.body_of(dim, 40, S.layout_of(layout, dim)[0]) == body
    assert {S.geometry(8)[1] % (64 // ((d + 3) // 4)) != 0 for d in S.GENERIC_DIMS} == {True, False}


@pytest.mark.parametrize("max_len", S.MAX_LENS)
@pytest.mark.parametrize("mode", S.ORDERS)
@pytest.mark.parametrize("name", S.NAMES)
def test_planner_invariants(name, mode, max_len):
    op = OPS[name]
    deg = op.lengths
    cap = min(max_len, 32)
    plan = S.planned_classes(op, mode, max_len)
    assert [w for w, _, _ in plan] == sorted(w for w, _, _ in plan)
    seen = []
    for w, order, meta in plan:
        _, R, _, _, B = S.geometry(w)
        assert order.dtype == np.int32 and meta.dtype == np.int32 and order.size == R * meta.size and meta.size > 0
        rows = order[order >= 0]
        assert (order[order < 0] == -1).all()
        assert S.padding_slots(order) < R and (order.reshape(-1, R)[:-1] >= 0).all()      # only the last tile is padded
        seen += rows.tolist()
        lo = max((v for v in S.WIDTHS if v < w), default=-1)
        assert all(min(lo, cap) < deg[r] <= min(w, cap) for r in rows), "the narrowest class that holds the row"
        by = S.meta_bytes(meta, w)
        for t in range(meta.size):
            tile = order[t * R:(t + 1) * R]
            # slot (rho % 4) * B + rho // 4  <=>  rank rho = 4 * (slot % B) + slot // B
            by_rank = [int(tile[(rho % 4) * B + rho // 4]) for rho in range(R)]
            d = [int(deg[r]) if r >= 0 else -1 for r in by_rank]
            assert d == sorted(d, reverse=True), "lengths do not increase with rank; padding slots come last"
            for bt in range(B):
                slots = [g * B + bt for g in range(4)]
                assert by[t, bt] == max(max(int(deg[tile[s]]) if tile[s] >= 0 else 0 for s in slots), 0)
    want = [r for r in op.range_rows() if deg[r] <= cap]
    assert sorted(seen) == want and len(set(seen)) == len(seen)


@pytest.mark.parametrize("width", S.WIDTHS)
def test_slab_reference_on_a_hand_laid_tile(width):
    """One tile of ``one_over``: the entry j of the row in slot s sits in load k = j // Wk at 8-byte position
    (k * R + s) * Wk + j % Wk, everything else is (-1, +0.0f)."""
    op = OPS["one_over"]
    order = [o for w, o, _ in S.kernel_classes(op) if w == width][0]
    L, R, Wk, PPR, _ = S.geometry(width)
    slab = S.slab_reference(op, width, order)
    assert slab.shape == (order.size * width, 2) and R * PPR == 64
    filled = np.zeros(slab.shape[0], bool)
    for t in range(order.size // R):
        for s in range(R):
            row = int(order[t * R + s])
            if row < 0:
                continue
            cols, vals = op.row(row)
            for j in range(len(cols)):
                at = ((t * L + j // Wk) * R + s) * Wk + j % Wk
                assert slab[at, 0] == cols[j] and slab[at, 1] == vals[j:j + 1].view(np.int32)[0]
                filled[at] = True
    assert (slab[~filled] == (-1, 0)).all() and filled.sum() == sum(len(op.row(int(r))[0]) for r in order if r >= 0)


@pytest.mark.parametrize("name", S.NAMES)
def test_emulation_is_within_the_running_sum_bound(name):
    """Per element  |emulation - fp64| <= (n + 2) * 2^-24 * (|a| * sum |val * x| + |b * r|)  for a row of n entries.

    Why: with round-to-nearest every fp32 operation returns its exact result times (1 + d), |d| <= u / (1 + u), u = 2^-24
    (no operand here is subnormal and an addition cannot underflow).  Product i carries its own rounding and those of the
    additions it takes part in: the first addition is to +0 and exact, so at most 1 + (n - 1) = n roundings; the scaling by
    ``a`` adds one and the final addition one more: n + 2.  The term b * r carries two.  k compounded factors with
    |d| <= u / (1 + u) deviate from 1 by at most k * u -- no second-order term (Jeannerod and Rump, "Improved error
    bounds for inner products in floating-point arithmetic", 2013) -- so the error is at most
    (n + 2) u |a| sum |val * x| + 2 u |b * r|, which the bound above covers.  The fp64 side rounds with 2^-53: 2^-29 of the
    bound, far below the distance the emulation keeps from it (it errs like sqrt(n) u, not n u)."""
    op = OPS[name]
    rows = S.tiled_rows(op)
    worst = 0.0
    for dim in (5, 64):
        x, r = S.table_values(name, dim, "x"), S.table_values(name, dim, "r")
        for a, with_r, b in S.EPILOGUES:
            got = S.emulate(op, x, rows, a, r if with_r else None, b)
            want, mag, n = S.evaluate_fp64(op, x, rows, a, r if with_r else None, b)
            assert got.dtype == np.float32 and got.shape == want.shape
            bound = (n[:, None] + 2) * 2.0 ** -24 * mag
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (name, dim, a, b)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    if op.cols.size:
        assert 0.0 < worst <= 1.0                # the emulation rounds: it is not the fp64 value


def _hand_op(cols, vals, table_rows):
    cols, vals = np.array(cols, np.int32), np.array(vals, np.float32)
    rowptr = np.array([0, len(cols)] + [len(cols)] * (table_rows - 1), np.int64)
    return S.TileOp("hand", rowptr, cols, vals, 0, 1, table_rows)


def test_hand_worked_row_of_three_entries():
    """Column 0: (1 + 2^-23)^2 = 1 + 2^-22 + 2^-46 rounds to 1 + 2^-22; minus (1 + 2^-22) gives +0 (a fused multiply-add
    would leave 2^-46); plus 0.5 * 3 = 1.5.   Column 1: the same product 1 + 2^-22, then 2^-24 twice: each time a tie
    that rounds back to the even 1 + 2^-22 (adding the two small terms first would give 1 + 3 * 2^-23).   Column 2:
    3 * (1 + 2^-23) = 3 + 3 * 2^-23 is a tie between 3 + 2^-22 and 3 + 2^-21 and rounds to the even 3 + 2^-21; then exact
    additions."""
    e = 2.0 ** -23
    op = _hand_op([0, 1, 2], [1 + e, -1.0, 0.5], 3)
    x = np.array([[1 + e, 1 + e, 3.0],
                  [1 + 2 * e, -(2.0 ** -24), 1.0],
                  [3.0, 2.0 ** -23, -2.0]], np.float32)
    got = S.emulate(op, x, [0])
    want = np.array([[1.5, 1 + 2 * e, (3 + 4 * e) - 1.0 - 1.0]], np.float32)
    assert S.bits(got).tolist() == S.bits(want).tolist()
    assert S.bits(got)[0].tolist() == [0x3FC00000, 0x3F800002, 0x3F800004]
    exact, _, _ = S.evaluate_fp64(op, x, [0])
    assert exact[0, 0] == 1.5 + e * e and exact[0, 1] == 1 + 3 * e + e * e and exact[0, 2] == 1 + 3 * e
    # the epilogue: a * acc rounded, then b * r rounded, then added
    r = np.array([[1 + e, 3.0, 0.1]] * 3, np.float32)
    got = S.emulate(op, x, [0], 0.75, r, 0.3)
    f = np.float32
    want = [f(f(f(0.75) * f(v)) + f(f(0.3) * rv)) for v, rv in zip(want[0], r[0])]
    assert S.bits(got)[0].tolist() == S.bits(np.array(want, np.float32)).tolist()


def test_hand_worked_empty_row_scaled_by_minus_one_is_minus_zero():
    op = _hand_op([], [], 2)
    x = np.ones((2, 4), np.float32)
    assert S.bits(S.emulate(op, x, [0])).ravel().tolist() == [0] * 4                               # +0.0f
    assert S.bits(S.emulate(op, x, [0], -1.0)).ravel().tolist() == [-(1 << 31)] * 4                # -0.0f: bits 0x80000000
    assert S.bits(S.emulate(op, x, [0], 0.0, np.full((2, 4), 2.0, np.float32), -2.0)).ravel().tolist() == \
        S.bits(np.full(4, -4.0, np.float32)).tolist()
    # a row whose terms cancel exactly is +0 under round-to-nearest, and -0 after a = -1
    op = _hand_op([0, 1], [1.5, -1.5], 2)
    assert S.bits(S.emulate(op, x, [0])).ravel().tolist() == [0] * 4
    assert S.bits(S.emulate(op, x, [0], -1.0)).ravel().tolist() == [-(1 << 31)] * 4


def test_arenas_mark_everything_that_must_not_be_read_or_written():
    op = OPS["item_half"]
    w, order, _ = S.kernel_classes(op)[0]
    rows = S.owned_rows(order)
    for layout in S.LAYOUTS:
        dim = 7
        stride, lead, tail = S.layout_of(layout, dim)
        a, s2, l2 = S.input_arena(op, dim, layout, "x", rows)
        assert (s2, l2) == (stride, lead) and a.size == lead + op.table_rows * stride + tail
        body = a[lead:lead + op.table_rows * stride].reshape(op.table_rows, stride)
        named = S.named_columns(op, rows)
        assert not np.isnan(body[named, :dim]).any() and np.isnan(a).sum() == a.size - named.size * dim
        want = S.wanted(op, dim, rows, S.EPILOGUES[1])
        y = S.expected_output(op, dim, layout, rows, want)
        assert (y != S.SENTINEL).sum() <= rows.size * dim and (y == S.SENTINEL).sum() >= y.size - rows.size * dim
    assert S.layout_of("view", 61)[1] > 0 and S.layout_of("pad4", 61)[0] == 65 and S.layout_of("pad12", 61)[0] == 73

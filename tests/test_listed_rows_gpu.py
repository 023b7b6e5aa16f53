"""The listed-rows hop launch by launch on the named row lists of tests/listed_rows_support.py: ``lgc_spmm_rows`` and
``lgc_spmm_rows_split`` called straight through the C ABI, so the test owns ``work``, ``partials`` and ``partial_rows`` and
reads all three back.

Nothing here carries a tolerance: ``work`` is compared with the plan arithmetic as integers, partial rows and results as
fp32 bit patterns against the numpy emulation of the kernels' contract (the sign of zero included).  Every call

* gathers from tables whose padding columns are NaN, and takes its epilogue rows from a table in which every row outside
  the listed rows of the range is NaN too (``r`` is indexed by row id, in the compact form as well);
* writes into ``y``, ``work`` and ``partials`` prefilled with a sentinel bit pattern, each a few rows longer than the call is
  told; the WHOLE allocations are compared afterwards: outside the ``dim`` columns of the written rows ``y`` keeps the
  sentinel -- unlisted rows, rows named only by ids outside ``[row_begin, row_end)``, padding columns of a strided table,
  the guard rows --, ``work`` beyond ``n_ids + 2`` ints and ``partials`` from the chunk count on likewise.
"""
import numpy as np
import pytest
import torch

import listed_rows_support as S
from gnn_ecommerce_amd import _native

pytestmark = pytest.mark.gpu

OPS = S.operators()
LISTS = S.lists()
_dev = {}


def on_device(name, device):
    """(rowptr int32, entries int32 [E, 2]) of an operator; uploaded once."""
    if name not in _dev:
        op = OPS[name]
        ent = np.zeros((op.cols.size, 2), np.int32)
        ent[:, 0], ent[:, 1] = op.cols, op.vals.view(np.int32)
        _dev[name] = (torch.from_numpy(op.rowptr.astype(np.int32)).to(device), torch.from_numpy(ent).to(device))
    return _dev[name]


def ids_on_device(rl, device):
    key = ("ids", rl.name)
    if key not in _dev:
        _dev[key] = torch.from_numpy(rl.ids).to(device)
    return _dev[key]


def tables_on_device(rl, dim, layout, device):
    """(x, r) as [table_rows, dim] views of strided tables: NaN in the padding columns, and in every row of ``r`` that is
    not a listed row of the range."""
    key = ("tables", rl.name, dim, layout)
    if key not in _dev:
        xs, _, rs = S.strides_of(layout, dim)
        x = torch.from_numpy(S.input_table(rl.op, dim, "x", xs)).to(device)
        r = torch.from_numpy(S.input_table(rl.op, dim, "r", rs, keep=np.unique(S.listed_range_rows(rl)))).to(device)
        _dev[key] = (x[:, :dim], r[:, :dim])
    return _dev[key]


def sentinel(shape, device):
    return torch.full(shape, int(S.SENTINEL), dtype=torch.int32, device=device)


class Call:
    """One list at one width, table layout, epilogue and (for the split form) partial table size."""

    def __init__(self, rl, dim, layout, epilogue, device):
        self.rl, self.dim, self.layout, self.epilogue, self.device = rl, dim, layout, epilogue, device
        self.op = OPS[rl.op]
        self.rowptr, self.entries = on_device(rl.op, device)
        self.ids = ids_on_device(rl, device)
        self.x, self.r = tables_on_device(rl, dim, layout, device)
        self.y_stride = S.strides_of(layout, dim)[1]

    def _y(self, rows):
        y = sentinel((rows + S.GUARD_ROWS, self.y_stride), self.device)
        return y, y.view(torch.float32)[:, :self.dim]

    def rows(self):
        """``lgc_spmm_rows``: y as int32 [table_rows + guard, y_stride]."""
        a, with_r, b = self.epilogue
        ya, y = self._y(self.op.table_rows)
        with torch.cuda.device(self.device):
            code = _native.load().lgc_spmm_rows(
                _native.ptr(self.rowptr), _native.ptr(self.entries), self.op.row_begin, self.op.row_end, _native.ptr(self.ids),
                self.rl.n_ids, self.op.table_rows, _native.ptr(self.x), self.x.stride(0), _native.ptr(y), y.stride(0),
                _native.ptr(self.r) if with_r else None, self.r.stride(0) if with_r else 0, float(a), float(b), self.dim,
                _native.stream_of(self.device))
        assert code == 0, (self.rl.name, self.dim, code)
        return ya.cpu().numpy()

    def split(self, partial_rows, compact=False):
        """``lgc_spmm_rows_split``: (y, work) as int32 arrays and partials as an int32 device tensor, guard rows included."""
        a, with_r, b = self.epilogue
        n = self.rl.n_ids
        y_rows = n if compact else self.op.table_rows
        ya, y = self._y(y_rows)
        work = sentinel((n + 2 + S.GUARD_ROWS,), self.device)
        partials = sentinel((partial_rows + S.GUARD_ROWS, self.dim), self.device)
        with torch.cuda.device(self.device):
            code = _native.load().lgc_spmm_rows_split(
                _native.ptr(self.rowptr), _native.ptr(self.entries), self.op.row_begin, self.op.row_end, _native.ptr(self.ids),
                n, self.op.table_rows, _native.ptr(self.x), self.x.stride(0), _native.ptr(y), y.stride(0), y_rows,
                _native.ptr(self.r) if with_r else None, self.r.stride(0) if with_r else 0, float(a), float(b), self.dim,
                1 if compact else 0, _native.ptr(work), _native.ptr(partials), partial_rows, _native.stream_of(self.device))
        assert code == 0, (self.rl.name, self.dim, code)
        return ya.cpu().numpy(), work.cpu().numpy(), partials


def first_difference(got, want):
    at = np.argwhere(got != want)[0]
    return f"row {int(at[0])}, column {int(at[1])}: got bits {int(got[tuple(at)]):#x}, want {int(want[tuple(at)]):#x}"


def same(got, want, *what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want), what + (first_difference(got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)),)


def cases(name, epilogues=S.EPILOGUES):
    """(dim, layout, epilogue) of a list: every width it runs at, layouts and epilogues in rotation -- every epilogue and
    every layout at one width, so each list sees them all."""
    dims = S.dims_of(name)
    mid = dims[len(dims) // 2]                      # 64 columns (4 lane groups); 4 columns for the lists of wide_hub
    out = [(mid, S.LAYOUTS[i % len(S.LAYOUTS)], e) for i, e in enumerate(epilogues)]
    out += [(mid, layout, epilogues[1]) for layout in S.LAYOUTS]
    for i, dim in enumerate(dims):
        out.append((dim, S.LAYOUTS[(i + 1) % len(S.LAYOUTS)], epilogues[(i + 1) % len(epilogues)]))
    return list(dict.fromkeys(out))


def check_partials(partials, rl, dim, partial_rows, what):
    """The slots of the cut positions hold the emulated chunk sums; from the chunk count on -- the guard rows behind the
    table included -- every slot keeps the sentinel."""
    slots, want, total = S.expected_partials(rl, dim, partial_rows)
    assert partials.shape == (partial_rows + S.GUARD_ROWS, dim) and total <= partial_rows
    assert bool((partials[total:] == int(S.SENTINEL)).all()), ("partials beyond the chunk count",) + tuple(what)
    same(partials[:total].cpu().numpy()[slots], want, "partials", *what)


def check_split(got, rl, dim, layout, epilogue, partial_rows, compact, what):
    """Everything one ``lgc_spmm_rows_split`` call leaves behind."""
    y, work, partials = got
    L = S.chunk_length(OPS[rl.op], rl.ids, partial_rows)
    same(work, S.expected_work(rl, partial_rows), "work", *what)
    check_partials(partials, rl, dim, partial_rows, what)
    same(y, S.expected_y(rl, dim, S.strides_of(layout, dim)[1], L, epilogue, compact), "y", *what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. lgc_spmm_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_spmm_rows_equals_the_emulation_and_writes_nothing_else(device, name):
    """Listed rows of the range hold the emulation's bits -- every row one span: stored order up to 32 entries, lane groups
    beyond --, everything else the sentinel; a second call gives the same bits."""
    rl = LISTS[name]
    for dim, layout, epilogue in cases(name):
        call = Call(rl, dim, layout, epilogue, device)
        got = call.rows()
        same(got, S.expected_y(rl, dim, call.y_stride, None, epilogue), name, dim, layout, epilogue)
        same(call.rows(), got, "second call", name, dim, layout, epilogue)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the plan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_the_plan_equals_the_index_arithmetic(device, name):
    """``work[0 .. n_ids + 1]`` after one call, at the default partial table and at the tight ones; the ints behind it are
    untouched."""
    rl = LISTS[name]
    dim = S.dims_of(name)[0]
    call = Call(rl, dim, "dense", S.EPILOGUES[0], device)
    for room in (S.DEFAULT_ROOM,) + S.TIGHT_ROOMS:
        _, work, _ = call.split(rl.n_ids + room)
        want = S.expected_work(rl, rl.n_ids + room)
        assert work.tolist() == want.tolist(), (name, room, int(np.flatnonzero(work != want)[0]))
        assert work[rl.n_ids + 1] == S.chunk_length(OPS[rl.op], rl.ids, rl.n_ids + room)


# ---------------------------------------------------------------------------------------------------------------------
# 3. partial rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_partial_rows_hold_the_raw_chunk_sums(device, name):
    """Slot w of a position cut into several chunks holds the emulated sum of chunk w - work[m] of its row, before any
    epilogue; every slot from the chunk count on, the guard rows behind the table included, keeps the sentinel."""
    rl = LISTS[name]
    partial_rows = S.partial_rows_of(rl)
    for dim in S.dims_of(name):
        for epilogue in (S.EPILOGUES[1], S.EPILOGUES[4]):           # raw sums: the same under any epilogue
            _, _, partials = Call(rl, dim, "dense", epilogue, device).split(partial_rows)
            check_partials(partials, rl, dim, partial_rows, (name, dim, epilogue))


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the result
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_split_result_equals_the_emulation_and_writes_nothing_else(device, name):
    """y[row_ids[m]]: rows of one chunk as one span, cut rows as their chunk sums combined by lane group; a second call
    gives the same bits."""
    rl = LISTS[name]
    partial_rows = S.partial_rows_of(rl)
    for dim, layout, epilogue in cases(name):
        call = Call(rl, dim, layout, epilogue, device)
        got = call.split(partial_rows)
        check_split(got, rl, dim, layout, epilogue, partial_rows, False, (name, dim, layout, epilogue))
        again = call.split(partial_rows)
        same(again[0], got[0], "second call, y", name, dim, layout, epilogue)
        same(again[1], got[1], "second call, work", name, dim, layout, epilogue)
        total = int(got[1][rl.n_ids])
        assert torch.equal(again[2][:total], got[2][:total]), ("second call, partials", name, dim, layout, epilogue)


@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_compact_result_is_written_by_list_position(device, name):
    """y[m] holds the bits of the non-compact y[row_ids[m]] -- every position of a repeated id the same --, a position with
    a foreign id keeps the sentinel, ``r`` is still indexed by row id and a padded ``y_stride`` is respected."""
    rl = LISTS[name]
    op = OPS[rl.op]
    partial_rows = S.partial_rows_of(rl)
    inside = np.flatnonzero(~S.is_foreign(op, rl.ids))
    for dim, layout, epilogue in cases(name, epilogues=(S.EPILOGUES[1], S.EPILOGUES[2], S.EPILOGUES[0])):
        call = Call(rl, dim, layout, epilogue, device)
        got = call.split(partial_rows, compact=True)
        check_split(got, rl, dim, layout, epilogue, partial_rows, True, (name, dim, layout, epilogue))
        y = got[0]
        plain = call.split(partial_rows)[0]
        assert y.shape == (rl.n_ids + S.GUARD_ROWS, call.y_stride)
        same(y[inside, :dim], plain[rl.ids[inside], :dim], "compact against plain", name, dim, layout, epilogue)
        keep = np.ones(y.shape[0], bool)
        keep[inside] = False
        assert (y[keep] == S.SENTINEL).all() and (y[:, dim:] == S.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. agreement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_both_entry_points_give_the_same_bits_for_rows_of_one_chunk(device, name):
    """At the default length every row of up to 256 entries, 33 to 256 included; rows of up to 32 entries follow the rule
    of ``lgc_spmm_tiles`` on both (test_listed_rows_host.py holds the emulation to ``tiles_support.emulate``)."""
    rl = LISTS[name]
    op = OPS[rl.op]
    rows = np.unique(S.listed_range_rows(rl))
    one_chunk = rows[op.lengths[rows] <= S.CHUNK_LEN]
    cut = rows[op.lengths[rows] > S.CHUNK_LEN]
    for dim, layout, epilogue in cases(name, epilogues=(S.EPILOGUES[1], S.EPILOGUES[4])):
        call = Call(rl, dim, layout, epilogue, device)
        direct, split = call.rows(), call.split(S.partial_rows_of(rl))[0]
        same(split[one_chunk], direct[one_chunk], name, dim, layout, epilogue)
        same(np.delete(split, cut, axis=0), np.delete(direct, cut, axis=0), "all but the cut rows", name, dim, layout, epilogue)
        if cut.size:
            assert (split[cut, :dim] != S.SENTINEL).all() and (direct[cut, :dim] != S.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. tight tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", S.TIGHT_ROOMS)
@pytest.mark.parametrize("name", S.LIST_NAMES)
def test_tight_partial_tables_lengthen_the_chunks(device, name, room):
    """``partial_rows = n_ids + 1 / 2 / 8``: the chunk length in ``work`` is the lengthened one, a multiple of 64, partial
    rows and result equal the emulation built with that length, the chunk count fits the table and nothing behind it is
    written."""
    rl = LISTS[name]
    partial_rows = rl.n_ids + room
    L = S.chunk_length(OPS[rl.op], rl.ids, partial_rows)
    assert L % S.WAVE == 0 and L >= S.CHUNK_LEN
    dims = S.dims_of(name)
    for i, dim in enumerate(dims):
        layout, epilogue = S.LAYOUTS[(i + room) % len(S.LAYOUTS)], S.EPILOGUES[(i + room) % len(S.EPILOGUES)]
        for compact in ((False, True) if i == 0 else (bool((i + room) % 2),)):
            got = Call(rl, dim, layout, epilogue, device).split(partial_rows, compact=compact)
            assert got[1][rl.n_ids + 1] == L and got[1][rl.n_ids] <= partial_rows
            check_split(got, rl, dim, layout, epilogue, partial_rows, compact, (name, room, dim, layout, epilogue, compact))

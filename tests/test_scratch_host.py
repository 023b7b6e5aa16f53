"""Launch stream and scratch ownership, the part that needs no device: the recorder of scratch_support on a fake
library, the header's list of stream-taking entries against ``_native.SIGNATURES``, and who owns a scratch buffer, on CPU
tensors.

The two cases ``test_hop_partials_have_one_owner`` and ``test_score_panel_has_one_owner`` fail on the commit before the
owner key: there ``Operator.partials`` / ``c_struct`` kept one buffer per width and ``_score_workspace`` dropped the
thread from its key, so two threads got the same storage."""
import ctypes
import threading
from ctypes import c_void_p

import pytest
import torch

import scratch_support as SS
from gnn_ecommerce_amd import _native, graph as G, propagate
from gnn_ecommerce_amd.graph import Operator

JOIN_TIMEOUT = 30.0


# ----------------------------------------------------------------------------------------
# the recorder
# ----------------------------------------------------------------------------------------
class FakeLibrary:
    """Entries by the real names; each returns something that depends on its arguments."""

    def __init__(self):
        self.log = []

    def lgc_lincomb(self, *args):
        self.log.append(("lgc_lincomb", args))
        return 7

    def lgc_apply(self, *args):
        self.log.append(("lgc_apply", args))
        return 0

    def lgc_seed_pull(self, *args):
        self.log.append(("lgc_seed_pull", args))
        return -3

    def lgc_spmm_rows_split(self, *args):
        return 0

    def lgc_dim_ok(self, dim):
        self.log.append(("lgc_dim_ok", (dim,)))
        return int(dim == 64)

    marker = "an attribute that is no entry"


def operator_struct(partials, sweep_partials=None):
    c = _native.OperatorC()
    c.partials = partials
    keep = [c]
    if sweep_partials is not None:
        sc = _native.SweepArraysC()
        sc.partials = sweep_partials
        c.sweep = ctypes.pointer(sc)
        keep.append(sc)
    return c, keep


def test_recorder_forwards_and_records():
    fake = FakeLibrary()
    rec = SS.LibraryRecorder(fake, current_stream=lambda: 0x51)
    assert rec.marker == fake.marker and rec.lgc_dim_ok(64) == 1 and rec.lgc_dim_ok(65) == 0
    assert rec.calls == [], "an entry without a stream parameter is forwarded, not recorded"

    # lgc_lincomb(y, y_stride, srcs, strides, coefs, n_terms, n_rows, dim, stream)
    assert rec.lgc_lincomb(1000, 64, None, None, None, 1, 10, 64, 0x51) == 7
    assert fake.log[-1] == ("lgc_lincomb", (1000, 64, None, None, None, 1, 10, 64, 0x51)), "arguments arrive unchanged"
    # an operator by reference, with and without a sweep; a NULL stream is stream 0
    c, keep = operator_struct(0x7000, 0x9000)
    args = (ctypes.byref(c), 10, 1, 64, 2, 64, None, 0, 1.0, 0.0, 64, None)
    assert rec.lgc_apply(*args) == 0
    c2, keep2 = operator_struct(0x7100)
    assert rec.lgc_apply(ctypes.pointer(c2), *args[1:-1], c_void_p(0x52)) == 0
    # lgc_seed_pull: partials, col_flag, col_slot, row_mark by the header's names
    pull = [0] * 20
    pull[9:13] = [0xA000, 0xB000, 0xC000, None]
    pull[19] = 0x51
    assert rec.lgc_seed_pull(*pull) == -3

    me = threading.get_ident()
    a, b, c_, d = rec.calls
    assert (a.name, a.n, a.thread, a.stream, a.current, a.scratch) == ("lgc_lincomb", 0, me, 0x51, 0x51, {})
    assert (b.name, b.n, b.stream, b.owner) == ("lgc_apply", 0, None, (0, me))
    assert b.scratch == {"operator0.partials": 0x7000, "operator0.sweep.partials": 0x9000}
    assert (c_.n, c_.stream) == (1, 0x52) and c_.scratch == {"operator0.partials": 0x7100, "operator0.sweep.partials": None}
    assert d.scratch == {"partials": 0xA000, "col_flag": 0xB000, "col_slot": 0xC000, "row_mark": None}
    assert d.result == -3 and d.returned
    assert [x.name for x in rec.take()] == ["lgc_lincomb", "lgc_apply", "lgc_apply", "lgc_seed_pull"] and rec.calls == []
    rec.lgc_apply(*args)
    assert rec.calls[0].n == 0, "take() starts the counts over"


def test_recorder_hooks_fire_in_order_and_per_thread():
    fake = FakeLibrary()
    rec = SS.LibraryRecorder(fake, current_stream=lambda: None)
    order = []
    rec.before("lgc_lincomb", 1, lambda call: order.append(("before", call.n, call.returned, len(fake.log))))
    rec.before("lgc_lincomb", 1, lambda call: order.append(("before again", call.n)))
    rec.after("lgc_lincomb", 1, lambda call: order.append(("after", call.n, call.returned, len(fake.log))))
    args = (1000, 64, None, None, None, 1, 10, 64, None)
    rec.lgc_lincomb(*args)
    assert order == [], "the hooks of call 1 do not fire at call 0"
    rec.lgc_lincomb(*args)
    assert order == [("before", 1, False, 1), ("before again", 1), ("after", 1, True, 2)]
    rec.lgc_lincomb(*args)
    assert len(order) == 3

    # another thread counts its own calls: its call 1 is its second, whatever this thread has done
    seen = []
    rec.before("lgc_lincomb", 1, lambda call: seen.append(call.thread))

    def worker():
        rec.lgc_lincomb(*args)
        rec.lgc_lincomb(*args)
    t = threading.Thread(target=worker)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive() and seen == [t.ident]
    with pytest.raises(AssertionError):
        rec.before("lgc_dim_ok", 0, lambda call: None)             # not a recorded entry


def test_recorder_hold_times_out_as_a_failure():
    fake = FakeLibrary()
    rec = SS.LibraryRecorder(fake, current_stream=lambda: None)
    never = threading.Event()
    rec.before("lgc_lincomb", 0, lambda call: rec.hold(never, "nobody sets this", timeout=0.05))
    with pytest.raises(AssertionError, match="nobody sets this"):
        rec.lgc_lincomb(1000, 64, None, None, None, 1, 10, 64, None)
    assert fake.log == [] and rec.calls[0].returned is False, "the held call never reached the library"
    released = threading.Event()
    released.set()
    rec.hold(released, "already set")


# ----------------------------------------------------------------------------------------
# the header's list
# ----------------------------------------------------------------------------------------
def test_stream_entries_match_the_signature_table():
    entries = SS.stream_entries()
    last = SS.ends_in_stream()
    print("entries with a stream parameter:", ", ".join(sorted(entries)))
    assert len(entries) > 50 and set(last) <= set(entries)
    # the one entry whose stream is not its last parameter (its error code is)
    assert sorted(set(entries) - set(last)) == ["lgc_sweep_dplan_create"]
    # ... equals the SIGNATURES entries that launch: an entry is in the recorder's list or in NO_LAUNCH, never in both
    assert set(entries) | SS.NO_LAUNCH == set(_native.SIGNATURES), \
        "a new entry: give it a stream parameter (it launches) or list it in scratch_support.NO_LAUNCH (it does not)"
    assert not set(entries) & SS.NO_LAUNCH
    for name, params in entries.items():
        argtypes = _native.SIGNATURES[name][1]
        assert len(argtypes) == len(params), name
        assert argtypes[params.index("stream")] is c_void_p, name
        assert params.count("stream") == 1, name
    for name in last:
        assert _native.SIGNATURES[name][1][-1] is c_void_p, name
    assert SS.LibraryRecorder(FakeLibrary()).recorded_entries == sorted(entries)
    for name, labels in SS.SCRATCH_ARGS.items():
        assert set(labels) <= set(entries[name]), f"{name}: the header has no parameter of that name"


# ----------------------------------------------------------------------------------------
# ownership on CPU tensors
# ----------------------------------------------------------------------------------------
def in_two_threads(fn):
    """``fn()`` in two worker threads that are alive at the same time (so that their ids differ), and here."""
    results, errors = {}, []
    gate = threading.Barrier(2, timeout=JOIN_TIMEOUT)

    def worker(tag):
        try:
            results[tag] = fn()
            gate.wait()                                     # neither ends before the other has its buffers
        except Exception as exc:                            # noqa: BLE001 - reported below
            errors.append(exc)
    threads = [threading.Thread(target=worker, args=(tag,)) for tag in ("a", "b")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in threads), "a straggler"
    assert not errors, errors
    return fn(), results["a"], results["b"]


def byte_range(t):
    return (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())


def assert_disjoint(ranges, what):
    ranges = sorted(ranges)
    for (lo0, hi0), (lo1, hi1) in zip(ranges, ranges[1:]):
        assert hi0 <= lo1, f"{what}: [{lo0:#x}, {hi0:#x}) and [{lo1:#x}, {hi1:#x}) overlap"


def check_owned(fn, what):
    """Same thread twice: the same storage, nothing allocated per call.  Three threads: three buffers that do not overlap."""
    first = fn()
    again = fn()
    firsts = first if isinstance(first, tuple) else (first,)
    agains = again if isinstance(again, tuple) else (again,)
    assert [byte_range(t) for t in firsts] == [byte_range(t) for t in agains], f"{what}: a second call allocated again"
    got = in_two_threads(fn)
    ranges = []
    for g in got:
        ranges += [byte_range(t) for t in (g if isinstance(g, tuple) else (g,))]
    assert len(ranges) == 3 * len(firsts)
    assert_disjoint(ranges, what)
    assert [byte_range(t) for t in (got[0] if isinstance(got[0], tuple) else (got[0],))] == [byte_range(t) for t in firsts], \
        f"{what}: this thread's buffer changed while others asked for theirs"


def small_operator():
    """Four rows of 9 entries in chunks of 4: every row has three partial rows."""
    rowptr = torch.arange(0, 37, 9, dtype=torch.int32)
    entries = torch.zeros((36, 2), dtype=torch.int32)
    op = Operator.build(4, rowptr, entries, 0, 4, short_max=0, chunk_len=4, tiles=False)
    assert op.plan.n_slots == 12
    return op


def test_hop_partials_have_one_owner():
    op = small_operator()
    check_owned(lambda: op.partials(8), "Operator.partials")
    assert tuple(op.partials(8).shape) == (12, 8)
    # another width is another buffer of the same owner
    assert_disjoint([byte_range(op.partials(8)), byte_range(op.partials(16))], "two widths")
    # an explicit owner is the key: the stream handle the launch will get
    cpu = torch.device("cpu")
    one, two = _native.scratch_owner(cpu, 0x51), _native.scratch_owner(cpu, 0x52)
    assert op.partials(8, one).data_ptr() == op.partials(8, one).data_ptr() != op.partials(8, two).data_ptr()


def test_operator_struct_is_cached_per_owner():
    op = small_operator()
    assert op.c_struct(8, 0) is op.c_struct(8, 0), "no new struct per hop"
    assert op.c_struct(8, 0).partials == op.partials(8).data_ptr()
    here, a, b = in_two_threads(lambda: op.c_struct(8, 0))
    assert here is op.c_struct(8, 0)
    assert len({here.partials, a.partials, b.partials}) == 3, "two threads launch with the same partial rows"
    n = 12 * 8 * 4
    assert_disjoint([(c.partials, c.partials + n) for c in (here, a, b)], "lgc_operator.partials")
    cpu = torch.device("cpu")
    one, two = _native.scratch_owner(cpu, 0x51), _native.scratch_owner(cpu, 0x52)
    assert op.c_struct(8, 0, one) is op.c_struct(8, 0, one) and op.c_struct(8, 0, one) is not op.c_struct(8, 0, two)
    assert op.c_struct(8, 0, one).partials == op.partials(8, one).data_ptr() != op.c_struct(8, 0, two).partials
    # everything but the scratch is the same operator
    for f in ("rowptr", "entries", "chunks", "multi", "row_begin", "row_end", "n_chunks", "n_multi"):
        assert getattr(op.c_struct(8, 0, one), f) == getattr(op.c_struct(8, 0, two), f), f


def test_score_panel_has_one_owner():
    cpu = torch.device("cpu")
    check_owned(lambda: propagate._score_workspace(cpu, 100), "_score_workspace")
    small = propagate._score_workspace(cpu, 100)
    assert propagate._score_workspace(cpu, 50) is small, "a smaller request reuses the panel"
    assert propagate._score_workspace(cpu, 200).numel() >= 200


def test_seed_buffers_and_listed_rows_scratch_have_one_owner():
    cpu = torch.device("cpu")
    check_owned(lambda: propagate._seed_map_buffers(cpu, 50), "_seed_map_buffers")
    check_owned(lambda: propagate._seed_mark_buffer(cpu, 50), "_seed_mark_buffer")
    check_owned(lambda: G._rows_split_scratch(cpu, 10, 8), "_rows_split_scratch")
    work, partials = G._rows_split_scratch(cpu, 10, 8)
    assert work.numel() >= 12 and tuple(partials.shape) == (4096 + G.ROWS_SPLIT_ROOM, 8)
    # the key: the owner triple and the width, the stream given or looked up
    assert _native.scratch_owner(cpu) == (cpu, 0, threading.get_ident()) == propagate._scratch_key(cpu)
    assert _native.scratch_owner(cpu, 0x51) == (cpu, 0x51, threading.get_ident())
    assert G._rows_split_scratch(cpu, 10, 8, 0x51)[1].data_ptr() != partials.data_ptr()
    assert G._rows_split_scratch(cpu, 10, 16)[1].data_ptr() != partials.data_ptr()

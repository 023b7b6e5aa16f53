"""Launch stream and scratch ownership on the device (the recorder, the blocker and the inventory are
tests/scratch_support.py).

A. every op of the inventory, run on a side stream while the default stream is kept busy: it finishes without waiting
   for the default stream, gives the bits of its default-stream run, and every launch it makes is handed the side stream;
B. the ops that hand scratch to the library, under four owners one after the other: the buffers of two owners never
   overlap, an owner gets the same buffers again, and every buffer handed to a launch is registered to the launch's own
   stream and thread;
C. two streams at once on one cached operator: 200 alternating hops per stream, then alternating layer sums, every
   output equal to its serial result.  This cannot fail on correct code and may pass on wrong code: B is the guarantee,
   C the demonstration;
D. two threads on the default stream, interleaved by the recorder's hooks so that the second one's scores are written
   between the first one's scoring and ranking launches.

Nothing here can fault: every buffer is sized by the same operator and width whoever uses it, so a race gives wrong
numbers only.  Every wait has a timeout and every thread is joined with one.
"""
import threading
import time

import numpy as np
import pytest
import torch

import scratch_support as SS
from eliminate_support import _coo
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, graph as G, propagate, synth
from gnn_ecommerce_amd.graph import PropGraph

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT = 60.0
BLOCK_FLOOR_MS = 50.0          # keeps (a) meaningful for microsecond ops
BLOCK_FACTOR = 20.0            # times the op's serial time: allocator and plan-cache misses under a new owner

_state = {}


@pytest.fixture()
def ctx(device):
    if "ctx" not in _state:
        _state["ctx"] = SS.Cases(device, lg)
        _state["s1"], _state["s2"] = torch.cuda.Stream(device), torch.cuda.Stream(device)
        _state["runs"] = {}
    return _state["ctx"]


@pytest.fixture()
def rec(monkeypatch):
    r = SS.LibraryRecorder(_native.load())
    monkeypatch.setattr(_native, "_lib", r)
    return r


def prepared(ctx, op, monkeypatch):
    if op.sweep:
        SS.force_sweep(monkeypatch, G)
    runs = _state["runs"]
    if op.name not in runs:
        runs[op.name] = op.make(ctx)
    return runs[op.name]


def names_of(calls):
    return {c.name for c in calls}


def in_thread(fn):
    """``fn()`` on a worker thread; its result, or its exception raised here.  A straggler is a failure."""
    box = {}

    def worker():
        try:
            box["result"] = fn()
        except BaseException as exc:                        # noqa: BLE001 - raised below
            box["error"] = exc
    t = threading.Thread(target=worker)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive(), "the worker thread did not come back"
    if "error" in box:
        raise box["error"]
    return box["result"], t.ident


# ----------------------------------------------------------------------------------------
# A. launch stream
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [op.name for op in SS.INVENTORY])
def test_every_launch_goes_to_the_current_stream(name, ctx, rec, monkeypatch, device):
    op = SS.BY_NAME[name]
    run = prepared(ctx, op, monkeypatch)
    default, s1 = torch.cuda.current_stream(device), _state["s1"]
    assert default.cuda_stream == torch.cuda.default_stream(device).cuda_stream != s1.cuda_stream
    try:
        want = SS.bits(run())                                   # builds the plans, too
        torch.cuda.synchronize()
        rec.clear()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        again = SS.bits(run())
        end.record()
        end.synchronize()
        serial_ms = start.elapsed_time(end)
        calls = rec.take()
        assert set(op.needs) <= names_of(calls), (name, "the case does not reach", set(op.needs) - names_of(calls))
        assert SS.differing(want, again) == [], (name, "two runs on the default stream differ")
        assert all((c.stream or 0) == default.cuda_stream == (c.current or 0) for c in calls), name

        block_ms = max(BLOCK_FLOOR_MS, BLOCK_FACTOR * serial_ms)
        s1.wait_stream(default)
        done = SS.blocker(default, block_ms)
        t0 = time.perf_counter()
        with torch.cuda.stream(s1):
            got = SS.bits(run())                                # the copies to the host ride on s1 and wait for s1 alone
        host_ms = (time.perf_counter() - t0) * 1e3
        blocked = not done.query()
        calls = rec.take()
        print(f"{name}: serial {serial_ms:.3f} ms, blocker {block_ms:.1f} ms, on the side stream {host_ms:.3f} ms, "
              f"{len(calls)} recorded calls")
    finally:
        torch.cuda.synchronize()
    if not op.syncs_device:
        assert blocked, (f"{name}: inconclusive -- the default stream's {block_ms:.0f} ms of work had finished when the op "
                         f"returned after {host_ms:.1f} ms: it waited for the default stream, or left work behind it")
    assert SS.differing(want, got) == [], (name, "the side stream's result differs from the default stream's")
    assert calls and set(op.needs) <= names_of(calls), name
    wrong = [(c.name, c.n, c.stream) for c in calls if (c.stream or 0) != s1.cuda_stream]
    assert not wrong, (name, "launches that were not handed the current stream", wrong)
    assert all((c.current or 0) == s1.cuda_stream for c in calls), name


# ----------------------------------------------------------------------------------------
# B. ownership
# ----------------------------------------------------------------------------------------
def operators_of(g):
    ops = [g.forward_op] + ([g._transpose_op] if g._transpose_op is not None else [])
    for v in g._halves.values():
        if isinstance(v, tuple):
            ops += list(v)
        elif v is not None:                                     # a ReducedGraph
            ops += [v.user_op_h, v.item_op_h, v.gram_op]
            cc = v._concat[0] if v._concat else None
            if cc is not None:
                ops += [cc.user_op, cc.item_op]
    return [o for o in ops if o is not None]


def registered_buffers(ctx):
    """address -> (bytes, (stream, thread) of the owner it is registered to) of every scratch buffer that lives across
    launches.  The sizes are checked against the plans here: partial rows x width x 4."""
    out = {}

    def add(t, owner, what):
        out[t.data_ptr()] = (t.numel() * t.element_size(), (owner[1], owner[2]), what)
    graphs = list(ctx._graphs.values()) + [lg.get_graph(ctx.ei, ctx.ew, SS.N, True)]
    for g in graphs:
        for op in operators_of(g):
            for (owner, dim), t in op._partials.items():
                assert tuple(t.shape) == (op.plan.n_slots, dim) and t.dtype == torch.float32
                add(t, owner, "hop partials")
            for sw in op._sweep.values():
                for (owner, dim), t in sw._partials.items():
                    assert tuple(t.shape) == (max(sw.dims["n_slots"], 1), dim) and t.dtype == torch.float32
                    add(t, owner, "sweep partials")
    for key, (work, partials) in G._rows_scratch.items():
        assert partials.size(0) == work.numel() - 2 + G.ROWS_SPLIT_ROOM and partials.size(1) == key[3]
        add(work, key, "listed rows: chunk numbers")
        add(partials, key, "listed rows: partials")
    for key, (flag, slot) in propagate._seed_maps.items():
        add(flag, key, "seed flags")
        add(slot, key, "seed slots")
    for key, mark in propagate._seed_marks.items():
        add(mark, key, "seed marks")
    for key, panel in propagate._score_workspaces.items():
        add(panel, key, "score panel")
    return out


def scratch_of(calls):
    """[(recorded owner, entry, label, address)] of every scratch address the calls handed over."""
    return [((c.stream or 0, c.thread), c.name, label, addr) for c in calls for label, addr in sorted(c.scratch.items())
            if addr is not None]


@pytest.mark.parametrize("name", [op.name for op in SS.INVENTORY if op.scratch])
def test_scratch_has_one_owner(name, ctx, rec, monkeypatch, device):
    op = SS.BY_NAME[name]
    run = prepared(ctx, op, monkeypatch)
    s1, s2 = _state["s1"], _state["s2"]
    default = torch.cuda.current_stream(device)
    want = SS.bits(run())
    torch.cuda.synchronize()
    rec.clear()
    me = threading.get_ident()
    runs = []                                                    # (who, stream handle, thread, bits, scratch)

    def on(stream, who):
        stream.wait_stream(default)
        with torch.cuda.stream(stream):
            got = SS.bits(run())
        torch.cuda.synchronize()
        runs.append((who, stream.cuda_stream, me, got, scratch_of(rec.take())))
    on(s1, "s1")
    on(s2, "s2")
    runs.append(("default", default.cuda_stream, me, SS.bits(run()), None))
    torch.cuda.synchronize()
    runs[-1] = runs[-1][:4] + (scratch_of(rec.take()),)
    got, ident = in_thread(lambda: SS.bits(run()))
    torch.cuda.synchronize()
    runs.append(("worker", default.cuda_stream, ident, got, scratch_of(rec.take())))
    on(s1, "s1 again")

    for who, _, _, got, scratch in runs:
        assert SS.differing(want, got) == [], (name, who, "differs from the default stream's result")
        assert scratch, (name, who, "handed no scratch to the library")
    assert [s[1:] for s in runs[0][4]] == [s[1:] for s in runs[4][4]], (name, "the same owner got other buffers the second time")
    # first the plain statement: no address is handed over under two owners
    first_user = {}
    for who, _, _, _, scratch in runs[:4]:
        for owner, entry, label, addr in scratch:
            other = first_user.setdefault(addr, (owner, who, entry, label))
            assert other[0] == owner, (name, f"{entry}'s {label} at {addr:#x} under {who} is {other[2]}'s {other[3]} under {other[1]}")

    known = registered_buffers(ctx)
    ranges = {}                                                  # recorded owner -> {(lo, hi)}
    for who, stream, thread, _, scratch in runs:
        streams = {owner[0] for owner, *_ in scratch}
        assert streams == {stream}, (name, who, "scratch handed to launches on other streams", streams)
        if name != "train_step":                                 # its backward launches from autograd's device thread
            assert {owner for owner, *_ in scratch} == {(stream, thread)}, (name, who)
        for owner, entry, label, addr in scratch:
            assert addr in known, (name, who, entry, label, hex(addr), "a scratch address nobody registered")
            size, registered_to, what = known[addr]
            if entry in ("lgc_score_rows", "lgc_mask_topk"):
                size = 40 * SS.N_ITEMS * 4                       # rows * n_items * 4 of this request
                assert size <= known[addr][0]
            assert registered_to == owner, (name, who, entry, label, what, "belongs to", registered_to, "handed to", owner)
            ranges.setdefault(owner, set()).add((addr, addr + size))
    assert len(ranges) >= 4 or name == "train_step", (name, "four owners", list(ranges))
    assert len({o[0] for o in ranges}) == 3, (name, "three streams", list(ranges))
    flat = sorted((lo, hi, owner) for owner, rs in ranges.items() for lo, hi in rs)
    for (lo0, hi0, o0), (lo1, hi1, o1) in zip(flat, flat[1:]):
        assert hi0 <= lo1 or o0 == o1, (name, f"owners {o0} and {o1} share [{lo1:#x}, {min(hi0, hi1):#x})")


# ----------------------------------------------------------------------------------------
# C. two streams at once
# ----------------------------------------------------------------------------------------
# 150,000 distinct pairs over 48 items need more than 3,000 users (3,000 x 48 = 144,000): 3,200, which keeps the item
# rows at about 3,100 entries -- 196 chunks of 16, some 9,400 partial rows per hop.
C_USERS, C_ITEMS, C_PAIRS = 3200, 48, 150_000
C_N = C_USERS + C_ITEMS
C_CALLS = 200
C_SUMS = 20


def crowded_graph(device, route, monkeypatch):
    if route == "sweep":
        monkeypatch.setattr(G, "USE_SWEEP", "1")
        monkeypatch.setattr(G, "SWEEP_WIDE", True)
    key = ("crowded", route)
    if key not in _state:
        rng = np.random.default_rng(150_000)
        flat = rng.choice(C_USERS * C_ITEMS, size=C_PAIRS, replace=False)
        ei, ew = _coo(C_USERS, list(zip((flat // C_ITEMS).tolist(), (flat % C_ITEMS).tolist())))
        kw = dict(short_max=0, chunk_len=16) if route == "chunks" else {}
        g = PropGraph(ei.to(device), ew.to(device), C_N, **kw)
        g.eliminate_max_deg = 0
        assert g.split == C_USERS
        _state[key] = g
    return _state[key]


def crowded_tables(device, dim):
    key = ("tables", dim)
    if key not in _state:
        x1 = synth.xavier_table(C_N, dim, 7).to(device)
        perm = torch.randperm(C_N, generator=torch.Generator().manual_seed(7)).to(device)
        _state[key] = (x1, (-3.0 * x1[perm]).contiguous())       # any mixed partial changes bits
    return _state[key]


def gate(default, streams, ms: float = 40.0):
    """Hold the streams back until the default stream has been busy for ``ms``: what is enqueued on them meanwhile is
    all there when they start, so the two streams run side by side instead of following the host's enqueue order."""
    done = SS.blocker(default, ms)
    for s in streams:
        s.wait_event(done)
    return done


@pytest.mark.parametrize("route,dim", [("chunks", 64), ("chunks", 90), ("sweep", 64), ("sweep", 90)])
def test_two_streams_share_one_operator(route, dim, device, monkeypatch):
    g = crowded_graph(device, route, monkeypatch)
    item_op = g.halves()[1]
    tables = crowded_tables(device, dim)
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    default = torch.cuda.current_stream(device)
    want = []
    for x in tables:
        out = torch.zeros_like(x)
        assert item_op.route(x, out).startswith("sweep" if route == "sweep" else ("split", "fused", "rows")), item_op.route(x, out)
        item_op.apply(x, out)
        want.append(out[C_USERS:].clone())
    if route == "chunks":
        assert item_op.plan.n_slots > 5000, "thousands of partial rows per hop"
    outs = [torch.zeros((C_CALLS, C_N, dim), device=device) for _ in (s1, s2)]
    torch.cuda.synchronize()
    held_back = gate(default, (s1, s2))
    t0 = time.perf_counter()
    for i in range(C_CALLS):                                     # no sync in between; the streams hold different tables
        with torch.cuda.stream(s1):
            item_op.apply(tables[i % 2], outs[0][i])
        with torch.cuda.stream(s2):
            item_op.apply(tables[(i + 1) % 2], outs[1][i])
    queued = not held_back.query()
    torch.cuda.synchronize()
    wrong = sum(int(not torch.equal(outs[s][i, C_USERS:], want[(i + s) % 2])) for s in (0, 1) for i in range(C_CALLS))
    print(f"{route} d{dim}: {wrong} of {2 * C_CALLS} hop outputs differ from their serial result "
          f"({(time.perf_counter() - t0) * 1e3:.0f} ms for the {2 * C_CALLS} hops; all queued behind the gate: {queued})")
    del outs

    alphas = tuple([0.25] * 4)                                   # K = 3
    sums_want = [propagate._layer_sum(g, x, alphas, False) for x in tables]
    torch.cuda.synchronize()
    got = [[], []]
    gate(default, (s1, s2))
    for i in range(C_SUMS):
        with torch.cuda.stream(s1):
            got[0].append(propagate._layer_sum(g, tables[i % 2], alphas, False))
        with torch.cuda.stream(s2):
            got[1].append(propagate._layer_sum(g, tables[(i + 1) % 2], alphas, False))
    torch.cuda.synchronize()
    wrong_sums = sum(int(not torch.equal(got[s][i], sums_want[(i + s) % 2])) for s in (0, 1) for i in range(C_SUMS))
    print(f"{route} d{dim}: {wrong_sums} of {2 * C_SUMS} layer sums differ from their serial result")
    assert wrong == 0 and wrong_sums == 0, (route, dim, wrong, wrong_sums)


# ----------------------------------------------------------------------------------------
# D. two threads, one stream
# ----------------------------------------------------------------------------------------
def test_two_threads_rank_their_own_scores(device, rec):
    n_users, n_items, dim, k = 64, 300, 64, 10
    t = synth.xavier_table(n_users + n_items, dim, 11).to(device)
    users_t, items_t = t[:n_users], t[n_users:]
    sel = {"A": torch.arange(0, 32, device=device), "B": torch.arange(32, 64, device=device)}
    assert propagate.panel_rows(n_items) >= 32, "one panel each"
    serial = {who: propagate.recommend_topk(users_t, s, items_t, None, k).cpu() for who, s in sel.items()}
    assert not torch.equal(serial["A"], serial["B"]), "the two requests must rank differently"
    torch.cuda.synchronize()
    rec.clear()

    ids, order = {}, []
    a_held, b_scored = threading.Event(), threading.Event()

    def hold_a(call):
        if call.thread == ids.get("A"):
            order.append("A waits before lgc_mask_topk")
            a_held.set()
            rec.hold(b_scored, "B's first lgc_score_rows has not returned")

    def b_done(call):
        if call.thread == ids.get("B"):
            order.append("B's lgc_score_rows returned")
            b_scored.set()
    rec.before("lgc_mask_topk", 0, hold_a)
    rec.after("lgc_score_rows", 0, b_done)

    got, errors = {}, []

    def request(who):
        try:
            ids[who] = threading.get_ident()
            if who == "B":
                rec.hold(a_held, "A has not reached its lgc_mask_topk")
            got[who] = propagate.recommend_topk(users_t, sel[who], items_t, None, k).cpu()
        except BaseException as exc:                             # noqa: BLE001 - reported below
            errors.append((who, exc))
            a_held.set()
            b_scored.set()                                       # nobody waits for a thread that has failed
    threads = [threading.Thread(target=request, args=(who,)) for who in ("A", "B")]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_TIMEOUT)
    torch.cuda.synchronize()
    assert not any(th.is_alive() for th in threads), "a straggler"
    assert not errors, errors
    assert order == ["A waits before lgc_mask_topk", "B's lgc_score_rows returned"], order
    calls = rec.take()
    assert all((c.stream or 0) == torch.cuda.default_stream(device).cuda_stream for c in calls), "both on the default stream"
    panels = {who: {c.scratch["out"] for c in calls if c.name == "lgc_score_rows" and c.thread == ids[who]} for who in "AB"}
    print("A got", "its own ranking" if torch.equal(got["A"], serial["A"]) else
          ("B's ranking" if torch.equal(got["A"], serial["B"]) else "neither ranking"), "; panels", panels)
    assert torch.equal(got["B"], serial["B"])
    assert torch.equal(got["A"], serial["A"]), "A ranked the scores B wrote between A's two launches"
    assert not panels["A"] & panels["B"], "two threads on one stream share the score panel"

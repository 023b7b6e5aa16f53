"""Launch stream and scratch ownership: a recorder around the native library, a stream blocker and the inventory of
public ops (tests/test_scratch_host.py, tests/test_scratch_gpu.py).

Two promises of the library are pinned here.  Every launch goes to the CURRENT stream: every ``lgc_*`` entry that
launches takes ``void *stream`` and every wrapper passes ``_native.stream_of(device)``.  And scratch that lives across
launches -- the partial rows one launch of a hop writes and a later one reads, the flags of the seeded backward, the
score panel between its scoring and its ranking launch -- has one owner, ``_native.scratch_owner``: a (device, stream,
host thread) triple.

``LibraryRecorder`` stands in for the ``CDLL`` of ``_native.load()`` (``monkeypatch.setattr(_native, "_lib", rec)``) and
notes, for every entry with a stream parameter, the stream it was handed, the current stream at that moment, the
calling thread and the scratch addresses among its arguments.  The inventory reuses the graph of layer_sum_support
(700 users x 45 items with a hub, an empty and a single-entry item row) and compares an op with ITSELF on another
stream or thread, bit for bit: the project promises run-to-run identical bits for all of them, so no reference is
needed beyond the op's own default-stream result.
"""
import ctypes
import os
import re
import struct
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import layer_sum_support as S
from tests_support import sampler_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
HOLD_TIMEOUT = 30.0

# Entries that never launch: size queries, route questions, the host planner and the host restatement of the concat
# builder.  Every other entry of _native.SIGNATURES must have a stream parameter (tests/test_scratch_host.py), so a new
# entry lands in this list or in the recorder's.
NO_LAUNCH = frozenset({
    "lgc_abi_version", "lgc_error_string", "lgc_dim_ok", "lgc_build_workspace_bytes", "lgc_row_plan_workspace_bytes",
    "lgc_tile_classes_workspace_bytes", "lgc_sweep_plan_create", "lgc_sweep_plan_dims", "lgc_sweep_plan_export",
    "lgc_sweep_plan_export_multi", "lgc_sweep_plan_free", "lgc_sweep_dplan_workspace_bytes", "lgc_sweep_dplan_dims",
    "lgc_sweep_dplan_export_multi", "lgc_sweep_dplan_free", "lgc_sweep_ok", "lgc_apply_route", "lgc_reduce_workspace_bytes",
    "lgc_reduce_gram_workspace_bytes", "lgc_reduce_concat_rows", "lgc_reduce_concat_host",
    "lgc_item_neighbors_workspace_bytes", "lgc_rerank_route", "lgc_rank_positions_workspace_bytes",
    "lgc_softmax_workspace_bytes", "lgc_retrieve_workspace_bytes"})

# scratch handed over as plain pointers, by the header's parameter names (lgc_operator arguments are read field by field)
SCRATCH_ARGS = {
    "lgc_seed_pull": ("partials", "col_flag", "col_slot", "row_mark"),
    "lgc_spmm_rows_split": ("work", "partials"),
    "lgc_score_rows": ("out",),          # the panel, when recommend_topk calls
    "lgc_mask_topk": ("scores",),
}


def header_prototypes(path: str = HEADER) -> Dict[str, List[str]]:
    """name -> parameter declarations of every ``lgc_*`` prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, args in re.findall(r"\b(lgc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        out[name] = [" ".join(a.split()) for a in args.split(",")]
    return out


def param_name(decl: str) -> str:
    return re.split(r"[\s\*]+", decl.strip())[-1]


def stream_entries(path: str = HEADER) -> Dict[str, List[str]]:
    """name -> parameter names of every entry that takes ``void *stream``.  All but lgc_sweep_dplan_create (whose last
    parameter is its error code) take it LAST; ``ends_in_stream`` tells them apart."""
    return {name: [param_name(d) for d in decls] for name, decls in header_prototypes(path).items()
            if any(re.fullmatch(r"void \*\s*stream", d) for d in decls)}


def ends_in_stream(path: str = HEADER) -> List[str]:
    return sorted(name for name, decls in header_prototypes(path).items() if re.fullmatch(r"void \*\s*stream", decls[-1]))


def _address(v) -> Optional[int]:
    if v is None:
        return None
    if isinstance(v, int):
        return v
    if isinstance(v, ctypes.c_void_p):
        return v.value
    return ctypes.cast(v, ctypes.c_void_p).value


def _struct_of(arg):
    """The structure behind ``ctypes.byref(s)``, ``ctypes.pointer(s)`` or ``s`` itself; None for anything else."""
    obj = getattr(arg, "_obj", None)                       # byref
    if obj is None and hasattr(arg, "contents"):
        try:
            obj = arg.contents
        except ValueError:                                  # NULL pointer
            return None
    if obj is None and isinstance(arg, ctypes.Structure):
        obj = arg
    return obj if isinstance(obj, ctypes.Structure) else None


@dataclass
class Call:
    name: str
    n: int                       # how many calls of this name the calling thread had made before
    thread: int
    stream: Optional[int]        # the stream argument, as an integer handle (None = NULL = stream 0)
    current: Optional[int]       # the current stream's handle at call time
    scratch: Dict[str, Optional[int]] = field(default_factory=dict)
    result: object = None
    returned: bool = False

    @property
    def owner(self):
        return (self.stream or 0, self.thread)


class LibraryRecorder:
    """Forwards every attribute to ``lib``; calls of the entries with a stream parameter are recorded first.

    ``before(name, n, fn)`` / ``after(name, n, fn)``: ``fn(call)`` runs on the calling thread right before (after) its
    n-th call (from 0, counted per thread) of ``name``.  A hook that must wait uses ``hold(event)``: 30 seconds at the
    most, and a timeout is an AssertionError, never a hang."""

    def __init__(self, lib, current_stream: Optional[Callable[[], Optional[int]]] = None, header: str = HEADER):
        self._lib = lib
        self._params = stream_entries(header)
        self._current = current_stream or _torch_current_stream
        self._lock = threading.Lock()
        self._counts: Dict[tuple, int] = {}
        self._hooks: Dict[tuple, list] = {}
        self._wrapped: Dict[str, Callable] = {}
        self.calls: List[Call] = []

    # -- what a test asks ----------------------------------------------------------------
    @property
    def recorded_entries(self) -> List[str]:
        return sorted(self._params)

    def before(self, name: str, n: int, fn: Callable[[Call], None]) -> None:
        assert name in self._params, f"{name} is not a recorded entry"
        self._hooks.setdefault(("before", name, n), []).append(fn)

    def after(self, name: str, n: int, fn: Callable[[Call], None]) -> None:
        assert name in self._params, f"{name} is not a recorded entry"
        self._hooks.setdefault(("after", name, n), []).append(fn)

    @staticmethod
    def hold(event: threading.Event, what: str = "", timeout: float = HOLD_TIMEOUT) -> None:
        if not event.wait(timeout=timeout):
            raise AssertionError(f"held for {timeout:g} s without being released: {what}")

    def clear(self) -> None:
        with self._lock:
            self.calls = []
            self._counts = {}

    def take(self) -> List[Call]:
        """The calls so far, and start over."""
        with self._lock:
            got, self.calls, self._counts = self.calls, [], {}
        return got

    # -- forwarding ------------------------------------------------------------------------
    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.__dict__.get("_params", {}):
            return fn
        got = self._wrapped.get(name)
        if got is None:
            got = self._wrapped[name] = self._wrap(name, fn)
        return got

    def _wrap(self, name: str, fn):
        params = self._params[name]
        at = params.index("stream")
        plain = [(label, params.index(label)) for label in SCRATCH_ARGS.get(name, ())]

        def call(*args):
            thread = threading.get_ident()
            rec = Call(name, 0, thread, _address(args[at]), self._current())
            for label, i in plain:
                rec.scratch[label] = _address(args[i])
            ops = 0
            for a in args:
                s = _struct_of(a)
                if s is not None and hasattr(s, "partials") and hasattr(s, "sweep"):       # lgc_operator
                    tag = f"operator{ops}"
                    ops += 1
                    rec.scratch[tag + ".partials"] = _address(s.partials)
                    rec.scratch[tag + ".sweep.partials"] = _address(s.sweep.contents.partials) if s.sweep else None
            with self._lock:
                rec.n = self._counts.get((name, thread), 0)
                self._counts[(name, thread)] = rec.n + 1
                self.calls.append(rec)
            for hook in self._hooks.get(("before", name, rec.n), ()):
                hook(rec)
            rec.result = fn(*args)
            rec.returned = True
            for hook in self._hooks.get(("after", name, rec.n), ()):
                hook(rec)
            return rec.result
        call.__name__ = name
        return call


def _torch_current_stream() -> Optional[int]:
    if not torch.cuda.is_available():
        return None
    return torch.cuda.current_stream(torch.cuda.current_device()).cuda_stream


# ----------------------------------------------------------------------------------------
# a stream kept busy for a given time
# ----------------------------------------------------------------------------------------
_cycles_per_ms: Dict[int, float] = {}


def _sleep_rate(device) -> float:
    """Cycles of ``torch.cuda._sleep`` per millisecond, measured once per session with events."""
    idx = torch.device(device).index or 0
    if idx not in _cycles_per_ms:
        with torch.cuda.device(idx):
            torch.cuda._sleep(1_000_000)                                    # warm
            torch.cuda.synchronize()
            cycles = 20_000_000
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            torch.cuda._sleep(cycles)
            end.record()
            end.synchronize()
            _cycles_per_ms[idx] = cycles / max(start.elapsed_time(end), 1e-3)
    return _cycles_per_ms[idx]


def blocker(stream: "torch.cuda.Stream", ms: float) -> "torch.cuda.Event":
    """Keep ``stream`` busy for about ``ms`` milliseconds from now on; returns the event recorded behind the work.
    While ``event.query()`` is False everything enqueued on the stream after this call has not started."""
    rate = _sleep_rate(stream.device)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(rate * ms))
        end = torch.cuda.Event()
        end.record(stream)
    return end


# ----------------------------------------------------------------------------------------
# results as bits
# ----------------------------------------------------------------------------------------
def bits(result) -> list:
    """Every tensor and number of a result (tuples, lists, dicts, named tuples and plain result objects are walked), as
    host bytes: two results are the same computation exactly when these lists are equal.  Copies run on the current
    stream and wait for it alone."""
    out = []

    def walk(v, path):
        if torch.is_tensor(v):
            t = v.detach().contiguous().cpu()
            out.append((path, str(t.dtype), tuple(t.shape), t.numpy().tobytes() if t.numel() else b""))
        elif isinstance(v, float):
            out.append((path, "float", struct.pack("d", v)))
        elif isinstance(v, (int, str, bool)) or v is None:
            out.append((path, "value", v))
        elif isinstance(v, dict):
            for k in sorted(v, key=str):
                walk(v[k], f"{path}.{k}")
        elif isinstance(v, (tuple, list)):
            for i, e in enumerate(v):
                walk(e, f"{path}[{i}]")
        elif hasattr(v, "__dict__"):
            for k in sorted(vars(v)):
                if not k.startswith("_"):
                    walk(getattr(v, k), f"{path}.{k}")
        else:
            raise TypeError(f"{path}: cannot compare a {type(v).__name__}")
    walk(result, "result")
    return out


def differing(a: list, b: list) -> List[str]:
    """Paths at which two ``bits`` lists differ."""
    if [x[:-1] for x in a] != [x[:-1] for x in b]:
        return ["<the results have different layouts>"]
    return [x[0] for x, y in zip(a, b) if x[-1] != y[-1]]


# ----------------------------------------------------------------------------------------
# the inventory
# ----------------------------------------------------------------------------------------
def force_sweep(monkeypatch, G) -> None:
    """The band sweep on the small graph: the knobs of test_layer_sum_paths_gpu.force_sweep (plans are built lazily, so
    they are set for the whole test)."""
    monkeypatch.setattr(G, "USE_SWEEP", "1")
    monkeypatch.setattr(G, "SWEEP_CFG", dict(G.SWEEP_CFG, **S.SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_CFG_WIDE", dict(G.SWEEP_CFG_WIDE, **S.SMALL_PLAN))
    monkeypatch.setattr(G, "SWEEP_WIDE", True)


@dataclass
class Op:
    """One public op on one small seeded case.  ``make(ctx)`` prepares its inputs (on the default stream, once) and
    returns ``run()``: one execution on whatever stream and thread it is called from, returning everything the op
    computes.  ``needs``: entries that must show up among the recorded calls (the case reaches the code it is meant
    for).  ``scratch``: hands scratch to the library (part B).  ``sweep``: runs under ``force_sweep``.
    ``syncs_device``: the op's own documentation says it waits for the whole device (DESIGN section 28 lists each)."""
    name: str
    make: Callable
    needs: tuple = ()
    scratch: bool = False
    sweep: bool = False
    syncs_device: bool = False


N_USERS, N_ITEMS, N = S.N_USERS, S.N_ITEMS, S.N
LAYERS = 3
BATCH = 5                      # 2 * 10 label pairs * SEED_ROWS_FACTOR (32) <= 745 rows: the seeded backward runs


class Cases:
    """Inputs shared by the inventory, built once per session on the default stream."""

    def __init__(self, device, lg):
        self.device, self.lg = device, lg
        self.ei_host, self.ew_host = S.edge_list()
        self.ei, self.ew = self.ei_host.to(device), self.ew_host.to(device)
        self._graphs, self._tables = {}, {}
        pairs = sorted(set(S.pairs()))
        self.pair_users = np.array([p[0] for p in pairs], dtype=np.int64)
        self.pair_items = np.array([p[1] for p in pairs], dtype=np.int64)
        rng = np.random.default_rng(28)
        self.users = torch.from_numpy(np.sort(rng.choice(N_USERS, size=40, replace=False))).to(device)
        self.listed = S.listed_rows(self.ei_host)[0].to(device)
        self.held_out = [sorted(set(rng.choice(N_ITEMS, size=1 + u % 4, replace=False).tolist())) for u in range(40)]
        gen = torch.Generator().manual_seed(28)
        self.batch_users = torch.randint(0, N_USERS, (BATCH,), generator=gen).to(device)
        self.batch_pos = (torch.randint(0, N_ITEMS, (BATCH,), generator=gen) + N_USERS).to(device)
        self.batch_neg = (torch.randint(0, N_ITEMS, (BATCH,), generator=gen) + N_USERS).to(device)

    def table(self, dim: int) -> torch.Tensor:
        if dim not in self._tables:
            from gnn_ecommerce_amd import synth
            self._tables[dim] = synth.xavier_table(N, dim, 100 + dim).to(self.device)
        return self._tables[dim]

    def graph(self, kind: str):
        """"chunk": every row cut into 16-entry chunks (short_max 0); "default": tiles for the short rows; "sweep": the
        default graph built while the band sweep is forced (the caller has set ``force_sweep``)."""
        if kind not in self._graphs:
            kw = dict(short_max=0, chunk_len=16) if kind == "chunk" else {}
            # own copies of the edge tensors: get_graph must not hand this graph to the model-level ops
            self._graphs[kind] = self.lg.PropGraph(self.ei.clone(), self.ew.clone(), N, **kw)
        return self._graphs[kind]

    def seen(self):
        lg, dev = self.lg, self.device
        ptr = np.zeros(N_USERS + 1, dtype=np.int64)
        np.add.at(ptr, self.pair_users + 1, 1)
        return lg.SeenLists(torch.from_numpy(np.cumsum(ptr)).to(dev), torch.from_numpy(self.pair_items.copy()).to(dev))

    def positives(self):
        return self.lg.PositiveLists.from_lists(self.users.cpu().tolist(), self.held_out, N_USERS, device=self.device)

    def model(self, dim: int = 64):
        """A fresh model on the same weights: nothing cached from an earlier run, the graph shared through get_graph."""
        lg = self.lg
        m = lg.LightGCN(N, dim, LAYERS)
        m.load_state_dict({"alpha": m.alpha, "embedding.weight": self.table(dim).cpu()})
        return m.to(self.device)


def _hop(kind: str, half: str, dim: int, epilogue: str = ""):
    def make(ctx):
        g = ctx.graph(kind)
        op = {"users": lambda: g.halves()[0], "items": lambda: g.halves()[1], "all": lambda: g.forward_op}[half]()
        x = ctx.table(dim)
        r = ctx.table(dim).flip(0).contiguous() if epilogue else None
        r2 = (ctx.table(dim) * 0.5).contiguous() if epilogue == "r2" else None

        def run():
            out = torch.zeros_like(x)
            if epilogue == "r2":
                assert op.takes_second_row(x, out, r), "the case must reach lgc_apply2"
                op.apply(x, out, a=0.75, r=r, b=0.5, r2=r2, b2=0.25)
            elif epilogue:
                op.apply(x, out, a=0.75, r=r, b=0.5)
            else:
                op.apply(x, out)
            return out, op.route(x, out, r)
        return run
    return make


def _apply_rows_split(dim: int):
    def make(ctx):
        from gnn_ecommerce_amd.graph import apply_rows
        op, x, rows = ctx.graph("default").halves()[1], ctx.table(dim), ctx.listed

        def run():
            out = torch.zeros_like(x)
            apply_rows(op, rows, x, out, a=0.5, r=x, b=0.25, split=True)
            return out
        return run
    return make


def _layer_sum(dim: int, transpose: bool = False, listed: bool = False, max_deg: int = 0):
    def make(ctx):
        from gnn_ecommerce_amd import propagate
        g, x = ctx.graph("sweep"), ctx.table(dim)
        alphas = tuple([1.0 / (LAYERS + 1)] * (LAYERS + 1))
        rows = ctx.listed if listed else None

        def run():
            g.eliminate_max_deg = max_deg
            try:
                if max_deg:
                    assert g.reduced() is not None, "the case must reach the reduced layers"
                out = propagate._layer_sum(g, x, alphas, transpose, rows)
            finally:
                g.eliminate_max_deg = None
            return out[rows] if listed else out                   # the other rows are left uninitialised by design
        return run
    return make


def _train_step(ctx):
    labels = torch.stack([torch.cat([ctx.batch_users, ctx.batch_users]), torch.cat([ctx.batch_pos, ctx.batch_neg])])

    def run():
        model = ctx.model()
        out = model(ctx.ei, labels, ctx.ew)
        loss = model.recommendation_loss(out[:BATCH], out[BATCH:], 0) * BATCH \
            + model.regularization_loss(ctx.batch_users, ctx.batch_pos, ctx.batch_neg, 1e-4)
        loss.backward()
        return out.detach(), loss.detach(), model.embedding.weight.grad
    return run


def _adam(ctx):
    from gnn_ecommerce_amd import optim
    w0, g0 = ctx.table(64), ctx.table(90)[:, :64].contiguous()

    def run():
        p = torch.nn.Parameter(w0.clone())
        opt = optim.Adam([p], lr=0.01)
        for scale in (1.0, -0.5):
            p.grad = g0 * scale
            opt.step()
        st = opt.state[p]
        return p.detach(), {k: v for k, v in st.items() if torch.is_tensor(v)}
    return run


def _recommend_topk(ctx):
    from gnn_ecommerce_amd import propagate
    t, seen = ctx.table(64), ctx.seen()

    def run():
        return propagate.recommend_topk(t[:N_USERS], ctx.users, t[N_USERS:], seen, 10, return_values=True)
    return run


def _evaluate_ranking(ctx):
    from gnn_ecommerce_amd import propagate
    t, seen, pos = ctx.table(64), ctx.seen(), ctx.positives()

    def run():
        return propagate.evaluate_ranking(t[:N_USERS], t[N_USERS:], seen, ctx.users, pos, (5, 10))
    return run


def _model_op(call):
    """An op of the model's serving surface: ``call(model, ctx)`` on a fresh model, so that the propagated table is
    computed by this run (on this run's stream), not taken from a cache."""
    def make(ctx):
        extra = {}

        def run():
            return call(ctx.model(), ctx, extra)
        return run
    return make


def _args(ctx):
    return ctx.ei, ctx.ew, N_USERS, N_ITEMS


def _full_rank(m, ctx, extra):
    if "seen" not in extra:
        extra["seen"], extra["pos"] = ctx.seen(), ctx.positives()
    return m.evaluate_full_rank(*_args(ctx), extra["seen"], ctx.users, extra["pos"], ks=(5, 20))


def _similar(m, ctx, extra):
    return m.similar_items(*_args(ctx), item_ids=[S.HUB, S.EMPTY, S.SINGLE, 1, 2], k=10)


def _retrieve(m, ctx, extra):
    if "seen" not in extra:
        extra["seen"] = ctx.seen()
        ok = torch.ones(N_ITEMS, dtype=torch.bool)
        ok[::5] = False
        extra["ok"] = ok
    return (m.recommend_filtered(*_args(ctx), extra["seen"], ctx.users, k=10, item_ok=extra["ok"]),
            m.item_audience(*_args(ctx), [S.HUB, S.SINGLE, 3], k=10))


def _rerank(m, ctx, extra):
    if "seen" not in extra:
        extra["seen"] = ctx.seen()
    from gnn_ecommerce_amd import propagate
    with torch.no_grad():
        t = m._serving_embedding(ctx.ei, ctx.ew).detach()
    top, value = propagate.recommend_topk(t[:N_USERS], ctx.users, t[N_USERS:], extra["seen"], 20, return_values=True)
    return (m.rerank_diverse(*_args(ctx), top, value, k=10, lam=0.5), m.list_diversity(*_args(ctx), top, ks=(5, 10, 20)))


def _sessions(ctx):
    from gnn_ecommerce_amd import SessionLists
    return SessionLists.from_lists([([S.HUB, 1, 2], None), ([S.SINGLE], [0.5]), ([3, 4, 6, 8], [1.0, 2.0, 1.0, 0.5])],
                                   device=ctx.device)


def _fold_in(m, ctx, extra):
    return m.embed_sessions(*_args(ctx), _sessions(ctx), init_users=[-1, 7, 12])


def _explain(m, ctx, extra):
    top = torch.tensor([[S.HUB, 1, 2], [3, 4, S.SINGLE]], dtype=torch.int64)
    return m.explain_topk(*_args(ctx), [7, 12], top, m=3)


def _softmax(m, ctx, extra):
    loss = m.softmax_loss(ctx.ei, ctx.ew, ctx.batch_users, ctx.batch_pos, ctx.batch_neg, temperature=0.5)
    loss.backward()
    return loss.detach(), m.embedding.weight.grad


def _paths(m, ctx, extra):
    top = torch.tensor([[S.HUB, 1, S.EMPTY], [3, 4, S.SINGLE]], dtype=torch.int64)
    return m.recommendation_paths(ctx.ei, ctx.ew, N_USERS, [7, S.ISOLATED], top)


def _sampler(hard: bool):
    def make(ctx):
        from gnn_ecommerce_amd import TripleSampler
        order, pos, ign = sampler_lists(N_USERS, N_ITEMS, 5)
        pu = np.array([u for u in order for _ in pos[u]], dtype=np.int64)
        pi = np.array([i for u in order for i in pos[u]], dtype=np.int64)
        iu = np.array([u for u in order for _ in ign[u]], dtype=np.int64)
        ii = np.array([i for u in order for i in ign[u]], dtype=np.int64)
        table = ctx.table(64)

        def run():
            s = TripleSampler.from_pairs(N_USERS, N_ITEMS, pu, pi, iu, ii, ctx.device, seed=3)
            got = [s.sample_hard(32, table, candidates=8) if hard else s.sample(32) for _ in range(2)]
            s.check()
            return got
        return run
    return make


def _build_graph(ctx):
    def run():
        g = ctx.lg.PropGraph(ctx.ei.clone(), ctx.ew.clone(), N)
        t = g.transpose_op
        f = g.forward_op
        return f.rowptr, f.entries, g.deg, g.dis, t.rowptr, t.entries, g.split
    return run


def _reduced(ctx):
    base = ctx.graph("default")

    def run():
        base._halves.pop(("reduced", 3, False), None)             # built again by this run
        base.eliminate_max_deg = 3
        try:
            red = base.reduced()
        finally:
            base.eliminate_max_deg = None
        c = red.csr
        return c.n_h, c.user_map, c.rowptr, c.entries, c.gram_rowptr, c.gram_entries
    return run


INVENTORY: List[Op] = (
    [Op(f"hop_chunks_items_d{d}", _hop("chunk", "items", d), ("lgc_apply",), scratch=True) for d in (64, 90)]
    + [Op(f"hop_chunks_whole_d{d}", _hop("chunk", "all", d, "r"), ("lgc_apply",), scratch=True) for d in (64, 90)]
    + [Op(f"hop_tiles_users_d{d}", _hop("default", "users", d), ("lgc_apply",)) for d in (64, 90)]
    + [Op(f"hop_sweep_items_d{d}", _hop("sweep", "items", d), ("lgc_apply",), scratch=True, sweep=True) for d in (64, 90)]
    + [Op(f"hop_sweep_items_r_d{d}", _hop("sweep", "items", d, "r"), ("lgc_apply",), scratch=True, sweep=True) for d in (64, 90)]
    + [Op(f"hop_sweep_items_r2_d{d}", _hop("sweep", "items", d, "r2"), ("lgc_apply2",), scratch=True, sweep=True) for d in (64, 90)]
    + [Op(f"apply_rows_split_d{d}", _apply_rows_split(d), ("lgc_spmm_rows_split",), scratch=True) for d in (64, 90)]
    + [Op("layer_sum_plain_d64", _layer_sum(64), ("lgc_apply",), sweep=True),
       Op("layer_sum_plain_d90", _layer_sum(90), ("lgc_apply",), sweep=True),
       # (on this graph the hub row keeps the last item step whole: listed_rows_pay; apply_rows_split_* has the split launch)
       Op("layer_sum_final_rows_d64", _layer_sum(64, listed=True), ("lgc_apply", "lgc_spmm_rows"), sweep=True),
       Op("layer_sum_reduced_d64", _layer_sum(64, max_deg=3), ("lgc_apply",), sweep=True),
       Op("layer_sum_transposed_d64", _layer_sum(64, transpose=True), ("lgc_apply",), sweep=True),
       Op("train_step", _train_step, ("lgc_pair_dot_rows", "lgc_seed_prepare", "lgc_seed_pull", "lgc_reg_rows", "lgc_bpr_loss"),
          scratch=True),
       Op("adam_step", _adam, ("lgc_adam_step",)),
       Op("recommend_topk", _recommend_topk, ("lgc_score_rows", "lgc_mask_topk"), scratch=True),
       Op("evaluate_ranking", _evaluate_ranking, ("lgc_rank_metrics", "lgc_column_sums", "lgc_topk_coverage")),
       Op("evaluate_full_rank", _model_op(_full_rank), ("lgc_rank_positions",)),
       Op("similar_items", _model_op(_similar), ("lgc_item_neighbors",)),
       Op("retrieve", _model_op(_retrieve), ("lgc_retrieve_topk",)),
       Op("rerank_diverse", _model_op(_rerank), ("lgc_rerank_mmr", "lgc_list_diversity")),
       Op("fold_in", _model_op(_fold_in), ("lgc_fold_in",)),
       Op("explain_topk", _model_op(_explain), ("lgc_attribute",)),
       Op("softmax_loss", _model_op(_softmax), ("lgc_softmax_batch",)),
       Op("sampler_sample", _sampler(False), ("lgc_sample_triples",)),
       Op("sampler_sample_hard", _sampler(True), ("lgc_sample_hard_triples",)),
       Op("shortest_paths", _model_op(_paths), ("lgc_bfs_init", "lgc_bfs_level")),
       Op("build_graph", _build_graph, ("lgc_build_csr", "lgc_bipartite_split")),
       Op("reduced_graph", _reduced, ("lgc_reduce_count", "lgc_reduce_fill", "lgc_reduce_gram_fill"))])

BY_NAME = {op.name: op for op in INVENTORY}
assert len(BY_NAME) == len(INVENTORY)

"""CPU-only checks of the path analysis (lgc_bfs_init / _level / _resolve / _backtrack and paths.py above them): the
symbols and the ABI number, argument validation that happens before any launch, the tests' own numpy BFS against the
fixture captured from upstream's compute_paths (and against networkx where it imports), and paths_frame."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native
import paths_support as ps

HEADER = os.path.join(ROOT, "include", "lgconv_hip.h")
E_INVAL, E_RANGE = -1, -4
BFS = ("lgc_bfs_init", "lgc_bfs_level", "lgc_bfs_resolve", "lgc_bfs_backtrack")


def test_four_entry_points_in_header_table_and_library_with_abi_14():
    lib = _native.load()
    header = open(HEADER).read()
    assert int(re.search(r"#define LGC_ABI_VERSION (\d+)", header).group(1)) == 14
    assert lib.lgc_abi_version() == 14 and _native.ABI_VERSION == 14
    assert "src/inference_lightgcn.py:85-119" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in BFS:
        assert re.search(rf"\bint {name}\s*\(", code) and name in _native.SIGNATURES and hasattr(lib, name)
        assert _native.SIGNATURES[name][1][-1] is ctypes.c_void_p                    # the last argument is the stream
    assert int(re.search(r"#define LGC_BFS_MAX_SOURCES (\d+)", code).group(1)) == _native.BFS_MAX_SOURCES == 64
    assert int(re.search(r"#define LGC_BFS_UNSET \((-\d+)\)", code).group(1)) == _native.BFS_UNSET
    assert _native.BFS_UNSET not in (-1, -2)                                         # those two are results
    for name in ("hop_distances", "shortest_paths", "paths_frame", "compute_paths"):
        assert name in lg.__all__ and callable(getattr(lg, name))
    assert callable(lg.LightGCN.recommendation_paths)


def test_argument_errors_come_before_any_launch():
    lib = _native.load()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below must end in validation
    two = ctypes.c_void_p(32)

    def init(**kw):
        a = dict(src=one, ns=5, n=100, seen=one, fr=one, status=one)
        a.update(kw)
        return lib.lgc_bfs_init(a["src"], a["ns"], a["n"], a["seen"], a["fr"], a["status"], None)
    for bad in (dict(src=None), dict(seen=None), dict(fr=None), dict(status=None), dict(ns=-1), dict(n=-1)):
        assert init(**bad) == E_INVAL, bad
    assert init(ns=65) == E_RANGE and init(n=2 ** 31) == E_RANGE and init(n=2 ** 40) == E_RANGE
    assert init(ns=0) == 0
    assert init(ns=0, n=2 ** 31) == E_RANGE                                           # still validated

    def level(**kw):
        a = dict(rp=one, ent=one, rb=0, re=100, sm=32, ch=one, nc=3, active=1, fin=one, fout=two, seen=one, cnt=one)
        a.update(kw)
        return lib.lgc_bfs_level(a["rp"], a["ent"], a["rb"], a["re"], a["sm"], a["ch"], a["nc"], a["active"], a["fin"],
                                 a["fout"], a["seen"], a["cnt"], None)
    for bad in (dict(rp=None), dict(ent=None), dict(fin=None), dict(fout=None), dict(seen=None), dict(cnt=None),
                dict(rb=-1), dict(rb=101), dict(sm=-1), dict(nc=-1), dict(ch=None), dict(fout=one)):
        assert level(**bad) == E_INVAL, bad
    assert level(re=2 ** 31 - 1) == E_RANGE
    assert level(active=0) == 0 and level(re=0) == 0 and level(active=0, ch=None, nc=0) == 0

    def resolve(**kw):
        a = dict(src=one, tgt=one, ns=5, nt=20, n=100, fr=one, level=0, dist=one, cnt=one, status=one)
        a.update(kw)
        return lib.lgc_bfs_resolve(a["src"], a["tgt"], a["ns"], a["nt"], a["n"], a["fr"], a["level"], a["dist"], a["cnt"],
                                   a["status"], None)
    for bad in (dict(src=None), dict(tgt=None), dict(fr=None), dict(dist=None), dict(cnt=None), dict(status=None),
                dict(ns=-1), dict(nt=-1), dict(n=-1), dict(level=-1)):
        assert resolve(**bad) == E_INVAL, bad
    assert resolve(ns=65) == E_RANGE and resolve(n=2 ** 31) == E_RANGE and resolve(nt=2 ** 31) == E_RANGE
    assert resolve(ns=0) == 0 and resolve(nt=0) == 0

    def back(**kw):
        a = dict(rp=one, ent=one, n=100, lev=one, nl=8, tgt=one, dist=one, ns=5, nt=20, paths=one, pl=8)
        a.update(kw)
        return lib.lgc_bfs_backtrack(a["rp"], a["ent"], a["n"], a["lev"], a["nl"], a["tgt"], a["dist"], a["ns"], a["nt"],
                                     a["paths"], a["pl"], None)
    for bad in (dict(rp=None), dict(ent=None), dict(lev=None), dict(tgt=None), dict(dist=None), dict(paths=None),
                dict(n=-1), dict(nl=0), dict(ns=-1), dict(nt=-1), dict(pl=0)):
        assert back(**bad) == E_INVAL, bad
    assert back(ns=65) == E_RANGE and back(n=2 ** 31) == E_RANGE and back(nt=2 ** 31) == E_RANGE
    assert back(ns=0) == 0 and back(nt=0) == 0


def test_numpy_bfs_reproduces_upstreams_path_lens():
    z = ps.fixture()
    n = int(z["n_users"]) + int(z["n_items"])
    got = ps.reference(z["edge_index"], n, z["out_user_id_idx"], z["out_top_rlvnt_itm"])
    assert got.tolist() == z["path_lens"].tolist()
    assert got.max() >= 5                                                             # a fixture with depth
    # and the stored paths are walks of the stored graph of exactly that length, from the user to the item
    edges = set(map(tuple, z["edge_index"].T.tolist()))
    for r, row in enumerate(ps.trimmed(z["paths"])):
        for c, walk in enumerate(row):
            assert len(walk) == got[r, c] + 1 and walk[0] == z["out_user_id_idx"][r] and walk[-1] == z["out_top_rlvnt_itm"][r, c]
            assert all(step in edges for step in zip(walk, walk[1:]))


def test_numpy_bfs_is_networkx_on_the_ladder():
    nx = pytest.importorskip("networkx")
    edge_index, sources, targets = ps.ladder()
    graph = nx.Graph(edge_index.T.tolist())
    graph.add_nodes_from(range(ps.N_NODES))
    ref = ps.ladder_reference()
    for r in (0, 2, 3, 4, 5, 17, 129):
        lengths = nx.single_source_shortest_path_length(graph, int(sources[r]))
        assert ref[r].tolist() == [lengths.get(int(t), -1) for t in targets[r]]
        capped = nx.single_source_shortest_path_length(graph, int(sources[r]), cutoff=ps.MAX_HOPS)
        ended = max(lengths.values()) + 1 <= ps.MAX_HOPS
        want = [capped.get(int(t), -2 if (int(t) in lengths or not ended) else -1) for t in targets[r]]
        assert ps.ladder_reference_max_hops()[r].tolist() == want


def test_the_ladder_reference_is_not_vacuous():
    ref = ps.ladder_reference()
    values = set(np.unique(ref).tolist())
    assert {0, 1, 3, 5, -1} <= values and max(values) >= 7
    assert ref[0, :ps.CHAIN].tolist() == [2 * j + 1 for j in range(ps.CHAIN)] and ref[2, 0] == 0
    assert (ref[4] == -1).all()                                                       # the isolated user
    capped = ps.ladder_reference_max_hops()
    assert {-1, -2} <= set(np.unique(capped).tolist()) and (capped[4] == -1).all()
    assert ((capped == ref) | (capped == -2)).all() and (capped == ref)[(ref >= 0) & (ref <= ps.MAX_HOPS)].all()


def test_paths_frame_rebuilds_upstreams_frame_from_the_fixtures_arrays():
    z = ps.fixture()
    # the arrays in the order of the incoming frame: upstream's rows, un-sorted
    pos = {int(u): r for r, u in enumerate(z["out_user_id_idx"])}
    rows = [pos[int(u)] for u in z["hit_user_id_idx"]]
    frame = lg.paths_frame(ps.fixture_hit_frame(z), z["path_lens"][rows], z["paths"][rows])
    ps.assert_frame_is_fixture(frame, z)
    import torch
    again = lg.paths_frame(ps.fixture_hit_frame(z), torch.from_numpy(z["path_lens"][rows]), torch.from_numpy(z["paths"][rows]))
    ps.assert_frame_is_fixture(again, z)


def test_paths_frame_gives_an_empty_path_for_a_pair_without_one():
    import pandas as pd
    hit = pd.DataFrame({"user_id_idx": [0, 1], "top_rlvnt_itm": [[5, 6], [5, 7]]})
    dist = np.array([[1, -1], [3, 5]], dtype=np.int32)
    paths = np.full((2, 2, 4), -1, dtype=np.int64)
    paths[0, 0, :2] = [0, 5]
    paths[1, 0] = [1, 6, 0, 5]                                                        # (1, 7): 5 hops, too long to be kept
    frame = lg.paths_frame(hit, dist, paths)
    assert frame["user_id_idx"].tolist() == [1, 0]                                    # [3, 5] sorts above [1, -1]
    assert frame["path_lens"].tolist() == [[3, 5], [1, -1]]
    assert frame["longer_than_3"].tolist() == [True, False]
    assert frame["paths"].tolist() == [[[1, 6, 0, 5], []], [[0, 5], []]]
    assert list(hit.columns) == ["user_id_idx", "top_rlvnt_itm"]                      # the incoming frame is left alone
    with pytest.raises(ValueError):
        lg.paths_frame(hit, dist[:1], paths)
    # whatever columns the incoming frame has travel with their rows, a shuffled index and a column named _row included
    more = hit.assign(_row=["a", "b"], note=[7, 8]).set_index(pd.Index([10, 3]))
    frame = lg.paths_frame(more, dist, paths)
    assert list(frame.columns) == ["user_id_idx", "top_rlvnt_itm", "_row", "note", "path_lens", "longer_than_3", "paths"]
    assert frame["_row"].tolist() == ["b", "a"] and frame["note"].tolist() == [8, 7] and frame.index.tolist() == [3, 10]
    assert frame["paths"].tolist() == [[[1, 6, 0, 5], []], [[0, 5], []]]

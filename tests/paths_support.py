"""What the two path test modules share: the ladder graph, its sources and targets, and the reference -- a plain
level-synchronous numpy BFS, one source at a time (no networkx, no scipy: the GPU box may have neither)."""
import functools

import numpy as np

from conftest import load_golden

N_USERS, N_ITEMS = 6200, 900
N_NODES = N_USERS + N_ITEMS
CHAIN = 12                      # u0 - i0 - u1 - ... - i11 - u12
HUB_ITEM = 20                   # linked to users 20 .. 5019 and to u12: a 5001-entry row
MAX_HOPS = 4


def item(i):
    return N_USERS + i


@functools.lru_cache(maxsize=None)
def ladder():
    """(edge_index int64 [2, 2E] symmetric, sources int64 [130], targets int64 [130, 20]); treat as read-only."""
    rng = np.random.default_rng(0)
    pairs = [(0, 0), (0, 0), (0, 0)]                                    # edge (u0, i0) listed three times
    pairs += [(j, j) for j in range(1, CHAIN)] + [(j + 1, j) for j in range(CHAIN)]
    fans = np.arange(20, 5020)
    pairs += [(CHAIN, HUB_ITEM)] + [(int(u), HUB_ITEM) for u in fans]
    for u in fans:                                                      # each of them: 1-3 items of [30, 600)
        for i in rng.choice(np.arange(30, 600), size=int(rng.integers(1, 4)), replace=False):
            pairs.append((int(u), int(i)))
    second = np.stack([rng.integers(5100, 6100, size=4000), rng.integers(700, 850, size=4000)], axis=1)
    pairs += [(int(u), int(i)) for u, i in second]                      # a second component; duplicates stay
    pairs = np.array(pairs, dtype=np.int64)                             # users 6100+ and items 850+ are isolated
    u, i = pairs[:, 0], pairs[:, 1] + N_USERS
    edge_index = np.stack([np.concatenate([u, i]), np.concatenate([i, u])])
    rng = np.random.default_rng(1)
    sources = np.concatenate([[0, 0, 3, CHAIN, 6150, 5100], rng.integers(N_USERS, size=124)]).astype(np.int64)
    targets = N_USERS + rng.integers(N_ITEMS, size=(sources.size, 20)).astype(np.int64)
    targets[0, :CHAIN] = N_USERS + np.arange(CHAIN)
    targets[1] = targets[0]
    targets[2, 0] = 3                                                   # a user as a target: the source itself
    return edge_index, sources, targets


def bfs_all(edge_index, n_nodes, source):
    """int32 [n_nodes]: hops from ``source`` along the edges' source -> target direction, -1 = unreachable."""
    src, dst = edge_index
    dist = np.full(n_nodes, -1, dtype=np.int32)
    if not 0 <= source < n_nodes:
        return dist
    frontier = np.zeros(n_nodes, dtype=bool)
    frontier[source] = True
    dist[source] = 0
    level = 0
    while frontier.any():
        level += 1
        nxt = np.zeros(n_nodes, dtype=bool)
        nxt[dst[frontier[src]]] = True
        nxt &= dist < 0
        dist[nxt] = level
        frontier = nxt
    return dist


def reference(edge_index, n_nodes, sources, targets, max_hops=None):
    """int32 [S, T] as hop_distances defines it.  With ``max_hops``: the distance where it is at most max_hops, -2
    where it is larger, and for a pair without a path -1 if the source's search ended (a level without a new node)
    within max_hops levels, else -2."""
    out = np.empty(targets.shape, dtype=np.int32)
    cache = {}
    for r, s in enumerate(sources.tolist()):
        if s not in cache:
            cache[s] = bfs_all(edge_index, n_nodes, s)
        d_all = cache[s]
        ok = (targets[r] >= 0) & (targets[r] < n_nodes)
        d = np.where(ok, d_all[np.clip(targets[r], 0, n_nodes - 1)], -1)
        if max_hops is not None and 0 <= s < n_nodes:
            ended = int(d_all.max()) + 1 <= max_hops               # the first level without a new node
            d = np.where(d > max_hops, -2, np.where((d < 0) & ok & (not ended), -2, d))
        out[r] = d
    return out


@functools.lru_cache(maxsize=None)
def ladder_reference():
    edge_index, sources, targets = ladder()
    return reference(edge_index, N_NODES, sources, targets)


@functools.lru_cache(maxsize=None)
def ladder_reference_max_hops():
    edge_index, sources, targets = ladder()
    return reference(edge_index, N_NODES, sources, targets, MAX_HOPS)


def fixture():
    return load_golden("paths_ref")


def fixture_hit_frame(z):
    """The frame upstream's prepare_hit_df returned (the columns compute_paths reads), rows in its order."""
    import pandas as pd
    return pd.DataFrame({"user_id_idx": z["hit_user_id_idx"], "top_rlvnt_itm": z["hit_top_rlvnt_itm"].tolist()},
                        index=z["hit_user_id_idx"])


def trimmed(paths):
    """[S, k, L] -1 padded -> lists of lists."""
    return [[[int(v) for v in walk if v >= 0] for walk in row] for row in np.asarray(paths)]


def assert_frame_is_fixture(frame, z):
    assert frame.index.tolist() == z["out_index"].tolist()
    assert frame["user_id_idx"].tolist() == z["out_user_id_idx"].tolist()
    assert list(frame.columns[-3:]) == ["path_lens", "longer_than_3", "paths"]
    assert [str(frame[c].dtype) for c in ("path_lens", "longer_than_3", "paths")] == z["out_dtypes"].tolist()
    assert frame["path_lens"].tolist() == z["path_lens"].tolist()
    assert all(type(v) is int for row in frame["path_lens"] for v in row)
    assert frame["longer_than_3"].tolist() == z["longer_than_3"].tolist()
    assert frame["paths"].tolist() == trimmed(z["paths"])

#!/usr/bin/env python3
"""Fixture for the path analysis, captured from the reference's OWN code (run once in the build container, which has
networkx: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paths.py):

  paths_ref.npz   src/inference_lightgcn.py: InferenceLightGCN.prepare_hit_df -> create_store_nx_graph's graph ->
                  compute_paths on a connected, tree-shaped user|item graph (a tree makes every shortest path unique, so
                  the stored paths are THE paths; no two users share a path_lens list, so upstream's unstable sort has
                  one answer).  PyG is met by the oracle's LGConv as in make_golden_serve.py; `jsonpickle` (not
                  installed, used only to write the graph file) is an empty module.  Stored: the edge list in
                  df_to_graph's layout, the metrics frame's columns (ragged lists padded with -1), and the resulting
                  frame: row order, path_lens, longer_than_3, paths padded with -1, the dtypes of the three columns.
Only arrays are stored; no reference source travels."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import pandas as pd
import torch

from make_golden import save                                   # noqa: E402
from make_golden_serve import shim_pyg                         # noqa: E402

N_USERS, N_ITEMS, K = 14, 12, 3


def tree_edges(rng):
    """A random tree over users [0, N_USERS) and items [N_USERS, N_USERS + N_ITEMS) whose every edge joins a user and
    an item: nodes join one at a time, each under a node of the other kind, half of the time the latest one (depth)."""
    users, items, edges = [0], [], []
    todo = [("i", j) for j in range(N_ITEMS)] + [("u", j) for j in range(1, N_USERS)]
    rng.shuffle(todo)
    if todo[0][0] != "i":                                       # the first node to join must be an item (under user 0)
        first = next(n for n, t in enumerate(todo) if t[0] == "i")
        todo[0], todo[first] = todo[first], todo[0]
    for kind, j in todo:
        pool = users if kind == "i" else items
        parent = pool[-1] if rng.random() < 0.5 else pool[int(rng.integers(len(pool)))]
        if kind == "i":
            edges.append((parent, j))
            items.append(j)
        else:
            edges.append((j, parent))
            users.append(j)
    return np.array(edges, dtype=np.int64)                      # (user, item index without offset)


def paths_fixture():
    shim_pyg()
    sys.modules["jsonpickle"] = types.ModuleType("jsonpickle")
    sys.path.insert(0, "/root/reference")
    from src.inference_lightgcn import InferenceLightGCN
    from src import utils_v2 as utils

    rng = np.random.default_rng(414)
    pairs = tree_edges(rng)
    df = pd.DataFrame({"user_id_idx": pairs[:, 0], "item_id_idx": pairs[:, 1] + N_USERS,
                       "weight": np.ones(len(pairs), dtype=np.float32)})
    edge_index, edge_weight = utils.df_to_graph(df, True)

    # the metrics frame MARK_MAPK leaves (src/lightgcn.py:184-190): k recommended items per user, the user's positives
    # and their overlap; two users without a hit, whom prepare_hit_df drops
    top = np.stack([rng.permutation(N_ITEMS)[:K] for _ in range(N_USERS)])
    positives = []
    for u in range(N_USERS):
        own = [int(top[u, int(rng.integers(K))])] if u not in (4, 9) else []
        other = [int(i) for i in rng.permutation(N_ITEMS)[:2] if i not in top[u]]
        positives.append(own + other or [int(next(i for i in range(N_ITEMS) if i not in top[u]))])
    metrics = pd.DataFrame({"user_id_idx": np.arange(N_USERS), "item_id_idx_list": positives,
                            "user_ID": np.arange(N_USERS), "top_rlvnt_itm": top.tolist()})
    metrics["overlap_item"] = [list(set(a).intersection(b)) for a, b in zip(metrics.item_id_idx_list, metrics.top_rlvnt_itm)]

    inf = InferenceLightGCN.__new__(InferenceLightGCN)
    inf.n_users, inf.n_items = N_USERS, N_ITEMS
    inf.edge_index, inf.edge_weight = edge_index, edge_weight
    pd.options.mode.chained_assignment = None
    hit_df = inf.prepare_hit_df(metrics.copy())
    import networkx as nx
    edges, _ = edge_index.split(int(len(edge_weight) / 2), dim=1)          # create_store_nx_graph, minus the file
    graph = nx.Graph(edges.t().tolist())
    assert nx.is_tree(graph) and graph.number_of_nodes() == N_USERS + N_ITEMS
    hit_users = hit_df["user_id_idx"].to_numpy().copy()
    hit_top = np.array(hit_df["top_rlvnt_itm"].tolist(), dtype=np.int64)
    out = inf.compute_paths(hit_df, graph)

    lens = np.array(out["path_lens"].tolist(), dtype=np.int32)
    assert len({tuple(r) for r in lens.tolist()}) == len(lens), "two users share a path_lens list"
    assert lens.max() >= 5 and out["longer_than_3"].any() and not out["longer_than_3"].all()
    width = int(lens.max()) + 1
    walks = np.full((len(out), K, width), -1, dtype=np.int64)
    for r, row in enumerate(out["paths"]):
        for c, walk in enumerate(row):
            walks[r, c, :len(walk)] = walk

    def padded(lists):
        w = max(len(x) for x in lists)
        return np.array([list(x) + [-1] * (w - len(x)) for x in lists], dtype=np.int64)

    save("paths_ref", n_users=N_USERS, n_items=N_ITEMS, k=K, edge_index=edge_index, edge_weight=edge_weight,
         metrics_user_id_idx=metrics["user_id_idx"].to_numpy(), metrics_top_rlvnt_itm=top,
         metrics_item_id_idx_list=padded(metrics["item_id_idx_list"]), metrics_overlap_item=padded(metrics["overlap_item"]),
         hit_user_id_idx=hit_users, hit_top_rlvnt_itm=hit_top,
         out_user_id_idx=out["user_id_idx"].to_numpy(), out_index=out.index.to_numpy(),
         out_top_rlvnt_itm=np.array(out["top_rlvnt_itm"].tolist(), dtype=np.int64),
         path_lens=lens, longer_than_3=out["longer_than_3"].to_numpy(), paths=walks,
         out_dtypes=np.array([str(out[c].dtype) for c in ("path_lens", "longer_than_3", "paths")]))
    print(out[["user_id_idx", "path_lens", "longer_than_3"]])


if __name__ == "__main__":
    paths_fixture()

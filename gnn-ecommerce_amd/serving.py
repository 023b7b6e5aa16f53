"""Handler-shaped serving on the drop-in model: the build-side counterpart of
torchserve/lightgcn_handler.py (initialize / preprocess / inference / postprocess, SURVEY.md 8a a-S).

TorchServe itself is out of scope (and not installed): the class takes the same ``context`` object TorchServe hands a
handler -- ``context.manifest['model']['serializedFile']``, ``context.system_properties['model_dir' | 'gpu_id']`` -- and
returns what upstream returns, ``[{'items': [[k item indices], ...]}]``.  What differs is where the time goes:
  * ``initialize`` loads the persisted graph (``ingest.save_serving_graph``) instead of re-reading the CSV and
    rebuilding the COO (lightgcn_handler.py:32-38), and keeps the purchased-items lists on the device as a CSR;
  * ``inference`` calls ``LightGCN.recommendK`` with the graph object and the purchase lists (``SeenLists``): the K-layer
    propagate is reused across requests, scores / mask / top-k stay on the device (lgc_mask_topk builds the request's
    mask rows as bitmasks in LDS; the dense ``[n_sel, n_items]`` mask upstream materialises never exists);
  * ``inference`` also answers for visitors the model was not trained on: next to a plain user id a request element may be
    ``{"items": [...], "weights": [...] (optional), "user": id (optional)}`` -- the items the visitor looked at, put in
    the cart or bought (relabelled item indices, as the answers), upstream's event weights, and for a known user with a
    fresh list the user whose trained layer-0 row to start from (``LightGCN.recommend_sessions``, fold-in);
  * a body ``{"requests": [...], "explain": m}`` (``requests`` = what the body is otherwise, ``1 <= m <= 8``) is answered
    with ``{"items": [...], "because": [...]}``: the same items, and for recommended item j of request element p
    ``because[p][j] = {"base": float, "score": float, "items": [[item, contribution], ...]}`` -- the m items of the
    visitor's own list that contributed most to that item's raw (unmasked) score (``LightGCN.explain_topk`` /
    ``explain_sessions``, score attribution);
  * a body ``{"similar": [item ids], "k": int (optional, 1 .. 64, default 20), "metric": "cosine" | "dot" (optional)}`` asks
    about ITEMS: it is answered with ``{"items": [[...]], "scores": [[...]]}``, per asked-about item the most similar other
    items of the catalogue and their similarities, best first (``LightGCN.similar_items``);
  * a body ``{"requests": [...], "diversify": lam, "candidates": N (optional), "metric": "cosine" | "dot" (optional)}``
    (``requests`` = what the body is otherwise, ``0 <= lam <= 1``, ``k <= N <= 256``, default ``min(5 k, 256, n_items)``) is
    answered with ``{"items": [[...]]}`` in request order: per request element its N best items re-ranked by greedy
    maximal marginal relevance, so that the k returned are relevant AND unlike each other (``LightGCN.recommend_diverse`` /
    ``rerank_diverse``).  ``lam = 1`` is the plain answer.  It does not combine with ``"explain"``;
  * a body ``{"requests": [...], "filter": {"allow": [item ids]} | {"deny": [item ids]}, "k": int (optional, 1 .. 64)}`` is
    answered with ``{"items": [[...]]}`` in request order: per request element the k best items that pass the catalogue
    filter, with the user's purchased items (a visitor's own purchased items) REMOVED instead of zeroed.  Next to what
    ``requests`` otherwise holds an element may carry ``"exclude": [item ids]`` (what is in the cart), and ``{"user": id,
    "exclude": [...]}`` without ``"items"`` is a trained user with exclusions.  Places that no item fills are dropped.  It
    does not combine with ``"explain"`` or ``"diversify"`` (``LightGCN.recommend_filtered``);
  * a body ``{"audience": [item ids], "k": int (optional, 1 .. 64, default 20), "deny_users": [user ids] (optional)}`` asks
    about ITEMS' audiences: it is answered with ``{"users": [[...]], "scores": [[...]]}``, per item the users who score it
    best, its buyers and the denied users left out (``LightGCN.item_audience``);
  * a body ``{"bought_together": [item ids], "k": int (optional, 1 .. 64, default 20), "measure": "count" | "cosine" |
    "jaccard" (optional, default "cosine"), "min_count": int (optional, at least 1), "allow": [item ids] | "deny": [item ids]
    (optional)}`` asks what is BOUGHT TOGETHER with items: it is answered with ``{"items": [[...]], "scores": [[...]],
    "counts": [[...]]}``, per item the items that share most buyers with it, their scores and the numbers of shared buyers,
    from the handler's purchase lists alone (``cooccur.CoPurchase``, built once at ``initialize``); the model is not asked;
  * a body ``{"itemknn": [{"items": [item ids], "weights": [...] (optional)}, ...], "k": int (optional, 1 .. 64, default 20),
    "allow": [item ids] | "deny": [item ids] (optional)}`` asks the ITEM-KNN baseline about baskets: it is answered with
    ``{"items": [[...]], "scores": [[...]], "votes": [[...]]}``, per basket the items with the best sum of co-purchase
    similarities to the basket's items, the basket's own items removed, their scores and how many basket items voted for each
    (``itemknn.ItemKNN``, fitted once, on first use, from the handler's ``CoPurchase``); the model is not asked.
"""
from __future__ import annotations

import os
from typing import List

import torch

from . import _native
from .foldin import SessionLists
from .graph import PropGraph
from .lightgcn import LightGCN
from .propagate import SeenLists
from .retrieve import BuyerLists
from .cooccur import MEASURES, CoPurchase
from .itemknn import ItemKNN
from .rerank import check_lam
from .similar import METRICS

GRAPH_FILE = "graph.safetensors"


def load_checkpoint(path: str) -> dict:
    """A checkpoint in the layout of src/utils_v2.py:214-232 (``model_state_dict`` + ``hyperparams``), read with the
    loader that executes nothing from the file."""
    return torch.load(path, map_location="cpu", weights_only=True)


class RecommendHandler:
    def __init__(self):
        self.initialized = False

    def initialize(self, context) -> None:
        self.manifest = context.manifest
        properties = context.system_properties
        model_dir = properties.get("model_dir")
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("serving needs a ROCm device (no CPU fallback)")
        self.device = torch.device("cuda:" + str(properties.get("gpu_id") or 0))
        model_pt_path = os.path.join(model_dir, self.manifest["model"]["serializedFile"])
        if not os.path.isfile(model_pt_path):
            raise RuntimeError("Missing the model.pt file")                     # lightgcn_handler.py:29-30
        graph_path = os.path.join(model_dir, GRAPH_FILE)
        if not os.path.isfile(graph_path):
            raise RuntimeError(f"Missing {GRAPH_FILE} (write it once with gnn_ecommerce_amd.ingest.save_serving_graph)")
        self.graph, extra, meta = PropGraph.load(graph_path, self.device, with_extra=True)
        try:
            self.n_users, self.n_items = int(meta["n_users"]), int(meta["n_items"])
            self.seen_ptr, self.seen_items = extra["seen_ptr"].to(self.device), extra["seen_items"].to(self.device)
        except (KeyError, ValueError) as exc:
            raise ValueError(f"{graph_path}: not a serving graph ({exc!r} missing or malformed)") from exc
        # everything the request path takes on trust is checked here, once: node counts against the graph, the stored
        # user|item split against n_users, and the purchase lists lgc_mask_topk indexes without bounds
        if self.n_users < 1 or self.n_items < 1 or self.n_users + self.n_items != self.graph.num_nodes:
            raise ValueError(f"{graph_path}: n_users {self.n_users} + n_items {self.n_items} != {self.graph.num_nodes} nodes")
        if self.graph.split is not None and self.graph.split != self.n_users:
            raise ValueError(f"{graph_path}: bipartite split {self.graph.split} != n_users {self.n_users}")
        self.seen = SeenLists(self.seen_ptr, self.seen_items).validate(self.n_users, graph_path + ": purchase lists")
        self.copurchase = CoPurchase.from_seen(self.seen, self.n_users, self.n_items)
        self.buyers = self.copurchase.buyers
        state = load_checkpoint(model_pt_path)
        hp = state["hyperparams"]
        self.model = LightGCN(self.n_users + self.n_items, hp["latent_dim"], hp["n_layers"])
        self.model.load_state_dict(state["model_state_dict"])
        self.model.to(self.device).eval()
        self.k = 20                                                              # lightgcn_handler.py:90
        self.initialized = True

    def preprocess(self, data):
        body = data[0].get("data")
        if body is None:
            body = data[0].get("body")
        return body

    def seen_rows(self, users: torch.Tensor) -> torch.Tensor:
        """Dense fp32 [len(users), n_items] rows of the purchased-items matrix, built on the device."""
        lo, hi = self.seen_ptr[users], self.seen_ptr[users + 1]
        counts = hi - lo
        rows = torch.repeat_interleave(torch.arange(users.numel(), device=self.device), counts)
        first = torch.cumsum(counts, 0) - counts
        pos = torch.arange(int(counts.sum().item()), device=self.device) - first[rows] + lo[rows]
        out = torch.zeros((users.numel(), self.n_items), dtype=torch.float32, device=self.device)
        out[rows, self.seen_items[pos]] = 1.0
        return out

    def parse_sessions(self, data):
        """A request with at least one dict element, split by kind: ``(id_pos, ids, session_pos, lists, init_users)`` --
        the positions and values of the plain user ids, the positions of the dict elements, their ``(items, weights)``
        pairs and the user each starts from (-1: none).  A malformed element raises ValueError."""
        id_pos, ids, session_pos, lists, init_users = [], [], [], [], []
        for pos, el in enumerate(data):
            if isinstance(el, dict):
                unknown = set(el) - {"items", "weights", "user"}
                if unknown or "items" not in el:
                    raise ValueError(f"request element {pos}: expected 'items' and optionally 'weights', 'user'; got {sorted(el)}")
                items, weights, user = el["items"], el.get("weights"), el.get("user")
                if not isinstance(items, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) for i in items):
                    raise ValueError(f"request element {pos}: 'items' must be a list of item indices")
                if any(i < 0 or i >= self.n_items for i in items):
                    raise ValueError(f"request element {pos}: item index outside [0, {self.n_items})")
                if weights is not None:
                    if (not isinstance(weights, (list, tuple))
                            or any(isinstance(w, bool) or not isinstance(w, (int, float)) for w in weights)):
                        raise ValueError(f"request element {pos}: 'weights' must be a list of numbers")
                    if len(weights) != len(items):
                        raise ValueError(f"request element {pos}: {len(items)} items but {len(weights)} weights")
                if user is not None:
                    if isinstance(user, bool) or not isinstance(user, int) or user < 0 or user >= self.n_users:
                        raise ValueError(f"request element {pos}: 'user' outside [0, {self.n_users})")
                session_pos.append(pos)
                lists.append((list(items), None if weights is None else list(weights)))
                init_users.append(-1 if user is None else user)
            elif isinstance(el, int) and not isinstance(el, bool):
                id_pos.append(pos)
                ids.append(el)
            else:
                raise ValueError(f"request element {pos}: expected a user id or a dict with 'items', got {type(el).__name__}")
        return id_pos, ids, session_pos, lists, init_users

    def parse_explain(self, body):
        """``(requests, m)`` of a body ``{"requests": [...], "explain": m}``; anything else raises ValueError."""
        unknown = set(body) - {"requests", "explain"}
        if unknown or "requests" not in body or "explain" not in body:
            raise ValueError(f"request body: expected 'requests' and 'explain', got {sorted(map(str, body))}")
        requests, m = body["requests"], body["explain"]
        if not isinstance(requests, (list, tuple)):
            raise ValueError("request body: 'requests' must be a list of user ids and / or dicts with 'items'")
        if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= _native.ATTR_MAX_TOP:
            raise ValueError(f"request body: 'explain' must be an integer in [1, {_native.ATTR_MAX_TOP}]")
        return list(requests), m

    def parse_similar(self, body):
        """``(item ids, k, metric)`` of a body ``{"similar": [...], "k": optional, "metric": optional}``.  A malformed body
        raises ValueError, an item id outside ``[0, n_items)`` IndexError."""
        unknown = set(body) - {"similar", "k", "metric"}
        if unknown or "similar" not in body:
            raise ValueError(f"request body: expected 'similar' and optionally 'k', 'metric'; got {sorted(map(str, body))}")
        ids, k, metric = body["similar"], body.get("k", self.k), body.get("metric", "cosine")
        if not isinstance(ids, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) for i in ids):
            raise ValueError("request body: 'similar' must be a list of item indices")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.NEIGHBORS_MAX_K:
            raise ValueError(f"request body: 'k' must be an integer in [1, {_native.NEIGHBORS_MAX_K}]")
        if not isinstance(metric, str) or metric not in METRICS:
            raise ValueError(f"request body: 'metric' must be one of {list(METRICS)}")
        if any(i < 0 or i >= self.n_items for i in ids):
            raise IndexError(f"item index outside [0, {self.n_items})")
        return list(ids), k, metric

    def inference_similar(self, ids, k: int, metric: str):
        """Per asked-about item the ``k`` most similar other items and their similarities, best first; places that no
        item fills (a catalogue of fewer than k + 1 items) are dropped."""
        if not ids:
            return {"items": [], "scores": []}
        with torch.no_grad():
            index, value = self.model.similar_items(self.graph, None, self.n_users, self.n_items, ids, k, metric)
        index, value = index.cpu().tolist(), value.cpu().tolist()
        keep = [[j for j, i in enumerate(row) if i >= 0] for row in index]
        return {"items": [[row[j] for j in js] for row, js in zip(index, keep)],
                "scores": [[row[j] for j in js] for row, js in zip(value, keep)]}

    @staticmethod
    def _id_list(ids, what: str):
        if not isinstance(ids, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) for i in ids):
            raise ValueError(f"request body: {what} must be a list of indices")
        return list(ids)

    def _parse_k(self, body):
        k = body.get("k", self.k)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.RETRIEVE_MAX_K:
            raise ValueError(f"request body: 'k' must be an integer in [1, {_native.RETRIEVE_MAX_K}]")
        return k

    def parse_filtered(self, body):
        """``(requests, excludes, item_ok, k)`` of a body ``{"requests": [...], "filter": {...}, "k": optional}``:
        ``requests`` without the ``"exclude"`` keys (``{"user": id, "exclude": [...]}`` becomes the plain id), ``excludes``
        one list or None per element, ``item_ok`` a host uint8 ``[n_items]`` tensor or None.  A malformed body raises
        ValueError, an id outside its table IndexError."""
        for other in ("explain", "diversify"):
            if other in body:
                raise ValueError(f"request body: 'filter' and '{other}' do not combine")
        unknown = set(body) - {"requests", "filter", "k"}
        if unknown or "requests" not in body or "filter" not in body:
            raise ValueError(f"request body: expected 'requests', 'filter' and optionally 'k'; got {sorted(map(str, body))}")
        requests, flt, k = body["requests"], body["filter"], self._parse_k(body)
        if not isinstance(requests, (list, tuple)):
            raise ValueError("request body: 'requests' must be a list of user ids and / or dicts")
        if not isinstance(flt, dict) or set(flt) - {"allow", "deny"} or len(flt) > 1:
            raise ValueError("request body: 'filter' must be {'allow': [ids]} or {'deny': [ids]}")
        item_ok = None
        for name, ids in flt.items():
            ids = self._id_list(ids, f"'filter.{name}'")
            if any(i < 0 or i >= self.n_items for i in ids):
                raise IndexError(f"item index outside [0, {self.n_items})")
            item_ok = torch.full((self.n_items,), 1 if name == "deny" else 0, dtype=torch.uint8)
            item_ok[torch.tensor(ids, dtype=torch.int64)] = 0 if name == "deny" else 1
        plain, excludes = [], []
        for pos, el in enumerate(requests):
            extra = None
            if isinstance(el, dict) and "exclude" in el:
                extra = self._id_list(el["exclude"], f"element {pos}: 'exclude'")
                if any(i < 0 or i >= self.n_items for i in extra):
                    raise IndexError(f"item index outside [0, {self.n_items})")
                el = {key: v for key, v in el.items() if key != "exclude"}
                if set(el) == {"user"}:                      # a trained user with exclusions
                    el = el["user"]
            if isinstance(el, bool) or not isinstance(el, (int, dict)):
                raise ValueError(f"request element {pos}: expected a user id or a dict, got {type(el).__name__}")
            if isinstance(el, int) and (el < 0 or el >= self.n_users):
                raise IndexError(f"user index outside [0, {self.n_users})")
            plain.append(el)
            excludes.append(extra)
        return plain, excludes, item_ok, k

    def inference_filtered(self, data, excludes, item_ok, k: int):
        """Per request element the ``k`` best items that pass ``item_ok``, the purchased items and the element's
        ``exclude`` removed: trained users and interaction lists through ``recommend_filtered``, in request order."""
        id_pos, ids, session_pos, lists, init_users = self.parse_sessions(data)
        answers = [None] * len(data)
        if item_ok is not None:
            item_ok = item_ok.to(self.device)

        def keep(index, positions):
            for pos, row in zip(positions, index.cpu().tolist()):
                answers[pos] = [i for i in row if i >= 0]
        with torch.no_grad():
            if ids:
                extra = [excludes[pos] for pos in id_pos]
                index, _ = self.model.recommend_filtered(self.graph, None, self.n_users, self.n_items, self.seen, ids, k, item_ok,
                                                         extra if any(e is not None for e in extra) else None)
                keep(index, id_pos)
            if lists:
                sessions = SessionLists.from_lists(lists, self.device).validate(self.n_items, "request")
                rows = self.model.embed_sessions(self.graph, None, self.n_users, self.n_items, sessions,
                                                 init_users if any(u >= 0 for u in init_users) else None)
                index, _ = self.model.recommend_filtered(self.graph, None, self.n_users, self.n_items, sessions.mask("purchased"),
                                                         None, k, item_ok, [excludes[pos] for pos in session_pos], queries=rows)
                keep(index, session_pos)
        return {"items": answers}

    def parse_audience(self, body):
        """``(item ids, k, user_ok)`` of a body ``{"audience": [...], "k": optional, "deny_users": optional}``; ``user_ok`` a
        host uint8 ``[n_users]`` tensor or None.  A malformed body raises ValueError, an id outside its table IndexError."""
        unknown = set(body) - {"audience", "k", "deny_users"}
        if unknown or "audience" not in body:
            raise ValueError(f"request body: expected 'audience' and optionally 'k', 'deny_users'; got {sorted(map(str, body))}")
        ids, k = self._id_list(body["audience"], "'audience'"), self._parse_k(body)
        user_ok = None
        if "deny_users" in body:
            deny = self._id_list(body["deny_users"], "'deny_users'")
            if any(u < 0 or u >= self.n_users for u in deny):
                raise IndexError(f"user index outside [0, {self.n_users})")
            user_ok = torch.ones(self.n_users, dtype=torch.uint8)
            user_ok[torch.tensor(deny, dtype=torch.int64)] = 0
        if any(i < 0 or i >= self.n_items for i in ids):
            raise IndexError(f"item index outside [0, {self.n_items})")
        return ids, k, user_ok

    def inference_audience(self, ids, k: int, user_ok):
        """Per asked-about item the ``k`` users who score it best and their scores, best first, without the users who
        bought it (the transpose of the purchase lists, built once) and without the denied users; empty places dropped."""
        if not ids:
            return {"users": [], "scores": []}
        if getattr(self, "buyers", None) is None:
            self.buyers = BuyerLists.from_seen(self.seen, self.n_users, self.n_items)
        with torch.no_grad():
            index, value = self.model.item_audience(self.graph, None, self.n_users, self.n_items, ids, k, self.buyers,
                                                    None if user_ok is None else user_ok.to(self.device))
        index, value = index.cpu().tolist(), value.cpu().tolist()
        keep = [[j for j, i in enumerate(row) if i >= 0] for row in index]
        return {"users": [[row[j] for j in js] for row, js in zip(index, keep)],
                "scores": [[row[j] for j in js] for row, js in zip(value, keep)]}

    def parse_bought_together(self, body):
        """``(item ids, k, measure, min_count, item_ok)`` of a body ``{"bought_together": [...], "k": optional, "measure":
        optional, "min_count": optional, "allow" | "deny": optional}``; ``item_ok`` a host uint8 ``[n_items]`` tensor or None.
        A malformed body raises ValueError, an id outside the catalogue IndexError."""
        unknown = set(body) - {"bought_together", "k", "measure", "min_count", "allow", "deny"}
        if unknown or "bought_together" not in body:
            raise ValueError("request body: expected 'bought_together' and optionally 'k', 'measure', 'min_count', 'allow' or "
                             f"'deny'; got {sorted(map(str, body))}")
        if "allow" in body and "deny" in body:
            raise ValueError("request body: 'allow' and 'deny' do not combine")
        ids, k = self._id_list(body["bought_together"], "'bought_together'"), body.get("k", self.k)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.COOCCUR_MAX_K:
            raise ValueError(f"request body: 'k' must be an integer in [1, {_native.COOCCUR_MAX_K}]")
        measure, min_count = body.get("measure", "cosine"), body.get("min_count", 1)
        if not isinstance(measure, str) or measure not in MEASURES:
            raise ValueError(f"request body: 'measure' must be one of {list(MEASURES)}")
        if isinstance(min_count, bool) or not isinstance(min_count, int) or not 1 <= min_count < 2 ** 31:
            raise ValueError("request body: 'min_count' must be an integer of at least 1")
        item_ok = None
        for name in ("allow", "deny"):
            if name in body:
                listed = self._id_list(body[name], f"'{name}'")
                if any(i < 0 or i >= self.n_items for i in listed):
                    raise IndexError(f"item index outside [0, {self.n_items})")
                item_ok = torch.full((self.n_items,), 1 if name == "deny" else 0, dtype=torch.uint8)
                item_ok[torch.tensor(listed, dtype=torch.int64)] = 0 if name == "deny" else 1
        if any(i < 0 or i >= self.n_items for i in ids):
            raise IndexError(f"item index outside [0, {self.n_items})")
        return ids, k, measure, min_count, item_ok

    def inference_bought_together(self, ids, k: int, measure: str, min_count: int, item_ok):
        """Per asked-about item the ``k`` items that share most buyers with it, their scores and the shared buyers of each,
        best first, from the purchase lists (transposed once); empty places dropped."""
        if not ids:
            return {"items": [], "scores": [], "counts": []}
        if getattr(self, "copurchase", None) is None:
            self.copurchase = CoPurchase.from_seen(self.seen, self.n_users, self.n_items)
        index, value, count = self.copurchase.neighbors(ids, k, measure, min_count, item_ok)
        index, value, count = index.cpu().tolist(), value.cpu().tolist(), count.cpu().tolist()
        keep = [[j for j, i in enumerate(row) if i >= 0] for row in index]
        return {"items": [[row[j] for j in js] for row, js in zip(index, keep)],
                "scores": [[row[j] for j in js] for row, js in zip(value, keep)],
                "counts": [[row[j] for j in js] for row, js in zip(count, keep)]}

    def parse_itemknn(self, body):
        """``(lists, k, item_ok)`` of a body ``{"itemknn": [{"items": [...], "weights": optional}, ...], "k": optional,
        "allow" | "deny": optional}``: ``lists`` one ``(items, weights or None)`` pair per basket, ``item_ok`` a host uint8
        ``[n_items]`` tensor or None.  A malformed body or basket raises ValueError, an id outside the catalogue IndexError."""
        unknown = set(body) - {"itemknn", "k", "allow", "deny"}
        if unknown or "itemknn" not in body:
            raise ValueError(f"request body: expected 'itemknn' and optionally 'k', 'allow' or 'deny'; got {sorted(map(str, body))}")
        if "allow" in body and "deny" in body:
            raise ValueError("request body: 'allow' and 'deny' do not combine")
        baskets, k = body["itemknn"], body.get("k", self.k)
        if not isinstance(baskets, (list, tuple)):
            raise ValueError("request body: 'itemknn' must be a list of baskets, dicts with 'items'")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _native.KNN_MAX_K:
            raise ValueError(f"request body: 'k' must be an integer in [1, {_native.KNN_MAX_K}]")
        lists = []
        for pos, el in enumerate(baskets):
            if not isinstance(el, dict) or set(el) - {"items", "weights"} or "items" not in el:
                raise ValueError(f"basket {pos}: expected a dict with 'items' and optionally 'weights'")
            items, weights = self._id_list(el["items"], f"basket {pos}: 'items'"), el.get("weights")
            if weights is not None:
                if (not isinstance(weights, (list, tuple))
                        or any(isinstance(w, bool) or not isinstance(w, (int, float)) for w in weights)):
                    raise ValueError(f"basket {pos}: 'weights' must be a list of numbers")
                if len(weights) != len(items):
                    raise ValueError(f"basket {pos}: {len(items)} items but {len(weights)} weights")
                weights = list(weights)
            lists.append((items, weights))
        item_ok = None
        for name in ("allow", "deny"):
            if name in body:
                listed = self._id_list(body[name], f"'{name}'")
                if any(i < 0 or i >= self.n_items for i in listed):
                    raise IndexError(f"item index outside [0, {self.n_items})")
                item_ok = torch.full((self.n_items,), 1 if name == "deny" else 0, dtype=torch.uint8)
                item_ok[torch.tensor(listed, dtype=torch.int64)] = 0 if name == "deny" else 1
        if any(i < 0 or i >= self.n_items for items, _ in lists for i in items):
            raise IndexError(f"item index outside [0, {self.n_items})")
        return lists, k, item_ok

    def inference_itemknn(self, lists, k: int, item_ok):
        """Per basket the ``k`` items with the best sum of co-purchase similarities to the basket's items, their scores and
        votes, best first, the basket's own items removed; empty places dropped.  The neighbour table is fitted on first
        use from the purchase lists and kept."""
        if not lists:
            return {"items": [], "scores": [], "votes": []}
        if getattr(self, "itemknn", None) is None:
            if getattr(self, "copurchase", None) is None:
                self.copurchase = CoPurchase.from_seen(self.seen, self.n_users, self.n_items)
            self.itemknn = ItemKNN.fit(self.copurchase)
        index, value, votes = self.itemknn.recommend_sessions(SessionLists.from_lists(lists, self.device), k, item_ok=item_ok)
        index, value, votes = index.cpu().tolist(), value.cpu().tolist(), votes.cpu().tolist()
        keep = [[j for j, i in enumerate(row) if i >= 0] for row in index]
        return {"items": [[row[j] for j in js] for row, js in zip(index, keep)],
                "scores": [[row[j] for j in js] for row, js in zip(value, keep)],
                "votes": [[row[j] for j in js] for row, js in zip(votes, keep)]}

    def parse_diversify(self, body):
        """``(requests, lam, candidates, metric)`` of a body ``{"requests": [...], "diversify": lam, "candidates": optional,
        "metric": optional}``.  A malformed body raises ValueError, a user id outside ``[0, n_users)`` IndexError."""
        if "diversify" in body and "explain" in body:
            raise ValueError("request body: 'diversify' and 'explain' do not combine")
        unknown = set(body) - {"requests", "diversify", "candidates", "metric"}
        if unknown or "requests" not in body or "diversify" not in body:
            raise ValueError("request body: expected 'requests', 'diversify' and optionally 'candidates', 'metric'; "
                             f"got {sorted(map(str, body))}")
        requests, metric = body["requests"], body.get("metric", "cosine")
        if not isinstance(requests, (list, tuple)):
            raise ValueError("request body: 'requests' must be a list of user ids and / or dicts with 'items'")
        try:
            lam = check_lam(body["diversify"])
        except ValueError as exc:
            raise ValueError("request body: 'diversify' must be a real number in [0, 1]") from exc
        top = _native.RERANK_MAX_CAND
        candidates = body.get("candidates", max(self.k, min(5 * self.k, top, self.n_items)))
        if isinstance(candidates, bool) or not isinstance(candidates, int) or not self.k <= candidates <= top:
            raise ValueError(f"request body: 'candidates' must be an integer in [{self.k}, {top}]")
        if not isinstance(metric, str) or metric not in METRICS:
            raise ValueError(f"request body: 'metric' must be one of {list(METRICS)}")
        for pos, el in enumerate(requests):
            if isinstance(el, dict):
                continue                                     # parse_sessions judges these
            if isinstance(el, bool) or not isinstance(el, int):
                raise ValueError(f"request element {pos}: expected a user id or a dict with 'items', got {type(el).__name__}")
            if el < 0 or el >= self.n_users:
                raise IndexError(f"user index outside [0, {self.n_users})")
        return list(requests), lam, candidates, metric

    def inference_diverse(self, data, lam: float, candidates: int, metric: str):
        """Per request element ``k`` items out of its ``candidates`` best, chosen by greedy maximal marginal relevance: plain
        ids through ``recommend_diverse``, interaction lists through ``recommend_sessions`` (with its masked scores) and
        ``rerank_diverse``; the answers come back in request order."""
        id_pos, ids, session_pos, lists, init_users = self.parse_sessions(data)
        answers = [None] * len(data)
        n_cand = min(candidates, self.n_items)
        with torch.no_grad():
            if ids:
                top = self.model.recommend_diverse(self.graph, None, self.n_users, self.n_items, self.seen, ids, self.k,
                                                   candidates, lam, metric)
                for pos, row in zip(id_pos, top.cpu().tolist()):
                    answers[pos] = row
            if lists:
                sessions = SessionLists.from_lists(lists, self.device).validate(self.n_items, "request")
                top, value = self.model.recommend_sessions(self.graph, None, self.n_users, self.n_items, sessions,
                                                           init_users if any(u >= 0 for u in init_users) else None, n_cand,
                                                           return_values=True)
                top = self.model.rerank_diverse(self.graph, None, self.n_users, self.n_items, top, value, self.k, lam, metric)
                for pos, row in zip(session_pos, top.cpu().tolist()):
                    answers[pos] = row
        return {"items": answers}

    def inference_explained(self, data, m: int):
        """The answer of ``inference(data)`` plus, per recommended item, the ``m`` items of the visitor's own list that
        contributed most to its score.  The scores explained are the raw ones: a seen item that the mask zeroed is
        explained by its score before the mask."""
        if any(isinstance(el, dict) for el in data):
            id_pos, ids, session_pos, lists, init_users = self.parse_sessions(data)
        else:                                                # ids alone: whatever the plain path takes (int(u))
            id_pos, ids, session_pos, lists, init_users = list(range(len(data))), [int(u) for u in data], [], [], []
        if not data:
            return {"items": [], "because": []}
        answers = self.inference(data)["items"]
        because = [None] * len(data)

        def rows_of(got, positions):
            base, total = got.base.cpu().tolist(), got.total.cpu().tolist()
            item, value = got.top_item.cpu().tolist(), got.top_value.cpu().tolist()
            for r, pos in enumerate(positions):
                because[pos] = [{"base": base[r][j], "score": total[r][j],
                                 "items": [[i, v] for i, v in zip(item[r][j], value[r][j]) if i >= 0]}
                                for j in range(len(answers[pos]))]
        with torch.no_grad():
            if ids:
                top = torch.tensor([answers[pos] for pos in id_pos], dtype=torch.int64)
                rows_of(self.model.explain_topk(self.graph, None, self.n_users, self.n_items, ids, top, m), id_pos)
            if lists:
                sessions = SessionLists.from_lists(lists, self.device).validate(self.n_items, "request")
                top = torch.tensor([answers[pos] for pos in session_pos], dtype=torch.int64)
                rows_of(self.model.explain_sessions(self.graph, None, self.n_users, self.n_items, sessions, top,
                                                    init_users if any(u >= 0 for u in init_users) else None, m), session_pos)
        return {"items": answers, "because": because}

    def inference(self, data, *args, **kwargs):
        if isinstance(data, dict):
            if "bought_together" in data:
                return self.inference_bought_together(*self.parse_bought_together(data))
            if "itemknn" in data:
                return self.inference_itemknn(*self.parse_itemknn(data))
            if "similar" in data:
                return self.inference_similar(*self.parse_similar(data))
            if "audience" in data:
                return self.inference_audience(*self.parse_audience(data))
            if "filter" in data:
                return self.inference_filtered(*self.parse_filtered(data))
            if "diversify" in data:
                return self.inference_diverse(*self.parse_diversify(data))
            return self.inference_explained(*self.parse_explain(data))
        if any(isinstance(el, dict) for el in data):
            return self._inference_sessions(data)
        users = [int(u) for u in data]
        if any(u < 0 or u >= self.n_users for u in users):      # upstream's embedding gather raises IndexError as well
            raise IndexError(f"user index outside [0, {self.n_users})")
        with torch.no_grad():
            # the purchase lists stay a CSR on the device; lgc_mask_topk turns the request's rows into LDS bitmasks
            frame = self.model.recommendK(self.graph, None, self.n_users, self.n_items, self.seen, list(data), self.k)
            return {"items": list(frame["top_rlvnt_itm"])}

    def _inference_sessions(self, data):
        """A request that holds interaction lists: the dict elements go through ``recommend_sessions`` in one batch, the
        plain ids through ``recommendK`` as a request of ids alone would; the answers come back in request order."""
        id_pos, ids, session_pos, lists, init_users = self.parse_sessions(data)
        if any(u < 0 or u >= self.n_users for u in ids):
            raise IndexError(f"user index outside [0, {self.n_users})")
        answers = [None] * len(data)
        with torch.no_grad():
            sessions = SessionLists.from_lists(lists, self.device).validate(self.n_items, "request")
            top = self.model.recommend_sessions(self.graph, None, self.n_users, self.n_items, sessions,
                                                init_users if any(u >= 0 for u in init_users) else None, self.k)
            if ids:
                frame = self.model.recommendK(self.graph, None, self.n_users, self.n_items, self.seen, ids, self.k)
                for pos, row in zip(id_pos, frame["top_rlvnt_itm"]):
                    answers[pos] = row
            for pos, row in zip(session_pos, top.cpu().tolist()):
                answers[pos] = row
        return {"items": answers}

    def postprocess(self, data) -> List[dict]:
        return [data]

    def handle(self, data, context=None):
        return self.postprocess(self.inference(self.preprocess(data)))

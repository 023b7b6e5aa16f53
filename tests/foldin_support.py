"""References for the fold-in tests (no product code here): an fp64 statement of the formula

    e = a0 * z + sum_k c_k * F[i_k],   c_k = dis[i_k] * w_k * d,   d = (sum_k w_k)^-1/2  (inf -> 0)

an fp32 numpy emulation of the order lgc_fold_in specifies (sequential degree, correctly rounded 1 / sqrt, every
product rounded, adds in list order, the a0 * z term last), the derived element bound, and the CPU-oracle side of the
identity: the fold table and the augmented one-way graph."""
import numpy as np
import torch

from oracle import lightgcn_oracle as oracle

U = 2.0 ** -24                     # unit roundoff of fp32
f32 = np.float32


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if lists else np.zeros(0, dtype=np.int64)
    return ptr, items.astype(np.int64)


def _row(ptr, items, weights, r, n_items):
    """Entries of row r that count: items in range (the others are skipped altogether), with their weights."""
    it = items[ptr[r]:ptr[r + 1]]
    w = np.ones(len(it), dtype=f32) if weights is None else weights[ptr[r]:ptr[r + 1]].astype(f32)
    ok = (it >= 0) & (it < n_items)
    return it[ok], w[ok]


def reference64(ptr, items, weights, item_dis, fold, init_rows, init, a0, normalize):
    """(y, S) in fp64: the formula on the fp32 inputs, and S = sum_k |c_k F[i_k]| + |a0 z| per element."""
    n_rows, (n_items, dim) = len(ptr) - 1, fold.shape
    y, s = np.zeros((n_rows, dim)), np.zeros((n_rows, dim))
    fold64 = fold.astype(np.float64)
    for r in range(n_rows):
        it, w = _row(ptr, items, weights, r, n_items)
        w = w.astype(np.float64)
        c = w
        if normalize:
            deg = w.sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                d = 1.0 / np.sqrt(deg) if len(w) else np.inf
            d = 0.0 if np.isinf(d) else d
            c = item_dis[it].astype(np.float64) * w * d
        terms = c[:, None] * fold64[it]
        y[r], s[r] = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        if init_rows is not None and 0 <= init_rows[r] < init.shape[0]:
            z = float(f32(a0)) * init[init_rows[r]].astype(np.float64)
            y[r] += z
            s[r] += np.abs(z)
    return y, s


def emulate32(ptr, items, weights, item_dis, fold, init_rows, init, a0, normalize):
    """The specified fp32 order, one rounding per operation (numpy's fp32 add, multiply, divide and sqrt are IEEE)."""
    n_rows, (n_items, dim) = len(ptr) - 1, fold.shape
    out = np.zeros((n_rows, dim), dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(n_rows):
            it, w = _row(ptr, items, weights, r, n_items)
            d = f32(1.0)
            if normalize:
                deg = f32(0.0)
                for wk in w:
                    deg = f32(deg + wk)
                d = f32(f32(1.0) / np.sqrt(deg, dtype=f32))
                if np.isinf(d):
                    d = f32(0.0)
            acc = np.zeros(dim, dtype=f32)
            for i, wk in zip(it, w):
                c = f32(f32(item_dis[i] * wk) * d) if normalize else wk
                acc = (acc + (c * fold[i]).astype(f32)).astype(f32)
            if init_rows is not None and 0 <= init_rows[r] < init.shape[0]:
                acc = (acc + (f32(a0) * init[init_rows[r]]).astype(f32)).astype(f32)
            out[r] = acc
    return out


def bound(ptr, items, n_items, s):
    """|y - y64| <= (1.5 n + 8) u S per element, n = the entries of the row that count.  Terms: the degree sum (n - 1) u,
    halved by the square root; 2 u for sqrt and divide; 2 u for the two products of c; u for the product with F;
    (n - 1) u for the adds; 2 u for the epilogue; 2.5 u of slack for second-order terms.  Valid for positive weights."""
    n = np.array([((items[ptr[r]:ptr[r + 1]] >= 0) & (items[ptr[r]:ptr[r + 1]] < n_items)).sum() for r in range(len(ptr) - 1)])
    return (1.5 * n + 8.0)[:, None] * U * s


# ---------------------------------------------------------------------------------------------------------------
# the oracle's side of the identity
# ---------------------------------------------------------------------------------------------------------------
def small_graph(n_users, n_items, n_pairs, seed):
    """(edge_index, edge_weight) in the reference's layout; every node has an edge; weights of the event rules."""
    rng = np.random.default_rng(seed)
    keys = np.unique(np.concatenate([np.arange(n_users) * n_items + rng.integers(n_items, size=n_users),
                                     rng.integers(n_users, size=n_items) * n_items + np.arange(n_items),
                                     rng.integers(n_users * n_items, size=n_pairs)]))
    rng.shuffle(keys)
    u, i = torch.from_numpy(keys // n_items), torch.from_numpy(keys % n_items + n_users)
    w = torch.from_numpy(np.array([0.01, 0.1, 1.0], dtype=f32)[rng.integers(3, size=len(keys))])
    return oracle.pairs_to_graph(u, i, w)


def oracle_fold_table(weight, alpha, edge_index, edge_weight, num_layers, n_users):
    """(F, item_dis) on the CPU: F = sum_{l<K} alpha_{l+1} x_l[items] with the oracle's hop, dis as its gcn_norm."""
    x = weight
    fold = x * alpha[1]
    for layer in range(1, num_layers):
        x = oracle.lgconv(x, edge_index, edge_weight)
        fold = fold + x * alpha[layer + 1]
    deg = torch.zeros(weight.size(0)).scatter_add_(0, edge_index[1], edge_weight)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0.0)
    return fold[n_users:].contiguous(), dis[n_users:].contiguous()


def augmented(weight, edge_index, edge_weight, n_users, lists, weights, init_rows):
    """The trained graph plus one node per list with ONE-WAY edges item -> node, and the node's layer-0 row (the row of
    ``init_rows[r]``, or zeros for -1).  Returns (weight, edge_index, edge_weight) of the larger graph."""
    n = weight.size(0)
    src = torch.cat([torch.as_tensor(x, dtype=torch.int64) + n_users for x in lists])
    dst = torch.cat([torch.full((len(x),), n + r, dtype=torch.int64) for r, x in enumerate(lists)])
    w = torch.cat([torch.as_tensor(x, dtype=torch.float32) for x in weights])
    rows = torch.stack([weight[u] if u >= 0 else torch.zeros(weight.size(1)) for u in init_rows])
    return (torch.cat([weight, rows]), torch.cat([edge_index, torch.stack([src, dst])], dim=1), torch.cat([edge_weight, w]))

"""Graphs and host restatements for the reference's TopologicalSort (1-byte messages, 4-byte sums), IncrementalPageRank (fp64
messages, 24-byte vertex property) and DeltaStepping at a size where every row class of the engine occurs
(tests/test_gpu_type_widths.py runs the applications, tests/test_type_widths_cpu.py checks what is stated here without a GPU).

The applications print only their first 10 or 25 vertices, so the generators put the interesting rows there."""
import numpy as np

from graphmat_amd.generators import splitmix64

N = 60000
# in-degrees of vertices 1..16 of the ladder graph: giant rows of five, three, two and two 4096-edge pieces (the giant threshold of such a
# graph is 4096), the largest wave row, both sides of GM_LONG_MID (1024) and of GM_SHORT_ROW (64), and the smallest rows
LADDER = (20000, 8193, 8192, 4097, 4096, 1025, 1024, 300, 129, 128, 65, 64, 63, 2, 1, 0)
# in-degrees of vertices 1..10 of the layered DAG, and the layer each of them lies in
DAG_LADDER = (20000, 8193, 4097, 4096, 1025, 300, 65, 64, 2, 1)
DAG_LADDER_LAYER = (0, 1, 3, 5, 7, 9, 12, 15, 18, 21)
DAG_LAYERS = 24


def _unique_pairs(src, dst):
    key = np.unique(src.astype(np.int64) * (1 << 32) + dst.astype(np.int64))
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)


def hashed_weights(src, dst, top):
    """1..top, a function of the edge's end points alone"""
    key = src.astype(np.uint64) * np.uint64(1 << 32) + dst.astype(np.uint64)
    return (1 + (splitmix64(key) % np.uint64(top))).astype(np.int32)


def ladder_edges(n=N, seed=7, weights="ones"):
    """Vertices 1..16 receive exactly LADDER[i] edges from distinct sources among 17..n; the other vertices lie on a ring
    17 -> 18 -> ... -> n -> 17 and receive about 3n random edges from anywhere.  No edge occurs twice.
    weights: "ones" -> 1, "hash" -> 1..64 by a hash of the end points.  Returns (nv, src, dst, val), 1-based ids."""
    rng = np.random.default_rng(seed)
    hubs = len(LADDER)
    rest = np.arange(hubs + 1, n + 1, dtype=np.int64)
    src, dst = [], []
    for h, deg in enumerate(LADDER):
        src.append(rng.choice(rest, size=deg, replace=False))
        dst.append(np.full(deg, h + 1, np.int64))
    src.append(rest)
    dst.append(np.roll(rest, -1))
    src.append(rng.integers(1, n + 1, size=3 * n))
    dst.append(rng.integers(hubs + 1, n + 1, size=3 * n))
    s, d = _unique_pairs(np.concatenate(src), np.concatenate(dst))
    order = rng.permutation(s.size)  # (the file order is not the stored order)
    s, d = s[order], d[order]
    val = np.ones(s.size, np.int32) if weights == "ones" else hashed_weights(s, d, 64)
    return n, s, d, val


def dag_layers(n=N):
    """layer of every vertex (index 0 unused): the ladder vertices as listed, the others by their id"""
    layer = np.arange(n + 1, dtype=np.int64) % DAG_LAYERS
    layer[1:len(DAG_LADDER) + 1] = DAG_LADDER_LAYER
    return layer


def layered_dag_edges(n=N, seed=11):
    """A DAG of DAG_LAYERS layers whose edges run only from a higher-numbered layer to a lower one.  Vertices 1..10 receive exactly
    DAG_LADDER[i] edges from distinct sources spread over all the layers above their own; every other vertex below the top layer receives
    about 3 edges from random vertices of higher layers.  No edge occurs twice.  Returns (nv, src, dst, val)."""
    rng = np.random.default_rng(seed)
    layer = dag_layers(n)
    ids = np.arange(1, n + 1, dtype=np.int64)
    others = ids[len(DAG_LADDER):]
    src, dst = [], []
    for i, deg in enumerate(DAG_LADDER):
        above = others[layer[others] > DAG_LADDER_LAYER[i]]
        src.append(rng.choice(above, size=deg, replace=False))
        dst.append(np.full(deg, i + 1, np.int64))
    for l in range(DAG_LAYERS - 1):
        here = others[layer[others] == l]
        above = ids[layer[ids] > l]
        src.append(rng.choice(above, size=3 * here.size))
        dst.append(np.repeat(here, 3))
    s, d = _unique_pairs(np.concatenate(src), np.concatenate(dst))
    order = rng.permutation(s.size)
    s, d = s[order], d[order]
    return n, s, d, np.ones(s.size, np.int32)


def topsort_orders(nv, src, dst, layer=None):
    """What TopologicalSort assigns: 0 to a vertex without in-edges, else 1 + the largest order among its in-neighbours.  With the
    layers of a layered DAG (edges from higher to lower layers) one vectorised pass per layer, from the top down; without them the
    passes are repeated until nothing moves (any DAG)."""
    order = np.zeros(nv + 1, np.int64)
    if layer is not None:
        assert (layer[src] > layer[dst]).all()
        for l in range(int(layer.max()) - 1, -1, -1):
            e = layer[dst] == l
            np.maximum.at(order, dst[e], order[src[e]] + 1)
        return order
    for _ in range(nv + 1):
        nxt = np.zeros(nv + 1, np.int64)
        np.maximum.at(nxt, dst, order[src] + 1)
        if (nxt == order).all():
            return order
        order = nxt
    raise ValueError("the graph has a cycle")


def kahn_orders(nv, src, dst):
    """The same by a plain Kahn pass (a queue of vertices whose in-edges are all accounted for); raises on a cycle."""
    out = [[] for _ in range(nv + 1)]
    pending = [0] * (nv + 1)
    for a, b in zip(src.tolist(), dst.tolist()):
        out[a].append(b)
        pending[b] += 1
    order = [0] * (nv + 1)
    queue = [v for v in range(1, nv + 1) if pending[v] == 0]
    done = 0
    while queue:
        nxt = []
        for v in queue:
            done += 1
            for w in out[v]:
                order[w] = max(order[w], order[v] + 1)
                pending[w] -= 1
                if pending[w] == 0:
                    nxt.append(w)
        queue = nxt
    if done != nv:
        raise ValueError("the graph has a cycle")
    return np.array(order, np.int64)


def file_order_spmv(nv, src, dst):
    """y = sum of the present messages over the in-edges, added in the order of the edge list (plain numpy loop)"""
    def spmv(msg, active):
        y = np.zeros(nv)
        got = np.zeros(nv, bool)
        for a, b in zip(src - 1, dst - 1):
            if active[a]:
                y[b] += msg[a]
                got[b] = True
        return y, got
    return spmv


def oracle_spmv(og):
    """the same through the oracle: the reference's fold order (ascending native id of the source), fp64.  The oracle multiplies by the
    edge value, which must be 1."""
    assert og.val is None or (og.val == 1).all()

    def spmv(msg, active):
        y, got = og.spmv_f64(msg, active.astype(np.uint8), ORACLE_TRANSPOSE)
        return y, got.astype(bool)
    return spmv


ORACLE_TRANSPOSE = 1  # messages travel along the out-edges: y[dst] += x[src]


def incremental_pagerank(nv, src, spmv, alpha=0.3):
    """IncrementalPageRank's recurrence (fp64 deltas, ACTIVE_ONLY, until no rank moves by more than 1e-8).
    Returns (pagerank[nv], out-degree[nv], iterations)."""
    outdeg = np.bincount(src - 1, minlength=nv)
    delta = np.full(nv, 0.3)
    pr = np.full(nv, 0.3)
    active = np.ones(nv, bool)
    iters = 0
    while True:
        msg = np.where(outdeg > 0, delta / np.maximum(outdeg, 1), 0.0)
        y, got = spmv(msg, active)
        old = pr.copy()
        big = got & (np.abs(delta) > 1e-8)
        delta[big] = 0.0
        delta[got] = delta[got] + (1.0 - alpha) * y[got]
        moved = got & (np.abs(delta) > 1e-8)
        pr[moved] = pr[moved] + delta[moved]
        active = np.abs(pr - old) > 1e-8
        iters += 1
        if not active.any():
            break
    return pr, outdeg, iters

"""Minimum spanning forest without a GPU: the graphs, a plain Kruskal as the reference and the complete verifier that the GPU tests
use (tests/test_gpu_spanning_forest.py imports them from here), the reference checked against networkx and scipy, the verifier
shown to reject wrong forests; the error convention of gm_run_spanning_forest; the symbol, the workspace slot names and the option
in the header, the binding and the library.

Semantics (exact integers): the undirected multigraph under the edge list -- directions do not matter, self-loops are ignored,
parallel and antiparallel edges are separate candidates; a weight is a signed int32.  A minimum spanning forest has nv - ncomponents
edges, spans every weakly connected component and has the minimum total weight (int64).  Every edge is reported as (u, v, w),
1-based, u < v, the rows sorted by (w, u, v).  With distinct weights the forest is unique; with ties only the total and the sorted
list of weights are."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests.test_components_cpu import restatement as component_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM_ERR_INVALID = 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------- graphs: edges are 1-based (src, dst, weight) --------------------------------------------------------------
def graph_a():   # three random blocks (so: several components), ties everywhere (weights 1..50), loops and duplicates; 2901..3000 without edges
    rng = np.random.default_rng(11); nv = 3000
    s, d = [], []
    for lo, hi, m in ((1, 1500, 11000), (1501, 2500, 7000), (2501, 2900, 2000)):
        s.append(rng.integers(lo, hi + 1, m)); d.append(rng.integers(lo, hi + 1, m))
    s, d = np.concatenate(s), np.concatenate(d)
    return nv, s.astype(np.int32), d.astype(np.int32), rng.integers(1, 51, len(s)).astype(np.int32)


def graph_d():   # A's edges with distinct weights: the forest is unique
    nv, s, d, _ = graph_a()
    return nv, s, d, (np.random.default_rng(12).permutation(len(s)) + 1).astype(np.int32)


def graph_p():   # a path whose weights increase along it (one round hooks a chain of 40 000 trees), and its reverse: ids, directions and weights the other way round
    n = 40000
    i = np.arange(1, n)
    s = np.concatenate([i, n + i + 1])
    d = np.concatenate([i + 1, n + i])
    w = np.concatenate([i, n - i])
    return 2 * n, s.astype(np.int32), d.astype(np.int32), w.astype(np.int32)


def graph_h():   # a hub (vertex 20001) with 20 000 leaves: a giant row; 5000 random edges among the leaves, all lighter than the hub's
    rng = np.random.default_rng(13); n = 20000
    s = np.concatenate([np.arange(1, n + 1), rng.integers(1, n + 1, 5000)])
    d = np.concatenate([np.full(n, n + 1), rng.integers(1, n + 1, 5000)])
    w = np.concatenate([rng.integers(1000, 2000, n), rng.integers(1, 100, 5000)])
    return n + 1, s.astype(np.int32), d.astype(np.int32), w.astype(np.int32)


def graph_e():   # equal weights on cycles (a wrong tie-break closes one): a ring of 4097, a 64 x 64 grid, K64; every weight is 7
    s, d = [], []
    ring = np.arange(1, 4098)
    s.append(ring); d.append(np.roll(ring, -1))
    g = 4097 + 1 + np.arange(64 * 64).reshape(64, 64)
    s += [g[:, :-1].ravel(), g[:-1, :].ravel()]; d += [g[:, 1:].ravel(), g[1:, :].ravel()]
    k = 4097 + 4096 + 1 + np.arange(64)
    a, b = np.triu_indices(64, 1)
    s.append(k[a]); d.append(k[b])
    s, d = np.concatenate(s), np.concatenate(d)
    return 4097 + 4096 + 64, s.astype(np.int32), d.astype(np.int32), np.full(len(s), 7, np.int32)


def graph_m():   # multigraph cases on three paths; 601..640 without edges
    a = np.arange(1, 200); b = np.arange(201, 400); c = np.arange(401, 600); loops = np.arange(1, 201)
    odd = c % 2 == 1
    s = [a, loops, b, b + 1, b, c, c + 1]
    d = [a + 1, loops, b + 1, b, b + 1, c + 1, c]
    w = [10 + a % 7, np.full(200, -100),            # a path, and a self-loop on each of its vertices that is lighter than everything
         np.full(199, 5), np.full(199, 3), np.full(199, 9),  # every pair three times, once the other way round: 3 must be reported
         np.full(199, 8), np.where(odd, 8, 6)]       # antiparallel pairs: equal weights on odd pairs, the way back lighter on even ones
    return 640, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32), np.concatenate(w).astype(np.int32)


def graph_n():   # the ends of int32, zero, ties and random negatives: the total leaves int32
    rng = np.random.default_rng(14); nv = 640
    s = rng.integers(1, nv + 1, 4000); d = rng.integers(1, nv + 1, 4000)
    w = rng.choice(np.array([INT32_MIN, -5, 0, 3, INT32_MAX], np.int64), 4000)
    neg = rng.random(4000) < 0.3
    w[neg] = rng.integers(INT32_MIN, 0, int(neg.sum()))
    return nv, s.astype(np.int32), d.astype(np.int32), w.astype(np.int32)


def graph_nd():  # N's edges with distinct weights over the whole of int32, both ends included
    nv, s, d, _ = graph_n()
    rng = np.random.default_rng(15)
    w = np.unique(np.concatenate([[INT32_MIN, INT32_MAX], rng.integers(INT32_MIN, INT32_MAX, 3 * len(s))]))
    w = np.concatenate([[INT32_MIN, INT32_MAX], rng.permutation(w[1:-1])[:len(s) - 2]])
    return nv, s, d, rng.permutation(w).astype(np.int32)


GRAPHS = {"A": graph_a, "D": graph_d, "P": graph_p, "H": graph_h, "E": graph_e, "M": graph_m, "N": graph_n, "ND": graph_nd}
NAMES = tuple(GRAPHS)
DISTINCT = ("D", "ND")
#         name: (vertices, edges, components)
EXPECTED = {"A": (3000, 20000, None), "D": (3000, 20000, None), "P": (80000, 79998, 2), "H": (20001, 25000, 1),
            "E": (8257, 4097 + 2 * 64 * 63 + 64 * 63 // 2, 3), "M": (640, 1394, 43), "N": (640, 4000, None), "ND": (640, 4000, None)}


# ---------------- the reference: a plain Kruskal --------------------------------------------------------------------------
def kruskal(nv, s, d, w):
    """(total as a Python int, edges int32 [k, 3] sorted by (w, u, v)): edges in ascending (weight, position), union-find."""
    parent = list(range(nv + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    order = np.lexsort((np.arange(len(w)), w))
    sl, dl, wl = s.tolist(), d.tolist(), w.tolist()
    out = []
    for i in order.tolist():
        a, b = find(sl[i]), find(dl[i])
        if a != b:
            parent[a] = b
            out.append((min(sl[i], dl[i]), max(sl[i], dl[i]), wl[i]))
    e = np.array(out, np.int32).reshape(-1, 3)
    e = e[np.lexsort((e[:, 1], e[:, 0], e[:, 2]))]
    return sum(x[2] for x in out), np.ascontiguousarray(e)


_kruskal_memo = {}


def kruskal_of(nv, s, d, w):
    """kruskal(), computed once per edge list."""
    key = (nv, hashlib.sha1(np.ascontiguousarray(s).tobytes() + np.ascontiguousarray(d).tobytes() + np.ascontiguousarray(w).tobytes()).hexdigest())
    if key not in _kruskal_memo:
        total, e = kruskal(nv, s, d, w)
        labels = component_labels(nv, s, d)[0]
        for a in (e, labels):
            a.setflags(write=False)
        _kruskal_memo[key] = (total, e, labels)
    return _kruskal_memo[key]


_memo = {}


def reference(name):
    """(nv, src, dst, weight, Kruskal's total, Kruskal's edges, the components' labels), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d, w = GRAPHS[name]()
        for a in (s, d, w):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, w) + kruskal_of(nv, s, d, w)
    return _memo[name]


# ---------------- the verifier --------------------------------------------------------------------------------------------
def check_forest(nv, s, d, w, total, edges):
    """Asserts that (total, edges) is a minimum spanning forest of the multigraph (nv, s, d, w) in the reported form.  Complete: a
    set of k = nv - ncomponents input edges that connects what the graph connects is a spanning forest (so acyclic), and one whose
    total is Kruskal's is a minimum one; it needs no uniqueness."""
    ref_total, ref_edges, labels = kruskal_of(nv, s, d, w)
    # 1. the form
    assert isinstance(edges, np.ndarray) and edges.dtype == np.int32 and edges.ndim == 2 and edges.shape[1] == 3, "int32 [k, 3]"
    k = edges.shape[0]
    u, v, ww = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), edges[:, 2].astype(np.int64)
    assert ((1 <= u) & (u < v) & (v <= nv)).all(), "1 <= u < v <= nv"
    assert (np.lexsort((v, u, ww)) == np.arange(k)).all(), "sorted by (w, u, v)"
    # 2. every row is an input edge, in either direction, with that weight
    lo = np.minimum(s, d).astype(np.int64); hi = np.maximum(s, d).astype(np.int64)
    keep = lo != hi
    given = set(zip(lo[keep].tolist(), hi[keep].tolist(), np.asarray(w)[keep].tolist()))
    foreign = [r for r in zip(u.tolist(), v.tolist(), ww.tolist()) if r not in given]
    assert not foreign, "%d rows are no input edge, first %s" % (len(foreign), foreign[0])
    # 3. the number of edges
    ncomp = len(np.unique(labels))
    assert k == nv - ncomp, "%d edges, the graph has %d vertices in %d components" % (k, nv, ncomp)
    # 4. the forest connects what the graph connects (with 3: it is acyclic)
    got = component_labels(nv, edges[:, 0], edges[:, 1])[0]
    assert (got == labels).all(), "the forest's components are not the graph's: first vertex %d" % (np.nonzero(got != labels)[0][0] + 1)
    # 5. the total
    assert int(total) == int(ww.sum()), "total %d, the rows sum to %d" % (total, int(ww.sum()))
    assert int(total) == ref_total, "total %d, Kruskal's is %d" % (total, ref_total)
    # 6. the weights
    assert (ww == ref_edges[:, 2]).all(), "the sorted weights are not Kruskal's"


# ---------------- the checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", NAMES)
def test_reference_passes_the_verifier(name):
    nv, s, d, w, total, edges, labels = reference(name)
    vertices, nedges, ncomp = EXPECTED[name]
    assert nv == vertices and len(s) == len(d) == len(w) == nedges and w.dtype == np.int32
    assert ncomp is None or len(np.unique(labels)) == ncomp
    check_forest(nv, s, d, w, total, edges)


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_networkx(name):
    """networkx on the simple graph that holds, per vertex pair, the lightest non-loop edge: the total and the sorted weights."""
    nx = pytest.importorskip("networkx")
    nv, s, d, w, total, edges, _ = reference(name)
    lightest = {}
    for a, b, x in zip(s.tolist(), d.tolist(), w.tolist()):
        if a != b:
            key = (min(a, b), max(a, b))
            if key not in lightest or x < lightest[key]:
                lightest[key] = x
    g = nx.Graph()
    g.add_nodes_from(range(1, nv + 1))
    g.add_weighted_edges_from((a, b, x) for (a, b), x in lightest.items())
    got = sorted(x["weight"] for _, _, x in nx.minimum_spanning_edges(g, algorithm="kruskal", data=True))
    assert sum(got) == total
    assert got == edges[:, 2].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_reference_edge_count_equals_scipy(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nv, s, d, w, total, edges, labels = reference(name)
    m = coo_matrix((np.ones(len(s), np.int8), (s - 1, d - 1)), shape=(nv, nv))
    n, _ = connected_components(m, directed=True, connection="weak")
    assert len(edges) == nv - n and len(np.unique(labels)) == n


def test_graph_shapes():
    """What the graphs are there for."""
    nv, s, d, w, total, edges, labels = reference("A")
    assert len(np.unique(labels)) > 100 and np.bincount(labels).max() >= 1000   # several large components, vertices without edges
    assert not np.isin(np.arange(2901, 3001), np.concatenate([s, d])).any()
    assert int((s == d).sum()) > 0 and len(np.unique(w)) == 50
    nv, s, d, w, total, edges, _ = reference("D")
    assert len(np.unique(w)) == len(w)
    nv, s, d, w, total, edges, _ = reference("P")
    assert (np.diff(w[:39999]) > 0).all() and (np.diff(w[39999:]) < 0).all() and len(edges) == 79998
    nv, s, d, w, total, edges, _ = reference("H")
    assert int((d == 20001).sum()) == 20000 and w[:20000].min() > w[20000:].max()
    nv, s, d, w, total, edges, _ = reference("E")
    assert (w == 7).all() and total == 7 * (8257 - 3)
    nv, s, d, w, total, edges, _ = reference("M")
    assert int((s == d).sum()) == 200 and w[s == d].max() < w[s != d].min()
    assert (edges[:, 0] != edges[:, 1]).all()
    pair_b = edges[(edges[:, 0] >= 201) & (edges[:, 1] <= 400)]
    assert len(pair_b) == 199 and (pair_b[:, 2] == 3).all()
    pair_c = edges[(edges[:, 0] >= 401) & (edges[:, 1] <= 600)]
    assert len(pair_c) == 199 and (pair_c[:, 2] == np.where(pair_c[:, 0] % 2 == 1, 8, 6)).all()
    nv, s, d, w, total, edges, _ = reference("N")
    assert set([INT32_MIN, -5, 0, 3, INT32_MAX]) <= set(w.tolist()) and not INT32_MIN <= total <= INT32_MAX
    nv, s, d, w, total, edges, _ = reference("ND")
    assert len(np.unique(w)) == len(w) and w.min() == INT32_MIN and w.max() == INT32_MAX


# the verifier must reject: a square 1-2-3-4 with a diagonal; its minimum spanning tree is the edges of weight 1, 2 and 3
SQUARE = (4, np.array([1, 2, 3, 4, 1], np.int32), np.array([2, 3, 4, 1, 3], np.int32), np.array([1, 2, 3, 4, 5], np.int32))


def rows(*r):
    return np.array(r, np.int32).reshape(-1, 3)


def test_verifier_accepts_the_squares_tree():
    check_forest(*SQUARE, 6, rows((1, 2, 1), (2, 3, 2), (3, 4, 3)))


@pytest.mark.parametrize("what, total, edges, message", [
    ("a cycle", 8, rows((1, 2, 1), (2, 3, 2), (1, 3, 5)), "components are not the graph's"),
    ("a non-minimal edge", 7, rows((1, 2, 1), (2, 3, 2), (1, 4, 4)), "Kruskal's is"),
    ("a foreign edge", 6, rows((1, 2, 1), (2, 3, 2), (2, 4, 3)), "no input edge"),
    ("a wrong weight", 6, rows((1, 2, 1), (2, 3, 2), (1, 4, 3)), "no input edge"),
    ("short an edge", 3, rows((1, 2, 1), (2, 3, 2)), "2 edges"),
    ("a wrong total", 7, rows((1, 2, 1), (2, 3, 2), (3, 4, 3)), "rows sum to"),
    ("unsorted", 6, rows((2, 3, 2), (1, 2, 1), (3, 4, 3)), "sorted"),
    ("u above v", 6, rows((2, 1, 1), (2, 3, 2), (3, 4, 3)), "u < v"),
])
def test_verifier_rejects(what, total, edges, message):
    with pytest.raises(AssertionError, match=message):
        check_forest(*SQUARE, total, edges)


def test_verifier_rejects_a_wrong_dtype():
    with pytest.raises(AssertionError, match="int32"):
        check_forest(*SQUARE, 6, rows((1, 2, 1), (2, 3, 2), (3, 4, 3)).astype(np.int64))


def test_error_convention(lib):
    n, total = C.c_int32(77), C.c_int64(78)
    fake = C.c_void_p(16)  # never dereferenced
    for args in ((None, fake, C.byref(n), C.byref(total)), (fake, None, C.byref(n), C.byref(total)), (fake, fake, None, C.byref(total)),
                 (fake, fake, C.byref(n), None)):
        assert lib.gm_run_spanning_forest(*args, None) == GM_ERR_INVALID
        assert b"null" in lib.gm_last_error()
    assert n.value == 77 and total.value == 78


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert ("int gm_run_spanning_forest(gm_graph_t* g, int32_t* d_edges /* [rows][3] */, int32_t* h_nedges, int64_t* h_total, "
            "gm_stream_t stream);") in header
    assert "gm_run_spanning_forest" in _lib.SIGNATURES and hasattr(lib, "gm_run_spanning_forest")
    for slot, number in (("GM_WS_MSF_EDGE_ROWS", 19), ("GM_WS_MSF_STATE", 20), ("GM_WS_MSF_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header
    assert lib.gm_version() == 107


def test_msf_form_option(lib):
    for form in range(12):
        assert lib.gm_set_option(b"msf_form", form) == 0
    assert lib.gm_set_option(b"msf_form", 12) == GM_ERR_INVALID and lib.gm_set_option(b"msf_form", -1) == GM_ERR_INVALID
    assert lib.gm_reset_options() == 0

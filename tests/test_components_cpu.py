"""Connected components without a GPU: the numpy restatement of the round scheme that the GPU tests compare with
(tests/test_gpu_components.py imports it from here), checked against scipy and against a plain breadth-first search; the error
convention of gm_run_connected_components; the symbol and the workspace slot names in the header, the binding and the library.

Semantics (exact integers): weakly connected components -- edge directions, duplicate edges and self-loops are ignored;
labels[v - 1] = the smallest 1-based vertex id of v's component, a vertex without edges is its own component.  The restatement
works like the kernels do: a forest parent[] with parent[x] <= x; a round reads the parents of both ends of every edge, hooks the
larger onto the smaller with np.minimum.at where they differ, then jumps every vertex to its root; it ends with the first round
that finds no difference.  Over vertex ids a tree's root is its smallest id, so the labels are the roots."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GM_ERR_INVALID = 1


# ---------------- graphs: edges are 1-based (src, dst) ----------------------------------------------------------------------
def graph_a():   # random and sparse: many small components, loops and duplicates; vertex 3000 is isolated
    rng = np.random.default_rng(7); nv = 3000
    s = rng.integers(1, nv, 2000)
    d = rng.integers(1, nv, 2000)
    return nv, s.astype(np.int32), d.astype(np.int32)


def graph_p():   # a path whose ids are shuffled: labels travel the full diameter, the parent chains are deep
    nv = 4097
    perm = np.random.default_rng(0).permutation(nv) + 1
    return nv, perm[:-1].astype(np.int32), perm[1:].astype(np.int32)


def graph_h():   # hubs with the largest ids: 20000 has 9308 in-edges (a giant OUT row), 19999 has 6000 out-edges (a long IN row)
    nv = 20000; rng = np.random.default_rng(3)
    x = rng.integers(17000, 18000, 300)
    s = [np.arange(2, 9010), np.full(6000, 19999), [1, 9500], x, np.arange(2, 302)]
    d = [np.full(9008, 20000), np.arange(10001, 16001), [9500, 9501], x, np.full(300, 20000)]
    return nv, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32)


def graph_k():   # two cliques joined by one edge that runs from the larger ids to the smaller; 81..128 isolated
    s, d = [], []
    for lo, hi in ((1, 40), (41, 80)):
        for i in range(lo, hi + 1):
            for j in range(i + 1, hi + 1):
                s.append(i); d.append(j)
    s.append(80); d.append(40)
    return 128, np.array(s, np.int32), np.array(d, np.int32)


def graph_r():   # the graph of tests/test_dropin_apps.py
    from graphmat_amd import generators
    nv, s, d, _ = generators.rmat_edges(11, 2, seed=9)
    return nv, np.asarray(s, np.int32), np.asarray(d, np.int32)


def fixture(name):
    from graphmat_amd import mtx
    nv, s, d, _ = mtx.read_mtx_bin(os.path.join(GOLDEN, name))
    return nv, s, d


GRAPHS = {"A": graph_a, "P": graph_p, "H": graph_h, "K": graph_k, "test": lambda: fixture("test.bin.mtx"),
          "upper": lambda: fixture("2_10_upper_triangle.bin.mtx"), "R": graph_r}
NAMES = tuple(GRAPHS)
#         name: (edges, components, largest component, rounds of the restatement, sum of the labels)
EXPECTED = {"A": (2000, 1050, 1314, 6, 1764141), "P": (4096, 1, 4097, 9, 4097), "H": (15610, 4990, 9009, 3, 141396477),
            "K": (1561, 49, 80, 3, 5096), "test": (13, 1, 8, 2, 8), "upper": (15069, 1, 1024, 2, 1024), "R": (4096, 972, 1068, 3, 1220485)}


# ---------------- the restatement -----------------------------------------------------------------------------------------
def restatement(nv, s, d):
    """(labels int32[nv] (index v - 1), rounds): min-hooking rounds with a full jump after each, as gm_components.hip runs them."""
    u = np.asarray(s, np.int64) - 1
    v = np.asarray(d, np.int64) - 1
    parent = np.arange(nv, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        ru, rv = parent[u], parent[v]
        differ = ru != rv
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ru, rv)[differ], np.minimum(ru, rv)[differ])
        while True:
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
        assert rounds <= nv
    return (parent + 1).astype(np.int32), rounds


def plain_bfs(nv, s, d):
    """The semantics written out: vertices in ascending order, each unlabelled one floods its component with its own id."""
    adj = [[] for _ in range(nv + 1)]
    for a, b in zip(s.tolist(), d.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    labels = np.zeros(nv, np.int32)
    for root in range(1, nv + 1):
        if labels[root - 1]:
            continue
        labels[root - 1] = root
        queue = [root]
        while queue:
            nxt = []
            for a in queue:
                for b in adj[a]:
                    if not labels[b - 1]:
                        labels[b - 1] = root
                        nxt.append(b)
            queue = nxt
    return labels


_memo = {}


def reference(name):
    """(nv, src, dst, labels of the restatement, its rounds), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d = GRAPHS[name]()
        labels, rounds = restatement(nv, s, d)
        for a in (s, d, labels):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, labels, rounds)
    return _memo[name]


def isolated(nv, s, d):
    """bool[nv]: vertices that no edge names"""
    seen = np.zeros(nv + 1, bool)
    seen[s] = True
    seen[d] = True
    return ~seen[1:]


# ---------------- the checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_table(name):
    nv, s, d, labels, rounds = reference(name)
    edges, ncomp, largest, table_rounds, checksum = EXPECTED[name]
    assert len(s) == len(d) == edges
    roots, sizes = np.unique(labels, return_counts=True)
    assert len(roots) == ncomp and int(sizes.max()) == largest
    assert rounds == table_rounds
    assert int(labels.astype(np.int64).sum()) == checksum
    assert (labels <= np.arange(1, nv + 1)).all() and (labels[labels - 1] == labels).all()
    iso = isolated(nv, s, d)
    assert (labels[iso] == np.nonzero(iso)[0] + 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_a_plain_bfs(name):
    nv, s, d, labels, _ = reference(name)
    assert (labels == plain_bfs(nv, s, d)).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nv, s, d, labels, _ = reference(name)
    m = coo_matrix((np.ones(len(s), np.int8), (s - 1, d - 1)), shape=(nv, nv))
    n, comp = connected_components(m, directed=True, connection="weak")
    assert n == EXPECTED[name][1]
    # scipy numbers the components as it likes: the smallest vertex id of each is what the labels are
    smallest = np.full(n, nv + 1, np.int64)
    np.minimum.at(smallest, comp, np.arange(1, nv + 1))
    assert (labels == smallest[comp]).all()


def test_graph_shapes():
    """What the graphs are there for."""
    nv, s, d, labels, _ = reference("A")
    assert not (s == 3000).any() and not (d == 3000).any() and labels[2999] == 3000
    assert int((s == d).sum()) > 0 and len(s) - len(np.unique(np.stack([s, d], 1), axis=0)) > 0  # loops and duplicates
    nv, s, d, labels, _ = reference("H")
    assert int((d == 20000).sum()) == 9308 and int((s == 19999).sum()) == 6000
    assert labels[19999] == 2 and labels[19998] == 10001 and labels[0] == labels[9499] == labels[9500] == 1
    nv, s, d, labels, _ = reference("K")
    assert (labels[:80] == 1).all() and (labels[80:] == np.arange(81, 129)).all()
    nv, s, d, labels, _ = reference("P")
    assert (np.sort(np.concatenate([s, d[-1:]])) == np.arange(1, 4098)).all() and (labels == 1).all()


def test_error_convention(lib):
    n = C.c_int32(77)
    fake = C.c_void_p(16)  # never dereferenced
    assert lib.gm_run_connected_components(None, fake, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_connected_components(fake, None, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert n.value == 77


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert "int gm_run_connected_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, gm_stream_t stream);" in header
    assert "gm_run_connected_components" in _lib.SIGNATURES and hasattr(lib, "gm_run_connected_components")
    for slot, number in (("GM_WS_CC_EDGE_ROWS", 19), ("GM_WS_CC_MIN", 20), ("GM_WS_CC_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header

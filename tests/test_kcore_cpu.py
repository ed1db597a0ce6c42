"""K-core decomposition without a GPU: the numpy restatement of the peel that the GPU tests compare with
(tests/test_gpu_kcore.py imports it from here), checked against a plainly written bucket peel and against networkx; the
one-adjacency rule of the adjacency build; the error convention of gm_run_kcore; the symbol and the workspace slot names in the
header, the binding and the library.

Semantics (exact integers): core numbers of the SIMPLE UNDIRECTED graph under the edge list -- edge directions are ignored,
self-loops dropped, duplicate edges and a pair u -> v, v -> u count once; core[v - 1] = the largest k such that v lies in a
subgraph whose vertices all have at least k neighbours, 0 for a vertex without neighbours.  The restatement works like the kernels
do: deg[] = simple degrees, all vertices alive.  A level takes k = the smallest deg among alive vertices; its first list is the
alive vertices with deg <= k; a pass gives every listed vertex core number k, takes one off the deg of each alive neighbour per
listed neighbour, and the vertices this brings down to k are the next list; the level ends with an empty list.  levels = the
number of distinct core numbers, passes = the number of lists processed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_components_cpu import GRAPHS as CC_GRAPHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM_ERR_INVALID = 1


# ---------------- graphs: edges are 1-based (src, dst) ----------------------------------------------------------------------
def graph_c():   # a 70-clique and a 30-clique joined by an edge, a path hanging off, a star of 4599 leaves, one loop, one antiparallel pair given twice
    s, d = [], []
    def clique(lo, hi):
        for i in range(lo, hi + 1):
            for j in range(i + 1, hi + 1):
                s.append(j); d.append(i)
    clique(1, 70); clique(71, 100); s.append(70); d.append(71)
    for i in range(101, 400): s.append(i); d.append(i + 1)
    s.append(100); d.append(101)
    for i in range(401, 5000): s.append(i); d.append(400)
    s += [5, 6, 6, 4500, 4500]; d += [6, 5, 5, 4500, 4501]
    return 5000, np.array(s, np.int32), np.array(d, np.int32)


def graph_m():   # three paths: one with a loop on every vertex, one with every edge twice, one with every edge in both directions; 601..640 isolated
    a = np.arange(1, 200); b = np.arange(201, 400); c = np.arange(401, 600)
    s = [a, np.arange(1, 201), b, b, c, c + 1]
    d = [a + 1, np.arange(1, 201), b + 1, b + 1, c + 1, c]
    return 640, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32)


def graph_r14():
    from graphmat_amd import generators
    nv, s, d, _ = generators.rmat_edges(14, 16, seed=1)
    return nv, np.asarray(s, np.int32), np.asarray(d, np.int32)


GRAPHS = dict(CC_GRAPHS)
GRAPHS.update({"R14": graph_r14, "C": graph_c, "M": graph_m})
NAMES = tuple(GRAPHS)
#         name: (edges, kmax, levels, passes, sum of core, vertices at kmax)
EXPECTED = {"A": (2000, 2, 3, 23, 2605, 396), "P": (4096, 1, 1, 2049, 4097, 4097), "H": (15610, 1, 2, 3, 15013, 15013),
            "K": (1561, 39, 2, 3, 3120, 80), "test": (13, 2, 1, 3, 16, 8), "upper": (15069, 19, 19, 83, 16198, 389),
            "R": (4096, 12, 13, 44, 3919, 55), "R14": (262144, 120, 69, 184, 229494, 454), "C": (7755, 69, 5, 7, 10901, 70),
            "M": (1195, 1, 2, 101, 600, 600)}


# ---------------- the simple undirected graph -------------------------------------------------------------------------------
def simple_pairs(nv, s, d):
    """The distinct unordered pairs {u, v}, u != v, 0-based: (lo, hi) with lo < hi."""
    u = np.asarray(s, np.int64) - 1
    v = np.asarray(d, np.int64) - 1
    keep = u != v
    key = np.unique(np.minimum(u, v)[keep] * nv + np.maximum(u, v)[keep])
    return key // nv, key % nv


def simple_adjacency(nv, s, d):
    """(rowptr int64[nv + 1], neighbours int64[2 * pairs]) of the symmetrised, de-duplicated, loop-free edge set."""
    lo, hi = simple_pairs(nv, s, d)
    rows = np.concatenate([lo, hi])
    cols = np.concatenate([hi, lo])
    order = np.argsort(rows, kind="stable")
    rowptr = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nv), out=rowptr[1:])
    return rowptr, cols[order]


def simple_degrees(nv, s, d):
    return np.diff(simple_adjacency(nv, s, d)[0])


def one_adjacency_degrees(nv, s, d, rows_are_dst):
    """Stage (a) of gm_kcore.hip on ONE adjacency (rows = destinations: GM_DIR_OUT; rows = sources: GM_DIR_IN): for every distinct
    non-loop entry (r, c): c is a neighbour of r; r is a neighbour of c unless row c holds r."""
    u = np.asarray(s, np.int64) - 1
    v = np.asarray(d, np.int64) - 1
    r, c = (v, u) if rows_are_dst else (u, v)
    keep = r != c
    key = np.unique(r[keep] * nv + c[keep])  # the distinct entries
    r, c = key // nv, key % nv
    row_c_holds_r = np.isin(c * nv + r, key)
    deg = np.bincount(r, minlength=nv)
    deg += np.bincount(c[~row_c_holds_r], minlength=nv)
    return deg


# ---------------- the restatement -----------------------------------------------------------------------------------------
def restatement(nv, s, d):
    """(core int32[nv] (index v - 1), levels, passes): the peel as gm_kcore.hip runs it."""
    rowptr, nbr = simple_adjacency(nv, s, d)
    deg = np.diff(rowptr).copy()
    alive = np.ones(nv, bool)
    core = np.full(nv, -1, np.int32)
    levels = passes = 0
    while alive.any():
        k = int(deg[alive].min())
        levels += 1
        frontier = np.nonzero(alive & (deg <= k))[0]
        while frontier.size:
            passes += 1
            core[frontier] = k
            alive[frontier] = False
            lens = rowptr[frontier + 1] - rowptr[frontier]
            starts = np.repeat(rowptr[frontier] - (np.cumsum(lens) - lens), lens)
            w = nbr[starts + np.arange(int(lens.sum()))]
            w = w[alive[w]]
            np.subtract.at(deg, w, 1)
            touched = np.unique(w)
            frontier = touched[deg[touched] <= k]  # they were above k: alive and not listed
        assert levels <= nv and passes <= nv
    return core, levels, passes


def bucket_peel(nv, s, d):
    """Batagelj-Zaversnik, written out: vertices in ascending order of their current degree; removing one lowers the degree of
    each later neighbour that is above it by one."""
    adj = [set() for _ in range(nv)]
    for a, b in zip(s.tolist(), d.tolist()):
        if a != b:
            adj[a - 1].add(b - 1)
            adj[b - 1].add(a - 1)
    deg = [len(x) for x in adj]
    md = max(deg) if nv else 0
    bins = [0] * (md + 2)
    for x in deg:
        bins[x + 1] += 1
    for i in range(1, md + 2):
        bins[i] += bins[i - 1]  # bins[x] = first position of degree x
    start = bins[:md + 1]
    pos = [0] * nv
    vert = [0] * nv
    fill = list(start)
    for v in range(nv):
        pos[v] = fill[deg[v]]
        vert[pos[v]] = v
        fill[deg[v]] += 1
    for i in range(nv):
        v = vert[i]
        for u in adj[v]:
            if deg[u] > deg[v]:
                du, pu = deg[u], pos[u]
                pw = start[du]
                w = vert[pw]
                if u != w:
                    pos[u], pos[w] = pw, pu
                    vert[pu], vert[pw] = w, u
                start[du] += 1
                deg[u] -= 1
    return np.array(deg, np.int32)


_memo = {}


def reference(name):
    """(nv, src, dst, core of the restatement, its levels, its passes), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d = GRAPHS[name]()
        core, levels, passes = restatement(nv, s, d)
        for a in (s, d, core):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, core, levels, passes)
    return _memo[name]


# ---------------- the checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_table(name):
    nv, s, d, core, levels, passes = reference(name)
    edges, kmax, table_levels, table_passes, checksum, at_kmax = EXPECTED[name]
    assert len(s) == len(d) == edges
    assert int(core.max()) == kmax
    assert levels == table_levels == len(np.unique(core))
    assert passes == table_passes
    assert int(core.astype(np.int64).sum()) == checksum
    assert int((core == kmax).sum()) == at_kmax
    deg = simple_degrees(nv, s, d)
    assert (core >= 0).all() and (core <= deg).all() and (core[deg == 0] == 0).all() and (core[deg > 0] >= 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_a_plain_bucket_peel(name):
    nv, s, d, core, _, _ = reference(name)
    assert (core == bucket_peel(nv, s, d)).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_networkx(name):
    nx = pytest.importorskip("networkx")
    nv, s, d, core, _, _ = reference(name)
    g = nx.Graph()
    g.add_nodes_from(range(1, nv + 1))
    g.add_edges_from((a, b) for a, b in zip(s.tolist(), d.tolist()) if a != b)
    cn = nx.core_number(g)
    assert (core == np.array([cn[v] for v in range(1, nv + 1)], np.int32)).all()


@pytest.mark.parametrize("name", NAMES)
def test_one_adjacency_gives_the_simple_degrees(name):
    nv, s, d, _, _, _ = reference(name)
    deg = simple_degrees(nv, s, d)
    assert (one_adjacency_degrees(nv, s, d, True) == deg).all()
    assert (one_adjacency_degrees(nv, s, d, False) == deg).all()


def test_graph_shapes():
    """What the graphs are there for."""
    nv, s, d, core, _, _ = reference("M")
    pairs = np.stack([s, d], 1)
    assert int((s == d).sum()) == 200                                                   # loops
    assert len(pairs) - len(np.unique(pairs, axis=0)) == 199                            # duplicates
    fwd = set(map(tuple, pairs[s != d].tolist()))
    assert sum((b, a) in fwd for a, b in fwd) == 2 * 199                                # antiparallel pairs
    assert (core[:600] == 1).all() and (core[600:] == 0).all()
    nv, s, d, core, _, _ = reference("C")
    deg = simple_degrees(nv, s, d)
    # the hub: 4599 leaves and the path's end.  The edge 4500 -> 4501 joins two of its leaves, so the hub lies in a triangle and has
    # core number 2 (networkx says so too), like these two leaves and the path from the 30-clique to the hub; every other leaf has 1
    assert deg[399] == 4599 + 1 and core[399] == 2 and core[4499] == core[4500] == 2
    assert (np.delete(core[400:4999], [4099, 4100]) == 1).all() and (core[100:399] == 2).all() and core[4999] == 0  # 5000 is isolated
    assert (core[:70] == 69).all() and (core[70:100] == 29).all()
    nv, s, d, core, _, _ = reference("H")
    assert int(simple_degrees(nv, s, d).max()) == 9008
    nv, s, d, _, _, _ = reference("R14")
    pairs = np.stack([s, d], 1)[s != d]
    assert len(pairs) - len(np.unique(pairs, axis=0)) == 33703 and int((s == d).sum()) == 308  # duplicates of non-loop edges; loops
    key =np.unique(s[s != d].astype(np.int64) * (nv + 1) + d[s != d])
    rkey = np.unique(d[s != d].astype(np.int64) * (nv + 1) + s[s != d])
    assert int(np.isin(key, rkey).sum()) == 2 * 15212


def test_error_convention(lib):
    n = C.c_int32(77)
    fake = C.c_void_p(16)  # never dereferenced
    assert lib.gm_run_kcore(None, fake, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_kcore(fake, None, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert n.value == 77


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert "int gm_run_kcore(gm_graph_t* g, int32_t* d_core, int32_t* h_kmax, gm_stream_t stream);" in header
    assert "gm_run_kcore" in _lib.SIGNATURES and hasattr(lib, "gm_run_kcore")
    for slot, number in (("GM_WS_KC_ADJ", 19), ("GM_WS_KC_STATE", 20), ("GM_WS_KC_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header

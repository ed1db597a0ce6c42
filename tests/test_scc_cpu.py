"""Strongly connected components without a GPU: the graphs, the table and the numpy restatement of the trim-and-colour scheme
that the GPU tests compare with (tests/test_gpu_scc.py imports them from here), checked against scipy, against a plainly written
iterative Tarjan and against the weakly connected components; the error convention of gm_run_strong_components; the symbol and the
workspace slot names in the header, the binding and the library.

Semantics (exact integers): labels[v - 1] = the smallest 1-based vertex id of v's strongly connected component.  Edge directions
matter, duplicate edges and self-loops do not; a vertex without edges, or with a self-loop only, is its own component.  The
restatement works like the kernels do: trim (an alive vertex without alive in-neighbours or without alive out-neighbours is its own
component) to a fixpoint, then a round: colours start as vertex ids and passes over the alive edges lower them to the smallest id
among the alive ancestors; a vertex that keeps its id is a root; passes against the edges mark what reaches a root within its
colour; the marked vertices get their colour as label and die.  Its passes are synchronous (a pass reads the values of the pass
before), so the kernels' passes can only be fewer."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_components_cpu import GRAPHS as CC_GRAPHS
from tests.test_components_cpu import reference as cc_reference
from tests.test_components_cpu import restatement as cc_restatement
from tests.test_kcore_cpu import graph_r14

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM_ERR_INVALID = 1


# ---------------- graphs: edges are 1-based (src, dst) ----------------------------------------------------------------------
def graph_y():   # two shuffled cycles (3000, 1000), the first feeds the second; a path of 97 feeds the first
    rng = np.random.default_rng(5); nv = 4097
    perm = rng.permutation(nv) + 1
    a, b, t = perm[:3000], perm[3000:4000], perm[4000:]
    s = [a, b, t[:-1], t[-1:], a[:1]]
    d = [np.roll(a, -1), np.roll(b, -1), t[1:], a[10:11], b[:1]]
    return nv, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32)


def graph_b():   # K's cliques with every edge both ways, joined one way; loops on 81..90; a 2-cycle with a duplicate; a path
    s, d = [], []
    for lo, hi in ((1, 40), (41, 80)):
        for i in range(lo, hi + 1):
            for j in range(i + 1, hi + 1):
                s += [i, j]; d += [j, i]
    s.append(80); d.append(40)
    for i in range(81, 91): s.append(i); d.append(i)
    s += [91, 91, 92, 93, 94]; d += [92, 92, 91, 94, 95]
    return 128, np.array(s, np.int32), np.array(d, np.int32)


def graph_g():   # H plus 3000 edges back out of its hub: an SCC around a giant OUT row; and a 2-cycle through the other hub, which has a loop
    nv, s, d = CC_GRAPHS["H"]()
    s = np.concatenate([s, np.full(3000, 20000), [12000, 19999]]).astype(np.int32)
    d = np.concatenate([d, np.arange(2, 3002), [19999, 19999]]).astype(np.int32)
    return nv, s, d


def graph_l():   # 60 directed triangles, each feeding later ones: one SCC per round; loops and duplicates; 181..192 isolated
    s, d = [], []
    for i in range(60):
        a = 3 * i + 1
        s += [a, a + 1, a + 2]; d += [a + 1, a + 2, a]
        if i + 1 < 60: s.append(a + 1); d.append(a + 5)
        if i + 7 < 60: s.append(a + 2); d.append(a + 21)
        if i % 10 == 0: s += [a, a]; d += [a, a + 1]
    return 192, np.array(s, np.int32), np.array(d, np.int32)


def graph_t():   # cycle 1..50 -> path 51..100 -> cycle 101..150 -> path 151..170 holding a 2-cycle; cycle 171..200 feeds the middle one
    c = lambda lo, hi: (list(range(lo, hi + 1)), list(range(lo + 1, hi + 1)) + [lo])
    s, d = [], []
    for lo, hi in ((1, 50), (101, 150), (171, 200)):
        a, b = c(lo, hi); s += a; d += b
    s += list(range(50, 100)) + [100]; d += list(range(51, 101)) + [130]
    s += [140] + list(range(151, 170)); d += [151] + list(range(152, 171))
    s += [185, 185, 160, 161, 7]; d += [120, 120, 161, 160, 7]
    return 256, np.array(s, np.int32), np.array(d, np.int32)


def graph_q():   # random, mean out-degree 1.5
    rng = np.random.default_rng(11); nv = 2000
    return nv, rng.integers(1, nv + 1, 3000).astype(np.int32), rng.integers(1, nv + 1, 3000).astype(np.int32)


GRAPHS = dict(CC_GRAPHS)
GRAPHS.update({"R14": graph_r14, "Y": graph_y, "B": graph_b, "G": graph_g, "L": graph_l, "T": graph_t, "Q": graph_q})
NAMES = tuple(GRAPHS)
#         name: (nv, edges, components, largest, SCCs > 1, trimmed, rounds, (trim, forward, backward passes), sum of labels)
EXPECTED = {"A": (3000, 2000, 2993, 8, 1, 2992, 1, (6, 8, 8), 4490780),
            "P": (4097, 4096, 4097, 1, 0, 4097, 0, (2049, 0, 0), 8394753),
            "H": (20000, 15610, 20000, 1, 0, 20000, 0, (2, 0, 0), 200010000),
            "K": (128, 1561, 128, 1, 0, 128, 0, (21, 0, 0), 8256),
            "test": (8, 13, 8, 1, 0, 8, 0, (3, 0, 0), 36),
            "upper": (1024, 15069, 1024, 1, 0, 1024, 0, (82, 0, 0), 524800),
            "R": (2048, 4096, 1487, 562, 1, 1486, 1, (2, 5, 6), 1705482),
            "R14": (16384, 262144, 6954, 9431, 1, 6953, 1, (2, 5, 5), 69959008),
            "Y": (4097, 4098, 99, 3000, 2, 97, 2, (97, 4000, 4000), 198995),
            "B": (128, 3136, 49, 40, 3, 46, 1, (2, 2, 2), 6695),
            "G": (20000, 18612, 16999, 3001, 2, 16997, 1, (2, 3, 3), 195483503),
            "L": (192, 304, 72, 3, 60, 12, 60, (1, 1196, 180), 18348),
            "T": (256, 206, 128, 50, 4, 124, 3, (68, 203, 102), 30010),
            "Q": (2000, 3000, 1274, 727, 1, 1273, 1, (10, 25, 27), 1290545)}
# (roots, vertices removed) of each round
PER_ROUND = {"Y": [(1, 3000), (1, 1000)], "T": [(2, 80), (1, 50), (1, 2)], "B": [(3, 82)], "G": [(2, 3003)], "L": [(1, 3)] * 60}


# ---------------- the restatement -----------------------------------------------------------------------------------------
def restatement(nv, s, d):
    """(labels int32[nv] (index v - 1), rounds, (trim, forward, backward passes), trimmed vertices, (roots, removed) per round)"""
    u = np.asarray(s, np.int64) - 1; v = np.asarray(d, np.int64) - 1
    k = u != v; u, v = u[k], v[k]
    ids = np.arange(1, nv + 1, dtype=np.int64)
    alive = np.ones(nv, bool); label = np.zeros(nv, np.int64)
    rounds = tp = fp = bp = trimmed = 0; per_round = []
    while True:
        while True:
            e = alive[u] & alive[v]
            indeg = np.bincount(v[e], minlength=nv); outdeg = np.bincount(u[e], minlength=nv)
            f = alive & ((indeg == 0) | (outdeg == 0))
            if not f.any(): break
            tp += 1; trimmed += int(f.sum()); label[f] = ids[f]; alive[f] = False
        if not alive.any(): break
        rounds += 1; eu, ev = u[e], v[e]; colour = ids.copy()
        while True:
            fp += 1; new = colour.copy(); np.minimum.at(new, ev, colour[eu])
            if (new == colour).all(): break
            colour = new
        mark = alive & (colour == ids); nroots = int(mark.sum())
        while True:
            bp += 1; c = mark[ev] & ~mark[eu] & (colour[eu] == colour[ev])
            if not c.any(): break
            mark[eu[c]] = True
        label[mark] = colour[mark]; alive[mark] = False; per_round.append((nroots, int(mark.sum())))
        assert rounds <= nv
    return label.astype(np.int32), rounds, (tp, fp, bp), trimmed, per_round


def tarjan(nv, s, d):
    """Tarjan's algorithm with an explicit stack; labels = the smallest vertex id of each component."""
    order = np.argsort(s, kind="stable")
    start = np.zeros(nv + 2, np.int64)
    np.cumsum(np.bincount(s, minlength=nv + 1), out=start[1:])
    start, nbr = start.tolist(), np.asarray(d)[order].tolist()
    index = [0] * (nv + 1); low = [0] * (nv + 1); on_stack = [False] * (nv + 1)
    labels = np.zeros(nv, np.int32)
    stack, counter = [], 0
    for root in range(1, nv + 1):
        if index[root]:
            continue
        counter += 1; index[root] = low[root] = counter
        stack.append(root); on_stack[root] = True
        work = [(root, start[root])]
        while work:
            a, at = work[-1]
            if at < start[a + 1]:
                work[-1] = (a, at + 1)
                b = nbr[at]
                if not index[b]:
                    counter += 1; index[b] = low[b] = counter
                    stack.append(b); on_stack[b] = True
                    work.append((b, start[b]))
                elif on_stack[b]:
                    low[a] = min(low[a], index[b])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[a])
                if low[a] == index[a]:
                    members = []
                    while True:
                        b = stack.pop(); on_stack[b] = False; members.append(b)
                        if b == a:
                            break
                    labels[np.array(members) - 1] = min(members)
    return labels


_memo = {}


def reference(name):
    """(nv, src, dst, labels of the restatement, rounds, (tp, fp, bp), trimmed, per_round), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d = GRAPHS[name]()
        labels, rounds, passes, trimmed, per_round = restatement(nv, s, d)
        for a in (s, d, labels):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, labels, rounds, passes, trimmed, per_round)
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
    nv, s, d, labels, rounds, passes, trimmed, per_round = reference(name)
    t_nv, edges, ncomp, largest, nbig, t_trimmed, t_rounds, t_passes, checksum = EXPECTED[name]
    assert nv == t_nv and len(s) == len(d) == edges
    roots, sizes = np.unique(labels, return_counts=True)
    assert len(roots) == ncomp and int(sizes.max()) == largest and int((sizes > 1).sum()) == nbig
    assert trimmed == t_trimmed and rounds == t_rounds and passes == t_passes
    assert int(labels.astype(np.int64).sum()) == checksum
    assert ncomp == trimmed + sum(r for r, _ in per_round) and nv == trimmed + sum(m for _, m in per_round)
    if name in PER_ROUND:
        assert per_round == PER_ROUND[name]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nv, s, d, labels = reference(name)[:4]
    m = coo_matrix((np.ones(len(s), np.int8), (s - 1, d - 1)), shape=(nv, nv))
    n, comp = connected_components(m, directed=True, connection="strong")
    assert n == EXPECTED[name][2]
    # scipy numbers the components as it likes: the smallest vertex id of each is what the labels are
    smallest = np.full(n, nv + 1, np.int64)
    np.minimum.at(smallest, comp, np.arange(1, nv + 1))
    assert (labels == smallest[comp]).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_tarjan(name):
    nv, s, d, labels = reference(name)[:4]
    assert (labels == tarjan(nv, s, d)).all()


@pytest.mark.parametrize("name", NAMES)
def test_labels_are_the_smallest_ids_and_refine_the_weak_components(name):
    nv, s, d, labels = reference(name)[:4]
    assert (labels <= np.arange(1, nv + 1)).all() and (labels[labels - 1] == labels).all()
    weak = cc_reference(name)[3] if name in CC_GRAPHS else cc_restatement(nv, s, d)[0]
    assert (labels >= weak).all()
    assert (weak[labels - 1] == weak).all()  # a strong component lies inside one weak component


def test_graph_shapes():
    """What the new graphs are there for."""
    labels = reference("G")[3]
    assert (np.nonzero(labels == 2)[0] + 1).tolist() == list(range(2, 3002)) + [20000]  # the SCC of 3001 around the giant OUT row
    assert (np.nonzero(labels == 12000)[0] + 1).tolist() == [12000, 19999]
    labels = reference("B")[3]
    assert (labels[80:90] == np.arange(81, 91)).all()  # a loop makes no component
    assert (np.nonzero(labels == 91)[0] + 1).tolist() == [91, 92]
    nv, s, d, labels, rounds, _, _, per_round = reference("T")
    assert rounds == 3 and per_round[2] == (1, 2) and (np.nonzero(labels == 160)[0] + 1).tolist() == [160, 161]


def test_error_convention(lib):
    n = C.c_int32(77)
    fake = C.c_void_p(16)  # never dereferenced
    assert lib.gm_run_strong_components(None, fake, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_strong_components(fake, None, C.byref(n), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert n.value == 77


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert "int gm_run_strong_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, gm_stream_t stream);" in header
    assert "gm_run_strong_components" in _lib.SIGNATURES and hasattr(lib, "gm_run_strong_components")
    for slot, number in (("GM_WS_SCC_EDGES", 19), ("GM_WS_SCC_STATE", 20), ("GM_WS_SCC_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header

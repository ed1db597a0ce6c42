"""Betweenness centrality without a GPU: the graphs, the table and the numpy restatement of the level-synchronous Brandes scheme that
the GPU tests compare with (tests/test_gpu_betweenness.py imports them from here), checked against networkx and against a plainly
written queue-based Brandes; the closed forms of the graphs F and Z; the error convention of gm_run_betweenness; the symbol and the
workspace slot names in the header, the binding and the library.

Semantics: Brandes (2001), unweighted, DIRECTED, unnormalised, endpoints not counted, on the simple directed graph under the edge
list (duplicate edges count once, self-loops are ignored).  For the sources S (1-based vertex ids; one listed twice counts twice)
    bc[v] = sum over s in S of delta_s(v),  delta_s(s) = 0,
    sigma_s(w) = the number of shortest s -> w paths,
    delta_s(v) = sum over v -> w with depth(w) = depth(v) + 1 of  sigma(v) / sigma(w) * (1 + delta_s(w))  (divide, then multiply).
fp64 throughout.  The restatement works like the kernels do, level by level, with np.add.at over the edges between two levels, on
np.unique of the non-loop edges.

The tolerance rtol(L, D, S) = 8 * (L * (D + 4) + S) * 2^-53 that two fp64 evaluations of these sums may differ by, whatever the
order of their additions (L = the largest eccentricity among the sources, D = the largest in- or out-degree of the raw edge list,
S = the number of sources).  To first order in u = 2^-53, for sums of positive terms in any order: a sum of k positive terms is
off by at most (k - 1) u relatively; sigma[w] is a sum of at most D sigmas of the level above, so rel(sigma at level l) <=
l * (D - 1) u <= L * D * u.  delta[v] is a sum of at most D terms, each a quotient (1 u), a sum 1 + delta (1 u) and a product (1 u)
of quantities that are themselves off: the two sigmas cancel to first order up to the level's own additions (counted in L * D
already), delta[w] carries the error of the level below.  By induction over the L levels, rel(delta) <= L * (D - 1 + 3) u + the
sigma part, together at most L * (D + 4) u with the level's own final rounding; the S additions into bc[v] add S * u.  That is
(L * (D + 4) + S) * u for ONE evaluation; both sides of a comparison round, which doubles it, and a factor 4 covers the terms of
second order and the slack of the first-order argument.  On the graphs here it is at most 2.02e-11 (R14); restatement and networkx were
seen to differ by at most 3.2e-15."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

from tests.test_scc_cpu import GRAPHS as SCC_GRAPHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM_ERR_INVALID = 1


# ---------------- graphs: edges are 1-based (src, dst) ----------------------------------------------------------------------
def graph_grid():   # directed 27 x 27 lattice, id = 27 i + j + 1, edges to (i + 1, j) and (i, j + 1): sigma is binomial, 52 levels
    k = 27
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    ids = (k * i + j + 1).astype(np.int32)
    s = np.concatenate([ids[:-1, :].ravel(), ids[:, :-1].ravel()])
    d = np.concatenate([ids[1:, :].ravel(), ids[:, 1:].ravel()])
    return k * k, s.astype(np.int32), d.astype(np.int32)


def graph_z():   # a chain of 45 diamonds of width 3: junction -> 3 middles -> next junction, ids in that order; sigma reaches 3^45
    s, d = [], []
    for i in range(45):
        a = 4 * i + 1
        for m in (a + 1, a + 2, a + 3):
            s += [a, m]; d += [m, a + 4]
    return 181, np.array(s, np.int32), np.array(d, np.int32)


def graph_f():   # a long out-row (vertex 1: 3000 simple entries, 200 duplicates), 3000 adds into one sigma word (3002), a long backward sum
    m = np.arange(2, 3002)
    s = np.concatenate([[3004], np.full(3000, 1), m, [3002], np.full(200, 1), [3002]])
    d = np.concatenate([[1], m, np.full(3000, 3002), [3003], np.arange(2, 202), [3002]])
    return 3100, s.astype(np.int32), d.astype(np.int32)


GRAPHS = {k: SCC_GRAPHS[k] for k in ("test", "K", "B", "L", "T", "R", "Q", "G", "Y", "R14")}
GRAPHS.update({"grid": graph_grid, "Z": graph_z, "F": graph_f})
NAMES = tuple(GRAPHS)
ALL = None  # every vertex
SOURCES = {"test": ALL, "K": ALL, "B": ALL, "L": ALL, "T": ALL, "grid": ALL, "Z": ALL, "R": [1, 2, 3, 5, 100, 2048], "Q": [1, 2, 3, 4],
           "G": [2, 20000, 19999, 12000, 1], "Y": [1], "R14": [1, 2, 3, 4], "F": [3004, 1]}
EXACT = ("test", "K", "B", "T", "G", "Y")  # every value is an integer or one exact term: equality whatever the order of the sums
# name: what is known of (largest eccentricity, max sigma, vertices reached by the source that reaches most, non-zero bc, sum of bc); None = not in the table
EXPECTED = {"R": (8, 40, 819, 359, 6896), "R14": (4, 369, 10924, 3785, 44193), "G": (2, None, 6001, 3, 8999),
            "Y": (2999, None, 4000, 3997, 5043001), "T": (None, None, None, None, 902520), "K": (None, None, None, 1, None),
            "grid": (52, 495918532948104, None, None, None), "Z": (90, None, None, None, None)}
G_REACHED = [3001, 3001, 6001, 6001, 3]


def simple_edges(nv, s, d):
    """0-based (u, v) of the simple directed graph: loops dropped, duplicates once, sorted by (u, v)."""
    u = np.asarray(s, np.int64) - 1; v = np.asarray(d, np.int64) - 1
    k = u != v
    pairs = np.unique(u[k] * nv + v[k])
    return pairs // nv, pairs % nv


# ---------------- the restatement -----------------------------------------------------------------------------------------
def single_source(nv, u, v, src):
    """(depth int32[nv], sigma float64[nv], delta float64[nv] with delta[src] as summed, eccentricity) of 1-based src over the simple edges"""
    depth = np.full(nv, -1, np.int32); sigma = np.zeros(nv, np.float64)
    depth[src - 1] = 0; sigma[src - 1] = 1.0
    levels = []
    order = np.argsort(u, kind="stable"); start = np.searchsorted(u[order], np.arange(nv + 1))
    frontier = np.array([src - 1], np.int64)
    while True:
        d = len(levels)
        idx = np.concatenate([order[start[x]:start[x + 1]] for x in frontier]) if frontier.size else np.zeros(0, np.int64)
        eu, ev = u[idx], v[idx]
        depth[ev[depth[ev] == -1]] = d + 1
        down = depth[ev] == d + 1
        if not down.any():
            break
        eu, ev = eu[down], ev[down]
        np.add.at(sigma, ev, sigma[eu])
        levels.append((eu, ev))
        frontier = np.unique(ev)
    delta = np.zeros(nv, np.float64)
    for eu, ev in reversed(levels):
        np.add.at(delta, eu, sigma[eu] / sigma[ev] * (1.0 + delta[ev]))
    return depth, sigma, delta, len(levels)


def restatement(nv, s, d, sources):
    """(bc float64[nv] (index v - 1), eccentricity per source, vertices reached per source (the source included), max sigma per source)"""
    u, v = simple_edges(nv, s, d)
    bc = np.zeros(nv, np.float64); ecc, reached, maxsig = [], [], []
    for src in sources:
        depth, sigma, delta, e = single_source(nv, u, v, src)
        delta[src - 1] = 0.0
        bc += delta
        ecc.append(e); reached.append(int((depth >= 0).sum())); maxsig.append(float(sigma.max()))
    return bc, ecc, reached, maxsig


def plain_brandes(nv, s, d, sources):
    """Brandes' algorithm as published: a queue, a stack, predecessor lists; adjacency as Python sets (so duplicates vanish)."""
    adj = [set() for _ in range(nv + 1)]
    for a, b in zip(np.asarray(s).tolist(), np.asarray(d).tolist()):
        if a != b:
            adj[a].add(b)
    adj = [sorted(x) for x in adj]
    bc = [0.0] * (nv + 1)
    for src in sources:
        stack, pred = [], {}
        sigma = {src: 1.0}; dist = {src: 0}
        q = deque([src])
        while q:
            a = q.popleft(); stack.append(a)
            for b in adj[a]:
                if b not in dist:
                    dist[b] = dist[a] + 1; sigma[b] = 0.0; pred[b] = []; q.append(b)
                if dist[b] == dist[a] + 1:
                    sigma[b] += sigma[a]; pred[b].append(a)
        delta = dict.fromkeys(stack, 0.0)
        while stack:
            b = stack.pop()
            for a in pred.get(b, ()):
                delta[a] += sigma[a] / sigma[b] * (1.0 + delta[b])
            if b != src:
                bc[b] += delta[b]
    return np.array(bc[1:], np.float64)


def max_degree(nv, s, d):
    return int(max(np.bincount(s, minlength=nv + 1).max(initial=0), np.bincount(d, minlength=nv + 1).max(initial=0)))


def rtol_of(levels, degree, nsources):
    return 8.0 * (levels * (degree + 4) + nsources) * 2.0 ** -53


_memo = {}


def reference(name):
    """(nv, src, dst, sources, bc, eccentricities, reached, max sigmas, rtol), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d = GRAPHS[name]()
        sources = list(range(1, nv + 1)) if SOURCES[name] is ALL else list(SOURCES[name])
        bc, ecc, reached, maxsig = restatement(nv, s, d, sources)
        for a in (s, d, bc):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, sources, bc, ecc, reached, maxsig, rtol_of(max(ecc), max_degree(nv, s, d), len(sources)))
    return _memo[name]


def assert_close(got, ref, rtol, what):
    """exact zeros where the reference has zeros; elsewhere within rtol * ref"""
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    zero = ref == 0
    assert (got[zero] == 0).all(), "%s: %d values differ from an exact 0" % (what, int((got[zero] != 0).sum()))
    err = np.abs(got[~zero] - ref[~zero]) / ref[~zero]
    worst = float(err.max(initial=0.0))
    print("%s: largest relative difference %.3g (bound %.3g)" % (what, worst, rtol))
    assert worst <= rtol, "%s: relative difference %.3g above %.3g" % (what, worst, rtol)


# ---------------- the checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_restatement_equals_the_table(name):
    nv, s, d, sources, bc, ecc, reached, maxsig, rtol = reference(name)
    t_ecc, t_sigma, t_reached, t_nonzero, t_sum = EXPECTED[name]
    if t_ecc is not None:
        assert max(ecc) <= t_ecc if name == "R" else max(ecc) == t_ecc
    if t_sigma is not None:
        assert max(maxsig) == t_sigma
    if t_reached is not None:
        assert max(reached) == t_reached
    if t_nonzero is not None:
        assert int((bc != 0).sum()) == t_nonzero
    if t_sum is not None:
        assert float(bc.sum()) == pytest.approx(t_sum, rel=rtol)
    assert rtol <= 2.1e-11  # (R14: 2.02e-11, the largest here)
    if name == "G":
        assert reached == G_REACHED
    if name == "K":
        assert bc.max() == 39.0
    if name == "R14":
        assert int(np.bincount(simple_edges(nv, s, d)[0]).max()) == 2447  # a long out-row


def to_networkx(nv, s, d):
    import networkx as nx
    G = nx.DiGraph()
    G.add_nodes_from(range(1, nv + 1))
    G.add_edges_from((a, b) for a, b in zip(s.tolist(), d.tolist()) if a != b)
    return G


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("G", "Y")])
def test_restatement_equals_networkx(name):
    import networkx as nx
    nv, s, d, sources, bc, ecc, _, _, rtol = reference(name)
    G = to_networkx(nv, s, d)
    if SOURCES[name] is ALL:
        ref = nx.betweenness_centrality(G, normalized=False)
    else:
        ref = nx.betweenness_centrality_subset(G, sources, list(G.nodes), normalized=False)
    assert_close(bc, np.array([ref[v] for v in range(1, nv + 1)], np.float64), rtol, name)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_plain_brandes(name):
    nv, s, d, sources, bc, _, _, _, rtol = reference(name)
    plain = plain_brandes(nv, s, d, sources)
    assert_close(bc, plain, rtol, name)
    if name in EXACT:
        assert (bc == plain).all()


def test_closed_forms_of_f():
    nv, s, d, sources, bc, ecc, reached, maxsig, _ = reference("F")
    u, v = simple_edges(nv, s, d)
    for src in sources:
        sigma = single_source(nv, u, v, src)[1]
        assert sigma[3001] == sigma[3002] == 3000.0
    assert bc[0] == pytest.approx(3002.0, rel=1e-12)
    assert (bc[1:3001] == 2.0 / 3000.0 + 2.0 / 3000.0).all() and bc[1] == pytest.approx(4.0 / 3000.0, rel=1e-15)
    assert bc[3001] == 2.0
    assert (bc[3002:] == 0).all()
    assert ecc == [4, 3] and reached == [3004, 3003] and max_degree(nv, s, d) == 3200


def test_closed_forms_of_z_and_grid():
    nv, s, d = GRAPHS["Z"]()
    assert nv == 181 and len(s) == 270
    u, v = simple_edges(nv, s, d)
    depth, sigma, _, e = single_source(nv, u, v, 1)
    assert e == 90 and sigma.max() > 2.0 ** 63  # (beyond int64; 3^45 is not exact in fp64 and every junction rounds: compared within a bound)
    assert sigma[180] == pytest.approx(3.0 ** 45, rel=90 * 4 * 2.0 ** -53)
    bc = restatement(nv, s, d, [1, 2, 6])[0]
    assert bc.max() == pytest.approx(516.0, rel=1e-12) and bc.sum() == pytest.approx(23192.0, rel=1e-12)
    nv, s, d = GRAPHS["grid"]()
    u, v = simple_edges(nv, s, d)
    depth, sigma, _, e = single_source(nv, u, v, 1)
    assert e == 52 and sigma.max() == 495918532948104.0 < 2.0 ** 53  # C(52, 26)
    assert depth[nv - 1] == 52 and sigma[27 * 3 + 4] == 35.0          # C(7, 3) at (3, 4)


@pytest.mark.parametrize("name", ["F", "B", "L", "T", "R", "Q"])
def test_duplicates_and_loops_change_nothing(name):
    nv, s, d, sources, bc = reference(name)[:5]
    u, v = simple_edges(nv, s, d)
    assert len(u) < len(s)  # the raw list does hold duplicates or loops
    again = restatement(nv, (u + 1).astype(np.int32), (v + 1).astype(np.int32), sources)[0]
    assert again.tobytes() == bc.tobytes()
    rng = np.random.default_rng(3)
    order = rng.permutation(len(s))  # the order of the raw list does not matter either
    loops = np.arange(1, nv + 1, 7, dtype=np.int32)
    s2, d2 = np.concatenate([s[order], s[:50], loops]), np.concatenate([d[order], d[:50], loops])
    assert restatement(nv, s2, d2, sources)[0].tobytes() == bc.tobytes()


def test_a_source_listed_twice_counts_twice():
    nv, s, d = GRAPHS["R"]()
    one = restatement(nv, s, d, [5])[0]
    assert (restatement(nv, s, d, [5, 5])[0] == 2 * one).all()


def test_error_convention(lib):
    fake = C.c_void_p(16)  # never dereferenced
    ids = (C.c_int32 * 2)(1, 0)
    assert lib.gm_run_betweenness(None, None, 0, fake, None, None, None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_betweenness(fake, None, 0, None, None, None, None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_betweenness(fake, ids, -1, fake, None, None, None) == GM_ERR_INVALID
    assert b"negative" in lib.gm_last_error()
    assert lib.gm_run_betweenness(fake, None, 2, fake, None, None, None) == GM_ERR_INVALID
    assert b"null source array" in lib.gm_last_error()
    assert lib.gm_run_betweenness(fake, ids, 2, fake, None, None, None) == GM_ERR_INVALID
    assert b"source id 0 " in lib.gm_last_error()
    ids[1] = -7
    assert lib.gm_run_betweenness(fake, ids, 2, fake, None, None, None) == GM_ERR_INVALID
    assert b"source id -7 " in lib.gm_last_error()


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert ("int gm_run_betweenness(gm_graph_t* g, const int32_t* h_sources, int32_t nsources,\n"
            "                       double* d_bc, int32_t* d_last_depth, double* d_last_sigma, gm_stream_t stream);") in header
    assert "gm_run_betweenness" in _lib.SIGNATURES and hasattr(lib, "gm_run_betweenness")
    for slot, number in (("GM_WS_BC_ORDER", 19), ("GM_WS_BC_STATE", 20), ("GM_WS_BC_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header

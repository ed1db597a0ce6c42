"""Betweenness centrality on the GPU against the numpy restatement of tests/test_betweenness_cpu.py (which checks it against networkx
and a plain queue-based Brandes there).

bc is compared as that file's docstring derives: exactly 0 where the reference has 0, elsewhere within
rtol = 8 * (L * (D + 4) + S) * 2^-53 of the reference (L = the largest eccentricity among the sources, D = the largest in- or
out-degree of the raw edge list, S = the number of sources), computed from the graph and the restatement, never from the code
under test.  Where every value is an integer or one exact term (EXACT, and F's entries) equality is required.  Depths are
integers; path counts are exact integers while below 2^53, whatever the order they were added in: equality on every graph but Z,
whose counts reach 3^45 and are compared within 90 * 4 * 2^-53.  The backward phase pulls in a fixed order, so two calls on one
graph build return the same bytes."""
import ctypes as C

import numpy as np
import pytest

from tests.test_betweenness_cpu import (EXACT, NAMES, SOURCES, assert_close, max_degree, reference, restatement, rtol_of, simple_edges,
                                        single_source)
from tests.test_scc_cpu import reference as scc_reference

pytestmark = pytest.mark.gpu


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_betweenness_cpu.py: reference())."""

    def __init__(self, api):
        self.api = api
        self.L = api._lib.lib()
        self._g = {}
        self._sp = {}

    def graph(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self._g:
            nv, s, d = reference(name)[:3]
            self._g[key] = self.api.Graph(nv, s, d, **kw)
        return self._g[key]

    def paths(self, name, src):
        """(depth, sigma) of the restatement from one source, computed once"""
        if (name, src) not in self._sp:
            nv, s, d = reference(name)[:3]
            u, v = simple_edges(nv, s, d)
            self._sp[(name, src)] = single_source(nv, u, v, src)[:2]
        return self._sp[(name, src)]


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return Cases(api)


def layouts(api):
    return (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE))


def arg(name):
    return None if SOURCES[name] is None else list(SOURCES[name])


@pytest.mark.parametrize("name", NAMES)
def test_bc_equals_the_restatement(cases, name):
    nv, s, d, sources, ref, ecc, reached, maxsig, rtol = reference(name)
    g = cases.graph(name)
    bc = g.betweenness(arg(name))
    st = g.last_stats()
    print("%s: %d sources, %d passes (eccentricities sum to %d), rtol %.3g" % (name, st["iterations"], st["spmv_launches"], sum(ecc), rtol))
    assert bc.shape == (nv,)
    assert_close(bc, ref, rtol, name)
    if name in EXACT:
        assert (bc == ref).all(), "%s: %d values differ" % (name, int((bc != ref).sum()))
    if name == "F":
        assert (bc[1:3001] == 2.0 / 3000.0 + 2.0 / 3000.0).all()
        assert bc[3001] == 2.0 and (bc[3002:] == 0).all()
    # conditions on the scheme, not measurements
    assert st["iterations"] == len(sources)
    assert sum(ecc) <= st["spmv_launches"] <= sum(2 * e + 2 for e in ecc)


@pytest.mark.parametrize("name", NAMES)
def test_shortest_path_counts(cases, name):
    nv, s, d, sources = reference(name)[:4]
    src = 1 if name == "Z" else sources[-1]
    ref_depth, ref_sigma = cases.paths(name, src)
    depth, sigma = cases.graph(name).shortest_path_counts(src)
    assert depth.dtype == np.int32 and sigma.dtype == np.float64 and depth.shape == sigma.shape == (nv,)
    assert (depth == ref_depth).all()
    assert ((sigma == 0) == (ref_depth < 0)).all()
    if name == "Z":
        assert sigma.max() > 2 ** 63
        ok = ref_sigma > 0
        assert (np.abs(sigma[ok] - ref_sigma[ok]) <= 90 * 4 * 2.0 ** -53 * ref_sigma[ok]).all()
    else:
        assert ref_sigma.max() < 2.0 ** 53 and (sigma == ref_sigma).all()


@pytest.mark.parametrize("name", ["R14", "grid", "F"])
def test_two_calls_give_the_same_bytes(cases, name):
    g = cases.graph(name)
    first = g.betweenness(arg(name))
    second = g.betweenness(arg(name))
    assert first.tobytes() == second.tobytes()


@pytest.mark.parametrize("name", ["R", "L", "F"])
def test_layouts_and_native_permutations(cases, name):
    """Whatever the device order (degree-ranked or native) and whatever the native permutation (ref_threads = 2)."""
    api = cases.api
    nv, s, d, sources, ref, ecc, _, _, rtol = reference(name)
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    ref_depth, ref_sigma = cases.paths(name, sources[-1])
    for kw in layouts(api):
        g = cases.graph(name, **kw)
        assert_close(g.betweenness(arg(name)), ref, rtol, "%s %s" % (name, kw))  # (with the exact zeros)
        depth, sigma = g.shortest_path_counts(sources[-1])
        assert (depth == ref_depth).all() and (sigma == ref_sigma).all(), kw


@pytest.mark.parametrize("name", ["R", "F", "T"])
def test_the_in_adjacency_alone_gives_the_same_bytes(cases, name):
    api = cases.api
    both = cases.graph(name).betweenness(arg(name))
    alone = cases.graph(name, directions=api.GM_DIR_IN).betweenness(arg(name))
    assert both.tobytes() == alone.tobytes()


def test_sources(cases):
    nv, s, d, sources, ref, _, _, _, rtol = reference("R")
    g = cases.graph("R")
    one = g.betweenness([5])
    assert (g.betweenness([5, 5]) == 2 * one).all() and one.any()
    joint = g.betweenness(sources)
    assert_close(g.betweenness(sources[:3]) + g.betweenness(sources[3:]), joint, rtol, "R in two calls")
    empty = g.betweenness([])
    assert empty.dtype == np.float64 and empty.shape == (nv,) and (empty == 0).all()
    assert g.last_stats()["iterations"] == 0 and g.last_stats()["spmv_launches"] == 0
    t = cases.graph("test")
    assert t.betweenness(None).tobytes() == t.betweenness(list(range(1, 9))).tobytes()
    assert t.betweenness(np.arange(1, 9, dtype=np.int64)).tobytes() == t.betweenness(None).tobytes()


@pytest.mark.parametrize("name", ["G", "F"])
def test_adjacencies_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    g.betweenness(arg(name))
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, _), (rp1, ci1, _) in zip(before, after):
        assert rp0.tobytes() == rp1.tobytes() and ci0.tobytes() == ci1.tobytes()


def test_the_five_calls_share_their_slots(cases):
    """Workspace slots 19-21 serve triangle counting, components, the k-core call, strong components and this one: each leaves the
    others' next call undisturbed."""
    nv, s, d = scc_reference("A")[:3]
    g = cases.api.Graph(nv, s, d)
    srcs = [1, 2, 3, 1500, 3000]
    ref, ecc = restatement(nv, s, d, srcs)[:2]
    first = {}
    for call in ("triangle_count", "betweenness", "connected_components", "betweenness", "core_numbers", "strong_components", "betweenness",
                 "triangle_count", "connected_components", "core_numbers", "strong_components", "betweenness"):
        if call == "betweenness":
            got = (0, g.betweenness(srcs))
        else:
            got = getattr(g, call)()
        if call not in first:
            first[call] = got
        assert got[0] == first[call][0] and got[1].tobytes() == first[call][1].tobytes(), call
    assert_close(first["betweenness"][1], ref, rtol_of(max(ecc), max_degree(nv, s, d), len(srcs)), "A after triangle counting")
    assert (first["strong_components"][1] == scc_reference("A")[3]).all()


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    g = api.Graph(200, empty, empty)
    bc = g.betweenness()
    assert bc.dtype == np.float64 and bc.shape == (200,) and (bc == 0).all()
    assert g.last_stats()["iterations"] == 200
    depth, sigma = g.shortest_path_counts(7)
    assert (np.delete(depth, 6) == -1).all() and depth[6] == 0 and sigma[6] == 1 and sigma.sum() == 1


def test_graph_of_one_self_loop(cases):
    api = cases.api
    g = api.Graph(70, np.array([33], np.int32), np.array([33], np.int32))
    assert (g.betweenness() == 0).all()
    depth, sigma = g.shortest_path_counts(33)
    assert depth[32] == 0 and sigma[32] == 1 and (np.delete(depth, 32) == -1).all()


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d = reference("R")[:3]
    ids = (C.c_int32 * 2)(1, 2)

    def outputs(g):
        return (torch.full((g.rows,), 7.0, dtype=torch.float64, device=g.device), torch.full((g.rows,), 7, dtype=torch.int32, device=g.device),
                torch.full((g.rows,), 7.0, dtype=torch.float64, device=g.device))

    def untouched(o):
        return all(bool((t == 7).all()) for t in o)

    g = api.Graph(nv, s, d, layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128))
    o = outputs(g)
    assert L.gm_run_betweenness(g.h, ids, 2, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None) == 4  # GM_ERR_UNSUPPORTED
    assert b"whole graphs" in L.gm_last_error() and untouched(o)
    with pytest.raises(api._lib.GMError):
        g.betweenness([1])
    g = api.Graph(nv, s, d, directions=api.GM_DIR_OUT)
    o = outputs(g)
    assert L.gm_run_betweenness(g.h, ids, 2, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None) == 4
    assert b"GM_DIR_IN" in L.gm_last_error() and untouched(o)
    with pytest.raises(api._lib.GMError):
        g.betweenness()
    g = cases.graph("R")
    o = outputs(g)
    for bad in (0, nv + 1):
        ids[1] = bad
        assert L.gm_run_betweenness(g.h, ids, 2, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None) == 1  # GM_ERR_INVALID
        assert (b"source id %d " % bad) in L.gm_last_error() and untouched(o)
        with pytest.raises(api._lib.GMError):
            g.betweenness([1, bad])
    assert L.gm_run_betweenness(g.h, ids, -1, o[0].data_ptr(), None, None, None) == 1 and untouched(o)
    assert L.gm_run_betweenness(g.h, None, 2, o[0].data_ptr(), None, None, None) == 1 and untouched(o)

"""Minimum spanning forest on the GPU against the verifier and the plain Kruskal of tests/test_spanning_forest_cpu.py (which checks
them against networkx and scipy there, and shows that the verifier rejects wrong forests).  Integers: every comparison is
equality.  With distinct weights the forest is unique, so every layout, native permutation and choice of adjacency must give the
same array; with ties the total and the sorted weights must be the same everywhere and every result must pass the verifier."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.test_spanning_forest_cpu import DISTINCT, NAMES, check_forest, reference

pytestmark = pytest.mark.gpu


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_spanning_forest_cpu.py: reference())."""

    def __init__(self, api):
        self.api = api
        self.L = api._lib.lib()
        self._g = {}

    def graph(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self._g:
            nv, s, d, w = reference(name)[:4]
            self._g[key] = self.api.Graph(nv, s, d, val=w, **kw)
        return self._g[key]


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return Cases(api)


def variants(api):
    """Device orders (degree-ranked or native), native permutations (ref_threads = 2) and the adjacency that is read."""
    return (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE),
            dict(directions=api.GM_DIR_OUT), dict(directions=api.GM_DIR_IN), dict(directions=api.GM_DIR_OUT | api.GM_DIR_IN))


def assert_real_permutations(cases, name):
    api = cases.api
    nv = reference(name)[0]
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    don, _ = cases.graph(name).maps_to_host()
    assert (don != np.arange(nv)).any()  # the degree-ranked device order is a real permutation here


@pytest.mark.parametrize("name", NAMES)
def test_forest_passes_the_verifier(cases, name):
    nv, s, d, w, ref_total, ref_edges, _ = reference(name)
    g = cases.graph(name)
    total, edges = g.spanning_forest()
    check_forest(nv, s, d, w, total, edges)
    # the derived bound of the rounds plus the last, empty pass; on P (one round hooks a chain of 40 000 trees) the call ends
    # because its loop bounds hold
    iterations = g.last_stats()["iterations"]
    print("%s: %d pick passes, %d jump passes" % (name, iterations, g.last_stats()["spmv_launches"]))
    assert 1 <= iterations <= int(math.floor(math.log2(nv))) + 1
    if name in DISTINCT:
        assert total == ref_total and edges.tobytes() == ref_edges.tobytes()


@pytest.mark.parametrize("name", DISTINCT)
def test_distinct_weights_give_the_one_forest_everywhere(cases, name):
    nv, s, d, w, ref_total, ref_edges, _ = reference(name)
    assert len(np.unique(w)) == len(w)
    assert_real_permutations(cases, name)
    for kw in variants(cases.api):
        total, edges = cases.graph(name, **kw).spanning_forest()
        assert total == ref_total, kw
        assert edges.dtype == np.int32 and edges.shape == ref_edges.shape and (edges == ref_edges).all(), kw


@pytest.mark.parametrize("name", ["A", "E", "M"])
def test_ties_keep_the_total_and_the_sorted_weights_everywhere(cases, name):
    nv, s, d, w, ref_total, ref_edges, _ = reference(name)
    assert_real_permutations(cases, name)
    for kw in variants(cases.api):
        total, edges = cases.graph(name, **kw).spanning_forest()
        check_forest(nv, s, d, w, total, edges)
        assert total == ref_total and (edges[:, 2] == ref_edges[:, 2]).all(), kw


def test_m_reports_the_lightest_copy_and_no_loop(cases):
    api = cases.api
    for kw in (dict(),) + variants(api):
        total, edges = cases.graph("M", **kw).spanning_forest()
        assert (edges[:, 0] < edges[:, 1]).all(), kw
        assert not (edges[:, 2] == -100).any(), kw  # the loops' weight
        b = edges[(edges[:, 0] >= 201) & (edges[:, 1] <= 400)]
        assert len(b) == 199 and (b[:, 2] == 3).all(), kw            # every pair is given with 5, 3 (the other way round) and 9
        c = edges[(edges[:, 0] >= 401) & (edges[:, 1] <= 600)]
        assert len(c) == 199 and (c[:, 2] == np.where(c[:, 0] % 2 == 1, 8, 6)).all(), kw  # antiparallel: 8 and 8, 8 and 6
        assert len(edges) == 3 * 199


def test_h_has_a_giant_row(cases):
    api = cases.api
    assert cases.graph("H").csr(api.GM_DIR_OUT).ngiant >= 1


def test_graph_without_values_weighs_every_edge_one(cases):
    api = cases.api
    nv, s, d, _, _, _, labels = reference("A")
    g = api.Graph(nv, s, d)
    total, edges = g.spanning_forest()
    assert total == len(edges) == nv - len(np.unique(labels))
    check_forest(nv, s, d, np.ones(len(s), np.int32), total, edges)


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    total, edges = api.Graph(200, empty, empty).spanning_forest()
    assert total == 0 and edges.dtype == np.int32 and edges.shape == (0, 3)


def test_graph_of_one_self_loop(cases):
    api = cases.api
    one = np.array([33], np.int32)
    total, edges = api.Graph(70, one, one, val=np.array([-9], np.int32)).spanning_forest()
    assert total == 0 and edges.dtype == np.int32 and edges.shape == (0, 3)


@pytest.mark.parametrize("name", ["A", "H"])
def test_second_call_and_adjacency_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    n1, total1, raw1 = g.spanning_forest_raw()
    n2, total2, raw2 = g.spanning_forest_raw()
    assert raw1.shape == (g.rows, 3)
    assert n1 == n2 and total1 == total2 and raw1.cpu().numpy().tobytes() == raw2.cpu().numpy().tobytes()
    unset = raw1.cpu().numpy()
    unset = unset[unset[:, 0] == 0]
    assert len(unset) == g.rows - n1 and (unset == 0).all()  # every slot that was not hooked holds (0, 0, 0)
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, v0), (rp1, ci1, v1) in zip(before, after):
        assert rp0.tobytes() == rp1.tobytes() and ci0.tobytes() == ci1.tobytes() and v0 is not None and v0.tobytes() == v1.tobytes()


def test_the_calls_share_their_slots(cases):
    """Workspace slots 19-21 serve this call, triangle counting, components and the k-core call: each leaves the others' next call
    undisturbed."""
    nv, s, d, w, ref_total, ref_edges, _ = reference("D")
    g = cases.graph("D")
    total0, edges0 = g.spanning_forest()
    tri1 = g.triangle_count()
    cc2 = g.connected_components()
    kc3 = g.core_numbers()
    total4, edges4 = g.spanning_forest()
    tri5 = g.triangle_count()
    cc6 = g.connected_components()
    kc7 = g.core_numbers()
    assert total0 == total4 == ref_total and edges0.tobytes() == edges4.tobytes() == ref_edges.tobytes()
    assert tri1[0] == tri5[0] and (tri1[1] == tri5[1]).all()
    assert cc2[0] == cc6[0] and (cc2[1] == cc6[1]).all() and cc2[0] == nv - len(ref_edges)
    assert kc3[0] == kc7[0] and (kc3[1] == kc7[1]).all()


def test_msf_form_does_not_change_the_result(cases):
    """The measurement knob: no look, no combining per wave, pointer doubling, one walk per round."""
    L = cases.L
    try:
        for name in ("D", "P", "H"):
            nv, s, d, w, ref_total, ref_edges, _ = reference(name)
            g = cases.graph(name)
            for form in (1, 2, 3, 4, 8, 11):
                assert L.gm_set_option(b"msf_form", form) == 0
                total, edges = g.spanning_forest()
                assert total == ref_total, (name, form)
                if name in DISTINCT:
                    assert edges.tobytes() == ref_edges.tobytes(), (name, form)
                else:
                    check_forest(nv, s, d, w, total, edges)
    finally:
        L.gm_reset_options()


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d, w = reference("A")[:4]
    n, total = C.c_int32(77), C.c_int64(78)
    g = api.Graph(nv, s, d, val=w, layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128))
    out = torch.full((g.rows, 3), 7, dtype=torch.int32, device=g.device)
    assert L.gm_run_spanning_forest(g.h, out.data_ptr(), C.byref(n), C.byref(total), None) == 4  # GM_ERR_UNSUPPORTED
    assert b"whole graphs" in L.gm_last_error()
    assert (out == 7).all() and n.value == 77 and total.value == 78
    with pytest.raises(api._lib.GMError):
        g.spanning_forest()

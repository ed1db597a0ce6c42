"""Connected components on the GPU against the numpy restatement of tests/test_components_cpu.py (which checks it against scipy
and a plain breadth-first search there).  Integers: every comparison is equality.  The labels are defined by the graph alone, so
every layout, native permutation and choice of adjacency must give the same array."""
import ctypes as C

import numpy as np
import pytest

from tests.test_components_cpu import EXPECTED, NAMES, isolated, reference

pytestmark = pytest.mark.gpu


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_components_cpu.py: reference())."""

    def __init__(self, api):
        self.api = api
        self.L = api._lib.lib()
        self._g = {}

    def graph(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self._g:
            nv, s, d, _, _ = reference(name)
            self._g[key] = self.api.Graph(nv, s, d, **kw)
        return self._g[key]


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return Cases(api)


def assert_equal_labels(got, ref, what):
    diff = np.nonzero(got != ref)[0]
    assert got.dtype == np.int32 and got.shape == ref.shape and diff.size == 0, \
        "%s: %d vertices differ, first vertex %d: %d instead of %d" % (what, diff.size, diff[0] + 1, got[diff[0]], ref[diff[0]])


@pytest.mark.parametrize("name", NAMES)
def test_labels_equal_the_restatement(cases, name):
    nv, s, d, ref, _ = reference(name)
    n, labels = cases.graph(name).connected_components()
    assert_equal_labels(labels, ref, name)
    assert n == EXPECTED[name][1]
    assert (labels <= np.arange(1, nv + 1)).all()
    iso = isolated(nv, s, d)
    assert (labels[iso] == np.nonzero(iso)[0] + 1).all()


@pytest.mark.parametrize("name", ["A", "P"])
def test_layouts_and_native_permutations(cases, name):
    """The minimum is taken over VERTEX ids, whatever the device order (degree-ranked or native) and whatever the native
    permutation (ref_threads = 2: no longer the identity at 3000 and 4097 vertices)."""
    api = cases.api
    nv, s, d, ref, _ = reference(name)
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    for kw in (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE)):
        n, labels = cases.graph(name, **kw).connected_components()
        assert_equal_labels(labels, ref, "%s %s" % (name, kw))
        assert n == EXPECTED[name][1]
    don, _ = cases.graph(name).maps_to_host()
    assert (don != np.arange(nv)).any()  # the degree-ranked device order is a real permutation here


@pytest.mark.parametrize("name", ["A", "H", "K"])
def test_either_adjacency_gives_the_same_labels(cases, name):
    api = cases.api
    nv, s, d, ref, _ = reference(name)
    for directions in (api.GM_DIR_OUT, api.GM_DIR_IN, api.GM_DIR_OUT | api.GM_DIR_IN):
        n, labels = cases.graph(name, directions=directions).connected_components()
        assert_equal_labels(labels, ref, "%s directions=%d" % (name, directions))
        assert n == EXPECTED[name][1]


def test_h_has_a_giant_row_and_its_hubs_lose_to_the_minimum(cases):
    api = cases.api
    g = cases.graph("H")
    assert g.csr(api.GM_DIR_OUT).ngiant >= 1
    rp, _, _ = g.csr_to_host(api.GM_DIR_IN)
    assert int(np.diff(rp).max()) == 6000  # the long row of the IN adjacency is another vertex's
    _, labels = g.connected_components()
    assert labels[19999] == 2 and labels[19998] == 10001 and labels[0] == labels[9499] == labels[9500] == 1


def test_rounds_do_not_follow_the_diameter(cases):
    """A condition, not a measurement: the restatement needs 9 rounds on the shuffled path of 4097 vertices (9-10 on seeds 0-4), a
    scheme linear in the diameter about 4096.  A GPU round may see newer parents than the restatement's and so differ by a few
    rounds, not by an order of magnitude."""
    g = cases.graph("P")
    g.connected_components()
    iterations = g.last_stats()["iterations"]
    print("hook passes on P: %d (restatement: %d)" % (iterations, reference("P")[4]))
    assert 1 <= iterations <= 32


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    n, labels = api.Graph(200, empty, empty).connected_components()
    assert n == 200 and labels.dtype == np.int32 and (labels == np.arange(1, 201)).all()


@pytest.mark.parametrize("name", ["A", "H"])
def test_second_call_and_adjacency_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    first = g.connected_components()
    second = g.connected_components()
    assert first[0] == second[0] and (first[1] == second[1]).all()
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, _), (rp1, ci1, _) in zip(before, after):
        assert (rp0 == rp1).all() and (ci0 == ci1).all()


def test_triangle_counting_and_components_share_their_slots(cases):
    """Workspace slots 19-21 serve both calls: each leaves the other's next call undisturbed."""
    nv, s, d, ref, _ = reference("A")
    g = cases.graph("A")
    total0, tri0 = g.triangle_count()
    n1, labels1 = g.connected_components()
    total2, tri2 = g.triangle_count()
    n3, labels3 = g.connected_components()
    assert total0 == total2 and (tri0 == tri2).all()
    assert n1 == n3 == EXPECTED["A"][1]
    assert_equal_labels(labels1, ref, "A after triangle counting")
    assert_equal_labels(labels3, ref, "A after triangle counting, twice")


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d, _, _ = reference("A")
    n = C.c_int32(77)
    g = api.Graph(nv, s, d, layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128))
    out = torch.full((g.rows,), 7, dtype=torch.int32, device=g.device)
    assert L.gm_run_connected_components(g.h, out.data_ptr(), C.byref(n), None) == 4  # GM_ERR_UNSUPPORTED
    assert b"whole graphs" in L.gm_last_error()
    assert (out == 7).all() and n.value == 77
    with pytest.raises(api._lib.GMError):
        g.connected_components()

"""Strongly connected components on the GPU against the numpy restatement of tests/test_scc_cpu.py (which checks it against scipy
and a plain Tarjan there).  Integers: every comparison is equality.  The labels are defined by the directed graph alone, so every
layout, native permutation and device order must give the same array; the rounds are defined by vertex ids alone, so their number
is the restatement's, and the passes can only be fewer (the restatement's are synchronous)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_scc_cpu import EXPECTED, NAMES, reference

pytestmark = pytest.mark.gpu


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_scc_cpu.py: reference())."""

    def __init__(self, api):
        self.api = api
        self.L = api._lib.lib()
        self._g = {}

    def graph(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self._g:
            nv, s, d = reference(name)[:3]
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


def layouts(api):
    return (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE))


@pytest.mark.parametrize("name", NAMES)
def test_labels_equal_the_restatement(cases, name):
    nv, s, d, ref, rounds, (tp, fp, bp), trimmed, per_round = reference(name)
    g = cases.graph(name)
    n, labels = g.strong_components()
    assert_equal_labels(labels, ref, name)
    assert n == EXPECTED[name][2] == len(np.unique(ref))
    # conditions on the scheme, not measurements: the rounds are the restatement's, the passes at most its
    st = g.last_stats()
    print("%s: %d rounds, %d passes (restatement: %d rounds, %d + %d + %d passes)" % (name, st["iterations"], st["spmv_launches"], rounds, tp, fp, bp))
    assert st["iterations"] == rounds
    assert 0 <= st["spmv_launches"] <= tp + fp + bp
    if rounds == 0:
        assert st["spmv_launches"] == tp


@pytest.mark.parametrize("name", ["A", "Y", "T", "L"])
def test_layouts_and_native_permutations(cases, name):
    """Whatever the device order (degree-ranked or native) and whatever the native permutation (ref_threads = 2)."""
    api = cases.api
    nv, s, d, ref, rounds = reference(name)[:5]
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    for kw in layouts(api):
        g = cases.graph(name, **kw)
        n, labels = g.strong_components()
        assert_equal_labels(labels, ref, "%s %s" % (name, kw))
        assert n == EXPECTED[name][2] and g.last_stats()["iterations"] == rounds


def test_the_degree_ranked_order_is_a_permutation_on_a(cases):
    don, _ = cases.graph("A").maps_to_host()
    assert (don != np.arange(reference("A")[0])).any()


def test_g_has_a_giant_row_and_the_hubs_components(cases):
    api = cases.api
    g = cases.graph("G")
    assert g.csr(api.GM_DIR_OUT).ngiant >= 1
    _, labels = g.strong_components()
    assert labels[19999] == 2
    assert (labels[1:3001] == 2).all()
    assert labels[11999] == labels[19998] == 12000


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    n, labels = api.Graph(200, empty, empty).strong_components()
    assert n == 200 and labels.dtype == np.int32 and (labels == np.arange(1, 201)).all()


def test_graph_of_one_self_loop(cases):
    api = cases.api
    n, labels = api.Graph(70, np.array([33], np.int32), np.array([33], np.int32)).strong_components()
    assert n == 70 and (labels == np.arange(1, 71)).all()


def test_graph_of_one_two_cycle(cases):
    api = cases.api
    n, labels = api.Graph(64, np.array([5, 9], np.int32), np.array([9, 5], np.int32)).strong_components()
    ref = np.arange(1, 65, dtype=np.int32)
    ref[8] = 5
    assert n == 63 and labels[8] == 5
    assert_equal_labels(labels, ref, "5 <-> 9")


@pytest.mark.parametrize("name", ["A", "G"])
def test_second_call_and_adjacencies_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    first = g.strong_components()
    second = g.strong_components()
    assert first[0] == second[0] and (first[1] == second[1]).all()
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, _), (rp1, ci1, _) in zip(before, after):
        assert rp0.tobytes() == rp1.tobytes() and ci0.tobytes() == ci1.tobytes()


def test_the_four_calls_share_their_slots(cases):
    """Workspace slots 19-21 serve triangle counting, components, the k-core call and this one: each leaves the others' next call
    undisturbed."""
    ref = reference("A")[3]
    g = cases.graph("A")
    first = {}
    for call in ("triangle_count", "strong_components", "connected_components", "core_numbers", "strong_components", "triangle_count",
                 "connected_components", "core_numbers"):
        total, per_vertex = getattr(g, call)()
        if call not in first:
            first[call] = (total, per_vertex)
        assert total == first[call][0] and (per_vertex == first[call][1]).all(), call
    assert first["strong_components"][0] == EXPECTED["A"][2]
    assert_equal_labels(first["strong_components"][1], ref, "A after triangle counting")


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d = reference("A")[:3]
    n = C.c_int32(77)
    g = api.Graph(nv, s, d, layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128))
    out = torch.full((g.rows,), 7, dtype=torch.int32, device=g.device)
    assert L.gm_run_strong_components(g.h, out.data_ptr(), C.byref(n), None) == 4  # GM_ERR_UNSUPPORTED
    assert b"whole graphs" in L.gm_last_error()
    assert (out == 7).all() and n.value == 77
    with pytest.raises(api._lib.GMError):
        g.strong_components()
    for directions in (api.GM_DIR_OUT, api.GM_DIR_IN):
        g = api.Graph(nv, s, d, directions=directions)
        out = torch.full((g.rows,), 7, dtype=torch.int32, device=g.device)
        assert L.gm_run_strong_components(g.h, out.data_ptr(), C.byref(n), None) == 4
        assert b"both adjacencies" in L.gm_last_error()
        assert (out == 7).all() and n.value == 77
        with pytest.raises(api._lib.GMError):
            g.strong_components()

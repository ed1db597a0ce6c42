"""K-core decomposition on the GPU against the numpy restatement of tests/test_kcore_cpu.py (which checks it against a plain bucket
peel and networkx there).  Integers: every comparison is equality.  The core numbers are defined by the simple undirected graph
under the edge list alone, so every layout, native permutation and choice of adjacency must give the same array."""
import ctypes as C

import numpy as np
import pytest

from tests.test_kcore_cpu import EXPECTED, NAMES, reference, simple_degrees

pytestmark = pytest.mark.gpu


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_kcore_cpu.py: reference())."""

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


def assert_equal_core(got, ref, what):
    diff = np.nonzero(got != ref)[0]
    assert got.dtype == np.int32 and got.shape == ref.shape and diff.size == 0, \
        "%s: %d vertices differ, first vertex %d: %d instead of %d" % (what, diff.size, diff[0] + 1, got[diff[0]], ref[diff[0]])


def layouts(api):
    return (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE))


@pytest.mark.parametrize("name", NAMES)
def test_core_numbers_equal_the_restatement(cases, name):
    nv, s, d, ref, levels, passes = reference(name)
    g = cases.graph(name)
    kmax, core = g.core_numbers()
    assert_equal_core(core, ref, name)
    assert kmax == EXPECTED[name][1] == int(ref.max())
    deg = simple_degrees(nv, s, d)
    assert (core[deg == 0] == 0).all() and (core <= deg).all()
    # conditions on the rounds, not measurements: a level per distinct core number (levels jump), and no more passes than the
    # restatement's (the kernels process the same lists; nothing follows chains)
    st = g.last_stats()
    print("%s: %d levels, %d passes (restatement: %d, %d)" % (name, st["spmv_launches"], st["iterations"], levels, passes))
    assert st["spmv_launches"] == len(np.unique(ref)) == levels
    assert 1 <= st["iterations"] <= passes


def test_levels_jump_on_c(cases):
    g = cases.graph("C")
    kmax, core = g.core_numbers()
    assert kmax == 69 and g.last_stats()["spmv_launches"] == 5


@pytest.mark.parametrize("name", ["A", "P", "M"])
def test_layouts_and_native_permutations(cases, name):
    """Whatever the device order (degree-ranked or native) and whatever the native permutation (ref_threads = 2: no longer the
    identity at 3000, 4097 and 640 vertices)."""
    api = cases.api
    nv, s, d, ref, _, _ = reference(name)
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    for kw in layouts(api):
        kmax, core = cases.graph(name, **kw).core_numbers()
        assert_equal_core(core, ref, "%s %s" % (name, kw))
        assert kmax == EXPECTED[name][1]
    don, _ = cases.graph(name).maps_to_host()
    assert (don != np.arange(nv)).any()  # the degree-ranked device order is a real permutation here


@pytest.mark.parametrize("name", ["A", "H", "C", "M", "R"])
def test_either_adjacency_gives_the_same_core_numbers(cases, name):
    """The simple adjacency built from GM_DIR_OUT alone, from GM_DIR_IN alone and from a graph that holds both."""
    api = cases.api
    nv, s, d, ref, _, _ = reference(name)
    for directions in (api.GM_DIR_OUT, api.GM_DIR_IN, api.GM_DIR_OUT | api.GM_DIR_IN):
        kmax, core = cases.graph(name, directions=directions).core_numbers()
        assert_equal_core(core, ref, "%s directions=%d" % (name, directions))
        assert kmax == EXPECTED[name][1]


def test_r_has_antiparallel_pairs():
    nv, s, d = reference("R")[:3]
    keep = s != d
    fwd = np.unique(s[keep].astype(np.int64) * (nv + 1) + d[keep])
    bwd = np.unique(d[keep].astype(np.int64) * (nv + 1) + s[keep])
    assert int(np.isin(fwd, bwd).sum()) == 2 * 140


def test_h_has_a_giant_row_and_the_hubs_core_numbers(cases):
    api = cases.api
    g = cases.graph("H")
    assert g.csr(api.GM_DIR_OUT).ngiant >= 1
    _, core = g.core_numbers()
    assert core[19999] == 1 and core[19998] == 1  # H's hubs: stars
    _, core = cases.graph("C").core_numbers()
    # C's hub has 4600 neighbours; two of its leaves (4500, 4501) are joined, so it lies in a triangle: 2, every other leaf 1
    assert core[399] == 2 and core[4499] == core[4500] == 2 and (np.delete(core[400:4999], [4099, 4100]) == 1).all()


def test_m_counts_no_loop_duplicate_or_reverse_edge(cases):
    api = cases.api
    for kw in (dict(),) + layouts(api):
        kmax, core = cases.graph("M", **kw).core_numbers()
        assert kmax == 1 and (core[:600] == 1).all() and (core[600:] == 0).all(), kw


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    kmax, core = api.Graph(200, empty, empty).core_numbers()
    assert kmax == 0 and core.dtype == np.int32 and core.shape == (200,) and (core == 0).all()


def test_graph_of_one_self_loop(cases):
    api = cases.api
    kmax, core = api.Graph(70, np.array([33], np.int32), np.array([33], np.int32)).core_numbers()
    assert kmax == 0 and core.dtype == np.int32 and (core == 0).all()


@pytest.mark.parametrize("name", ["A", "H"])
def test_second_call_and_adjacency_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    first = g.core_numbers()
    second = g.core_numbers()
    assert first[0] == second[0] and (first[1] == second[1]).all()
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, _), (rp1, ci1, _) in zip(before, after):
        assert rp0.tobytes() == rp1.tobytes() and ci0.tobytes() == ci1.tobytes()


def test_the_three_calls_share_their_slots(cases):
    """Workspace slots 19-21 serve triangle counting, components and the k-core call: each leaves the others' next call undisturbed."""
    nv, s, d, ref, _, _ = reference("A")
    g = cases.graph("A")
    total0, tri0 = g.triangle_count()
    kmax1, core1 = g.core_numbers()
    n2, labels2 = g.connected_components()
    kmax3, core3 = g.core_numbers()
    total4, tri4 = g.triangle_count()
    n5, labels5 = g.connected_components()
    assert total0 == total4 and (tri0 == tri4).all()
    assert n2 == n5 and (labels2 == labels5).all()
    assert kmax1 == kmax3 == EXPECTED["A"][1]
    assert_equal_core(core1, ref, "A after triangle counting")
    assert_equal_core(core3, ref, "A after components")


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d = reference("A")[:3]
    kmax = C.c_int32(77)
    g = api.Graph(nv, s, d, layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128))
    out = torch.full((g.rows,), 7, dtype=torch.int32, device=g.device)
    assert L.gm_run_kcore(g.h, out.data_ptr(), C.byref(kmax), None) == 4  # GM_ERR_UNSUPPORTED
    assert b"whole graphs" in L.gm_last_error()
    assert (out == 7).all() and kmax.value == 77
    with pytest.raises(api._lib.GMError):
        g.core_numbers()

"""Triangle counting on the GPU against the numpy restatement of tests/test_triangles_cpu.py (which checks it against a plain
two-pointer merge there).  Integers: every comparison is equality.  Every graph runs through the three values of option
"tc_form" (0 automatic, 1 the row kernel wherever a row's own list can be staged, 2 the pieces kernel only)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_triangles_cpu import EXPECTED, reference

pytestmark = pytest.mark.gpu
FORMS = (0, 1, 2)
NAMES = ("A", "B", "C", "Cd", "test", "upper")


class Cases:
    """Graphs on the GPU, built once per module (the references are kept by tests/test_triangles_cpu.py: reference())."""

    def __init__(self, api):
        self.api = api
        self.L = api._lib.lib()
        self._g = {}

    def graph(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self._g:
            nv, s, d, _ = reference(name)
            self._g[key] = self.api.Graph(nv, s, d, **kw)
        return self._g[key]

    def count(self, g, form):
        assert self.L.gm_set_option(b"tc_form", form) == 0
        return g.triangle_count()


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return Cases(api)


def assert_equal_counts(got, ref, what):
    diff = np.nonzero(got != ref)[0]
    assert got.dtype == np.int64 and got.shape == ref.shape and diff.size == 0, \
        "%s: %d vertices differ, first vertex %d: %d instead of %d" % (what, diff.size, diff[0] + 1, got[diff[0]], ref[diff[0]])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_the_restatement(cases, name, form):
    nv, s, d, ref = reference(name)
    total, tri = cases.count(cases.graph(name), form)
    assert_equal_counts(tri, ref, "%s tc_form=%d" % (name, form))
    assert total == int(ref.sum()) == EXPECTED[name][1]
    # isolated vertices and vertices without in-edges get 0
    no_in = np.bincount(d, minlength=nv + 1)[1:] == 0
    assert no_in.any() and (tri[no_in] == 0).all()
    if name == "A":
        assert tri[299] == 0  # vertex 300 has no edge at all


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["A", "C"])
def test_layouts_and_native_permutations(cases, name, form):
    """Device ids are not a sort order: the keys come from the native order, whatever the device order (degree-ranked or
    native) and whatever the native permutation (ref_threads = 2: no longer the identity at 300 and 9000 vertices)."""
    api = cases.api
    nv, s, d, ref = reference(name)
    assert (api.native_index(nv, 2 * 16) != np.arange(nv)).any()
    for kw in (dict(layout=api.GM_LAYOUT_NATIVE), dict(ref_threads=2), dict(ref_threads=2, layout=api.GM_LAYOUT_NATIVE)):
        total, tri = cases.count(cases.graph(name, **kw), form)
        assert_equal_counts(tri, ref, "%s %s tc_form=%d" % (name, kw, form))
        assert total == EXPECTED[name][1]
    don, _ = cases.graph(name).maps_to_host()
    assert (don != np.arange(nv)).any()  # the degree-ranked device order is a real permutation here


def test_c_has_a_giant_row_and_a_list_beyond_the_lds_share(cases):
    api = cases.api
    g = cases.graph("C")
    assert g.csr(api.GM_DIR_OUT).ngiant >= 1
    rp, _, _ = g.csr_to_host(api.GM_DIR_IN)
    assert int(np.diff(rp).max()) > 2048  # more keys than a wave's 8 KB of LDS hold at either key width


def test_graph_without_edges(cases):
    api = cases.api
    empty = np.zeros(0, np.int32)
    g = api.Graph(200, empty, empty)
    for form in FORMS:
        total, tri = cases.count(g, form)
        assert total == 0 and tri.shape == (200,) and (tri == 0).all()


@pytest.mark.parametrize("name", ["A", "C"])
def test_second_call_and_adjacency_untouched(cases, name):
    api = cases.api
    g = cases.graph(name)
    before = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    first = cases.count(g, 0)
    second = cases.count(g, 0)
    assert first[0] == second[0] and (first[1] == second[1]).all()
    after = [g.csr_to_host(dr) for dr in (api.GM_DIR_OUT, api.GM_DIR_IN)]
    for (rp0, ci0, _), (rp1, ci1, _) in zip(before, after):
        assert (rp0 == rp1).all() and (ci0 == ci1).all()


def _flags(cases, g):
    """(duplicates, pieces) of the last call: the first two words of workspace slot GM_WS_TC_FLAG"""
    api = cases.api
    ptr, size, ext = C.c_void_p(), C.c_size_t(), C.c_int()
    assert cases.L.gm_graph_workspace_info(g.h, api._lib.GM_WS_TC_FLAG, C.byref(ptr), C.byref(size), C.byref(ext)) == 0 and ptr.value
    words = np.zeros(2, np.uint32)
    api.copy_from_device(words, ptr.value)
    return int(words[0]), int(words[1])


def test_key_width_follows_the_duplicates(cases):
    for name, duplicates in (("A", 1), ("C", 1), ("Cd", 0), ("B", 0), ("upper", 0)):
        g = cases.graph(name)
        cases.count(g, 0)
        assert _flags(cases, g)[0] == duplicates, name


def test_forms_deal_the_rows_differently_and_reset_brings_the_automatic_form_back(cases):
    b, c = cases.graph("B"), cases.graph("C")
    cases.count(b, 1)
    assert _flags(cases, b)[1] == 0          # B: every list can be staged, the row kernel takes everything
    assert cases.L.gm_reset_options() == 0
    b.triangle_count()
    automatic = _flags(cases, b)[1]
    cases.count(b, 2)
    assert 0 < automatic == _flags(cases, b)[1]  # (the automatic form deals every row to the pieces kernel)
    cases.count(c, 1)
    rows_first = _flags(cases, c)[1]
    cases.count(c, 2)
    # form 1: vertex 1's row alone (its list cannot be staged), 9008 in-edges in pieces of 64; form 2: every row
    assert rows_first == (9008 + 63) // 64 < _flags(cases, c)[1]


def test_refusals(cases):
    import torch
    api = cases.api
    L = cases.L
    nv, s, d, _ = reference("A")
    total = C.c_uint64(77)
    for kw, text in ((dict(directions=api.GM_DIR_OUT), b"both directions"),
                     (dict(layout=api.GM_LAYOUT_NATIVE, row_range=(0, 128)), b"whole graphs")):
        g = api.Graph(nv, s, d, **kw)
        out = torch.full((g.rows,), 7, dtype=torch.int64, device=g.device)
        assert L.gm_run_triangle_count(g.h, out.data_ptr(), C.byref(total), None) == 4  # GM_ERR_UNSUPPORTED
        assert text in L.gm_last_error()
        assert (out == 7).all() and total.value == 77
        with pytest.raises(api._lib.GMError):
            g.triangle_count()

"""Triangle counting without a GPU: the numpy restatement the GPU tests compare with (tests/test_gpu_triangles.py imports it from
here), checked against a plain two-pointer merge and a dense formula; the error convention of gm_run_triangle_count; option
"tc_form"; the symbol in the header, the binding and the library.

Semantics (exact integers): out(v) = the sorted multiset of the destinations of v's edges, duplicates and self-loops kept;
c(u, v) = sum over x of min(multiplicity of x in out(u), in out(v)); triangles[v] = sum over the input edges u -> v of c(u, v).
The restatement encodes a list entry as (dst << 32) | occurrence index: the multiset intersection is then the set intersection
of the pairs.  No oracle program exists for this application."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GM_ERR_INVALID = 1


# ---------------- graphs: the smallest at which each path of the kernels can go wrong -----------------------------------
def graph_a():   # random, vertex 300 isolated: 181 duplicate edges, 25 self-loops -> 64-bit keys
    rng = np.random.default_rng(7); nv, ne = 300, 6000
    return nv, rng.integers(1, nv, ne).astype(np.int32), rng.integers(1, nv, ne).astype(np.int32)


def graph_b():   # list lengths on every boundary of 16 / 64 / 128 / 256, neighbours of very different length intersected
    L = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257); last = len(L); s = []; d = []
    for j, n in enumerate(L, start=1):
        owners = sorted({min(j + 1, last), last} - {j})
        tgt = owners + list(range(20, 20 + n - len(owners)))
        s += [j] * len(tgt); d += tgt
    return 300, np.array(s, np.int32), np.array(d, np.int32)


def graph_c():   # vertex 1: 9008 in-edges (a giant OUT row) and a 6001-entry list (beyond one wave's LDS share); duplicates and loops
    rng = np.random.default_rng(3); nv = 9000
    s = [np.arange(2, nv + 1), np.full(6000, 1), rng.integers(1, nv + 1, 14000), np.full(300, 2)]
    d = [np.full(nv - 1, 1), np.arange(2, 6002), rng.integers(1, nv + 1, 14000), rng.integers(1, 40, 300)]
    return nv, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32)


def dedupe(nv, s, d):   # graph Cd = dedupe(*graph_c()): the same shape on 32-bit keys
    p = np.unique(np.stack([s, d], 1), axis=0); p = p[p[:, 0] != p[:, 1]]
    return nv, p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)


def fixture(name):
    from graphmat_amd import mtx
    nv, s, d, _ = mtx.read_mtx_bin(os.path.join(GOLDEN, name))
    return nv, s, d


GRAPHS = {"A": graph_a, "B": graph_b, "C": graph_c, "Cd": lambda: dedupe(*graph_c()),
          "test": lambda: fixture("test.bin.mtx"), "upper": lambda: fixture("2_10_upper_triangle.bin.mtx")}
#         name: (edges, total)
EXPECTED = {"A": (6000, 8438), "B": (886, 1098), "C": (29299, 32212), "Cd": (29031, 29844), "test": (13, 6), "upper": (15069, 17158)}


# ---------------- the restatement -----------------------------------------------------------------------------------------
def restatement(nv, s, d):
    """triangles int64[nv] (index v - 1): one np.intersect1d of pair-encoded lists per input edge."""
    s = np.asarray(s, np.int64)
    d = np.asarray(d, np.int64)
    order = np.lexsort((d, s))
    ss, dd = s[order], d[order]
    idx = np.arange(len(ss), dtype=np.int64)
    same = np.zeros(len(ss), bool)
    same[1:] = (ss[1:] == ss[:-1]) & (dd[1:] == dd[:-1])
    occurrence = idx - np.maximum.accumulate(np.where(same, 0, idx))
    keys = (dd << 32) | occurrence
    ptr = np.searchsorted(ss, np.arange(1, nv + 2))
    lists = [keys[ptr[v]:ptr[v + 1]] for v in range(nv)]
    tri = np.zeros(nv, np.int64)
    for u, v in zip(s, d):
        tri[v - 1] += len(np.intersect1d(lists[u - 1], lists[v - 1], assume_unique=True))
    return tri


def plain_merge(nv, s, d):
    """The semantics written out: sorted multisets and a two-pointer merge that advances both pointers on an equal pair."""
    out = [[] for _ in range(nv)]
    for u, v in zip(s, d):
        out[u - 1].append(int(v))
    for lst in out:
        lst.sort()
    tri = np.zeros(nv, np.int64)
    for u, v in zip(s, d):
        a, b = out[u - 1], out[v - 1]
        i = j = c = 0
        while i < len(a) and j < len(b):
            if a[i] == b[j]:
                c += 1; i += 1; j += 1
            elif a[i] < b[j]:
                i += 1
            else:
                j += 1
        tri[v - 1] += c
    return tri


_memo = {}


def reference(name):
    """(nv, src, dst, triangles of the restatement), computed once per process and read-only."""
    if name not in _memo:
        nv, s, d = GRAPHS[name]()
        tri = restatement(nv, s, d)
        for a in (s, d, tri):
            a.setflags(write=False)
        _memo[name] = (nv, s, d, tri)
    return _memo[name]


# ---------------- the checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from graphmat_amd import build
    build.build()
    from graphmat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", ["A", "B", "test", "upper"])
def test_restatement_equals_the_plain_merge(name):
    nv, s, d, tri = reference(name)
    assert len(s) == EXPECTED[name][0]
    assert (tri == plain_merge(nv, s, d)).all()
    assert int(tri.sum()) == EXPECTED[name][1]


@pytest.mark.parametrize("name", ["C", "Cd"])
def test_restatement_totals_of_the_large_graphs(name):
    nv, s, d, tri = reference(name)
    assert len(s) == EXPECTED[name][0] and int(tri.sum()) == EXPECTED[name][1]


def test_graph_shapes():
    """What the graphs are there for: duplicates and loops in A and C and none in Cd, B's largest count, C's long lists."""
    nv, s, d, tri = reference("A")
    assert len(s) - len(np.unique(np.stack([s, d], 1), axis=0)) == 181 and int((s == d).sum()) == 25
    assert not (s == 300).any() and not (d == 300).any() and tri[299] == 0
    assert int(reference("B")[3].max()) == 608
    nv, s, d, tri = reference("C")
    assert int((d == 1).sum()) == 9008 and int((s == 1).sum()) == 6001
    nv, s, d, tri = reference("Cd")
    assert len(np.unique(np.stack([s, d], 1), axis=0)) == len(s) and not (s == d).any()


def test_fixture_counts():
    assert reference("test")[3].tolist() == [0, 1, 1, 1, 1, 2, 0, 0]
    nv, s, d, tri = reference("upper")
    assert tri[:10].tolist() == [0, 30, 53, 64, 53, 49, 56, 24, 102, 55]
    # a formula independent of the restatement: on a 0/1 upper-triangular matrix the total is sum((U @ U) * U)
    U = np.zeros((nv, nv), np.int64)
    U[s - 1, d - 1] = 1
    assert int(U.sum()) == len(s) and (s < d).all()
    assert int(((U @ U) * U).sum()) == 17158 == int(tri.sum())


def test_error_convention(lib):
    total = C.c_uint64(77)
    fake = C.c_void_p(16)  # never dereferenced
    assert lib.gm_run_triangle_count(None, fake, C.byref(total), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert lib.gm_run_triangle_count(fake, None, C.byref(total), None) == GM_ERR_INVALID
    assert b"null" in lib.gm_last_error()
    assert total.value == 77


def test_tc_form_option(lib):
    for form in (0, 1, 2):
        assert lib.gm_set_option(b"tc_form", form) == 0
    assert lib.gm_set_option(b"tc_form", 3) == GM_ERR_INVALID and lib.gm_set_option(b"tc_form", -1) == GM_ERR_INVALID
    # (the library has no getter for its options: that the reset brings 0 back is seen where it has an effect, in
    # tests/test_gpu_triangles.py::test_reset_brings_the_automatic_form_back)
    assert lib.gm_reset_options() == 0


def test_symbol_in_header_binding_and_library(lib):
    from graphmat_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphmat_hip.h")).read()
    assert "int gm_run_triangle_count(gm_graph_t* g, int64_t* d_triangles, uint64_t* h_total, gm_stream_t stream);" in header
    assert "gm_run_triangle_count" in _lib.SIGNATURES and hasattr(lib, "gm_run_triangle_count")
    for slot, number in (("GM_WS_TC_KEYS", 19), ("GM_WS_TC_PLAN", 20), ("GM_WS_TC_FLAG", 21)):
        assert getattr(_lib, slot) == number and "#define %s %d\n" % (slot, number) in header
    assert "#define GM_WS_SLOTS 22\n" in header

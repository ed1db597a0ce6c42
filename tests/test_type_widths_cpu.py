"""What tests/test_gpu_type_widths.py relies on, checked without a GPU: the generated graphs have the rows they claim to have,
and the host restatements of TopologicalSort and IncrementalPageRank agree with plainer ones."""
import os

import numpy as np
import pytest

from graphmat_amd.mtx import read_mtx_bin
from tests.support import type_width_graphs as tw


@pytest.fixture(scope="module")
def dag():
    return tw.layered_dag_edges()


@pytest.fixture(scope="module")
def ladder():
    return tw.ladder_edges(weights="hash")


def test_ladder_graph_has_the_stated_rows(ladder):
    nv, s, d, v = ladder
    assert nv == tw.N and 4 * nv < s.size < 5 * nv  # 47 K ladder edges, the ring, about 3n random ones
    assert s.min() >= 1 and s.max() <= nv and d.min() >= 1 and d.max() <= nv
    indeg = np.bincount(d, minlength=nv + 1)
    assert indeg[1:17].tolist() == list(tw.LADDER)
    assert np.unique(s.astype(np.int64) * (1 << 32) + d).size == s.size  # no edge twice: the ids of a row are distinct
    assert (indeg[17:] >= 1).all()  # the ring
    # the giant threshold of such a graph (smallest power of two >= 4096 that leaves at most 1024 rows above it) is 4096
    assert (indeg > 4096).sum() == 4 and indeg[17:].max() <= 64
    assert v.min() == 1 and v.max() == 64 and np.unique(v).size == 64
    # delta = 32 splits the edges into a light and a heavy graph that both keep a giant row
    for part in (v <= 32, v > 32):
        assert np.bincount(d[part], minlength=nv + 1).max() > 4096
    # ... and the same edges again with unit weights (what IncrementalPageRank's oracle multiplies by)
    nv1, s1, d1, v1 = tw.ladder_edges(weights="ones")
    assert (s1 == s).all() and (d1 == d).all() and (v1 == 1).all()


def test_layered_dag_has_the_stated_rows(dag):
    nv, s, d, v = dag
    layer = tw.dag_layers(nv)
    assert nv == tw.N and layer.max() == tw.DAG_LAYERS - 1 and layer[1] == 0
    assert (layer[s] > layer[d]).all()  # acyclic, and no path is longer than the number of layers
    indeg = np.bincount(d, minlength=nv + 1)
    assert indeg[1:11].tolist() == list(tw.DAG_LADDER)
    assert np.unique(s.astype(np.int64) * (1 << 32) + d).size == s.size
    for i, deg in enumerate(tw.DAG_LADDER):  # the sources of a ladder row are spread over all the layers above it
        if deg >= 64:
            assert set(layer[s[d == i + 1]].tolist()) == set(range(tw.DAG_LADDER_LAYER[i] + 1, tw.DAG_LAYERS))
    rest = indeg[11:][layer[11:] < tw.DAG_LAYERS - 1]
    assert 2.5 < rest.mean() <= 3.0 and (indeg[11:][layer[11:] == tw.DAG_LAYERS - 1] == 0).all()
    assert np.bincount(s, minlength=nv + 1)[1:11].sum() > 0  # ladder rows below the top have out-edges: their counts matter downstream


def test_topsort_restatement_equals_a_kahn_pass(golden_dir, dag):
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, "2_10_upper_triangle.bin.mtx"))
    assert (tw.topsort_orders(nv, s, d) == tw.kahn_orders(nv, s, d)).all()
    level = np.zeros(nv + 1, np.int64)  # (the pass of test_reference_topological_sort_app_unchanged: src < dst in this fixture)
    for a, b in sorted(zip(s.tolist(), d.tolist())):
        level[b] = max(level[b], level[a] + 1)
    assert (tw.topsort_orders(nv, s, d) == level).all()
    nv, s, d, v = dag
    layer = tw.dag_layers(nv)
    order = tw.topsort_orders(nv, s, d, layer)
    assert (order == tw.kahn_orders(nv, s, d)).all()
    assert order.max() <= tw.DAG_LAYERS - 1 and order[1] == order.max()  # vertex 1 is among the last to finish
    assert len(set(order[1:11].tolist())) >= 5  # the printed rows do not all say the same
    with pytest.raises(ValueError):
        tw.kahn_orders(3, np.array([1, 2, 3]), np.array([2, 3, 1]))
    with pytest.raises(ValueError):
        tw.topsort_orders(3, np.array([1, 2, 3]), np.array([2, 3, 1]))


def test_incremental_pagerank_restatement_through_the_oracle(golden_dir):
    """the recurrence with the oracle's fp64 multiply equals the plain numpy loop of test_reference_incremental_pagerank_app_unchanged
    on its fixture, bit for bit"""
    from oracle import binding as ob
    ob.build()
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, "test.bin.mtx"))
    pr0, deg0, it0 = tw.incremental_pagerank(nv, s, tw.file_order_spmv(nv, s, d))
    og = ob.OracleGraph(nv, s, d, np.ones(s.size, np.int32), 1)
    pr1, deg1, it1 = tw.incremental_pagerank(nv, s, tw.oracle_spmv(og))
    assert it0 == it1 and (deg0 == deg1).all()
    assert (pr0.view(np.uint64) == pr1.view(np.uint64)).all()
    # the loop of the existing test, as it stands there
    outdeg = np.bincount(s - 1, minlength=nv)
    delta = np.full(nv, 0.3)
    pr = np.full(nv, 0.3)
    active = np.ones(nv, bool)
    iters = 0
    while True:
        msg = np.where(outdeg > 0, delta / np.maximum(outdeg, 1), 0.0)
        y = np.zeros(nv)
        got = np.zeros(nv, bool)
        for a, b in zip(s - 1, d - 1):
            if active[a]:
                y[b] += msg[a]
                got[b] = True
        old = pr.copy()
        for i in np.where(got)[0]:
            if abs(delta[i]) > 1e-8:
                delta[i] = 0.0
            delta[i] += (1.0 - 0.3) * y[i]
            if abs(delta[i]) > 1e-8:
                pr[i] += delta[i]
        active = np.abs(pr - old) > 1e-8
        iters += 1
        if not active.any():
            break
    assert iters == it1 and (pr.view(np.uint64) == pr1.view(np.uint64)).all()


def test_oracle_multiply_folds_a_giant_row_in_native_order():
    """on the ladder graph the bits of a hub's fp64 sum depend on the order of its terms: the oracle's is the ascending native id of the
    source, which a sorted numpy accumulation restates for the rows the applications print"""
    from oracle import binding as ob
    ob.build()
    nv, s, d, v = tw.ladder_edges(weights="ones")
    og = ob.OracleGraph(nv, s, d, v, 1)
    x = 1.0 / (np.arange(nv) % 97 + 1.0) + (np.arange(nv) % 13) * 0.37
    active = np.arange(nv) % 3 != 1
    y, got = tw.oracle_spmv(og)(x, active)
    nat = np.array([ob.vertex_to_native(u, 16, nv) for u in range(1, nv + 1)])
    differs = 0
    for row in range(1, 17):
        srcs = s[d == row]
        srcs = srcs[active[srcs - 1]]
        assert got[row - 1] == (srcs.size > 0)
        terms = x[srcs[np.argsort(nat[srcs - 1], kind="stable")] - 1]
        acc = 0.0
        for i, t in enumerate(terms.tolist()):
            acc = t if i == 0 else acc + t
        assert np.float64(acc).view(np.uint64) == y[row - 1].view(np.uint64), row
        differs += int(np.float64(np.sum(np.sort(terms))).view(np.uint64) != y[row - 1].view(np.uint64))
    assert differs >= 3  # (another order gives other bits on the long rows: the comparison can tell)

"""Message, reduction, vertex-property and edge types that are not four bytes wide, on graphs with every row class.

apps/message_widths.cpp runs nine type shapes (1-, 2-, 3-, 8- and 12-byte messages and reductions, 1- and 24-byte vertex properties,
1- and 8-byte edge values) on a graph with giant rows of two to five pieces, wave rows on both sides of GM_LONG_MID and short rows
on both sides of GM_SHORT_ROW, and compares every vertex byte for byte with a host restatement of run_graph_program -- here as it
stands, with every step kind of the iteration loop forced, on column tiles, under the guided pull and with each ordered giant-row
strategy.  The reference's unchanged TopologicalSort (bool messages), IncrementalPageRank (fp64 sums, 24-byte property) and
DeltaStepping then run at the same scale, with one, two and three ranks.  All comparisons are exact.  Needs an MI355X."""
import os
import re

import numpy as np
import pytest

from tests.support import type_width_graphs as tw
from tests.test_dropin_apps import FORCED_STEPS, OWN_APPS, REF_APPS, _need, _run

pytestmark = pytest.mark.gpu

CASES = ["1 bool->int", "1 bool->int, declared commutative", "2 uchar->uchar", "2 uchar->uchar, declared commutative", "3 ushort->ushort",
         "3 ushort->ushort, declared last", "4 uchar->ull", "5a double->double, all vertices", "5b double->double, active only", "6 float->double",
         "7 3 bytes->3 bytes", "8 12 bytes->12 bytes", "9 int->int over uchar edges"]
DECLARED = {"1 bool->int, declared commutative": 1, "2 uchar->uchar, declared commutative": 1, "3 ushort->ushort, declared last": 2}
ONE = {"GRAPHMAT_NUM_THREADS": "1"}  # the layout parameter of the oracle (else: OMP_NUM_THREADS)


def _widths(env=None):
    return _run(_need(os.path.join(OWN_APPS, "message_widths")), env=env)


def _case_lines(text):
    return [l for l in text.splitlines() if re.match(r"^\d[ab]? .*: \d+ of \d+ vertices differ", l)]


def _sections(text):
    return {name: body for name, body in re.findall(r"^== ([^\n]*)\n(.*?)(?=^== |^reduce strategy of case )", text, flags=re.S | re.M)}


def _steps(section):
    return re.findall(r"^GraphMat\(HIP\):   step: (.*)$", section, flags=re.M)


@pytest.fixture(scope="module")
def plain():
    return _widths()


def test_every_width_equals_the_host_restatement(plain):
    assert "WIDTHS PASS" in plain, plain[-3000:]
    lines = _case_lines(plain)
    assert [l.split(":")[0] for l in lines] == CASES
    for l in lines:
        assert ": 0 of 60000 vertices differ" in l, l
    m = re.search(r"(\d+) giant rows in (\d+) pieces, (\d+) wave rows \((\d+) long\), (\d+) row-blocks", plain)
    assert m and int(m.group(1)) >= 3 and int(m.group(2)) >= 12 and int(m.group(3)) > 0 and int(m.group(4)) > 0 and int(m.group(5)) > 0
    sect = _sections(plain)
    assert sorted(sect) == sorted(CASES)
    for name in CASES:  # the device ran as many iterations as the host restatement (the runs until convergence stop in the same one)
        done = re.findall(r"^Completed (\d+) iterations", sect[name], flags=re.M)
        assert len(done) == 1 and re.search(r"vertices differ from the host's ordered fold after %s iterations$" % done[0], sect[name], flags=re.M), name
    strategies = dict(re.findall(r"^reduce strategy of case (.*): (\d)$", plain, flags=re.M))
    assert strategies == {c: str(DECLARED.get(c, 0)) for c in CASES}  # nothing declared, nothing trusted: the ordered fold


def test_default_options_take_top_down_steps_for_the_declared_programs(plain):
    text = _widths(env={"GRAPHMAT_VERBOSE": "1"})
    assert _case_lines(text) == _case_lines(plain)
    sect = _sections(text)
    assert sorted(sect) == sorted(CASES)
    for name in CASES:
        assert "reduce strategy %d " % DECLARED.get(name, 0) in sect[name], name
        assert (_steps(sect[name]) != []) == (name in DECLARED), name  # (only programs that may take top-down steps print their steps)
    last = _steps(sect["3 ushort->ushort, declared last"])
    assert "bits push" in last or "list push" in last, last
    assert "messages are evaluated on demand" in sect["3 ushort->ushort, declared last"]


@pytest.mark.parametrize("probe", [False, True])
@pytest.mark.parametrize("regime", sorted(FORCED_STEPS))
def test_forced_step_regimes(plain, regime, probe):
    """every step kind of the loop with 1- and 2-byte messages and reductions: k_push_bid / k_push_combine / k_push_finish / k_push_resolve,
    the padded (id, message) entries, the messages of listed vertices (k_send_list)"""
    env = {"GRAPHMAT_OPTIONS": FORCED_STEPS[regime], "GRAPHMAT_VERBOSE": "1"}
    if probe:
        env["GRAPHMAT_TRUST_PROBE"] = "1"
    text = _widths(env=env)
    assert "ignoring" not in text, text[-1500:]
    assert _case_lines(text) == _case_lines(plain)
    sect = _sections(text)
    for name, strategy in DECLARED.items():
        steps = _steps(sect[name])
        assert "reduce strategy %d " % strategy in sect[name] and steps != []
        if regime == "pull only":
            assert set(steps) == {"pull"}, (name, steps)
        elif regime == "list whenever possible":
            assert "list push" in steps and set(steps) <= {"list push", "pull"}, (name, steps)  # (pull: an active set that owns every edge)
        elif strategy == 2:
            assert "pull with dense push" in steps, (name, steps)
        else:  # (no dense push for a commutative fold: such steps are pulls)
            assert set(steps) <= {"pull", "list push"}, (name, steps)
    if probe:  # what the probe makes of the undeclared programs: wrapping +, min, a = b are recognised, the others keep the ordered fold
        want = {"1 bool->int": 1, "2 uchar->uchar": 1, "3 ushort->ushort": 2, "4 uchar->ull": 1, "9 int->int over uchar edges": 1}
        for name in CASES:
            if name not in DECLARED:
                assert "reduce strategy %d " % want.get(name, 0) in sect[name], name
        if regime == "list whenever possible":
            for name in ("1 bool->int", "2 uchar->uchar", "3 ushort->ushort"):
                assert "list push" in _steps(sect[name]), name


@pytest.mark.parametrize("env,evidence", [
    ({"GRAPHMAT_COL_TILES": "3"}, "tiles"),
    ({"GRAPHMAT_OPTIONS": "guided_pull=2"}, "guided"),
    ({"GRAPHMAT_OPTIONS": "ordered_giant_two_pass=0"}, None),
    ({"GRAPHMAT_OPTIONS": "ordered_giant_two_pass=1"}, None),
    ({"GRAPHMAT_OPTIONS": "sweep_form=64", "GRAPHMAT_COL_TILES": "3"}, "tiles"),
], ids=["tiles", "guided-pull", "giant-one-wave", "giant-two-pass", "tiles-sparse-sweep"])
def test_tiles_giant_row_strategies_and_guided_pull(plain, env, evidence):
    """the fallbacks of the sweep, the column tiles and the giant-row strategies for types they do not take: same bytes on every path"""
    text = _widths(env=dict(env, GRAPHMAT_VERBOSE="1"))
    assert "ignoring" not in text, text[-1500:]
    assert _case_lines(text) == _case_lines(plain)
    sect = _sections(text)
    if evidence == "tiles":
        # every graph is cut into column tiles; the sweep's structure exists only where it can carry the edge values (4 bytes: the int and
        # float graphs) -- the unsigned char and double graphs have none, so case 9 (4-byte messages and sums, which the sweep would take)
        # must not go through it.  No case has 4-byte messages AND sums over 4-byte values: all of them take the tiles or the plain passes
        four_byte_values = [c for c in CASES if c[0] in "134678"]
        for name in CASES:
            m = re.search(r"^   graph: ([2-9]) column tiles, sweep of (\d+) rows \(value bytes (\d)\)$", sect[name], flags=re.M)
            assert m, (name, sect[name][:300])
            assert (int(m.group(2)) > 0, int(m.group(3))) == ((True, 4) if name in four_byte_values else (False, 0)), (name, m.group(0))
            assert "through the sweep" not in sect[name] and "ride the sweep" not in sect[name], name
    if evidence == "guided":  # the undeclared ACTIVE_ONLY programs running until convergence
        for name in ("1 bool->int", "2 uchar->uchar", "3 ushort->ushort"):
            assert "guided pull: iterations whose active set" in sect[name] and "   guided pull: " in sect[name], name


# ---- the reference's unchanged applications at the same scale -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dag(tmp_path_factory):
    from graphmat_amd.mtx import write_mtx_bin
    nv, s, d, v = tw.layered_dag_edges()
    path = str(tmp_path_factory.mktemp("widths") / "layered_dag.bin.mtx")
    write_mtx_bin(path, nv, s, d, v)
    return path, tw.topsort_orders(nv, s, d, tw.dag_layers(nv))


@pytest.fixture(scope="module")
def ladder(tmp_path_factory):
    from graphmat_amd.mtx import write_mtx_bin
    nv, s, d, v = tw.ladder_edges(weights="hash")
    where = tmp_path_factory.mktemp("widths")
    hashed, ones = str(where / "ladder_hash.bin.mtx"), str(where / "ladder_ones.bin.mtx")
    write_mtx_bin(hashed, nv, s, d, v)
    write_mtx_bin(ones, nv, s, d, np.ones(s.size, np.int32))
    return nv, s, d, v, hashed, ones


TOPSORT_LINES = r"^(Top Sort order \d+ : \d+|Completed \d+ iterations.*|Topological Sort not possible.*)$"


def _topsort_rows(text):
    return {int(a): int(b) for a, b in re.findall(r"^Top Sort order (\d+) : (\d+)$", text, flags=re.M)}


def test_reference_topological_sort_on_a_layered_dag(dag):
    """bool messages counted into 4-byte sums on giant, wave and short rows: one miscounted decrement anywhere leaves a vertex without an
    order and the application reports a cycle"""
    path, order = dag
    text = _run(_need(os.path.join(REF_APPS, "TopologicalSort")), path, env=ONE)
    assert "Graph has cycles" not in text, text[-1500:]
    assert _topsort_rows(text) == {v: int(order[v]) for v in range(1, 11)}
    assert "Completed %d iterations" % (int(order.max()) + 1) in text


@pytest.mark.parametrize("regime", sorted(FORCED_STEPS))
def test_reference_topological_sort_under_forced_steps(dag, regime):
    path, order = dag
    exe = _need(os.path.join(REF_APPS, "TopologicalSort"))
    base = [l for l in _run(exe, path, env=ONE).splitlines() if re.match(TOPSORT_LINES, l)]
    text = _run(exe, path, env=dict(ONE, GRAPHMAT_OPTIONS=FORCED_STEPS[regime], GRAPHMAT_VERBOSE="1", GRAPHMAT_TRUST_PROBE="1"))
    assert "ignoring" not in text and "Graph has cycles" not in text, text[-1500:]
    assert [l for l in text.splitlines() if re.match(TOPSORT_LINES, l)] == base
    assert _topsort_rows(text) == {v: int(order[v]) for v in range(1, 11)}
    assert "reduce strategy 1" in text  # (the wrapping + of both programs is recognised: the top-down steps are open to them)


def _pagerank_rows(text):
    return {int(a): (int(b), c) for a, b, c in re.findall(r"^(\d+) : (\d+) ([0-9.]+)$", text, flags=re.M)}


def _expected_pagerank(ladder, ref_threads):
    from oracle import binding as ob
    ob.build()
    nv, s, d, v, hashed, ones = ladder
    og = ob.OracleGraph(nv, s, d, np.ones(s.size, np.int32), ref_threads)
    pr, outdeg, iters = tw.incremental_pagerank(nv, s, tw.oracle_spmv(og))
    return {i + 1: (int(outdeg[i]), "%f" % pr[i]) for i in range(25)}, iters


def test_reference_incremental_pagerank_on_the_ladder_graph(ladder):
    """fp64 messages and sums, a 24-byte vertex property, a sparse message vector: the hubs' sums carry the bits of the reference's order"""
    want, iters = _expected_pagerank(ladder, 1)
    text = _run(_need(os.path.join(REF_APPS, "IncrementalPageRank")), ladder[5], env=ONE)
    assert _pagerank_rows(text) == want
    assert "Completed %d iterations" % iters in text


def _distance_rows(text):
    return {int(a): b for a, b in re.findall(r"^(\d+) : distance = (\d+|INF)$", text, flags=re.M)}


@pytest.mark.parametrize("delta", [32, 1000])
def test_reference_delta_stepping_on_the_ladder_graph(ladder, delta):
    """two graphs (light and heavy edges) that share one vertex-property vector, each with giant rows; delta = 1000: the heavy graph is empty"""
    from oracle import binding as ob
    ob.build()
    nv, s, d, v, hashed, ones = ladder
    for part in (v <= 32, v > 32):
        assert np.bincount(d[part], minlength=nv + 1).max() > 4096
    source = int(s[d == 1][0])  # an in-neighbour of the largest hub
    dist, _ = ob.OracleGraph(nv, s, d, v, 1).sssp(source)
    text = _run(_need(os.path.join(REF_APPS, "DeltaStepping")), hashed, delta, source, env=ONE)
    assert "Reachable vertices = %d " % int((dist != 0xFFFFFFFF).sum()) in text, text[-1500:]
    assert _distance_rows(text) == {i + 1: ("INF" if dist[i] == 0xFFFFFFFF else str(int(dist[i]))) for i in range(25)}


@pytest.mark.parametrize("nranks", [2, 3])
def test_reference_topological_sort_one_process_per_shard(dag, tmp_path, monkeypatch, nranks):
    """the first exchange of a message vector with 1-byte elements"""
    from tests.test_gpu_multirank_apps import _launch
    monkeypatch.setenv("GRAPHMAT_NUM_THREADS", "1")
    path, order = dag
    outs = _launch(_need(os.path.join(REF_APPS, "TopologicalSort")), [path], nranks, tmp_path, "shm")
    seen = {}
    for text in outs:
        assert "Graph has cycles" not in text, text[-1500:]
        for vid, o in _topsort_rows(text).items():
            assert vid not in seen, "vertex %d printed by two ranks" % vid
            seen[vid] = o
    assert seen == {v: int(order[v]) for v in range(1, 11)}


@pytest.mark.parametrize("nranks", [2, 3])
def test_reference_incremental_pagerank_one_process_per_shard(ladder, tmp_path, monkeypatch, nranks):
    """the first sparse (id, message) exchange with 8-byte messages; the fold order depends on the rank count through the id permutation"""
    from tests.test_gpu_multirank_apps import _launch
    monkeypatch.setenv("GRAPHMAT_NUM_THREADS", "1")
    want, iters = _expected_pagerank(ladder, nranks)
    outs = _launch(_need(os.path.join(REF_APPS, "IncrementalPageRank")), [ladder[5]], nranks, tmp_path, "shm")
    seen = {}
    for text in outs:
        assert "Completed %d iterations" % iters in text, text[-1500:]
        for vid, row in _pagerank_rows(text).items():
            assert vid not in seen, "vertex %d printed by two ranks" % vid
            seen[vid] = row
    assert seen == want

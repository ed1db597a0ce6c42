"""Every step kind of the iteration loop (engine.hpp: run_loop) against the oracle, bit for bit.

An ACTIVE_ONLY program that runs until convergence (BFS, SSSP) takes, per iteration, a pull, a pull whose multiply is a
top-down bid pass resolved over all vertices ("dense push"), a list-based top-down step or a top-down step straight from
the active bitmap ("bits push"), chosen from the size of the active set and three engine options.  With the default
options small graphs only ever see one mix of them.  Here the options are set so that graphs of a few hundred thousand
edges reach every branch, and every run is checked three ways:

  * the result equals oracle.binding.OracleGraph's: BFS depth, parent and iteration count, SSSP dist and iteration count.
    No tolerances;
  * the steps the run took (notes 5 and 6 of the graph, graphmat_hip.h) equal the rule of run_loop restated in numpy and
    fed with the active sets the ORACLE's result implies -- which tests the host's choice and the frontier statistics
    that k_frontier_stats / k_apply / k_push_finish count on the device together;
  * (without a GPU) that prediction contains the step kinds the case exists for, so a case that can no longer reach its
    kernel fails instead of passing vacuously.

All regimes of a graph run on ONE Graph object, in a fixed and then in the reversed order, BFS and SSSP interleaved, so
that whatever one run leaves in the graph's scratch (the bid slots, the lists, the row-filter bits) is what the next finds.

The "mixed" regime of the issue comes in two forms.  With push_edge_permille=1000 a level is pushed whenever it owns fewer
edges than the graph has and at most 65536 vertices, which on these graphs is every level: such a run mixes list steps
with dense-push steps (BFS) or pulls (SSSP, which has no dense push), two kinds.  The third kind in one BFS run comes from
the second form, push_edge_permille between the shares of two levels: the levels above it are pulls.

Out of scope here:
  * the k_frontier_list rebuild: a pull level with more than 4 Mi frontier edges followed by a small active set
    (build_list false in step_pull).  The bound is a constant, not an option; it stays covered only by the RMAT-22 / 26 tests;
  * the overflow of the sweep's bin for short rows above 64 edges: a separate change.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from graphmat_amd import generators as gen

MAXD = 0xFFFFFFFF
CAP = 65536  # kernels.hpp: kSparseListCap
PULL, LIST, BITS, DENSE = 0, 1, 2, 3
KIND_NAMES = ("pull", "list", "bits", "dense-push")
DEFAULTS = {"push_edge_permille": 50, "bits_step_edges": 2 << 20, "sparse_step_edges": 1 << 20, "debug_flags": 0}


# ---------------- the predictor: run_loop's rule in plain numpy ------------------------------------------------------------
def predict_kinds(stats, nnz, opts, reduce_last):
    """stats: (vertices, out-edges, max out-degree) of every iteration's active set -> the step kind of every iteration."""
    o = dict(DEFAULTS, **opts)
    can_push = not (o["debug_flags"] & 32)
    kinds = []
    for v, e, m in stats:
        push = can_push and 0 < v <= CAP and e * 1000 < nnz * o["push_edge_permille"]
        sparse = push and e <= o["sparse_step_edges"]
        dense = push and not sparse and reduce_last
        bits = can_push and not push and reduce_last and v > CAP and e <= o["bits_step_edges"] and m <= 64
        kinds.append(BITS if bits else LIST if sparse else DENSE if dense else PULL)
    return kinds


def expected_notes(kinds):
    n5 = 0
    for k, shift in ((PULL, 0), (LIST, 16), (BITS, 32), (DENSE, 48)):
        n5 |= min(kinds.count(k), 0xFFFF) << shift
    n6 = 0
    for i, k in enumerate(kinds[:32]):
        n6 |= k << (2 * i)
    return n5, n6


def _set_stats(active, outdeg):
    deg = outdeg[active]
    return int(deg.size), int(deg.sum()), int(deg.max()) if deg.size else 0


def bfs_level_stats(depth, iterations, outdeg):
    """level k of the oracle's depths is the active set of iteration k"""
    return [_set_stats(np.nonzero(depth == k)[0], outdeg) for k in range(iterations)]


def sssp_rounds(nv, s, d, w, source):
    """The synchronous iteration: every round relaxes the out-edges of the vertices whose distance changed in the round
    before, all from the distances of before the round.  Returns (dist uint32, stats of every round's active set)."""
    outdeg = np.bincount(s - 1, minlength=nv)
    dist = np.full(nv, MAXD, np.int64)
    dist[source - 1] = 0
    active = np.zeros(nv, bool)
    active[source - 1] = True
    stats = []
    while True:
        stats.append(_set_stats(np.nonzero(active)[0], outdeg))
        m = active[s - 1]
        new = dist.copy()
        np.minimum.at(new, d[m] - 1, dist[s[m] - 1] + w[m])
        active = new != dist
        dist = new
        if not active.any():
            break
    assert dist.max() <= MAXD
    return dist.astype(np.uint32), stats


# ---------------- regimes ----------------------------------------------------------------------------------------------------
def _share_permille(es, nnz):
    """a push_edge_permille between the shares of two levels: the largest p for which some level is still above it
    (a pull) while the next smaller level is below it (pushed); None when the levels leave no integer in between"""
    es = sorted(set(es), reverse=True)
    for hi, lo in zip(es[:-1], es[1:]):
        p = hi * 1000 // nnz  # the largest p with nnz * p <= hi * 1000: the level `hi` is not pushed
        if 1 <= p <= 1000 and lo * 1000 < nnz * p:
            return int(p)
    return None


def regime_options(name, stats, nnz):
    es = [e for _, e, _ in stats]
    if name == "default":
        return {}
    if name == "pull only":
        return {"push_edge_permille": 0}
    if name == "no top-down":
        return {"debug_flags": 32}
    if name == "no top-down, no lazy send":
        return {"debug_flags": 32 | 256}
    if name == "list":
        return {"push_edge_permille": 1000, "sparse_step_edges": 0x7FFFFFFF}
    if name == "dense push":
        return {"push_edge_permille": 1000, "sparse_step_edges": 0}
    if name == "mixed":
        return {"push_edge_permille": 1000, "sparse_step_edges": int(np.median(es))}
    if name == "mixed, pull above a share":
        p = _share_permille(es, nnz)
        return {"push_edge_permille": 1000 if p is None else p, "sparse_step_edges": int(np.median(es))}
    if name == "bits off":
        return {"bits_step_edges": 0}
    if name == "push":
        return {"push_edge_permille": 1000}
    if name == "push, bits off":
        return {"push_edge_permille": 1000, "bits_step_edges": 0}
    raise KeyError(name)


ALL_REGIMES = ("default", "pull only", "no top-down", "no top-down, no lazy send", "list", "dense push", "mixed",
               "mixed, pull above a share", "bits off")


# ---------------- graphs -------------------------------------------------------------------------------------------------------
def native_index(nv, nparts):
    """native id (0-based) of vertex v+1: the permutation of include/Graph.h"""
    v = np.arange(nv, dtype=np.int64)
    h = nv // nparts
    return np.where(v >= h * nparts, v, (v // nparts) + (v % nparts) * h)


def _layered(width, special_degree=0, cross=500):
    """source -> `width` middle vertices -> one leaf each (test_gpu_parity.py: test_bfs_active_set_sizes_around_the_top_down_limits);
    `cross` random further middle -> leaf edges, or one middle vertex with exactly `special_degree` out-edges"""
    rng = np.random.default_rng(width)
    mid = np.arange(2, 2 + width, dtype=np.int32)
    leaf = mid + width
    if special_degree:
        sp = mid[width // 3]
        extra_s = np.full(special_degree - 1, sp, np.int32)
        extra_d = rng.choice(leaf, special_degree - 1).astype(np.int32)  # (duplicates among them count as edges)
    else:
        extra_s = rng.choice(mid, cross).astype(np.int32)
        extra_d = rng.choice(leaf, cross).astype(np.int32)
    s = np.concatenate([np.full(width, 1, np.int32), mid, extra_s])
    d = np.concatenate([mid, leaf, extra_d])
    return 1 + 2 * width, s, d, None


def _piece_boundaries(nparts):
    """source -> three hubs of out-degree exactly 1024, 1025 and 4097 (one, two and five 1024-edge pieces; the last piece of two
    of them holds a single edge) whose destinations overlap heavily, and four vertices without out-edges that sit between the
    hubs in native order, which is the device order of the native layout.  The parents of the destinations are decided by
    atomicMax over pieces of different sources."""
    nv = 8192 + 5
    rng = np.random.default_rng(1024)
    inv = np.argsort(native_index(nv, nparts))  # inv[native id] = vertex - 1
    lvl1 = (inv[100:107] + 1).astype(np.int32)  # seven vertices with consecutive native ids
    assert 1 not in lvl1
    hubs, plain = lvl1[[0, 2, 5]], lvl1[[1, 3, 4, 6]]
    rest = np.setdiff1d(np.arange(2, nv + 1, dtype=np.int32), lvl1)
    pool, tail = rest[:4097], rest[4097:4097 + 50]
    s = [np.full(7, 1, np.int32)]
    d = [lvl1]
    for hub, deg in zip(hubs, (1024, 1025, 4097)):
        s.append(np.full(deg, hub, np.int32))
        d.append(rng.permutation(pool)[:deg] if deg == 4097 else rng.choice(pool, deg, replace=True).astype(np.int32))
    s.append(pool[:50])  # a short further level, so that the hubs' level does not own (almost) every edge
    d.append(tail)
    s, d = np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32)
    outdeg = np.bincount(s - 1, minlength=nv)
    assert sorted(outdeg[hubs - 1].tolist()) == [1024, 1025, 4097] and (outdeg[plain - 1] == 0).all()
    return nv, s, d, None


def _sssp_collisions():
    """the layered weighted graph of test_gpu_parity.py: test_sssp_small_active_sets_with_colliding_relaxations (duplicate edges with
    different weights), plus per layer one edge between two of its vertices and one edge back to the layer above: vertices that
    are active in a step are destinations of the same step, and vertices change more than once"""
    rng = np.random.default_rng(42)
    layers = [np.array([1])] + [np.arange(a, b) for a, b in ((2, 52), (52, 252), (252, 1252), (1252, 1300))]
    s, d = [], []
    for up, down in zip(layers[:-1], layers[1:]):
        for v in down:
            for u in rng.choice(up, size=min(len(up), 6), replace=True):  # duplicates on purpose
                s.append(int(u)); d.append(int(v))
    w = rng.integers(1, 100, len(s)).tolist()
    for up, down in zip(layers[:-1], layers[1:]):
        a, b = (int(x) for x in rng.choice(down, 2, replace=False))
        s.append(a); d.append(b); w.append(1)                       # inside the layer
        s.append(b); d.append(int(rng.choice(up))); w.append(1)     # back to the layer above
    return 1400, np.array(s, np.int32), np.array(d, np.int32), np.array(w, np.int32)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(nv, src, dst, val) of a named case; arrays are shared between the tests and never written"""
    kind, _, arg = name.partition(":")
    if kind == "rmat":
        scale = 14
        while True:
            nv, s, d, w = gen.rmat_edges(scale, 16, seed=14, weights="hash")
            if np.bincount(s - 1, minlength=nv).max() >= 2049:  # at least three 1024-edge pieces
                break
            scale += 1
        g = (nv, s, d, w)
    elif kind == "pieces":
        g = _piece_boundaries(int(arg))
    elif kind == "capacity":
        g = _layered(int(arg))
    elif kind == "degree":
        g = _layered(70000, special_degree=int(arg))
    elif kind == "collisions":
        g = _sssp_collisions()
    else:
        raise KeyError(name)
    for a in g[1:]:
        if a is not None:
            a.setflags(write=False)
    return g


def rmat_sources():
    nv, s, d, _ = graph("rmat")
    outdeg, indeg = np.bincount(s - 1, minlength=nv), np.bincount(d - 1, minlength=nv)
    hub = int(outdeg.argmax()) + 1
    assert outdeg[hub - 1] >= 2049
    sink = int(np.nonzero((outdeg == 0) & (indeg > 0))[0][0]) + 1
    isolated = int(np.nonzero((outdeg == 0) & (indeg == 0))[0][0]) + 1
    ordinary = int(s[len(s) // 2])
    out = {"vertex 1": 1, "hub": hub, "sink": sink, "isolated": isolated, "ordinary": ordinary}
    if hub == 1:  # RMAT without id scrambling: vertex 1 is the hub itself -- one run for both
        del out["hub"]
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, threads):
    from oracle import binding as ob
    nv, s, d, w = graph(name)
    return ob.OracleGraph(nv, s, d, w, ref_threads=threads)


@functools.lru_cache(maxsize=None)
def oracle_bfs(name, threads, source):
    depth, parent, it, _ = oracle(name, threads).bfs(source)
    return depth, parent, it


@functools.lru_cache(maxsize=None)
def oracle_sssp(name, threads, source):
    return oracle(name, threads).sssp(source)


@functools.lru_cache(maxsize=None)
def active_sets(name, prog, source):
    """(vertices, out-edges, max out-degree) of every iteration's active set, from the oracle's result"""
    nv, s, d, w = graph(name)
    outdeg = np.bincount(s - 1, minlength=nv)
    if prog == "bfs":
        depth, _, it = oracle_bfs(name, 1, source)
        assert it == int(depth[depth != MAXD].max()) + 1
        return tuple(bfs_level_stats(depth, it, outdeg))
    dist, stats = sssp_rounds(nv, s, d, w, source)
    odist, oit = oracle_sssp(name, 1, source)
    assert np.array_equal(dist, odist) and len(stats) == oit, "the numpy restatement of SSSP is not the oracle's iteration"
    return tuple(stats)


class Run:
    """one program run of a case: what to set, what the oracle says, which steps the loop must take"""

    def __init__(self, name, prog, source, regime, must=None):
        self.name, self.prog, self.source, self.regime, self.must = name, prog, source, regime, must
        self.stats = active_sets(name, prog, source)
        self.nnz = len(graph(name)[1])
        self.opts = regime_options(regime, self.stats, self.nnz)
        self.kinds = predict_kinds(self.stats, self.nnz, self.opts, reduce_last=(prog == "bfs"))

    def __repr__(self):
        return "%s %s from %d under '%s' %r: %s" % (self.name, self.prog, self.source, self.regime, self.opts,
                                                    " ".join(KIND_NAMES[k] for k in self.kinds))


@functools.lru_cache(maxsize=None)
def plan(case):
    """the runs of a case, in their fixed order"""
    runs = []
    if case == "rmat":
        real = ("vertex 1", "hub", "ordinary")
        for regime in ALL_REGIMES:
            for label, src in rmat_sources().items():
                for prog in ("bfs", "sssp"):
                    must = None
                    if label in real:
                        if regime == "list":
                            must = "list"
                        elif regime == "dense push" and prog == "bfs":
                            must = "dense"
                        elif regime == "mixed":
                            must = "list+dense" if prog == "bfs" else "list+pull"
                        elif regime == "mixed, pull above a share":
                            must = "three kinds" if prog == "bfs" else "list+pull"
                    elif regime == "default":
                        must = "one empty iteration"
                    runs.append(Run("rmat", prog, src, regime, must))
    elif case.startswith("pieces:"):
        for regime, must in (("list", "list hubs"), ("dense push", "dense"), ("default", None), ("mixed", None)):
            runs.append(Run(case, "bfs", 1, regime, must))
    elif case.startswith("capacity:"):
        over = int(case.split(":")[1]) > CAP
        runs.append(Run(case, "bfs", 1, "push", "list then bits" if over else "list then list"))
        runs.append(Run(case, "bfs", 1, "push, bits off", "list then pull" if over else "list then list"))
        runs.append(Run(case, "bfs", 1, "default", None))
    elif case.startswith("degree:"):
        flip = "list then bits" if int(case.split(":")[1]) <= 64 else "list then pull"
        runs.append(Run(case, "bfs", 1, "push", flip))
        runs.append(Run(case, "bfs", 1, "default", flip.replace("list then", "pull then")))
    elif case == "collisions":
        for regime, must in (("pull only", "all pull"), ("list", "list"), ("mixed", "list+pull")):
            runs.append(Run(case, "sssp", 1, regime, must))
    else:
        raise KeyError(case)
    return tuple(runs)


CASES = ("rmat", "pieces:16", "pieces:48", "capacity:65536", "capacity:65537", "capacity:70000", "degree:64", "degree:65", "collisions")


# ---------------- the reachability guard (no GPU) ----------------------------------------------------------------------------
def _reaches(run):
    k, st = run.kinds, run.stats
    if run.must is None:
        return True
    if run.must == "list":
        return LIST in k
    if run.must == "list hubs":  # the hubs' level itself: seven listed sources, the piece counts 1, 2 and 5 among zeros
        return st[1] == (7, 1024 + 1025 + 4097, 4097) and k[0] == LIST and k[1] == LIST
    if run.must == "dense":
        return DENSE in k and not any(kind == LIST and e > 0 for kind, (_, e, _) in zip(k, st))
    if run.must == "list+dense":
        return LIST in k and DENSE in k
    if run.must == "list+pull":
        return LIST in k and PULL in k
    if run.must == "three kinds":
        return len(set(k)) >= 3
    if run.must == "one empty iteration":
        return len(k) == 1 and st[0] == (1, 0, 0)
    if run.must == "all pull":
        return set(k) == {PULL}
    first, then, second = run.must.split()  # "<kind> then <kind>": the first two iterations
    assert then == "then"
    return (k[0], k[1]) == (KIND_NAMES.index(first), KIND_NAMES.index(second))


@pytest.mark.parametrize("case", CASES)
def test_every_case_reaches_the_steps_it_exists_for(case):
    """The predictor fed with the oracle's result yields the kinds each graph x regime was written for.  (For SSSP this also
    checks that the numpy restatement of the iteration is the oracle's: same distances, same number of rounds.)"""
    runs = plan(case)
    assert runs
    for run in runs:
        assert len(run.kinds) == len(run.stats) >= 1
        assert _reaches(run), "%r does not reach '%s'; active sets %r" % (run, run.must, run.stats)
    if case == "rmat":
        src = rmat_sources()
        nv, s, d, w = graph("rmat")
        outdeg = np.bincount(s - 1, minlength=nv)
        assert outdeg[src.get("hub", 1) - 1] == outdeg.max() >= 2049 and outdeg[src["sink"] - 1] == 0 and outdeg[src["isolated"] - 1] == 0
        assert plan("rmat")[0].stats[0] == (1, int(outdeg.max()), int(outdeg.max()))  # the first run starts from the hub
        assert len({r.regime for r in runs}) == len(ALL_REGIMES) and len(runs) == len(ALL_REGIMES) * len(src) * 2
    if case.startswith("capacity:"):
        width = int(case.split(":")[1])
        assert runs[0].stats[1][0] == width  # level 1's k_push_finish lists exactly `width` changed vertices
    if case.startswith("degree:"):
        assert runs[0].stats[1][2] == int(case.split(":")[1]) and runs[0].stats[1][0] == 70000


def test_predictor_rule_on_hand_made_active_sets():
    """the rule itself, at its thresholds (independent of any graph)"""
    nnz = 1000000
    assert predict_kinds([(1, 49999, 9), (1, 50000, 9)], nnz, {}, True) == [LIST, PULL]  # strictly below 50 permille
    assert predict_kinds([(CAP, 10, 1), (CAP + 1, 10, 1)], nnz, {}, True) == [LIST, BITS]
    assert predict_kinds([(CAP + 1, 10, 64), (CAP + 1, 10, 65)], nnz, {}, True) == [BITS, PULL]
    assert predict_kinds([(CAP + 1, 10, 1)], nnz, {}, False) == [PULL]  # bids need an a=b program
    assert predict_kinds([(5, 11, 3), (5, 10, 3), (5, 0, 0)], nnz, {"sparse_step_edges": 10}, True) == [DENSE, LIST, LIST]
    assert predict_kinds([(5, 11, 3), (5, 10, 3)], nnz, {"sparse_step_edges": 10}, False) == [PULL, LIST]
    assert predict_kinds([(0, 0, 0)], nnz, {}, True) == [PULL]
    assert predict_kinds([(5, 10, 3)], nnz, {"debug_flags": 32}, True) == [PULL]
    assert predict_kinds([(CAP + 1, 1, 1), (CAP + 1, 0, 0)], nnz, {"bits_step_edges": 0}, True) == [PULL, BITS]
    assert expected_notes([PULL, LIST, LIST, BITS, DENSE]) == (1 | 2 << 16 | 1 << 32 | 1 << 48, 0b11_10_01_01_00)
    assert expected_notes([DENSE] * 40)[1] == (1 << 64) - 1 and expected_notes([LIST] * 70000)[0] == 0xFFFF << 16


# ---------------- the GPU runs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return api


def _notes(api, g):
    L = api._lib.lib()
    out = []
    for slot in (5, 6):
        v = C.c_int64(0)
        assert L.gm_graph_note_get(g.h, slot, C.byref(v)) == 0, "note %d was never set" % slot
        out.append(v.value & 0xFFFFFFFFFFFFFFFF)
    return tuple(out)


def _kinds_of_notes(n5, n6, iterations):
    return "%s; counts pull %d list %d bits %d dense-push %d" % (
        " ".join(KIND_NAMES[(n6 >> (2 * i)) & 3] for i in range(min(iterations, 32))), n5 & 0xFFFF, (n5 >> 16) & 0xFFFF,
        (n5 >> 32) & 0xFFFF, (n5 >> 48) & 0xFFFF)


def _check(api, g, run, threads):
    L = api._lib.lib()
    L.gm_reset_options()
    for key, value in run.opts.items():
        api._lib.check(L.gm_set_option(key.encode(), int(value)))
    if run.prog == "bfs":
        depth, parent, it = g.bfs(run.source)
        od, op, oit = oracle_bfs(run.name, threads, run.source)
        assert it == oit, "%r: %d iterations, the oracle %d" % (run, it, oit)
        assert np.array_equal(depth, od), "%r: %d depths differ" % (run, int((depth != od).sum()))
        assert np.array_equal(parent, op), "%r: %d parents differ" % (run, int((parent != op).sum()))
    else:
        dist, it = g.sssp(run.source)
        odist, oit = oracle_sssp(run.name, threads, run.source)
        assert it == oit, "%r: %d iterations, the oracle %d" % (run, it, oit)
        assert np.array_equal(dist, odist), "%r: %d distances differ" % (run, int((dist != odist).sum()))
    n5, n6 = _notes(api, g)
    assert (n5, n6) == expected_notes(run.kinds), "%r: the run took %s" % (run, _kinds_of_notes(n5, n6, it))


def _run_case(api, case, threads, layout):
    nv, s, d, w = graph(plan(case)[0].name)
    g = api.Graph(nv, s, d, w, ref_threads=threads, layout=layout)
    try:
        assert g.csr(api.GM_DIR_OUT).nnz == len(s)
        runs = plan(case)
        for order in (runs, runs[::-1]):
            for run in order:
                _check(api, g, run, threads)
    finally:
        api._lib.lib().gm_reset_options()
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads,layout", [(1, 1), (3, 0)])
def test_rmat_every_regime_bfs_and_sssp(env, threads, layout):
    """RMAT scale 14 with hashed weights; sources: vertex 1, the vertex of largest out-degree (at least three 1024-edge pieces; in this
    generator vertex 1 itself), an ordinary vertex, one with in-edges only, an isolated one, BFS and SSSP under every regime, forwards and backwards on one Graph."""
    _run_case(env, "rmat", threads, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("threads,layout", [(1, 0), (3, 0), (1, 1)])
def test_bfs_hubs_at_the_piece_boundaries(env, threads, layout):
    """out-degrees 1024, 1025 and 4097 with overlapping destinations and listed vertices without out-edges between them: the
    parents are decided by atomicMax over pieces of different sources (k_push_bid with and without the touched list)"""
    _run_case(env, "pieces:%d" % (16 * threads), threads, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [65536, 65537, 70000])
def test_bfs_list_push_lists_up_to_and_over_the_capacity(env, width):
    """level 1 is a list push from one source of `width` edges whose k_push_finish lists exactly, one more than and well over
    kSparseListCap changed vertices; the next level is a list step again (exactly at the capacity) or falls to the bits push,
    or to a pull with bits_step_edges=0"""
    for threads, layout in ((1, 1), (2, 0)):
        _run_case(env, "capacity:%d" % width, threads, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [64, 65])
def test_bfs_bits_push_degree_boundary(env, degree):
    """70000 middle vertices of out-degree 1 and one of out-degree 64 (bits push) or 65 (pull): the oracle's result both times"""
    _run_case(env, "degree:%d" % degree, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 3])
def test_sssp_colliding_relaxations_pull_list_and_mixed(env, threads):
    """many sources relax the same destination in one step, duplicate edges with different weights, active vertices that are
    destinations of the same step: the compare-and-swap fold of k_push_combine against the pull's"""
    _run_case(env, "collisions", threads, 1)

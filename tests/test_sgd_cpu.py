"""CPU-only proof of the inputs of tests/test_gpu_sgd.py: the degree ladder really holds every boundary it names, the
exact-integer case really is exact (and the oracle agrees with plain int64 arithmetic on it), and the random case leaves the
oracle finite with every vertex that has an edge moved -- before a GPU sees any of them."""
import numpy as np
import pytest

from tests.test_gpu_sgd import (BIP_IDLE_USERS, BIP_ITEM_DEGREES, EXACT_STEP, LADDER_DEGREES, LADDER_PAIRS, N_FILLER, N_ISOLATED,
                                assert_exact_in, bipartite_ladder, integer_latent, integer_sgd, ladder_graph, oracle_run,
                                random_latent)


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    binding.build()
    return binding


@pytest.fixture(scope="module")
def ladder():
    return ladder_graph()


def test_ladder_degree_table(ladder):
    nv, s, d, r, table = ladder
    assert nv % 2 == 1 and 4200 <= nv <= 4400 and 50000 <= s.size <= 70000
    assert s.min() >= 1 and d.min() >= 1 and s.max() <= nv and d.max() <= nv
    assert r.min() == 1 and r.max() == 5
    indeg = np.bincount(d - 1, minlength=nv)
    outdeg = np.bincount(s - 1, minlength=nv)
    # the table is what the edge list holds, for every vertex that is not a filler
    assert sorted(table) == list(range(N_FILLER + 1, nv + 1))
    for v, (din, dout) in table.items():
        assert (indeg[v - 1], outdeg[v - 1]) == (din, dout), v
    pairs = list(table.values())
    # every prescribed pair, and every degree of the ladder in each direction on a vertex that has both directions
    for p in LADDER_PAIRS + ((1, 4097), (4097, 1), (64, 65), (65, 64), (16, 17), (17, 16), (1025, 15), (15, 1025), (9000, 2),
                             (0, 33), (33, 0)):
        assert p in pairs, p
    both = [(a, b) for a, b in pairs if a > 0 and b > 0]
    for deg in LADDER_DEGREES:
        assert any(a == deg for a, _ in both), ("in", deg)
        assert any(b == deg for _, b in both), ("out", deg)
    assert pairs.count((0, 0)) == N_ISOLATED >= 3
    assert int(((indeg == 0) & (outdeg == 0)).sum()) == N_ISOLATED  # (fillers all have an edge)
    loops = s[(s == d) & (s > N_FILLER)]  # (random filler edges may be self loops too)
    assert sorted(np.bincount(loops)[np.unique(loops)].tolist()) == [1, 2]  # one self loop, one self loop twice
    # most fillers have edges in both directions as well: the continuation is the common case here, not the exception
    assert int(((indeg > 0) & (outdeg > 0)).sum()) > N_FILLER // 2
    # and the generator is deterministic
    nv2, s2, d2, r2, table2 = ladder_graph()
    assert nv2 == nv and np.array_equal(s, s2) and np.array_equal(d, d2) and np.array_equal(r, r2) and table == table2


def test_bipartite_ladder_shape():
    nv, nu, ni, s, d, r = bipartite_ladder()
    assert ni % 2 == 1 and nv == nu + ni
    assert s.min() >= 1 and s.max() <= nu - BIP_IDLE_USERS and d.min() > nu and d.max() <= nv
    indeg = np.bincount(d - 1, minlength=nv)[nu:]
    assert indeg.tolist() == list(BIP_ITEM_DEGREES)
    assert set(LADDER_DEGREES) <= set(indeg.tolist()) and indeg.tolist().count(0) == 3 and indeg[0] == 0 and indeg[-1] == 0
    outdeg = np.bincount(s - 1, minlength=nv)[:nu]
    assert (outdeg[nu - BIP_IDLE_USERS:] == 0).all() and (outdeg[:nu - BIP_IDLE_USERS] > 0).all()


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("K,dtype", [(128, np.float32), (20, np.float32), (20, np.float64)])
def test_exact_case_is_exact_and_the_oracle_agrees(ob, ladder, K, dtype, threads):
    nv, s, d, r, _ = ladder
    lv = integer_latent(nv, K, dtype)
    assert lv.min() == -2 and lv.max() == 2
    want, wsq, y, yabs_max = integer_sgd(nv, s, d, r, lv)
    assert_exact_in(dtype, y, yabs_max, wsq)  # the 2^22 guard (and the partial sums')
    assert np.array_equal(want.astype(dtype).astype(np.float64), want)  # the result is representable
    og = ob.OracleGraph(nv, s, d, r, threads)
    out, it = og.sgd(lv, 0.0, EXACT_STEP, 1)
    assert it == 1 and np.array_equal(out.astype(np.float64), want)
    tot, sq = og.rmse_sum(lv)
    assert np.array_equal(sq.astype(np.float64), wsq.astype(np.float64))
    # (the oracle's TOTAL is a serial sum in `dtype`: in fp32 it passes 2^24 and rounds at every step, so it is no yardstick
    # for this case -- the GPU test compares the library's total, accumulated in double, with the integer sum)
    if dtype == np.float64:
        assert tot == float(wsq.sum())
    # each rating counts once per direction: an independent total over the edge list
    P = lv.astype(np.int64)
    err = r - (P[s - 1] * P[d - 1]).sum(axis=1)
    assert int(y.sum()) == int(((P[s - 1] + P[d - 1]) * err[:, None]).sum())


def test_exact_case_on_the_bipartite_ladder(ob):
    nv, nu, ni, s, d, r = bipartite_ladder()
    lv = integer_latent(nv, 128, np.float32)
    want, wsq, y, yabs_max = integer_sgd(nv, s, d, r, lv)
    assert_exact_in(np.float32, y, yabs_max, wsq)
    out, _ = ob.OracleGraph(nv, s, d, r, 1).sgd(lv, 0.0, EXACT_STEP, 1)
    assert np.array_equal(out.astype(np.float64), want)


@pytest.mark.parametrize("K,dtype,step", [(128, np.float32, 1e-4), (20, np.float32, 1e-4), (20, np.float64, 3.5e-7)])
def test_random_case_stays_finite_and_moves_every_vertex_with_an_edge(ob, ladder, K, dtype, step):
    nv, s, d, r, _ = ladder
    lv = random_latent(nv, K, dtype)
    assert (lv < 0).any() and (lv > 0).any()
    out, sq, tot = oracle_run(ob, "ladder", nv, s, d, r, lv, 1, 0.001, step, 3)
    assert np.isfinite(out).all() and float(np.abs(out).max()) < 10.0 and np.isfinite(tot)
    has_edge = (np.bincount(s - 1, minlength=nv) + np.bincount(d - 1, minlength=nv)) > 0
    assert np.array_equal(out[~has_edge], lv[~has_edge])
    assert (out != lv).any(axis=1)[has_edge].all()
    if K == 128:
        # rounding-sensitive: the oracle built with fused multiply-adds gives other bits, so bit equality discriminates
        fused, _ = ob.OracleGraph(nv, s, d, r, 1, fused=True).sgd(lv, 0.001, step, 3)
        assert int((fused != out).sum()) > 100

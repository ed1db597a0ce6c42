"""SGD / RMSE on graphs where a vertex has edges in BOTH directions, at every boundary of the kernels that run them.

SgdP folds a vertex's in-edges and then continues the same running value over its out-edges (ALL_EDGES: the AT pass, then
the A pass into the same y).  On a bipartite ratings graph no vertex has both, so the continuation -- `has = accumulate &&
prev_bits[row]` and the reload of acc[] from y in k_sgd_multiply / k_sgd_multiply_mfma, ACC_READ_PREV in the engine -- never
runs.  The degree-ladder graph below gives one vertex every (in-degree, out-degree) pair that matters: the 16-edge tile of
k_sgd_multiply (1, 15, 16, 17, 31 .. 49), the 64-edge tile of the matrix-core form and GM_SHORT_ROW (63, 64, 65, 127 .. 129),
GM_LONG_MID (1023 .. 1025) and the giant threshold (4095 .. 4097, 9000), with pairs that cross the row classes so that the
engine's two passes take different kernels for one row.

Two yardsticks: the oracle, bit for bit, on rounding-sensitive values (mixed signs); and plain int64 arithmetic on inputs
for which every floating-point operation is exact, independent of the oracle and of any fold order -- which also makes the
matrix-core form exactly testable.  Every GPU test asserts the path it means to test (graphmat_hip.h: GM_NOTE_SGD_PATH).
The helpers need no GPU; tests/test_sgd_cpu.py proves the inputs before a GPU sees them.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---------------- inputs (no GPU) -------------------------------------------------------------------------------------------
LADDER_DEGREES = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 9000)
# (in-degree, out-degree) of one extra vertex each.  The first block crosses the row classes (short <= 64 < wave rows, long
# wave rows > 1024, giant >= 4096) or has one direction empty; the second walks the remaining degrees once in each direction.
_CROSSING = ((1, 4097), (4097, 1), (64, 65), (65, 64), (16, 17), (17, 16), (1025, 15), (15, 1025), (9000, 2), (2, 9000),
             (0, 33), (33, 0))
_REST = (31, 32, 33, 47, 48, 49, 63, 127, 128, 129, 1023, 1024, 4095, 4096)
LADDER_PAIRS = _CROSSING + tuple((_REST[i], _REST[(i + 1) % len(_REST)]) for i in range(len(_REST)))
N_FILLER, N_FILLER_EDGES, N_ISOLATED = 4200, 6000, 5

GM_SGD_PATH_ENGINE, GM_SGD_PATH_VECTOR, GM_SGD_PATH_MFMA, GM_SGD_PATH_RING = 0, 1, 2, 3
GM_NOTE_SGD_PATH = 8
GM_SHORT_ROW = 64


def ladder_graph(seed=3):
    """(nv, src, dst, rating, table): about 4 200 filler vertices with 6 000 random edges among them, then one vertex per
    LADDER_PAIRS entry whose in-edges come from and out-edges go to random fillers (duplicates allowed), a vertex with one self
    loop, a vertex with the same self loop twice, and isolated vertices.  table = {vertex id: (in-degree, out-degree)} of every
    vertex that is not a filler.  Ratings 1..5, nv odd, edges in shuffled order."""
    rng = np.random.default_rng(seed)
    src = [rng.integers(1, N_FILLER + 1, N_FILLER_EDGES)]
    dst = [rng.integers(1, N_FILLER + 1, N_FILLER_EDGES)]
    table = {}
    v = N_FILLER
    for din, dout in LADDER_PAIRS:
        v += 1
        src += [rng.integers(1, N_FILLER + 1, din), np.full(dout, v)]
        dst += [np.full(din, v), rng.integers(1, N_FILLER + 1, dout)]
        table[v] = (din, dout)
    v += 1
    src.append([v]); dst.append([v]); table[v] = (1, 1)              # one self loop
    v += 1
    src.append([v, v]); dst.append([v, v]); table[v] = (2, 2)        # the same self loop twice
    for _ in range(N_ISOLATED):
        v += 1
        table[v] = (0, 0)
    nv = v
    assert nv % 2 == 1
    s = np.concatenate(src).astype(np.int32)
    d = np.concatenate(dst).astype(np.int32)
    order = rng.permutation(s.size)
    s, d = np.ascontiguousarray(s[order]), np.ascontiguousarray(d[order])
    r = rng.integers(1, 6, s.size).astype(np.int32)
    return nv, s, d, r, table


BIP_USERS, BIP_IDLE_USERS = 1501, 9
# item in-degrees in item order; 0 = an item nobody rated (one first, one in the middle, one last).  27 items: odd.
BIP_ITEM_DEGREES = (0,) + LADDER_DEGREES[:12] + (0,) + LADDER_DEGREES[12:] + (0,)


def bipartite_ladder(seed=5):
    """(nv, nu, ni, src, dst, rating): users 1..nu, items nu+1..nu+ni; item j is rated BIP_ITEM_DEGREES[j] times by random
    users (duplicates allowed, and needed: 9000 ratings from 1 492 users); the last BIP_IDLE_USERS users rate nothing."""
    rng = np.random.default_rng(seed)
    nu, ni = BIP_USERS, len(BIP_ITEM_DEGREES)
    assert ni % 2 == 1
    src, dst = [], []
    for j, deg in enumerate(BIP_ITEM_DEGREES):
        src.append(rng.integers(1, nu - BIP_IDLE_USERS + 1, deg))
        dst.append(np.full(deg, nu + 1 + j))
    s = np.concatenate(src).astype(np.int32)
    d = np.concatenate(dst).astype(np.int32)
    order = rng.permutation(s.size)
    s, d = np.ascontiguousarray(s[order]), np.ascontiguousarray(d[order])
    r = rng.integers(1, 6, s.size).astype(np.int32)
    return nu + ni, nu, ni, s, d, r


def random_latent(nv, K, dtype, seed=17):
    """standard normal * 0.3: mixed signs, the dot products cancel"""
    return (np.random.default_rng(seed).standard_normal((nv, K)) * 0.3).astype(dtype)


def integer_latent(nv, K, dtype, seed=19):
    return np.random.default_rng(seed).integers(-2, 3, (nv, K)).astype(dtype)


EXACT_STEP = 2.0 ** -10


def integer_sgd(nv, s, d, r, lv):
    """One SGD iteration (lambda = 0, step = 2^-10) and the RMSE pass of the INPUT, in int64: per edge (s, d, r) the error
    r - lv[s].lv[d] is counted once into y[d] (scaled by lv[s]) and once into y[s] (scaled by lv[d]); sqerr belongs to s.
    Returns (new latent as float64, sqerr int64[nv], y int64, largest sum of |terms| of any component of y)."""
    P = np.asarray(lv).astype(np.int64)
    assert np.array_equal(P, lv)
    a, b = P[s - 1], P[d - 1]
    err = r.astype(np.int64) - (a * b).sum(axis=1)
    y = np.zeros_like(P)
    yabs = np.zeros_like(P)
    np.add.at(y, d - 1, a * err[:, None])
    np.add.at(y, s - 1, b * err[:, None])
    np.add.at(yabs, d - 1, np.abs(a * err[:, None]))
    np.add.at(yabs, s - 1, np.abs(b * err[:, None]))
    sq = np.zeros(nv, np.int64)
    np.add.at(sq, s - 1, err * err)
    new = P.astype(np.float64) + EXACT_STEP * y.astype(np.float64)
    return new, sq, y, int(yabs.max())


def assert_exact_in(dtype, y, yabs_max, sq):
    """every operation of the run is exact in `dtype`, in any fold order: all partial sums are integers below 2^24"""
    assert int(np.abs(y).max()) < 2 ** 22
    assert yabs_max < 2 ** 24
    assert int(sq.max()) < 2 ** 24  # (fp32's bound; fp64 has room to spare)


_oracle_cache = {}


def oracle_run(ob, tag, nv, s, d, r, lv, threads, lam, step, iterations):
    """(latent after the run, sqerr per vertex after it, their total) from the oracle; computed once per input"""
    key = (tag, lv.shape[1], lv.dtype.str, threads, lam, step, iterations, lv.tobytes()[:64])
    if key not in _oracle_cache:
        og = ob.OracleGraph(nv, s, d, r, threads)
        out, it = og.sgd(lv, lam, step, iterations)
        assert it == iterations
        tot, sq = og.rmse_sum(out)
        for a in (out, sq):
            a.setflags(write=False)
        _oracle_cache[key] = (out, sq, tot)
    return _oracle_cache[key]


# ---------------- GPU side --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    from oracle import binding as ob
    return api, ob


@pytest.fixture(scope="module")
def ladder():
    return ladder_graph()


@pytest.fixture(scope="module")
def bip():
    return bipartite_ladder()


def sgd_path(g):
    v = C.c_int64(-1)
    assert g.L.gm_graph_note_get(g.h, GM_NOTE_SGD_PATH, C.byref(v)) == 0, "no SGD / RMSE call has recorded its path"
    return v.value


def set_option(api, key, value):
    api._lib.check(api._lib.lib().gm_set_option(key, value))


def assert_ladder_csr(api, g, nv, s, d, table):
    """the library's own adjacency holds the ladder: row lengths per vertex, a giant row and a wave row in each direction"""
    indeg = np.bincount(d - 1, minlength=nv)
    outdeg = np.bincount(s - 1, minlength=nv)
    dov = g.dev_of_vertex.cpu().numpy()
    for direction, deg in ((api.GM_DIR_OUT, indeg), (api.GM_DIR_IN, outdeg)):  # GM_DIR_OUT: rows = destinations
        rp, _, vv = g.csr_to_host(direction)
        rowlen = np.diff(rp)
        assert vv is not None and np.array_equal(rowlen[dov], deg)
        c = g.csr(direction)
        assert c.ngiant >= 1, "no giant row in direction %d" % direction
        assert c.short_row == GM_SHORT_ROW and int((rowlen > GM_SHORT_ROW).sum()) >= 1 and int((rowlen <= GM_SHORT_ROW).sum()) >= 1


SGD_CONFIGS = {  # name: (K, dtype, step, force_ordered, path)
    "k128_f32_dedicated": (128, np.float32, 1e-4, 0, GM_SGD_PATH_VECTOR),
    "k128_f32_engine": (128, np.float32, 1e-4, 1, GM_SGD_PATH_ENGINE),
    "k20_f32": (20, np.float32, 1e-4, 0, GM_SGD_PATH_ENGINE),
    "k20_f64": (20, np.float64, 3.5e-7, 0, GM_SGD_PATH_ENGINE),
}


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("config", sorted(SGD_CONFIGS))
def test_ladder_random_values_equal_the_oracle_bit_for_bit(env, ladder, config, threads, layout):
    """Three iterations on rounding-sensitive values (the fused and the unfused build of the oracle differ on inputs of this
    shape): every component must carry the oracle's bits -- DESIGN §4 / §6 state the dedicated kernels bit-identical and the
    ordered fold exact, and both sides are built without contraction.  Then the RMSE pass of the result."""
    api, ob = env
    K, dtype, step, force, path = SGD_CONFIGS[config]
    nv, s, d, r, table = ladder
    lv = random_latent(nv, K, dtype)
    olv, osq, otot = oracle_run(ob, "ladder", nv, s, d, r, lv, threads, 0.001, step, 3)
    g = api.Graph(nv, s, d, r, ref_threads=threads, layout=layout)
    assert_ladder_csr(api, g, nv, s, d, table)
    set_option(api, b"force_ordered", force)
    out, it = g.sgd(lv, 0.001, step, 3)
    assert it == 3 and sgd_path(g) == path
    assert out.dtype == dtype
    diff = out != olv
    print("%s threads=%d layout=%d: %d of %d components differ from the oracle (%d vertices), max |diff| %.3g" % (
        config, threads, layout, int(diff.sum()), diff.size, int(diff.any(axis=1).sum()), float(np.abs(out - olv).max())))
    assert np.array_equal(out, olv)
    has_edge = (np.bincount(s - 1, minlength=nv) + np.bincount(d - 1, minlength=nv)) > 0
    assert int((~has_edge).sum()) == N_ISOLATED
    assert np.array_equal(out[~has_edge].view(np.uint8), lv[~has_edge].view(np.uint8)), "an isolated vertex changed"
    assert (out != lv).any(axis=1)[has_edge].all(), "a vertex with an edge kept its input"
    tot, sq = g.rmse_sum(out)
    assert sgd_path(g) == path
    assert np.array_equal(sq, osq)
    assert abs(tot - otot) <= 1e-6 * abs(otot)  # (gm_reduce_sum_* sums in its own tree order)
    g.close()


EXACT_CONFIGS = dict(SGD_CONFIGS)
EXACT_CONFIGS["k128_f32_matrix_core"] = (128, np.float32, None, 0, GM_SGD_PATH_MFMA)


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("config", sorted(EXACT_CONFIGS))
def test_ladder_exact_integers_equal_plain_arithmetic(env, ladder, config, threads):
    """Independent of the oracle: integer latent values in -2..2, lambda = 0, step = 2^-10, one iteration.  Every fp32 / fp64
    operation is exact, so any fold order gives the int64 result -- each rating counted once per direction, with the right rows
    of x and the right rating.  The first exact test of the matrix-core form (its order of summation does not matter here)."""
    api, _ = env
    K, dtype, _, force, path = EXACT_CONFIGS[config]
    nv, s, d, r, _ = ladder
    lv = integer_latent(nv, K, dtype)
    want, wsq, y, yabs_max = integer_sgd(nv, s, d, r, lv)
    assert_exact_in(dtype, y, yabs_max, wsq)
    g = api.Graph(nv, s, d, r, ref_threads=threads)
    set_option(api, b"force_ordered", force)
    set_option(api, b"sgd_mfma", 1 if path == GM_SGD_PATH_MFMA else 0)
    out, it = g.sgd(lv, 0.0, EXACT_STEP, 1)
    assert it == 1 and sgd_path(g) == path
    bad = (out.astype(np.float64) != want).any(axis=1)
    print("%s threads=%d: %d vertices differ from the integer evaluation" % (config, threads, int(bad.sum())))
    assert np.array_equal(out.astype(np.float64), want)
    tot, sq = g.rmse_sum(lv)  # (the matrix-core option has no RMSE form: the vector kernel)
    assert sgd_path(g) == (GM_SGD_PATH_VECTOR if path == GM_SGD_PATH_MFMA else path)
    assert np.array_equal(sq.astype(np.float64), wsq.astype(np.float64))
    assert abs(tot - float(wsq.sum())) <= 1e-6 * float(wsq.sum())
    g.close()


@pytest.mark.parametrize("config", ["k128_f32_dedicated", "k20_f32"])
def test_ladder_on_a_tiled_device_order(env, ladder, config):
    """SGD does not use the column tiles but runs on the device order they impose (tile, then degree rank)."""
    api, ob = env
    K, dtype, step, force, path = SGD_CONFIGS[config]
    nv, s, d, r, _ = ladder
    lv = random_latent(nv, K, dtype)
    olv, osq, _ = oracle_run(ob, "ladder", nv, s, d, r, lv, 3, 0.001, step, 3)
    set_option(api, b"tile_min_row", 64)
    g = api.Graph(nv, s, d, r, ref_threads=3, col_tiles=4)
    assert g.col_tiles > 1
    out, it = g.sgd(lv, 0.001, step, 3)
    assert it == 3 and sgd_path(g) == path
    assert np.array_equal(out, olv)
    _, sq = g.rmse_sum(out)
    assert np.array_equal(sq, osq)
    g.close()


# ---------------- gm_run_sgd_bipartite on one rank ---------------------------------------------------------------------------
def _bipartite_checks(g, moved, lv, out, nu):
    assert moved == 0, "one rank receives nothing"
    assert sgd_path(g) == GM_SGD_PATH_RING
    idle = np.zeros(lv.shape[0], bool)
    idle[nu - BIP_IDLE_USERS:nu] = True
    idle[nu:][np.array(BIP_ITEM_DEGREES) == 0] = True
    assert np.array_equal(out[idle].view(np.uint8), lv[idle].view(np.uint8)), "an unrated item or an idle user changed"
    assert (out != lv).any(axis=1)[~idle].all()


@pytest.mark.parametrize("blocks", [0, 1, 3, len(BIP_ITEM_DEGREES), len(BIP_ITEM_DEGREES) + 5])
def test_bipartite_ring_on_one_rank(env, bip, blocks):
    """With no communicator gm_run_sgd_bipartite is a single-GPU iteration: the row-list form of k_sgd_multiply (an odd item
    count cuts the second wave of the last workgroup off), k_rows_pack / k_rows_unpack / k_rows_in_range, for every way of
    cutting the items into blocks.  Oracle bits, Graph.sgd's bits, and plain integers on the exact input."""
    api, ob = env
    nv, nu, ni, s, d, r = bip
    lv = random_latent(nv, 128, np.float32)
    olv, _, _ = oracle_run(ob, "bipartite", nv, s, d, r, lv, 1, 0.001, 1e-4, 3)
    g = api.Graph(nv, s, d, r, ref_threads=1)
    ref, it = g.sgd(lv, 0.001, 1e-4, 3)
    assert it == 3 and sgd_path(g) == GM_SGD_PATH_VECTOR
    out, it, moved = g.sgd_bipartite(lv, nu, ni, 0.001, 1e-4, 3, blocks=blocks)
    assert it == 3
    _bipartite_checks(g, moved, lv, out, nu)
    assert np.array_equal(out, olv) and np.array_equal(out, ref)
    ilv = integer_latent(nv, 128, np.float32)
    want, wsq, y, yabs_max = integer_sgd(nv, s, d, r, ilv)
    assert_exact_in(np.float32, y, yabs_max, wsq)
    out, it, moved = g.sgd_bipartite(ilv, nu, ni, 0.0, EXACT_STEP, 1, blocks=blocks)
    assert it == 1 and moved == 0 and sgd_path(g) == GM_SGD_PATH_RING
    assert np.array_equal(out.astype(np.float64), want)
    g.close()


def test_sgd_refusals(env, bip):
    """What gm_run_sgd_bipartite and gm_run_sgd do not take is refused with its error code and message, before any kernel
    touches the vertex state."""
    api, _ = env
    import torch
    nv, nu, ni, s, d, r = bip
    L = api._lib.lib()
    g = api.Graph(nv, s, d, r, ref_threads=1)
    # K = 20: only the dedicated K = 128 fp32 kernels walk the ring
    with pytest.raises(api._lib.GMError, match=r"error 4: .*only K=128 fp32"):
        g.sgd_bipartite(random_latent(nv, 20, np.float32), nu, ni, 0.001, 1e-4, 1)
    assert L.gm_graph_note_get(g.h, GM_NOTE_SGD_PATH, C.byref(C.c_int64(0))) == 1  # (no path was taken: the note is unset)
    # an item row outside the graph: found before any kernel indexes with it
    st, K = g._latent_to_device(random_latent(nv, 128, np.float32))
    before = st.clone()
    good = g.dev_of_vertex[nu:nu + ni].to(torch.int32).contiguous()
    for bad_row in (g.rows, -1):
        rows = good.clone()
        rows[ni // 2] = bad_row
        it = C.c_int(-7)
        rc = L.gm_run_sgd_bipartite(g.h, st.data_ptr(), 128, 4, rows.data_ptr(), ni, 3, 0.001, 1e-4, 1, C.byref(it), api._stream())
        assert rc == 1 and b"outside" in L.gm_last_error(), (rc, L.gm_last_error())
        torch.cuda.synchronize()
        assert torch.equal(st, before) and it.value == -7
    # gm_run_sgd: K = 64 is not in the menu
    st64, _ = g._latent_to_device(random_latent(nv, 64, np.float32))
    rc = L.gm_run_sgd(g.h, st64.data_ptr(), 64, 4, 0.001, 1e-4, 1, None, api._stream())
    assert rc == 4 and b"not in the fixed menu" in L.gm_last_error(), (rc, L.gm_last_error())
    g.close()
    # a graph built without edge values has no ratings
    g0 = api.Graph(nv, s, d, None, ref_threads=1)
    with pytest.raises(api._lib.GMError, match=r"error 1: .*4-byte values"):
        g0.sgd_bipartite(random_latent(nv, 128, np.float32), nu, ni, 0.001, 1e-4, 1)
    g0.close()
    # one shard of a sharded graph: the ring wants each rank's ratings as a whole graph (refused before anything runs)
    for shard in (0, 1):
        gs = api.Graph(nv, s, d, r, ref_threads=1, nshards=2, shard=shard)
        assert gs.rows < gs.ndevice
        with pytest.raises(api._lib.GMError, match=r"error 1: .*needs an unsharded graph"):
            gs.sgd_bipartite(random_latent(nv, 128, np.float32), nu, ni, 0.001, 1e-4, 1)
        gs.close()

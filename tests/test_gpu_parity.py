"""Parity of the HIP path (through the C-ABI) against the oracle.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphmat_amd import generators as gen
from graphmat_amd.mtx import read_mtx_bin

MAXD = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    from oracle import binding as ob
    return api, ob


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------- golden fixtures -------------------------------------------------------------
def test_G1_pagerank_fixture(env, golden_dir):
    api, ob = env
    ref = json.load(open(os.path.join(golden_dir, "reference_outputs.json")))["G1_pagerank_test_bin_mtx"]
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, ref["file"]))
    g = api.Graph(nv, s, d, v)
    pr, deg, it = g.pagerank(-1)
    assert deg.tolist() == ref["out_degree"]
    assert it == ref["pagerank_iterations"]
    assert ["%.6f" % x for x in pr] == ref["pagerank_6dp"]
    opr, oit, _ = ob.OracleGraph(nv, s, d, v, 1).pagerank(-1)
    assert oit == it and (f32bits(pr) == f32bits(opr)).all()


def test_G2_bfs_fixtures(env, golden_dir):
    api, ob = env
    ref = json.load(open(os.path.join(golden_dir, "reference_outputs.json")))
    r = ref["G2_bfs_test_bin_mtx"]
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, r["file"]))
    depth, parent, it = api.Graph(nv, s, d, v).bfs(r["source"])
    assert it == r["iterations"] and depth.tolist() == r["depth"]
    assert parent.astype(np.int64).tolist() == r["parent"]
    r = ref["G2_bfs_2_10_upper_triangle"]
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, r["file"]))
    depth, parent, it = api.Graph(nv, s, d, v).bfs(r["source"])
    assert it == r["iterations"] and int((depth != MAXD).sum()) == r["reachable"]
    assert depth[:10].tolist() == r["first10_depth"]
    assert parent[:10].astype(np.int64).tolist() == r["first10_parent"]
    od, op, oit, _ = ob.OracleGraph(nv, s, d, v, 1).bfs(r["source"])
    assert (depth == od).all() and (parent == op).all() and it == oit


def test_G3_sgd_fixture(env, golden_dir):
    api, ob = env
    from tests.test_oracle_golden import rand_r_latent
    r = json.load(open(os.path.join(golden_dir, "reference_outputs.json")))["G3_sgd_ratings7"]
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, r["file"]))
    g = api.Graph(nv, s, d, v)
    lv = rand_r_latent(nv, r["K"])
    e0, _ = g.rmse_sum(lv)
    assert "%.6f" % np.sqrt(e0 / len(s)) == r["rmse_before_6dp"]
    lv2, it = g.sgd(lv, r["lambda"], r["step"], r["iterations"])
    e1, _ = g.rmse_sum(lv2)
    assert it == r["iterations"] and "%.6f" % np.sqrt(e1 / len(s)) == r["rmse_after_6dp"]
    olv, _ = ob.OracleGraph(nv, s, d, v, 1).sgd(lv, r["lambda"], r["step"], r["iterations"])
    np.testing.assert_allclose(lv2, olv, rtol=1e-6, atol=0)  # tolerance stated by north_star; observed: exact


# ---------------- structure ---------------------------------------------------------------------
def test_rmat_device_generator_matches_numpy(env):
    api, _ = env
    for scale, ef, seed in ((8, 16, 1), (13, 8, 7)):
        nv, s, d, v = gen.rmat_edges(scale, ef, seed, weights="hash")
        dnv, ds, dd, dv = api.rmat_on_device(scale, ef, seed, weights=True)
        assert dnv == nv
        assert (ds.cpu().numpy() == s).all() and (dd.cpu().numpy() == d).all() and (dv.cpu().numpy() == v).all()


@pytest.mark.parametrize("threads,layout", [(1, 0), (3, 0), (1, 1), (2, 1)])
def test_csr_build_order(env, threads, layout):
    """rows in device order; inside a row the columns follow ascending NATIVE id (the reference's
    reduction order), duplicates kept in input order; both directions, both layouts."""
    api, _ = env
    nv, s, d, v = gen.rmat_edges(10, 16, 3, weights="hash")
    v = np.arange(len(s), dtype=np.int32)  # unique values expose the duplicate order
    g = api.Graph(nv, s, d, v, ref_threads=threads, layout=layout)
    don, nod = g.maps_to_host()
    assert sorted(don.tolist()) == list(range(nv)) and (nod[don] == np.arange(nv)).all()
    nat = api.native_index(nv, threads * 16)
    sn, dn = nat[s - 1], nat[d - 1]
    for direction, rows, cols in ((api.GM_DIR_OUT, dn, sn), (api.GM_DIR_IN, sn, dn)):
        rp, ci, vv = g.csr_to_host(direction)
        order = np.lexsort((np.arange(len(s)), cols, don[rows]))  # stable: device row, native col, input position
        assert (ci == don[cols[order]]).all() and (vv == v[order]).all()
        assert (rp == np.searchsorted(don[rows[order]], np.arange(nv + 1))).all()
    if layout == 1:  # busiest vertices first
        deg = np.bincount(sn, minlength=nv) + np.bincount(dn, minlength=nv)
        assert (np.diff(deg[nod]) <= 0).all()


def _giant_rows_folded_again(api, g):
    """White box: the engine keeps, in workspace slot GM_WS_SPECULATION of the graph, [ngchunk + 2] chunk boundaries of 8 bytes and then one flag per giant row that
    k_giant_verify_chunks* sets when a chunk of the row fails its proof (engine.hpp: multiply_out).  (rows folded again, giant rows), or None."""
    import ctypes as C
    ca = g.csr(api.GM_DIR_OUT)
    ptr, size, ext = C.c_void_p(), C.c_size_t(), C.c_int()
    if api._lib.lib().gm_graph_workspace_info(g.h, api._lib.GM_WS_SPECULATION, C.byref(ptr), C.byref(size), C.byref(ext)) != 0 or not ptr.value:
        return None
    if size.value < (ca.ngchunk + 2) * 8 + ca.ngiant * 4:
        return None
    redo = np.zeros(ca.ngiant, dtype=np.int32)
    api.copy_from_device(redo, ptr.value + (ca.ngchunk + 2) * 8)
    return int((redo != 0).sum()), int(ca.ngiant)


def test_ordered_float_sum_giant_rows_speculated_and_proven(env):
    """PageRank with the ORDERED fold forced (the program then declares REDUCE_ORDERED: `c = a; reduce(c, b)` in stored order, SPMV.h:54-59) on a
    graph whose hub rows span several 8192-product chunks: the giant rows are replayed as float sums and every chunk is proven with the
    program's own reduce_function (kernels.hpp: k_giant_verify_chunks) -- no row has to be folded again, and the bits are the oracle's."""
    api, ob = env
    nv, s, d, v = gen.rmat_edges(18, 16, seed=5)
    og = ob.OracleGraph(nv, s, d, v, 1)
    g = api.Graph(nv, s, d, v, ref_threads=1, layout=1)
    ca = g.csr(api.GM_DIR_OUT)
    assert ca.ngiant > 0 and ca.ngchunk > 2 * ca.ngiant, (ca.ngiant, ca.ngchunk)  # (pieces of 4096: rows of several chunks among them)
    api._lib.lib().gm_set_option(b"force_ordered", 1)
    try:
        pr, deg, it = g.pagerank(6)
        opr, oit, _ = og.pagerank(6)
        assert (f32bits(pr) == f32bits(opr)).all()
        again = _giant_rows_folded_again(api, g)
        assert again is not None and again[0] == 0 and again[1] == ca.ngiant, again
        # the same run without the speculation (one chain per giant row): the same bits
        api._lib.lib().gm_set_option(b"ordered_giant_two_pass", 1)
        pr1, _, _ = g.pagerank(6)
        assert (f32bits(pr1) == f32bits(opr)).all()
    finally:
        api._lib.lib().gm_reset_options()


# ---------------- programs on synthetic graphs -----------------------------------------------------
@pytest.mark.parametrize("scale,threads,layout", [(10, 1, 1), (12, 4, 0), (14, 1, 1), (16, 2, 1), (16, 1, 0)])
def test_pagerank_bit_exact_rmat(env, scale, threads, layout):
    api, ob = env
    nv, s, d, v = gen.rmat_edges(scale, 16, seed=scale)
    og = ob.OracleGraph(nv, s, d, v, threads)
    g = api.Graph(nv, s, d, v, ref_threads=threads, layout=layout)
    for force in (0, 1):
        api._lib.lib().gm_set_option(b"force_ordered", force)
        pr, deg, it = g.pagerank(10)
        opr, oit, _ = og.pagerank(10)
        assert (deg == og.degree()).all()
        assert it == oit == 10
        assert (f32bits(pr) == f32bits(opr)).all(), "pagerank bits differ (force_ordered=%d)" % force
    api._lib.lib().gm_set_option(b"force_ordered", 0)


def test_uniform_random_graph_against_oracle(env):
    """A graph without any skew -- every vertex has exactly 16 out-edges to uniformly drawn distinct destinations, the
    shape of the reference's own random test graphs (test/generator.h:73-105) -- where ranking vertices by degree buys
    nothing: PageRank (fixed count, forced column tiles too), BFS and SSSP must still equal the oracle bit for bit."""
    api, ob = env
    nv, s, d, v = gen.uniform_out_regular_edges(1 << 16, 16, seed=9)
    og = ob.OracleGraph(nv, s, d, v, 2)
    opr, oit, _ = og.pagerank(8)
    for tiles in (0, 3):
        g = api.Graph(nv, s, d, v, ref_threads=2, col_tiles=tiles)
        pr, deg, it = g.pagerank(8)
        assert (deg == og.degree()).all() and (deg == 16).all()
        assert it == oit == 8 and (f32bits(pr) == f32bits(opr)).all(), "tiles=%d" % tiles
    depth, parent, itb = g.bfs(3)
    od, op, oitb, _ = og.bfs(3)
    assert itb == oitb and (depth == od).all() and (parent == op).all()
    dist, its = g.sssp(3)
    odist, oits = og.sssp(3)
    assert its == oits and (dist == odist).all()


def test_pagerank_until_convergence(env):
    api, ob = env
    nv, s, d, v = gen.rmat_edges(12, 16, seed=5)
    pr, deg, it = api.Graph(nv, s, d, v).pagerank(-1)
    opr, oit, _ = ob.OracleGraph(nv, s, d, v, 1).pagerank(-1)
    assert it == oit and (f32bits(pr) == f32bits(opr)).all()


@pytest.mark.parametrize("scale,threads,layout", [(10, 1, 1), (13, 4, 0), (16, 1, 1)])
def test_bfs_bit_exact_rmat(env, scale, threads, layout):
    api, ob = env
    nv, s, d, v = gen.rmat_edges(scale, 16, seed=100 + scale)
    og = ob.OracleGraph(nv, s, d, v, threads)
    g = api.Graph(nv, s, d, v, ref_threads=threads, layout=layout)
    for source in (1, 2, int(s[len(s) // 2])):
        depth, parent, it = g.bfs(source)
        od, op, oit, _ = og.bfs(source)
        assert it == oit and (depth == od).all()
        assert (parent == op).all(), "BFS parents differ"


def test_sssp_bit_exact(env, golden_dir):
    api, ob = env
    nv, s, d, v = read_mtx_bin(os.path.join(golden_dir, "2_10_upper_triangle.bin.mtx"))
    dist, it = api.Graph(nv, s, d, v).sssp(1)
    odist, oit = ob.OracleGraph(nv, s, d, v, 1).sssp(1)
    assert it == oit and (dist == odist).all()
    nv, s, d, v = gen.rmat_edges(13, 16, seed=11, weights="hash")
    dist, it = api.Graph(nv, s, d, v, ref_threads=2).sssp(1)
    odist, oit = ob.OracleGraph(nv, s, d, v, 2).sssp(1)
    assert it == oit and (dist == odist).all()


@pytest.mark.parametrize("degrees", [(65, 127, 128, 129, 200), (64, 65, 1024, 1025, 4096, 4097, 70, 300, 90, 91, 92, 93, 94, 95, 96, 97, 98, 99, 100),
                                     tuple(range(65, 65 + 40))])
def test_pagerank_rows_around_the_wave_kernels_boundaries(env, degrees):
    """in-degrees at the chunk (64), group (16 rows per wave) and long-row (1024 / 4096 edges) boundaries of the
    ordered wave kernels, a partial last group, duplicates: fp32 sums bit-exact against the oracle"""
    api, ob = env
    rng = np.random.default_rng(len(degrees))
    nsrc = 6000
    s, d = [], []
    for i, deg in enumerate(degrees):
        t = nsrc + 1 + i
        srcs = rng.integers(1, nsrc + 1, deg)  # with repetitions
        s.extend(srcs.tolist()); d.extend([t] * deg)
    # give the sources out-edges among themselves so that their ranks differ
    a = rng.integers(1, nsrc + 1, 20000); b = rng.integers(1, nsrc + 1, 20000)
    s.extend(a.tolist()); d.extend(b.tolist())
    s, d = np.array(s, np.int32), np.array(d, np.int32)
    nv = nsrc + len(degrees) + 5
    for threads, layout in ((1, 1), (2, 0)):
        g = api.Graph(nv, s, d, None, ref_threads=threads, layout=layout)
        pr, deg_out, it = g.pagerank(6)
        opr, oit, _ = ob.OracleGraph(nv, s, d, None, threads).pagerank(6)
        assert it == oit == 6 and np.array_equal(f32bits(pr), f32bits(opr))


def test_sssp_small_active_sets_with_colliding_relaxations(env):
    """Layered weighted graph whose active sets stay tiny, so every level is a list-based top-down step
    (k_push_combine): many sources relax the same destination in one step (compare-and-swap fold of min),
    duplicate edges included."""
    api, ob = env
    rng = np.random.default_rng(42)
    layers = [np.array([1])] + [np.arange(a, b) for a, b in ((2, 52), (52, 252), (252, 1252), (1252, 1300))]
    s, d = [], []
    for up, down in zip(layers[:-1], layers[1:]):
        for v in down:
            for u in rng.choice(up, size=min(len(up), 6), replace=True):  # duplicates on purpose
                s.append(int(u)); d.append(int(v))
    s, d = np.array(s, np.int32), np.array(d, np.int32)
    w = rng.integers(1, 100, len(s)).astype(np.int32)
    nv = 1400  # the last 100 vertices are unreachable
    for threads in (1, 3):
        dist, it = api.Graph(nv, s, d, w, ref_threads=threads).sssp(1)
        odist, oit = ob.OracleGraph(nv, s, d, w, threads).sssp(1)
        assert it == oit and np.array_equal(dist, odist)
    assert (dist[1300:] == 0xFFFFFFFF).all() and dist[0] == 0 and (dist[1:1299] < 0xFFFFFFFF).all()


@pytest.mark.parametrize("n", [100, 500])
def test_bfs_depths_closed_form(env, n):
    """The reference's own BFS tests (test/test_bfs.cpp:97-236) against the HIP path."""
    api, _ = env
    h = n // 2
    i = np.arange(1, n + 1)
    g = api.Graph(*gen.upper_triangular_edges(n))
    depth = g.bfs(1)[0]
    assert depth[0] == 0 and (depth[1:] == 1).all()
    depth = g.bfs(h)[0]
    assert (depth[: h - 1] == MAXD).all() and depth[h - 1] == 0 and (depth[h:] == 1).all()
    g = api.Graph(*gen.dense_edges(n))
    for src in (1, h):
        exp = np.ones(n, np.uint32)
        exp[src - 1] = 0
        assert (g.bfs(src)[0] == exp).all()
    g = api.Graph(*gen.chain_edges(n))
    assert (g.bfs(1)[0] == (i - 1)).all()
    assert (g.bfs(h)[0] == np.where(i < h, h + i, i - h)).all()


# ---------------- the exact fp32 replay on long rows ---------------------------------------------
def _pagerank_custom(api, ob, nv, s, d, pr0, deg, alpha, iters, threads=1, col_tiles=1, graph_out=None):
    import torch
    g = api.Graph(nv, s, d, np.ones(len(s), np.int32), ref_threads=threads, col_tiles=col_tiles)
    if graph_out is not None:
        graph_out.append(g)  # (the caller looks at the graph's structure and scratch afterwards)
    st = torch.zeros((nv, 2), dtype=torch.int32, device=g.device)
    st[:, 0] = g.to_device_order(f32bits(pr0).view(np.int32))
    st[:, 1] = g.to_device_order(np.asarray(deg, np.int32))
    out = []
    for force in (0, 1):
        api._lib.lib().gm_set_option(b"force_ordered", force)
        s2 = st.clone()
        g.run_pagerank(s2, iters, alpha)
        out.append(g.to_vertex_order(s2[:, 0].contiguous().view(torch.float32)).cpu().numpy())
    api._lib.lib().gm_set_option(b"force_ordered", 0)
    opr, _, _ = ob.OracleGraph(nv, s, d, None, threads).pagerank(iters, alpha, pr0, deg)
    return out[0], out[1], opr


@pytest.mark.parametrize("kind", ["ties", "wide", "mixed_sign", "tiny"])
def test_long_row_float_sum_is_bit_exact(env, kind):
    """Star graphs: every vertex points at a few hubs, so hub rows (thousands of terms) take
    the long-row kernel.  alpha=0 makes pagerank := the fp32 row sum, exposing every bit."""
    api, ob = env
    rng = np.random.default_rng(42)
    nv = 40000
    hubs = np.array([1, 2, 3, 777, 40000])
    src = np.repeat(np.arange(1, nv + 1), len(hubs)).astype(np.int32)
    dst = np.tile(hubs, nv).astype(np.int32)
    keep = rng.random(len(src)) < 0.7
    src, dst = src[keep], dst[keep]
    if kind == "ties":      # few mantissa bits: round-to-even ties everywhere
        pr0 = (rng.integers(1, 64, nv) * np.float32(2.0) ** rng.integers(-12, 3, nv)).astype(np.float32)
    elif kind == "wide":    # 30 binades of magnitudes, full mantissas
        pr0 = (rng.random(nv).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 10, nv)).astype(np.float32)
    elif kind == "mixed_sign":  # must fall back to the serial fold
        pr0 = rng.standard_normal(nv).astype(np.float32)
    else:                   # subnormal-scale terms
        pr0 = (rng.random(nv) * 1e-38).astype(np.float32)
        pr0[::7] = 0
    deg = np.ones(nv, np.int32)
    a, b, o = _pagerank_custom(api, ob, nv, src, dst, pr0, deg, 0.0, 1)
    assert (f32bits(a) == f32bits(o)).all(), "exact replay differs from the oracle"
    assert (f32bits(b) == f32bits(o)).all(), "serial long-row fold differs from the oracle"


@pytest.mark.parametrize("two_pass,maps", [(0, 1), (1, 1), (2, 1), (2, 0)])
def test_giant_row_strategies_against_the_oracle(env, two_pass, maps):
    """Every strategy the engine has for giant rows (engine.hpp: giant_rows), chosen by the options ordered_giant_two_pass (0: one wave per
    row gathers and folds, 1: products stream + ordered fold, 2: speculated and proven) and giant_maps (the float sum's replay with piece
    maps, or one workgroup per row), on the star graph of test_long_row_float_sum_is_bit_exact: ~28 000 in-edges per hub, i.e. 7 pieces and
    more than 3 chunks of 8192 products per row, so every pass has several pieces and several chunks per row.  alpha = 0 makes pagerank := the
    fp32 row sum; both the declared float sum and the forced ordered fold must give the oracle's bits, and where the speculation runs on
    values of one sign every chunk must be proven."""
    api, ob = env
    L = api._lib.lib()
    rng = np.random.default_rng(42)
    nv = 40000
    hubs = np.array([1, 2, 3, 777, 40000])
    src = np.repeat(np.arange(1, nv + 1), len(hubs)).astype(np.int32)
    dst = np.tile(hubs, nv).astype(np.int32)
    keep = rng.random(len(src)) < 0.7
    src, dst = src[keep], dst[keep]
    values = {"wide": (rng.random(nv).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 10, nv)).astype(np.float32),
              "mixed_sign": rng.standard_normal(nv).astype(np.float32)}
    deg = np.ones(nv, np.int32)
    try:
        api._lib.check(L.gm_set_option(b"ordered_giant_two_pass", two_pass))
        api._lib.check(L.gm_set_option(b"giant_maps", maps))
        for kind, pr0 in values.items():
            graphs = []
            a, b, o = _pagerank_custom(api, ob, nv, src, dst, pr0, deg, 0.0, 2, graph_out=graphs)
            ca = graphs[0].csr(api.GM_DIR_OUT)
            assert ca.ngiant == 5 and ca.ngchunk > 2 * ca.ngiant, (ca.ngiant, ca.ngchunk)
            assert (f32bits(a) == f32bits(o)).all(), "declared float sum differs from the oracle (%s)" % kind
            assert (f32bits(b) == f32bits(o)).all(), "forced ordered fold differs from the oracle (%s)" % kind
            if two_pass == 2 and kind == "wide":  # (the last run of the helper is the forced ordered fold: speculated, every chunk proven)
                assert _giant_rows_folded_again(api, graphs[0]) == (0, ca.ngiant)
    finally:
        api._lib.check(L.gm_reset_options())


@pytest.mark.parametrize("kind,tiles", [("uniform", 1), ("ties", 1), ("growing", 1), ("uniform", 3), ("ties", 4)])
def test_giant_rows_replayed_by_many_workgroups(env, kind, tiles):
    """Hub rows of ~200 K terms (25 chunks of 8192): most chunks get a precomputed ulp-map (kernels.hpp: gchunk_state: composed by
    k_giant_terms against the binade the previous pass left as a hint) that k_spmv_giant only applies, the chunks around binade crossings are replayed as before; with column
    tiles a row's pieces continue from the value y holds.  alpha = 0 makes pagerank := the fp32 row sum.  The bits must be
    the oracle's (the serial loop's) with the maps on, and the map path must really have been taken."""
    import ctypes as C
    api, ob = env
    L = api._lib.lib()
    rng = np.random.default_rng(7)
    nv = 300000
    hubs = np.array([1, 5, 4242, 300000])
    src = np.repeat(np.arange(1, nv + 1), len(hubs)).astype(np.int32)
    dst = np.tile(hubs, nv).astype(np.int32)
    keep = rng.random(len(src)) < 0.7
    src, dst = src[keep], dst[keep]
    if kind == "uniform":   # full mantissas, one order of magnitude: S sits in each binade for ever longer stretches
        pr0 = (0.5 + 0.5 * rng.random(nv)).astype(np.float32)
    elif kind == "ties":    # few mantissa bits: round-to-even ties everywhere
        pr0 = (rng.integers(1, 64, nv) * np.float32(2.0) ** rng.integers(-6, 3, nv)).astype(np.float32)
    else:                   # terms grow along the row: the estimate of S is far from uniform
        pr0 = (np.arange(1, nv + 1) / nv * rng.random(nv) * 8).astype(np.float32)
    deg = np.ones(nv, np.int32)
    deg[hubs - 1] = 1 << 20  # the hubs' own (huge, after the first iteration) values barely enter the next sums
    cnt = (C.c_int64 * 4)()
    L.gm_debug_counters(cnt)  # reset
    # (two iterations: the first pass over a giant row leaves the binade hints the second one's maps are composed for)
    a, b, o = _pagerank_custom(api, ob, nv, src, dst, pr0, deg, 0.0, 2, col_tiles=tiles)
    L.gm_debug_counters(cnt)
    assert (f32bits(a) == f32bits(o)).all(), "giant rows with chunk maps differ from the oracle"
    assert (f32bits(b) == f32bits(o)).all()
    assert cnt[2] > 0, "no chunk took the precomputed map"
    # and the single-workgroup replay (maps off) gives the same bits
    L.gm_set_option(b"giant_maps", 0)
    try:
        a2, _, _ = _pagerank_custom(api, ob, nv, src, dst, pr0, deg, 0.0, 2, col_tiles=tiles)
    finally:
        L.gm_set_option(b"giant_maps", 1)
    assert (f32bits(a2) == f32bits(o)).all()


def test_edge_cases(env):
    api, ob = env
    # vertices without edges, nv not a multiple of 32, self loops and duplicates
    nv = 77
    s = np.array([1, 1, 1, 5, 5, 77, 77, 3], np.int32)
    d = np.array([2, 2, 2, 5, 6, 1, 1, 77], np.int32)
    v = np.ones(len(s), np.int32)
    g = api.Graph(nv, s, d, v)
    og = ob.OracleGraph(nv, s, d, v, 1)
    pr, deg, it = g.pagerank(5)
    opr, _, _ = og.pagerank(5)
    assert (deg == og.degree()).all() and (f32bits(pr) == f32bits(opr)).all()
    depth, parent, it = g.bfs(1)
    od, op, oit, _ = og.bfs(1)
    assert (depth == od).all() and (parent == op).all() and it == oit
    # graph with no edges at all: nothing is applied, one iteration
    g0 = api.Graph(64, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    pr, deg, it = g0.pagerank(-1)
    assert it == 1 and (pr == np.float32(0.3)).all() and (deg == 0).all()


@pytest.mark.parametrize("width", [1000, 65536, 65537, 200000])
def test_bfs_active_set_sizes_around_the_top_down_limits(env, width):
    """source -> `width` middle vertices -> one leaf each (plus a few cross edges): the active set of
    level 2 has exactly `width` vertices, i.e. below, at and above the list capacity of the top-down
    steps (65536), and the middle vertices arrive in 64..1024-entry batches of the LDS list builder."""
    api, ob = env
    rng = np.random.default_rng(width)
    mid = np.arange(2, 2 + width, dtype=np.int32)
    leaf = mid + width
    extra_s = rng.choice(mid, 500).astype(np.int32)
    extra_d = rng.choice(leaf, 500).astype(np.int32)
    s = np.concatenate([np.full(width, 1, np.int32), mid, extra_s])
    d = np.concatenate([mid, leaf, extra_d])
    nv = 1 + 2 * width
    for threads in (1, 2):
        g = api.Graph(nv, s, d, None, ref_threads=threads)
        depth, parent, it = g.bfs(1)
        od, op, oit, _ = ob.OracleGraph(nv, s, d, None, ref_threads=threads).bfs(1)
        assert it == oit and np.array_equal(depth, od) and np.array_equal(parent, op)
        assert depth.max() == 2 and (depth == 1).sum() == width


def test_fullscale_property_checker_agrees_with_oracle_regime():
    """The independent torch property checks used at RMAT-26 (tools/fullscale_checks.py) pass at a
    scale where the oracle parity is also tested (they must agree on what 'correct' means)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fullscale_checks.py"), "--scale", "16",
                          "--ref-threads", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and "ALL PASS" in out.stdout.decode(), out.stdout.decode()[-2000:]


@pytest.mark.parametrize("K,dtype,generic", [(20, np.float32, 0), (128, np.float32, 0), (128, np.float32, 1),
                                             (20, np.float64, 0)])
def test_sgd_synthetic_ratings(env, K, dtype, generic):
    """SGD / RMSE (3-operand multiply: process_message sees the destination's latent vector) on a
    synthetic bipartite ratings graph, incl. the K=128 fp32 shape of BASELINE config 5.
    Tolerance 1e-6 relative (north_star); the folds are in reference order, observed exact."""
    api, ob = env
    # K=128 fp32 has a dedicated kernel pair (gm_programs.hip k_sgd_*); generic=1 forces the same
    # program through the generic engine instead: both must equal the oracle
    api._lib.lib().gm_set_option(b"force_ordered", generic)
    rng = np.random.default_rng(7)
    nu, ni, nr = 300, 60, 4000
    s = rng.integers(1, nu + 1, nr).astype(np.int32)
    d = (nu + rng.integers(1, ni + 1, nr)).astype(np.int32)
    v = rng.integers(1, 6, nr).astype(np.int32)
    nv = nu + ni
    lv = rng.random((nv, K)).astype(dtype)
    g = api.Graph(nv, s, d, v, ref_threads=1)
    og = ob.OracleGraph(nv, s, d, v, 1)
    e0, sq0 = g.rmse_sum(lv)
    oe0, osq0 = og.rmse_sum(lv)
    np.testing.assert_allclose(sq0, osq0, rtol=1e-6, atol=0)
    assert abs(e0 - oe0) <= 1e-6 * abs(oe0)
    step = 1e-4 if dtype == np.float32 else 3.5e-7
    lv2, it = g.sgd(lv, 0.001, step, 3)
    olv2, oit = og.sgd(lv, 0.001, step, 3)
    assert it == oit == 3
    api._lib.lib().gm_set_option(b"force_ordered", 0)
    np.testing.assert_allclose(lv2, olv2, rtol=1e-6, atol=0)
    assert not np.array_equal(lv2, lv)
    if K == 128:
        assert np.array_equal(lv2, olv2), "K=128 fp32: folds are in reference order, expected bit-exact"


def test_sgd_k128_matrix_core_option_deviation_bound(env):
    """gm_set_option("sgd_mfma", 1): the dot products of the K = 128 fp32 SGD kernels on the matrix cores
    (k_sgd_multiply_mfma, v_mfma_f32_4x4x1_16b_f32).  A matrix instruction sums its four-term partial dots in its own order,
    so this form is NOT the reference's sequential K-term dot: it is an opt-in measurement form (it loses 1.6x to the vector
    form, profiles/r04_sgd_k128.md), outside north_star's 1e-6 bar by design.  This test states and pins its deviation:
    within 1e-4 of the oracle relative to the vectors' scale (measured: 1.1e-5 at 1e9 ratings; element-wise up to 8e-4 on components near zero), really different from
    the default form -- and the default form stays within 1e-6 (observed: bit-exact)."""
    api, ob = env
    L = api._lib.lib()
    rng = np.random.default_rng(11)
    nu, ni, nr, K = 400, 80, 6000, 128
    s = rng.integers(1, nu + 1, nr).astype(np.int32)
    d = (nu + rng.integers(1, ni + 1, nr)).astype(np.int32)
    v = rng.integers(1, 6, nr).astype(np.int32)
    nv = nu + ni
    lv = rng.random((nv, K)).astype(np.float32)
    og = ob.OracleGraph(nv, s, d, v, 1)
    olv, _ = og.sgd(lv, 0.001, 1e-4, 3)
    g = api.Graph(nv, s, d, v, ref_threads=1)
    try:
        api._lib.check(L.gm_set_option(b"sgd_mfma", 0))
        lv0, _ = g.sgd(lv, 0.001, 1e-4, 3)
        np.testing.assert_allclose(lv0, olv, rtol=1e-6, atol=0)
        api._lib.check(L.gm_set_option(b"sgd_mfma", 1))
        lv1, _ = g.sgd(lv, 0.001, 1e-4, 3)
    finally:
        L.gm_set_option(b"sgd_mfma", 0)
    # (components near zero make an element-wise relative error meaningless -- 8e-4 on a component of 1e-3: the bound is on the
    # deviation relative to the vector's scale, and element-wise on the components that are not tiny)
    scale_ = float(np.abs(olv).max())
    dev = float(np.abs(lv1 - olv).max()) / scale_
    assert dev <= 1e-4, dev
    # ... and it is not "the reference built with FMA" either: against the restatement compiled with the reference's own flags
    # (oracle/libgm_oracle_fma.so: fused multiply-adds, same summation order) the deviation is the same size, two orders of magnitude
    # above that build's own distance from the unfused one (tests/test_oracle_golden.py: 1.2e-7 of the scale)
    olv_f, _ = ob.OracleGraph(nv, s, d, v, 1, fused=True).sgd(lv, 0.001, 1e-4, 3)
    dev_f = float(np.abs(lv1 - olv_f).max()) / scale_
    spread = float(np.abs(olv_f - olv).max()) / scale_
    print("sgd_mfma: %.3g of the scale from the unfused oracle, %.3g from the fused one; the two oracles are %.3g apart" % (dev, dev_f, spread))
    assert dev_f <= 1e-4 and spread <= 1e-6
    big = np.abs(olv) >= 1e-2 * scale_
    rel = np.abs(lv1 - olv)[big] / np.abs(olv)[big]
    assert float(rel.max()) <= 2e-3, float(rel.max())
    assert not np.array_equal(lv1, lv)  # (it ran)
    g.close()


def test_config2_rmat22_against_oracle(env):
    """BASELINE config 2 at full size: PageRank on RMAT-22 (67 M edges), bit-exact fp32 against the
    oracle (fixed count and until convergence), plus BFS depth/parent.  The edges come from the
    device generator (bit-identical to the numpy one, tested above)."""
    api, ob = env
    nv, src, dst, _ = api.rmat_on_device(22, 16, 1)
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    ob.lib().gmo_set_num_threads(16)
    og = ob.OracleGraph(nv, s, d, None, ref_threads=1)
    g = api.Graph(nv, src, dst, None, ref_threads=1, keep_values=False)
    del src, dst
    pr, deg, it = g.pagerank(10)
    odeg = og.degree()
    opr, oit, _ = og.pagerank(10, degree=odeg)
    assert (deg == odeg).all() and it == oit == 10
    assert (f32bits(pr) == f32bits(opr)).all(), "RMAT-22 PageRank differs from the oracle"
    pr, deg, it = g.pagerank(-1)
    opr, oit, _ = og.pagerank(-1, degree=odeg)
    assert it == oit, "until-convergence iteration count differs (%d vs %d)" % (it, oit)
    assert (f32bits(pr) == f32bits(opr)).all()
    depth, parent, it = g.bfs(1)
    od, op, oit, _ = og.bfs(1)
    assert it == oit and (depth == od).all() and (parent == op).all()
    # the same configuration on the COLUMN-TILED multiply (what bench.py times at RMAT-26, where the tile count
    # is chosen automatically): forced 4 and 6 tiles against the same oracle result, bit for bit
    opr, oit, _ = og.pagerank(10, degree=odeg)
    g.close()
    for tiles in (4, 6):
        nv, src, dst, _ = api.rmat_on_device(22, 16, 1)
        gt = api.Graph(nv, src, dst, None, ref_threads=1, keep_values=False, col_tiles=tiles)
        del src, dst
        assert gt.col_tiles == tiles
        pr, deg, it = gt.pagerank(10)
        assert (deg == odeg).all() and it == 10
        assert (f32bits(pr) == f32bits(opr)).all(), "RMAT-22 PageRank with %d column tiles differs from the oracle" % tiles
        gt.close()


@pytest.mark.timeout(900)
def test_fullscale_pagerank_rmat26_tiled_equals_untiled():
    """The headline configuration (PageRank on RMAT-26) runs on automatically chosen column tiles; the CPU oracle
    cannot hold 1.07 G edges.  This ties the timed path to the oracle-tested one: 10 iterations on the automatic
    tiling and on the untiled graph (col_tiles=1) must leave bit-identical vertex state
    (tools/fullscale_checks.py --tiled-vs-untiled; the untiled kernels are the ones compared with the oracle at
    RMAT-10..22, the forced-tile ones at RMAT-10..22 above and in test_gpu_tiles.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fullscale_checks.py"), "--scale", "26",
                          "--tiled-vs-untiled", "10"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=850)
    text = out.stdout.decode()
    assert out.returncode == 0 and "TILED == UNTILED" in text, text[-3000:]


def test_sgd_with_giant_rows(env):
    """3-operand ordered fold on rows longer than the giant threshold (two items rated by thousands
    of users): such rows of a plain REDUCE_ORDERED program take the wave kernel."""
    api, ob = env
    rng = np.random.default_rng(11)
    nu, ni, nr = 9000, 2, 14000
    s = rng.integers(1, nu + 1, nr).astype(np.int32)
    d = (nu + rng.integers(1, ni + 1, nr)).astype(np.int32)
    v = rng.integers(1, 6, nr).astype(np.int32)
    nv = nu + ni
    lv = rng.random((nv, 20)).astype(np.float64)
    g = api.Graph(nv, s, d, v)
    c = g.csr(api.GM_DIR_OUT)
    assert c.ngiant >= 2
    og = ob.OracleGraph(nv, s, d, v, 1)
    lv2, it = g.sgd(lv, 0.001, 3.5e-7, 2)
    olv2, oit = og.sgd(lv, 0.001, 3.5e-7, 2)
    np.testing.assert_allclose(lv2, olv2, rtol=1e-6, atol=0)
    e, sq = g.rmse_sum(lv2)
    oe, osq = og.rmse_sum(olv2)
    np.testing.assert_allclose(sq, osq, rtol=1e-6, atol=0)


def test_edge_ids_are_validated(env):
    """ids outside 1..nvertices would index device arrays out of bounds: GM_ERR_INVALID with a message
    (the reference asserts this only in __DEBUG builds, include/GMDP/utils/edgelist.h)."""
    api, _ = env
    for s, d in (([0, 1, 2], [1, 2, 3]), ([1, 2, 3], [2, 3, 9]), ([1, -4, 3], [2, 3, 1])):
        with pytest.raises(RuntimeError, match="outside"):
            api.Graph(8, np.array(s, np.int32), np.array(d, np.int32), None)
    g = api.Graph(8, np.array([1, 8], np.int32), np.array([8, 1], np.int32), None)  # the extremes are fine
    assert g.nnz_input == 2


@pytest.mark.timeout(900)
def test_fullscale_bfs_parents_rmat26():
    """BASELINE config 3 at its full size: BFS on RMAT-26 (1.07 G edges); depth and EVERY parent are checked
    against the defining properties of the reference's result (BFS levels; parent = the previous-level
    in-neighbour with the largest native id), evaluated independently with torch on the edge list
    (tools/fullscale_checks.py), together with PageRank's degree pass and run-to-run reproducibility."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fullscale_checks.py"), "--scale", "26"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=850)
    text = out.stdout.decode()
    assert out.returncode == 0 and "ALL PASS" in text, text[-3000:]
    assert text.count("=> PASS") >= 3


def test_mapreduce_closed_forms_device(env):
    """test/test_reduce.cpp:39-65 on the C-ABI reductions (the device side of MapReduce, include/GMDP/singlenode/
    reduce.h:51-99): 1000 doubled ones sum to 2000; a segment with entries 1, 10, 200, 300 set has 4 present entries."""
    import ctypes as C
    import torch
    api, _ = env
    L = api._lib.lib()
    x = torch.full((1000,), 2.0, dtype=torch.float32, device="cuda")
    out = C.c_double(0)
    api._lib.check(L.gm_reduce_sum_f32(x.data_ptr(), 1000, 1, C.byref(out), None))
    assert out.value == 2000.0
    xd = torch.full((1000, 3), 2.0, dtype=torch.float64, device="cuda")  # strided: one field of a wider record
    api._lib.check(L.gm_reduce_sum_f64(xd.data_ptr(), 1000, 3, C.byref(out), None))
    assert out.value == 2000.0
    bits = torch.zeros(34, dtype=torch.int32, device="cuda")
    for i in (0, 9, 199, 299):
        bits[i >> 5] |= 1 << (i & 31)
    cnt = C.c_int64(0)
    api._lib.check(L.gm_popcount_bits(bits.data_ptr(), 1000, C.byref(cnt), None))
    assert cnt.value == 4

"""The short rows' fold that also applies and sends (kernels.hpp: k_short_fold, FUSED; engine.hpp: multiply_out_swept / step_pull).

In a fixed-count run of a program without an iteration hook the fold behind the sweep applies the row it has just folded and writes the next
iteration's message; the sweep's and the giant rows get a masked apply + send pass (k_apply_send_masked), rows without in-edges are not visited
again.  Note 7 of the graph counts the multiplies of the last run that took the path; sweep_form bit 9 (512) refuses it.  Every PageRank
comparison is on fp32 bits against the oracle.  All cases force the stream path on small graphs the way test_short_rows_ride_the_sweep does
(sweep_form bit 8, sweep_long_row 256).  Needs an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphmat_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


_cache = {}


def _rmat(ob, scale, keep):
    """the RMAT input and its oracle graph, made once per (scale, values)"""
    key = (scale, keep)
    if key not in _cache:
        nv, s, d, v = gen.rmat_edges(scale, 16, 11, weights="hash")
        og = ob.OracleGraph(nv, s, d, v if keep else None, ref_threads=1)
        _cache[key] = (nv, s, d, v, og, {})
    return _cache[key]


def _oracle_pr(entry, iterations):
    og, memo = entry[4], entry[5]
    if iterations not in memo:
        memo[iterations] = og.pagerank(iterations)[:2]
    return memo[iterations]


def _note(L, g, slot):
    v = C.c_int64(-1)
    assert L.gm_graph_note_get(g.h, slot, C.byref(v)) == 0, "note %d was never set" % slot
    return v.value


def _force_stream_path(api, L, form=256):
    api._lib.check(L.gm_reset_options())
    api._lib.check(L.gm_set_option(b"sweep_long_row", 256))
    api._lib.check(L.gm_set_option(b"sweep_form", form))


@pytest.mark.parametrize("scale,tiles", [(13, 2), (16, 4)])
@pytest.mark.parametrize("keep", [False, True])
def test_rmat_through_the_fused_fold(env, scale, tiles, keep):
    """7 iterations: the oracle's bits, six multiplies through the fused fold (note 7) of seven through the fold (note 4); refused by
    sweep_form bit 9 on the same graph: the same bits, note 7 reads 0."""
    api, ob = env
    L = api._lib.lib()
    entry = _rmat(ob, scale, keep)
    nv, s, d, v = entry[:4]
    opr, oit = _oracle_pr(entry, 7)
    try:
        _force_stream_path(api, L)
        g = api.Graph(nv, s, d, v if keep else None, ref_threads=1, keep_values=keep, col_tiles=tiles)
        pr, _, it = g.pagerank(7)
        assert it == oit == 7 and (f32bits(pr) == f32bits(opr)).all()
        assert _note(L, g, 7) == 6 and _note(L, g, 4) == 7
        pr, _, it = g.pagerank(7)  # (a second run on the same graph: the rest mask is reused)
        assert it == 7 and (f32bits(pr) == f32bits(opr)).all() and _note(L, g, 7) == 6
        api._lib.check(L.gm_set_option(b"sweep_form", 256 | 512))
        pr2, _, it2 = g.pagerank(7)
        assert it2 == 7 and (f32bits(pr2) == f32bits(opr)).all()
        assert _note(L, g, 7) == 0 and _note(L, g, 4) == 7
        g.close()
    finally:
        api._lib.check(L.gm_reset_options())


def test_hand_over_to_the_last_plain_iteration(env):
    """1 and 2 iterations (note 7 reads 0 and 1: the last iteration of a run always takes the plain fold and the plain apply), and a run until
    convergence, which never takes the path."""
    api, ob = env
    L = api._lib.lib()
    entry = _rmat(ob, 13, False)
    nv, s, d, v, og = entry[:5]
    try:
        _force_stream_path(api, L)
        g = api.Graph(nv, s, d, None, ref_threads=1, keep_values=False, col_tiles=2)
        for iters, fused in ((1, 0), (2, 1)):
            opr, oit = _oracle_pr(entry, iters)
            pr, _, it = g.pagerank(iters)
            assert it == oit == iters and (f32bits(pr) == f32bits(opr)).all(), iters
            assert _note(L, g, 7) == fused and _note(L, g, 4) == iters
        opr, oit = _oracle_pr(entry, -1)
        pr, _, it = g.pagerank(-1)
        assert it == oit and (f32bits(pr) == f32bits(opr)).all()
        assert _note(L, g, 7) == 0 and _note(L, g, 4) == it
        g.close()
    finally:
        api._lib.check(L.gm_reset_options())


def test_several_sweep_launches_in_front_of_the_fused_fold(env):
    """sweep_acc_rows 2 / sweep_long_slots 1 on RMAT-16: the sweep takes several launches, all of them in front of the fold that overwrites x"""
    api, ob = env
    L = api._lib.lib()
    entry = _rmat(ob, 16, False)
    nv, s, d, v = entry[:4]
    opr, oit = _oracle_pr(entry, 7)
    try:
        _force_stream_path(api, L)
        api._lib.check(L.gm_set_option(b"sweep_acc_rows", 2))
        api._lib.check(L.gm_set_option(b"sweep_long_slots", 1))
        g = api.Graph(nv, s, d, None, ref_threads=1, keep_values=False, col_tiles=3)
        sw = api._lib.Sweep()
        assert L.gm_graph_sweep(g.h, C.byref(sw)) == 0 and sw.nsets > 1
        pr, _, it = g.pagerank(7)
        assert it == oit == 7 and (f32bits(pr) == f32bits(opr)).all()
        assert _note(L, g, 7) == 6 and _note(L, g, 4) == 7
        g.close()
    finally:
        api._lib.check(L.gm_reset_options())


def test_many_row_bins_and_rows_nobody_visits(env):
    """RMAT-13 plus a chain of 40 000 vertices with one in-edge each -- bins of thousands of 1-edge rows (more than a full bin's 12 288 products
    of them): a thread folds a row in each of many rounds, far past the rounds requested before the loop -- plus 3 000 vertices with an out-edge into the RMAT part and no in-edge: live rows that no kernel touches
    after the run's first send."""
    api, ob = env
    L = api._lib.lib()
    nv0, s0, d0, _ = gen.rmat_edges(13, 16, 11, weights="hash")
    nchain, nsrc = 40000, 3000
    chain = np.arange(nv0 + 1, nv0 + nchain + 1, dtype=np.int64)
    cs = np.concatenate([[1], chain[:-1]])  # vertex 1 -> first chain vertex -> second -> ...
    srcs = np.arange(nv0 + nchain + 1, nv0 + nchain + nsrc + 1, dtype=np.int64)
    sd = 1 + (np.arange(nsrc, dtype=np.int64) * 7919) % nv0
    s = np.concatenate([np.asarray(s0, np.int64), cs, srcs]).astype(np.int32)
    d = np.concatenate([np.asarray(d0, np.int64), chain, sd]).astype(np.int32)
    nv = nv0 + nchain + nsrc
    og = ob.OracleGraph(nv, s, d, None, ref_threads=1)
    opr, oit, _ = og.pagerank(7)
    odeg = og.degree()
    try:
        _force_stream_path(api, L)
        g = api.Graph(nv, s, d, None, ref_threads=1, keep_values=False, col_tiles=2)
        sw = api._lib.Sweep()
        assert L.gm_graph_sweep(g.h, C.byref(sw)) == 0 and sw.nstream > 0 and sw.nbins > 0
        binrow = np.zeros(sw.nbins + 1, np.uint32)
        api.copy_from_device(binrow, sw.sbin_row)
        rows_per_bin = np.diff(binrow.astype(np.int64))
        if not (rows_per_bin > 2048).any():
            pytest.skip("no bin of more than 2048 rows (largest: %d): the shape does not reach the rounds past the first requests" % int(rows_per_bin.max()))
        pr, deg, it = g.pagerank(7)
        assert it == oit == 7 and (f32bits(pr) == f32bits(opr)).all()
        assert (np.asarray(deg, np.int64) == np.asarray(odeg, np.int64)).all()
        assert _note(L, g, 7) == 6 and _note(L, g, 4) == 7
        api._lib.check(L.gm_set_option(b"sweep_form", 256 | 512))  # the plain fold walks the same bins
        pr2, deg2, _ = g.pagerank(7)
        assert (f32bits(pr2) == f32bits(opr)).all() and (np.asarray(deg2, np.int64) == np.asarray(odeg, np.int64)).all() and _note(L, g, 7) == 0
        g.close()
    finally:
        api._lib.check(L.gm_reset_options())


def test_programs_with_an_iteration_hook_keep_the_plain_path(env):
    """apps/mutating_program.cpp (programs whose do_every_iteration changes what send_message computes) under the forcing options still passes
    its three fuse_apply_send lines (GRAPHMAT_OPTIONS carries engine options only: sweep_form).  Its messages are doubles, which the sweep does not take, so options alone cannot bring it onto the swept
    path; the C-ABI's program with a hook of its own, BFS, runs on the graph of the first case under the same options: the oracle's result,
    note 7 reads 0."""
    api, ob = env
    L = api._lib.lib()
    exe = os.path.join(ROOT, "build", "apps", "mutating_program")
    assert os.path.exists(exe), "build/apps/mutating_program is missing: tools/build_apps.py makes it"
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                       env=dict(os.environ, GRAPHMAT_OPTIONS="sweep_form=256"))
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "MUTATING PASS" in text, text[-2000:]
    assert "fuse_apply_send=1: steady ok, every-time ok, sometimes ok" in text and "fuse_apply_send=0: steady ok, every-time ok, sometimes ok" in text
    entry = _rmat(ob, 13, False)
    nv, s, d, v, og = entry[:5]
    od, op, oit, _ = og.bfs(1)
    try:
        _force_stream_path(api, L)
        g = api.Graph(nv, s, d, None, ref_threads=1, keep_values=False, col_tiles=2)
        depth, parent, it = g.bfs(1)
        assert it == oit and (depth == od).all() and (parent == op).all()
        assert _note(L, g, 7) == 0
        g.close()
    finally:
        api._lib.check(L.gm_reset_options())

#!/usr/bin/env python3
"""Digest of everything the graph build lays out in HBM, for a fixed list of small graphs and option settings: one JSON line per
case with the scalar fields of gm_csr_t (both directions and every column tile), gm_sweep_t and gm_blocked_t and a sha256 of every
device array over its documented extent (include/graphmat_hip.h; padding behind it is not hashed -- some of it is never written).
Two builds of the library lay a graph out identically iff their outputs are equal:

    python tools/layout_digest.py > digest.jsonl          # every case
    python tools/layout_digest.py 3 7a                    # some of them
"""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphmat_amd import _lib, api  # noqa: E402
from graphmat_amd import generators as gen  # noqa: E402


def sha(ptr, count, dtype):
    """sha256 of `count` items of `dtype` at device pointer `ptr` (None: no such array)"""
    if not ptr or count <= 0:
        return None
    h = np.zeros(int(count), dtype)
    api.copy_from_device(h, ptr)
    return hashlib.sha256(h.tobytes()).hexdigest()


def scalars(st):
    return {n: getattr(st, n) for n, t in st._fields_ if t is not C.c_void_p}


def csr_digest(c, prev=None):
    words = (c.nrows + 31) // 32
    out = scalars(c)
    out["sha"] = {
        "rowptr": sha(c.rowptr, c.nrows + 1, np.int64), "colidx": sha(c.colidx, c.nnz, np.int32), "vals": sha(c.vals, c.nnz * c.val_bytes, np.uint8),
        "rowbits": sha(c.rowbits, words, np.uint32), "seg_row": sha(c.seg_row, c.nseg + 1, np.int32), "blk_seg": sha(c.blk_seg, c.nblk, np.int32),
        "mid_row": sha(c.mid_row, c.nmid, np.int32), "giant_row": sha(c.giant_row, c.ngiant, np.int32), "gchunk_row": sha(c.gchunk_row, c.ngchunk, np.int32),
        "gchunk_edge": sha(c.gchunk_edge, c.ngchunk, np.int64), "gterm_off": sha(c.gterm_off, c.ngiant + 1, np.int64), "umid_row": sha(c.umid_row, c.numid, np.int32),
        "prev_bits": sha(prev, words, np.uint32)}
    return out


def sweep_digest(sw):
    nblk = sw.nsets * 256 * sw.nslices
    v = sw.val_bytes == 4
    out = scalars(sw)
    out["sha"] = {
        "slice_base": sha(sw.slice_base, sw.nslices + 1, np.int32),
        "scol": sha(sw.scol, sw.nentries, np.uint32), "sval": sha(sw.sval, sw.nentries if v else 0, np.uint32), "src_pos": sha(sw.src_pos, sw.nentries, np.uint32),
        "gbase": sha(sw.gbase, sw.ngroups + 1, np.uint32), "wrow": sha(sw.wrow, nblk * 17, np.uint32), "wfirst": sha(sw.wfirst, nblk * 17, np.uint32),
        "row_of_slot": sha(sw.row_of_slot, sw.nsets * 256 * sw.acc_rows, np.int32), "lrow_of_slot": sha(sw.lrow_of_slot, sw.nsets * 256 * sw.long_slots, np.int32),
        "lcol": sha(sw.lcol, sw.nedges_long, np.uint32), "lval": sha(sw.lval, sw.nedges_long if v else 0, np.uint32), "lsrc_pos": sha(sw.lsrc_pos, sw.nedges_long, np.uint32),
        "lps": sha(sw.lps, nblk * sw.long_slots + 1, np.uint32),
        "gcol": sha(sw.gcol, sw.ngiant_edges, np.uint32), "gval": sha(sw.gval, sw.ngiant_edges if v else 0, np.uint32), "gdst": sha(sw.gdst, sw.ngiant_edges, np.uint32),
        "gslice": sha(sw.gslice, sw.nslices + 1, np.uint32), "gsrc_pos": sha(sw.gsrc_pos, sw.ngiant_edges, np.uint32),
        "srow": sha(sw.srow, sw.nshort_rows, np.int32), "soff": sha(sw.soff, sw.nshort_rows + 1, np.uint32), "sbin_row": sha(sw.sbin_row, sw.nbins + 1, np.uint32),
        "schunk": sha(sw.schunk, sw.nbins * sw.nslices * 2, np.uint32), "sinv": sha(sw.sinv, sw.nstream_slots, np.uint16),
        "wrow_stream": sha(sw.wrow_stream, nblk * 17, np.uint32)}
    return out


def blocked_digest(bl):
    v = bl.val_bytes == 4
    out = scalars(bl)
    out["sha"] = {
        "ecol": sha(bl.ecol, bl.nentries, np.uint32), "erow": sha(bl.erow, bl.nentries, np.uint16), "woff": sha(bl.woff, bl.nblocks * bl.nslices * 17, np.uint32),
        "row_of": sha(bl.row_of, bl.nblocks * 32768, np.int32), "step_count": sha(bl.step_count, 8 * bl.nsteps, np.uint32),
        "eval": sha(bl.eval, bl.nentries if v else 0, np.uint32), "epos": sha(bl.epos, bl.nentries if v else 0, np.uint32)}
    return out


def graph_digest(g):
    L = g.L
    out = {"desc": {"row_lo": g.row_lo, "row_hi": g.row_hi, "ndevice": g.ndevice, "xchg_rows": g.xchg_rows, "col_tiles": g.col_tiles}}
    don, nod = C.c_void_p(), C.c_void_p()
    _lib.check(L.gm_graph_maps(g.h, C.byref(don), C.byref(nod)))
    out["maps"] = {"dev_of_native": sha(don.value, g.nv, np.int32), "native_of_dev": sha(nod.value, g.ndevice, np.int32)}
    out["out"] = csr_digest(g.csr(api.GM_DIR_OUT))
    out["in"] = csr_digest(g.csr(api.GM_DIR_IN))
    nt = C.c_int(0)
    _lib.check(L.gm_graph_tiles(g.h, api.GM_DIR_OUT, C.byref(nt)))
    out["tiles"] = [csr_digest(*g.tile(api.GM_DIR_OUT, t)) for t in range(nt.value)] if nt.value > 1 else []
    sw, bl = _lib.Sweep(), _lib.Blocked()
    _lib.check(L.gm_graph_sweep(g.h, C.byref(sw)))
    _lib.check(L.gm_graph_blocked(g.h, C.byref(bl)))
    out["sweep"] = sweep_digest(sw)
    out["blocked"] = blocked_digest(bl)
    return out, sw, bl


@functools.lru_cache(maxsize=None)
def rmat(scale):
    return gen.rmat_edges(scale, 16, 11, weights="hash")


def build(edges, opts=(), keep=False, **kw):
    L = _lib.lib()
    for k, val in opts:
        _lib.check(L.gm_set_option(k.encode(), val))
    nv, s, d, v = edges
    return api.Graph(nv, s, d, v if keep else None, keep_values=keep, **kw)


def plain(make_edges, scale, opts=(), keep=False, expect=None, **kw):
    def run():
        g = build(make_edges(scale), opts, keep, **kw)
        dig, sw, bl = graph_digest(g)
        assert expect is None or expect(g, sw, bl), "the case no longer covers what it is listed for"
        g.close()
        return dig
    return run


def case_giant():
    """RMAT-15 with values, giant_row lowered until the sweep carries giant edges"""
    for limit in (4096, 2048, 1024, 512, 256, 128, 64):
        g = build(rmat(15), [("giant_row", limit)], True, col_tiles=3)
        dig, sw, _ = graph_digest(g)
        ngiant = g.csr(api.GM_DIR_OUT).ngiant
        g.close()
        if ngiant > 0 and sw.ngiant_edges > 0:
            dig["giant_row_option"] = limit
            return dig
    raise SystemExit("case 6: no giant_row setting gives the sweep giant edges")


def case_refresh():
    """the graph of case 2 after gm_graph_set_vals with permuted values, then gm_graph_sync_tile_vals"""
    g = build(rmat(15), [("sweep_long_row", 256)], True, col_tiles=3, ref_threads=2)
    _, _, vv = g.csr_to_host(api.GM_DIR_OUT)
    new = np.ascontiguousarray(vv[np.random.default_rng(5).permutation(len(vv))], np.int32)
    _lib.check(g.L.gm_graph_set_vals(g.h, api.GM_DIR_OUT, new.ctypes.data_as(C.c_void_p)))
    _lib.check(g.L.gm_graph_sync_tile_vals(g.h, None))
    dig, sw, _ = graph_digest(g)
    assert sw.src_pos and sw.lsrc_pos
    g.close()
    return dig


@functools.lru_cache(maxsize=None)
def uniform(scale):
    return gen.uniform_out_regular_edges(1 << scale, 16, seed=3)


CASES = {
    "1": plain(rmat, 13, col_tiles=2, ref_threads=1, expect=lambda g, sw, bl: sw.nrows > 0),
    "2": plain(rmat, 15, [("sweep_long_row", 256)], True, col_tiles=3, ref_threads=2, expect=lambda g, sw, bl: sw.src_pos and sw.lsrc_pos and sw.nrows_long > 0),
    "3": plain(rmat, 16, [("sweep_long_row", 256), ("sweep_acc_rows", 2), ("sweep_long_slots", 1)], col_tiles=3, ref_threads=1, expect=lambda g, sw, bl: sw.nsets > 1),
    "4": plain(rmat, 16, [("sweep_stream", 0)], col_tiles=4, expect=lambda g, sw, bl: sw.nrows > 0 and sw.nstream == 0),
    "5": plain(rmat, 16, [("sweep_waves", 12)], col_tiles=3, expect=lambda g, sw, bl: sw.waves == 12),
    "6": case_giant,
    "7a": plain(uniform, 14, [("blocked_rows", 1)], False, col_tiles=3, ref_threads=1, expect=lambda g, sw, bl: bl.nrows > 0 and bl.val_bytes == 0),
    "7b": plain(uniform, 15, [("blocked_rows", 1)], True, col_tiles=2, ref_threads=1, expect=lambda g, sw, bl: bl.nrows > 0 and bl.val_bytes == 4),
    "8": case_refresh,
    "9": plain(rmat, 15, keep=False, nshards=2, shard=0, col_tiles=3, expect=lambda g, sw, bl: sw.nsub == 2 and sw.nrows > 0),
    "10": plain(rmat, 13, col_tiles=1, expect=lambda g, sw, bl: g.col_tiles == 1 and sw.nslices == 0),
}


def main():
    L = _lib.lib()
    for name in (sys.argv[1:] or list(CASES)):
        try:
            _lib.check(L.gm_reset_options())
            dig = CASES[name]()
        finally:
            _lib.check(L.gm_reset_options())
        print(json.dumps({"case": name, **dig}, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()

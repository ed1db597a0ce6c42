#!/usr/bin/env python3
"""Which kernels does a swept multiply launch, and in which order?  One small configuration per process, to be run under
`rocprofv3 --kernel-trace`; two builds of the library schedule the swept multiply alike iff their listings are equal.

    rocprofv3 --kernel-trace -d out/form0 -- python tools/swept_dispatches.py run form0
    python tools/swept_dispatches.py list out/form0 > form0.txt      # every dispatch of the run as `queue kernel grid workgroup`

`run sharded` wants two ranks (python -m torch.distributed.run --nproc-per-node 2) and GRAPHMAT_RCCL_LIBRARY naming the test
suite's shared-memory transport.  All configurations: RMAT-16 with edge factor 16 (the uniform 2^14 graph for `blocked`),
sweep_long_row=256, 4 column tiles, PageRank with 3 iterations (`sssp`: the library's SSSP from vertex 1, every step a pull)."""
import ctypes as C
import glob
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#          options on top of sweep_long_row=256
CONFIGS = {
    "form0": [("sweep_form", 0)], "form1": [("sweep_form", 1)], "form2": [("sweep_form", 2)],
    "form3": [("sweep_form", 3)], "form11": [("sweep_form", 11)],  # (bits 0-1 = 3: taken as 0)
    "form9": [("sweep_form", 9)], "form10": [("sweep_form", 10)],  # (bit 3: the giant rows leave the placement to bits 0-1)
    "giant_form0": [("giant_row", 4096), ("sweep_form", 0)], "giant_form8": [("giant_row", 4096), ("sweep_form", 8)],
    "giant_form16": [("giant_row", 4096), ("sweep_form", 16)],
    "waves12": [("sweep_waves", 12)], "waves12_giant": [("sweep_waves", 12), ("giant_row", 4096)],
    "stream": [("sweep_form", 256)], "stream_plain_fold": [("sweep_form", 256 | 512)],
    "sssp": [("sweep_form", 64), ("debug_flags", 32)],
    "blocked": [("blocked_rows", 1)],  # (the uniform graph: no swept rows, multiply_out_blocked)
    "blocked_swept": [("blocked_rows", 1)],  # (RMAT: the column-blocked stream behind the sweep)
    "sharded": [("sweep_form", 256)],
}


def run(name):
    from graphmat_amd import _lib, api
    from graphmat_amd import generators as gen
    L = _lib.lib()
    _lib.check(L.gm_reset_options())
    for k, v in [("sweep_long_row", 256)] + CONFIGS[name]:
        _lib.check(L.gm_set_option(k.encode(), v))
    if name == "blocked":
        nv, s, d, v = gen.uniform_out_regular_edges(1 << 14, 16, seed=3)
    else:
        nv, s, d, v = gen.rmat_edges(16, 16, 5, weights="hash")
    kw = {}
    if name == "sharded":
        import torch
        import torch.distributed as dist
        from graphmat_amd.dist import attach_native_exchange, init_native_rccl
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        init_native_rccl(device=torch.device("cuda", 0))
        kw = dict(device=0, nshards=world, shard=rank)
    keep = name == "sssp"
    g = api.Graph(nv, s, d, v if keep else None, keep_values=keep, col_tiles=4, **kw)
    if name == "sharded":
        attach_native_exchange(g)
    if name == "sssp":
        _, it = g.sssp(1)
    else:
        _, _, it = g.pagerank(3)
    sw, bl = _lib.Sweep(), _lib.Blocked()
    _lib.check(L.gm_graph_sweep(g.h, C.byref(sw)))
    _lib.check(L.gm_graph_blocked(g.h, C.byref(bl)))
    notes = {}
    for note in ("GM_NOTE_SPARSE_SWEEPS", "GM_NOTE_SHORT_FOLDS", "GM_NOTE_FOLD_APPLIES"):
        n = C.c_int64(-1)
        L.gm_graph_note_get(g.h, getattr(_lib, note), C.byref(n))
        notes[note] = n.value
    print("%s: %d iterations, %d multiply launches; sweep rows %d (long %d) sets %d waves %d nsub %d stream edges %d giant edges %d; giant rows %d; blocked rows %d; %s"
          % (name, it, g.last_stats()["spmv_launches"], sw.nrows, sw.nrows_long, sw.nsets, sw.waves, sw.nsub, sw.nstream, sw.ngiant_edges, g.csr(api.GM_DIR_OUT).ngiant,
             bl.nrows, notes), flush=True)
    g.close()
    _lib.check(L.gm_reset_options())
    if name == "sharded":
        dist.destroy_process_group()


def listing(db_path):
    db = sqlite3.connect(db_path)
    tables = [n for (n,) in db.execute("select name from sqlite_master where type='table'")]
    kd = next((n for n in tables if n.startswith("rocpd_kernel_dispatch")), None)
    ks = next((n for n in tables if n.startswith("rocpd_info_kernel_symbol")), None)
    if kd is None or ks is None:  # (a process that launched nothing, such as the launcher of the ranks)
        return ""
    rows = db.execute("select d.queue_id, s.kernel_name, d.grid_size_x, d.grid_size_y, d.grid_size_z, d.workgroup_size_x, d.workgroup_size_y, d.workgroup_size_z "
                      "from %s d join %s s on d.kernel_id = s.id order by d.dispatch_id" % (kd, ks)).fetchall()
    queues = {}  # (a queue's id differs from run to run: queues are numbered by their first dispatch)
    per_queue = {}
    for q, name, *dims in rows:
        k = queues.setdefault(q, len(queues))
        per_queue.setdefault(k, []).append("q%d %s grid %dx%dx%d workgroup %dx%dx%d" % ((k, name) + tuple(dims)))
    return "\n".join(line for k in sorted(per_queue) for line in per_queue[k]) + "\n"


def main():
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:  # one process, one database; the listings of a run's processes in an order that does not depend on their ids
        dbs = sorted(glob.glob(os.path.join(sys.argv[2], "**", "*.db"), recursive=True))
        assert dbs, "no rocprofv3 database under " + sys.argv[2]
        for text in sorted(listing(p) for p in dbs):
            if text.strip():
                sys.stdout.write("---- a process: %d dispatches\n%s" % (text.count("\n"), text))


if __name__ == "__main__":
    main()

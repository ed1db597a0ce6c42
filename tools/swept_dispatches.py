#!/usr/bin/env python3
"""Which kernels does a run launch, and in which order?  One small configuration per process, to be run under
`rocprofv3 --kernel-trace`; two builds of the library schedule a configuration alike iff their listings are equal.  The first
group of configurations pins the swept multiply, the others the iteration loop around it (engine.hpp: run_loop, step_pull, the
two sharded schedules).

    rocprofv3 --kernel-trace -d out/form0 -- python tools/swept_dispatches.py run form0
    python tools/swept_dispatches.py list out/form0 > form0.txt      # every dispatch of the run as `queue kernel grid workgroup`

The configurations in SHARDED want two ranks (python -m torch.distributed.run --nproc-per-node 2) and GRAPHMAT_RCCL_LIBRARY
naming the test suite's shared-memory transport; with GM_EXCHANGE=callback they run over the torch.distributed callback
instead and print every exchange call (kind, element bytes, the two host words handed in), which a trace does not show.
`app NAME` starts a program of build/apps as a child process on a graph written for it (the child is what the trace sees).
Unless said otherwise: RMAT-16 with edge factor 16, sweep_long_row=256, 4 column tiles, PageRank with 3 iterations.
Every run prints the graph's notes (3, 4, 7: sweeps of a sparse x, short folds, fused folds; 5, 6: the step kinds) and the
multiply launches; GRAPHMAT_VERBOSE=1 adds the engine's own lines."""
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
    "sharded": [("sweep_form", 256)],  # run_swept_sharded
    # ---- the iteration loop: fused-pass and path variants of fixed-count PageRank
    "pr_nofuse": [("fuse_apply_send", 0)], "pr_trace": [("iteration_trace", 1)],
    "pr_tiled": [("debug_flags", 16)],  # (no auxiliary stream: the sweep is not taken, the column tiles are)
    "pr_csr": [],                       # (no column tiles: the whole-graph CSR's kernels)
    # ---- the library's BFS (a = b, lazy send) and SSSP (commutative) until convergence
    "bfs": [], "bfs_push": [("push_edge_permille", 1000), ("sparse_step_edges", 4096)],  # pulls and lists / lists and dense pushes
    "bfs_bits": [],  # the layered graph: 1 -> 70000 middle vertices (one of out-degree 64) -> leaves: a pull, then bits pushes
    "sssp_lists": [("push_edge_permille", 1000), ("sparse_step_edges", 0x7FFFFFFF)],
    # ---- ALL_EDGES over every vertex (the generic SGD, K = 20 doubles, 2 iterations, RMAT-12)
    "sgd": [],
    # ---- two ranks
    "two_stage": [],   # an unsliced layout: run_two_stage
    "sharded_bfs": [],  # ACTIVE_ONLY until convergence: the sparse exchange
}
SHARDED = ("sharded", "two_stage", "sharded_bfs")
#       program of build/apps, its arguments behind the graph, its environment; the graph: rmat SCALE | star
APPS = {
    "guided_list": ("untraited_programs", ["5", "2"], {"GRAPHMAT_OPTIONS": "guided_pull=2"}, "rmat 14"),
    "guided_bitmap": ("untraited_programs", ["1", "1"], {"GRAPHMAT_OPTIONS": "guided_pull=2"}, "star"),  # (70000 active vertices: marked from the bitmap)
    "label_propagation": ("label_propagation", [], {}, "rmat 12"),  # ALL_EDGES, ACTIVE_ONLY
    "bfs_bottom_up": ("bfs_bottom_up", ["3"], {}, "rmat 14"),       # a row filter
}


def layered(width, special_degree):
    """1 -> `width` middle vertices -> one leaf each; one middle vertex has special_degree out-edges"""
    import numpy as np
    rng = np.random.default_rng(width)
    mid = np.arange(2, 2 + width, dtype=np.int32)
    leaf = mid + width
    extra_s = np.full(special_degree - 1, mid[width // 3], np.int32)
    extra_d = rng.choice(leaf, special_degree - 1).astype(np.int32)
    return 1 + 2 * width, np.concatenate([np.full(width, 1, np.int32), mid, extra_s]), np.concatenate([mid, leaf, extra_d]), None


def star(width=70000, tails=1000):
    """1 -> `width` middle vertices, the first `tails` of them -> one leaf each; small edge values"""
    import numpy as np
    mid = np.arange(2, 2 + width, dtype=np.int32)
    s = np.concatenate([np.full(width, 1, np.int32), mid[:tails]])
    d = np.concatenate([mid, mid[:tails] + width])
    return 1 + width + tails, s, d, (1 + (np.arange(s.size, dtype=np.int64) * 7919) % 97).astype(np.int32)


def logged_exchange(g, ex, rank):
    """the callback exchange of g, every call printed by rank 0 before it is carried out"""
    from graphmat_amd import _lib
    names = {getattr(_lib, n): n for n in dir(_lib) if n.startswith("GM_XCHG_")}
    inner = ex.callback()
    count = [0]

    def fn(ctx, kind, d_ptr, elt_bytes, d_bits, h_flag):
        if rank == 0:
            words = (int(h_flag[0]), int(h_flag[1])) if h_flag and kind != _lib.GM_XCHG_CONVERGED else (int(h_flag[0]),) if h_flag else ()
            print("exchange %d: %s elt %d words %s" % (count[0], names.get(kind, kind), int(elt_bytes), words), flush=True)
        count[0] += 1
        return inner(ctx, kind, d_ptr, elt_bytes, d_bits, h_flag)
    cb = _lib.EXCHANGE_FN(fn)
    g._cb = (cb, inner, ex)  # keep alive
    _lib.check(_lib.lib().gm_graph_set_exchange(g.h, cb, None))
    _lib.check(_lib.lib().gm_graph_set_exchange_caps(g.h, _lib.GM_XCAP_SPARSE))  # (a new callback starts without capabilities)


def run(name):
    from graphmat_amd import _lib, api
    from graphmat_amd import generators as gen
    L = _lib.lib()
    _lib.check(L.gm_reset_options())
    for k, v in [("sweep_long_row", 256)] + CONFIGS[name]:
        _lib.check(L.gm_set_option(k.encode(), v))
    if name == "blocked":
        nv, s, d, v = gen.uniform_out_regular_edges(1 << 14, 16, seed=3)
    elif name == "bfs_bits":
        nv, s, d, v = layered(70000, 64)
    else:
        nv, s, d, v = gen.rmat_edges(12 if name == "sgd" else 16, 16, 5, weights="hash")
    kw = {}
    native = os.environ.get("GM_EXCHANGE", "native") == "native"
    if name in SHARDED:
        import torch
        import torch.distributed as dist
        from graphmat_amd.dist import attach_exchange, attach_native_exchange, init_native_rccl
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        if native:
            init_native_rccl(device=torch.device("cuda", 0))
        kw = dict(device=0, nshards=world, shard=rank)
    keep = name in ("sssp", "sssp_lists", "sgd")
    tiles = 1 if name in ("pr_csr", "two_stage", "sgd", "bfs_bits") else 4
    g = api.Graph(nv, s, d, v if keep else None, keep_values=keep, col_tiles=tiles, **kw)
    if name in SHARDED:
        if native:
            attach_native_exchange(g)
        else:
            logged_exchange(g, attach_exchange(g), rank)
    if name in ("sssp", "sssp_lists"):
        _, it = g.sssp(1)
    elif name in ("bfs", "bfs_push", "bfs_bits", "sharded_bfs"):
        _, _, it = g.bfs(1)
    elif name == "sgd":
        import numpy as np
        _, it = g.sgd(np.random.default_rng(1).random((nv, 20)) * 0.1, 0.001, 1e-4, 2)
    else:
        _, _, it = g.pagerank(3)
    sw, bl = _lib.Sweep(), _lib.Blocked()
    _lib.check(L.gm_graph_sweep(g.h, C.byref(sw)))
    _lib.check(L.gm_graph_blocked(g.h, C.byref(bl)))
    notes = {}
    for note in ("GM_NOTE_SPARSE_SWEEPS", "GM_NOTE_SHORT_FOLDS", "GM_NOTE_FOLD_APPLIES", "GM_NOTE_STEP_COUNTS", "GM_NOTE_STEP_KINDS"):
        n = C.c_int64(-1)
        L.gm_graph_note_get(g.h, getattr(_lib, note), C.byref(n))
        notes[note] = n.value
    k6 = notes["GM_NOTE_STEP_KINDS"] & 0xFFFFFFFFFFFFFFFF  # (all pulls for the sharded fixed-count schedules, which count no steps)
    kinds = " ".join(("pull", "list", "bits", "dense-push")[(k6 >> (2 * i)) & 3] for i in range(min(it, 32)))
    stats = g.last_stats()
    print("%s: %d iterations, %d multiply launches; sweep rows %d (long %d) sets %d waves %d nsub %d stream edges %d giant edges %d; giant rows %d; blocked rows %d; %s; steps: %s; sparse exchanges %d"
          % (name, it, stats["spmv_launches"], sw.nrows, sw.nrows_long, sw.nsets, sw.waves, sw.nsub, sw.nstream, sw.ngiant_edges, g.csr(api.GM_DIR_OUT).ngiant,
             bl.nrows, notes, kinds, stats["sparse_exchanges"]), flush=True)
    g.close()
    _lib.check(L.gm_reset_options())
    if name in SHARDED:
        dist.destroy_process_group()


def app(name):
    """a program of build/apps on its graph, as a child process (this one never touches the GPU)"""
    import subprocess
    import tempfile
    from graphmat_amd import generators as gen
    from graphmat_amd.mtx import write_mtx_bin
    exe, args, env, graph = APPS[name]
    nv, s, d, v = star() if graph == "star" else gen.rmat_edges(int(graph.split()[1]), 16, 5, weights="hash")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".bin.mtx")
        write_mtx_bin(path, nv, s, d, v)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = subprocess.run([os.path.join(root, "build", "apps", exe), path] + args, env=dict(os.environ, GRAPHMAT_NUM_THREADS="1", **env))
    sys.exit(out.returncode)


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
    elif sys.argv[1] == "app":
        app(sys.argv[2])
    else:  # one process, one database; the listings of a run's processes in an order that does not depend on their ids
        dbs = sorted(glob.glob(os.path.join(sys.argv[2], "**", "*.db"), recursive=True))
        assert dbs, "no rocprofv3 database under " + sys.argv[2]
        for text in sorted(listing(p) for p in dbs):
            if text.strip():
                sys.stdout.write("---- a process: %d dispatches\n%s" % (text.count("\n"), text))


if __name__ == "__main__":
    main()

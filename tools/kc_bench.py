#!/usr/bin/env python3
"""K-core timing: gm_run_kcore on an RMAT graph.

The graph: the generator's raw RMAT edges of the given scale, made on the device (duplicates, antiparallel pairs and loops stay:
the call's adjacency build drops them).  The run is a child process under a time limit: the child builds the graph, warms up once
(the workspaces are allocated there), times `--reps` calls with the host clock (the call returns after the stream has finished)
and prints one JSON line: the median ms, kmax, the levels and peel passes, the simple edges (distinct unordered pairs without
loops, counted here from the edge list) and simple edges per second of the whole call, and the split of the device time between the
adjacency build, the peel and the finish (gm_graph_last_stats)."""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def simple_edges(nv, src, dst):
    """distinct unordered pairs {u, v}, u != v (on the device)"""
    import torch
    u, v = src.to(torch.int64), dst.to(torch.int64)
    keep = u != v
    return int(torch.unique(torch.minimum(u, v)[keep] * (nv + 1) + torch.maximum(u, v)[keep]).numel())


def child(args):
    import torch
    from graphmat_amd import api, _lib
    L = _lib.lib()
    nv, src, dst, _ = api.rmat_on_device(args.scale, args.edge_factor, seed=args.seed)
    ne = int(src.numel())
    nsimple = simple_edges(nv, src, dst)
    g = api.Graph(nv, src, dst, directions=args.directions)
    del src, dst
    core = torch.zeros(g.rows, dtype=torch.int32, device=g.device)
    kmax = C.c_int32(0)
    _lib.check(L.gm_run_kcore(g.h, core.data_ptr(), C.byref(kmax), None))  # warm-up (allocates the workspaces)
    first = core.clone()
    ms, stats = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _lib.check(L.gm_run_kcore(g.h, core.data_ptr(), C.byref(kmax), None))
        ms.append((time.perf_counter() - t0) * 1e3)
        stats.append(g.last_stats())
    mid = sorted(range(args.reps), key=lambda i: ms[i])[args.reps // 2]
    st = stats[mid]
    assert bool((core == first).all())
    print(json.dumps({"scale": args.scale, "vertices": nv, "edges": ne, "simple_edges": nsimple, "directions": args.directions,
                      "ms": round(ms[mid], 3), "kmax": int(kmax.value), "levels": st["spmv_launches"], "passes": st["iterations"],
                      "simple_edges_per_s": round(nsimple / (ms[mid] * 1e-3)), "send_ms": round(st["send_ms"], 3),
                      "spmv_ms": round(st["spmv_ms"], 3), "apply_ms": round(st["apply_ms"], 3), "device_ms": round(st["total_ms"], 3),
                      "core_sum": int(core.to(torch.int64).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--directions", type=int, default=3, help="adjacencies the graph is built with: 1 = GM_DIR_OUT, 2 = GM_DIR_IN, 3 = both")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take (graph build, warm-up and repetitions)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--scale", str(args.scale), "--edge-factor", str(args.edge_factor), "--seed", str(args.seed),
           "--reps", str(args.reps), "--directions", str(args.directions), "--child"]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"scale": args.scale, "error": "no result within %g s" % args.limit}), flush=True)
        sys.exit(1)
    if out.returncode != 0:
        sys.stderr.write(out.stderr.decode()[-2000:])
        print(json.dumps({"scale": args.scale, "error": "exit status %d" % out.returncode}), flush=True)
        sys.exit(1)
    print([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1], flush=True)


if __name__ == "__main__":
    main()

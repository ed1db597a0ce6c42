#!/usr/bin/env python3
"""Betweenness-centrality timing: gm_run_betweenness from k sources on an RMAT graph or on a uniform random one (no skew).

The graph: the generator's raw edges of the given scale, made on the device (duplicates and loops stay: the call ignores them),
built with both adjacencies (Graph.bfs, the yardstick, wants them; the call itself reads GM_DIR_IN only).  The k sources
(default 4) are drawn by seed among the vertices with out-edges.  The run is a child process under a time limit: the child builds
the graph, warms up once (the workspaces are allocated there), times `--reps` calls with the host clock (the call returns after
the stream has finished) and prints one JSON line: the median ms per call and per source, the passes (forward plus backward level
passes), the split of the device time between set-up, the forward phases and the backward phases (gm_graph_last_stats), whether
all calls returned the same bytes, and -- only as a yardstick, it computes less -- the time of Graph.bfs from the same sources."""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    import torch
    from graphmat_amd import api, _lib
    L = _lib.lib()
    make = api.rmat_on_device if args.graph == "rmat" else api.uniform_on_device
    nv, src, dst, _ = make(args.scale, args.edge_factor, seed=args.seed)
    ne = int(src.numel())
    with_out = torch.unique(src).cpu().numpy()
    g = api.Graph(nv, src, dst)
    del src, dst
    rng = np.random.default_rng(args.seed)
    sources = np.sort(rng.choice(with_out, size=min(args.sources, len(with_out)), replace=False)).astype(np.int32)
    k = int(sources.size)
    bc = torch.zeros(g.rows, dtype=torch.float64, device=g.device)
    run = lambda: _lib.check(L.gm_run_betweenness(g.h, sources.ctypes.data, k, bc.data_ptr(), None, None, None))
    run()  # warm-up (allocates the workspaces)
    first = bc.clone()
    ms, stats, same = [], [], True
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
        stats.append(g.last_stats())
        same = same and bool((bc == first).all())
    mid = sorted(range(args.reps), key=lambda i: ms[i])[args.reps // 2]
    st = stats[mid]
    bfs_ms, levels = 0.0, 0
    for s in sources.tolist():
        g.bfs(s)  # (warm-up of this source's path through the engine)
        _, _, it = g.bfs(s)
        bfs_ms += g.last_wall_ms
        levels += it
    print(json.dumps({"graph": args.graph, "scale": args.scale, "vertices": nv, "edges": ne, "sources": k, "ms": round(ms[mid], 3),
                      "ms_per_source": round(ms[mid] / max(k, 1), 3), "passes": st["spmv_launches"], "send_ms": round(st["send_ms"], 3),
                      "spmv_ms": round(st["spmv_ms"], 3), "apply_ms": round(st["apply_ms"], 3), "device_ms": round(st["total_ms"], 3),
                      "same_bytes": same, "nonzero": int((bc != 0).sum()), "bc_max": float(bc.max()), "bfs_ms": round(bfs_ms, 3),
                      "bfs_iterations": levels}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=("rmat", "uniform"), default="rmat")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take (graph build, warm-up and repetitions)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--graph", args.graph, "--scale", str(args.scale), "--edge-factor", str(args.edge_factor),
           "--seed", str(args.seed), "--sources", str(args.sources), "--reps", str(args.reps), "--child"]
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

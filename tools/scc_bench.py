#!/usr/bin/env python3
"""Strong-components timing: gm_run_strong_components on an RMAT graph or on a uniform random one (no skew).

The graph: the generator's raw edges of the given scale, made on the device (duplicates and loops stay: the call ignores them),
built with both adjacencies.  The run is a child process under a time limit: the child builds the graph, warms up once (the
workspaces are allocated there), times `--reps` calls with the host clock (the call returns after the stream has finished) and
prints one JSON line: the median ms, the rounds, the passes (trim lists, forward and backward passes), the split of the device
time between set-up with the first trim, the rounds with their trims and the rest (gm_graph_last_stats), the number of components
and the size of the largest."""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    from graphmat_amd import api, _lib
    L = _lib.lib()
    make = api.rmat_on_device if args.graph == "rmat" else api.uniform_on_device
    nv, src, dst, _ = make(args.scale, args.edge_factor, seed=args.seed)
    ne = int(src.numel())
    g = api.Graph(nv, src, dst)
    del src, dst
    labels = torch.zeros(g.rows, dtype=torch.int32, device=g.device)
    n = C.c_int32(0)
    _lib.check(L.gm_run_strong_components(g.h, labels.data_ptr(), C.byref(n), None))  # warm-up (allocates the workspaces)
    first = labels.clone()
    ms, stats = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _lib.check(L.gm_run_strong_components(g.h, labels.data_ptr(), C.byref(n), None))
        ms.append((time.perf_counter() - t0) * 1e3)
        stats.append(g.last_stats())
    mid = sorted(range(args.reps), key=lambda i: ms[i])[args.reps // 2]
    st = stats[mid]
    assert bool((labels == first).all())
    sizes = torch.bincount(labels[labels > 0].to(torch.int64))
    assert int((sizes > 0).sum()) == n.value
    print(json.dumps({"graph": args.graph, "scale": args.scale, "vertices": nv, "edges": ne, "ms": round(ms[mid], 3), "rounds": st["iterations"],
                      "passes": st["spmv_launches"], "send_ms": round(st["send_ms"], 3), "spmv_ms": round(st["spmv_ms"], 3),
                      "apply_ms": round(st["apply_ms"], 3), "device_ms": round(st["total_ms"], 3), "ncomponents": int(n.value),
                      "largest": int(sizes.max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=("rmat", "uniform"), default="rmat")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take (graph build, warm-up and repetitions)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--graph", args.graph, "--scale", str(args.scale), "--edge-factor", str(args.edge_factor),
           "--seed", str(args.seed), "--reps", str(args.reps), "--child"]
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

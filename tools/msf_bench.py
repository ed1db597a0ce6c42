#!/usr/bin/env python3
"""Minimum-spanning-forest timing: gm_run_spanning_forest on an RMAT or a uniform random graph with int32 weights.

The graph: the generator's raw edges of the given scale, made on the device (duplicates and loops stay: parallel edges are separate
candidates, loops are ignored); RMAT carries the generator's weights, the uniform graph seeded ones in 1..2^20.  A run is a child
process under a time limit: the child builds the graph, warms up once (the workspaces are allocated there), times `--reps` calls
with the host clock (the call returns after the stream has finished) for every value of option "msf_form" asked for, then times
Graph.connected_components() on the same graph in the same way -- the yardstick: it makes the same kind of passes -- and prints
one JSON line per form: the median ms, the pick passes over the edges (`rounds`, the last one that found nothing included), the
jump passes, edges per second of the whole call, the split of the device time between set-up (init + edge rows), the rounds and
the output (gm_graph_last_stats), the forest's edges and total, the components call's median ms and the ratio of the two."""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_run(reps, call, stats):
    import torch
    ms, st = [], []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        st.append(stats())
    mid = sorted(range(reps), key=lambda i: ms[i])[reps // 2]
    return ms[mid], st[mid]


def child(args):
    import torch
    from graphmat_amd import api, _lib
    L = _lib.lib()
    if args.graph == "rmat":
        nv, src, dst, val = api.rmat_on_device(args.scale, args.edge_factor, seed=args.seed, weights=True)
    else:
        nv, src, dst, _ = api.uniform_on_device(args.scale, args.edge_factor, seed=args.seed)
        gen = torch.Generator(device=src.device)
        gen.manual_seed(args.seed)
        val = torch.randint(1, (1 << 20) + 1, (src.numel(),), dtype=torch.int32, device=src.device, generator=gen)
    ne = int(src.numel())
    g = api.Graph(nv, src, dst, val=val, directions=args.directions)
    del src, dst, val
    edges = torch.zeros((g.rows, 3), dtype=torch.int32, device=g.device)
    n, total = C.c_int32(0), C.c_int64(0)
    labels = torch.zeros(g.rows, dtype=torch.int32, device=g.device)
    ncomp = C.c_int32(0)

    def forest():
        _lib.check(L.gm_run_spanning_forest(g.h, edges.data_ptr(), C.byref(n), C.byref(total), None))

    def components():
        _lib.check(L.gm_run_connected_components(g.h, labels.data_ptr(), C.byref(ncomp), None))

    components()  # warm-up (allocates the workspaces)
    cc_ms, cc_st = median_run(args.reps, components, g.last_stats)
    forest()
    first = edges.clone()
    for form in args.forms:
        _lib.check(L.gm_set_option(b"msf_form", form))
        forest()
        ms, st = median_run(args.reps, forest, g.last_stats)
        assert bool((edges == first).all()) and n.value == nv - ncomp.value
        print(json.dumps({"graph": args.graph, "scale": args.scale, "msf_form": form, "vertices": nv, "edges": ne, "directions": args.directions,
                          "ms": round(ms, 3), "rounds": st["iterations"], "jump_passes": st["spmv_launches"], "edges_per_s": round(ne / (ms * 1e-3)),
                          "send_ms": round(st["send_ms"], 3), "spmv_ms": round(st["spmv_ms"], 3), "apply_ms": round(st["apply_ms"], 3),
                          "device_ms": round(st["total_ms"], 3), "forest_edges": int(n.value), "total": int(total.value),
                          "components_ms": round(cc_ms, 3), "components_rounds": cc_st["iterations"], "times_components": round(ms / cc_ms, 2)}), flush=True)
    L.gm_reset_options()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--graph", choices=("rmat", "uniform"), default="rmat")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", default="0", help='values of option "msf_form" to time, comma-separated (graphmat_hip.h: gm_set_option)')
    ap.add_argument("--directions", type=int, default=3, help="adjacencies the graph is built with: 1 = GM_DIR_OUT, 2 = GM_DIR_IN, 3 = both")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take (graph build, warm-up and repetitions)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.forms = [int(f) for f in str(args.forms).split(",")]
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--scale", str(args.scale), "--graph", args.graph, "--edge-factor", str(args.edge_factor),
           "--seed", str(args.seed), "--reps", str(args.reps), "--forms", ",".join(map(str, args.forms)), "--directions", str(args.directions), "--child"]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"scale": args.scale, "error": "no result within %g s" % args.limit}), flush=True)
        sys.exit(1)
    if out.returncode != 0:
        sys.stderr.write(out.stderr.decode()[-2000:])
        print(json.dumps({"scale": args.scale, "error": "exit status %d" % out.returncode}), flush=True)
        sys.exit(1)
    for l in out.stdout.decode().splitlines():
        if l.startswith("{"):
            print(l, flush=True)


if __name__ == "__main__":
    main()

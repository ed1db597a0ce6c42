#!/usr/bin/env python3
"""Triangle-counting timing: gm_run_triangle_count on an RMAT graph for the three values of option "tc_form".

The graph: RMAT edges of the given scale generated on the device, oriented src < dst, duplicates and loops dropped (the total is
then the graph's triangle count).  Every form runs in a child process of its own under its own time limit (a form that is
hopeless at a scale must not cost the others their figures): the child builds the graph, warms up once, times `--reps` calls with
the host clock (the call ends in a stream synchronise) and prints one JSON line: the median ms, intersected edges per second, the
total, and the split of the device time between the keys pass and the plan + count kernels (gm_graph_last_stats).  The parent
prints the lines and checks that the totals agree."""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    from graphmat_amd import api, _lib
    L = _lib.lib()
    nv, src, dst, _ = api.rmat_on_device(args.scale, args.edge_factor, seed=args.seed)
    lo, hi = torch.minimum(src, dst).to(torch.int64), torch.maximum(src, dst).to(torch.int64)
    pairs = torch.unique((lo << 32) | hi)
    pairs = pairs[(pairs >> 32) != (pairs & 0xFFFFFFFF)]
    src, dst = (pairs >> 32).to(torch.int32), (pairs & 0xFFFFFFFF).to(torch.int32)
    ne = int(src.numel())
    del lo, hi, pairs
    g = api.Graph(nv, src, dst)
    del src, dst
    _lib.check(L.gm_set_option(b"tc_form", args.form))
    tri = torch.zeros(g.rows, dtype=torch.int64, device=g.device)
    total = C.c_uint64(0)
    _lib.check(L.gm_run_triangle_count(g.h, tri.data_ptr(), C.byref(total), None))  # warm-up (allocates the workspaces)
    ms, keys_ms, count_ms = [], [], []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _lib.check(L.gm_run_triangle_count(g.h, tri.data_ptr(), C.byref(total), None))
        ms.append((time.perf_counter() - t0) * 1e3)
        st = g.last_stats()
        keys_ms.append(st["send_ms"]); count_ms.append(st["spmv_ms"])
    mid = sorted(range(args.reps), key=lambda i: ms[i])[args.reps // 2]
    assert int(tri.sum()) == total.value
    print(json.dumps({"scale": args.scale, "tc_form": args.form, "vertices": nv, "edges": ne, "ms": round(ms[mid], 3),
                      "keys_ms": round(keys_ms[mid], 3), "count_ms": round(count_ms[mid], 3),
                      "edges_per_s": round(ne / (ms[mid] * 1e-3)), "total": int(total.value), "giant_rows": int(g.csr(api.GM_DIR_OUT).ngiant)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", default="0,1,2")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a form may take (graph build, warm-up and repetitions)")
    ap.add_argument("--form", type=int, default=None, help=argparse.SUPPRESS)  # (the child's)
    args = ap.parse_args()
    if args.form is not None:
        return child(args)
    totals = {}
    for form in [int(x) for x in args.forms.split(",") if x]:
        cmd = [sys.executable, os.path.abspath(__file__), "--scale", str(args.scale), "--edge-factor", str(args.edge_factor), "--seed", str(args.seed),
               "--reps", str(args.reps), "--form", str(form)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"scale": args.scale, "tc_form": form, "error": "no result within %g s" % args.limit}), flush=True)
            sys.exit(1)  # (a form that hangs has the GPU: nothing more is started on it)
        if out.returncode != 0:
            sys.stderr.write(out.stderr.decode()[-2000:])
            print(json.dumps({"scale": args.scale, "tc_form": form, "error": "exit status %d" % out.returncode}), flush=True)
            sys.exit(1)
        line = [l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        totals[form] = json.loads(line)["total"]
    assert len(set(totals.values())) == 1, "the forms disagree: %s" % totals
    print("totals agree: %d" % next(iter(totals.values())), flush=True)


if __name__ == "__main__":
    main()

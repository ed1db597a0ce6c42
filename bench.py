#!/usr/bin/env python3
"""bench.py -- PageRank on a synthetic RMAT graph, GTEPS per iteration + achieved HBM GB/s.

One "step" = one PageRank iteration (send -> multiply+reduce -> apply) over the whole
graph through libgraphmat_hip.so.  N>1: one process per GPU (torch.distributed, backend
nccl = RCCL), rows sharded 1-D by edge-balanced native ranges, x all-gathered per step.

  python bench.py --gpus 1 --steps 20 --warmup 3            # RMAT-26, the metric's config
  python bench.py --scale 22                                # BASELINE.json configs[1]

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for every field).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# the cpu_baseline leg (OpenMP) follows the reference's README.md:30-39: threads spread over the cores and
# pinned, memory interleaved over the NUMA nodes (set_mempolicy below).  libgomp reads these when it is
# loaded, which `import torch` does.
os.environ.setdefault("OMP_PROC_BIND", "spread")
os.environ.setdefault("OMP_PLACES", "cores")

import numpy as np
import torch

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def log(rank, *a):
    if rank == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def interleave_memory(on):
    """set_mempolicy(MPOL_INTERLEAVE over all online NUMA nodes) for this process, or back to the default."""
    try:
        nodes = 0
        for part in open("/sys/devices/system/node/online").read().strip().split(","):
            lo, _, hi = part.partition("-")
            nodes = max(nodes, int(hi or lo) + 1)
        if nodes < 2:
            return False
        libc = C.CDLL(None, use_errno=True)
        mask = (C.c_ulong * 16)()
        for n in range(nodes):
            mask[n // 64] |= 1 << (n % 64)
        MPOL_DEFAULT, MPOL_INTERLEAVE, SYS_set_mempolicy = 0, 3, 238  # x86_64
        rc = libc.syscall(SYS_set_mempolicy, MPOL_INTERLEAVE if on else MPOL_DEFAULT, mask if on else None, 1024 if on else 0)
        return rc == 0 and on
    except Exception:
        return False


def physical_cores():
    """(logical, physical) core counts of this host (physical = distinct (package, core id) pairs in /proc/cpuinfo)."""
    logical = os.cpu_count() or 1
    try:
        pairs = set()
        pkg = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pkg = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if pkg is not None and core is not None:
                    pairs.add((pkg, core))
                pkg = core = None
        if pkg is not None and core is not None:
            pairs.add((pkg, core))
        return logical, (len(pairs) or logical)
    except Exception:
        return logical, logical


def cpu_baseline(scale, iters, rank, scale2=0):
    """The oracle (CPU restatement of the reference algorithm, OpenMP `schedule(dynamic, 1)` over the reference's row
    partitions like include/GMDP/singlenode/spmspv.h:48) timed on this box's host cores on a bounded sample
    (RMAT-<scale>, same generator and seed as the GPU run).  Two knobs, tuned like a user of the reference would tune
    OMP_NUM_THREADS (README.md:30-39 of the reference), but DECOUPLED: the layout parameter (the reference cuts
    num_threads * 16 row partitions and walks a column list per partition, so its work grows with the partition count:
    at 2048 partitions nearly every edge has a column entry of its own) and the number of OpenMP threads that share the
    partitions.  Every (layout, threads) pair with threads <= partitions / 2 is judged on 10 iterations; the best one is
    then timed in three blocks of `iters` / 3 iterations -- `value` is the MEDIAN block, the spread is reported next
    to it, with the time per phase and a STREAM triad at the same thread counts (what the memory system delivers)."""
    from graphmat_amd import api
    from oracle import binding as ob
    logical, physical = physical_cores()
    interleaved = interleave_memory(True)   # what `numactl -i all` does (the reference's README.md:30-39)
    nv, s, d, _ = api.rmat_on_device(scale, 16, 1)
    s = s.cpu().numpy()
    d = d.cpu().numpy()
    L = ob.lib()
    L.gmo_phase_seconds.argtypes = [C.POINTER(C.c_double), C.c_int]
    L.gmo_phase_seconds.restype = None
    L.gmo_stream_triad_gbs.argtypes = [C.c_longlong, C.c_int]
    L.gmo_stream_triad_gbs.restype = C.c_double
    threads = sorted({c for c in (8, 16, 32, 64, 128, 256, physical) if c <= max(physical, 8) and c <= logical} or {logical})
    triad = []
    for t in threads:
        L.gmo_set_num_threads(t)
        triad.append({"threads": t, "gbps": round(L.gmo_stream_triad_gbs(1 << 26, 3), 1)})
    log(rank, "cpu_baseline: STREAM triad (3 x 512 MiB) " + ", ".join("%d thr %.0f GB/s" % (x["threads"], x["gbps"]) for x in triad))
    cands = []  # one per layout: (probe seconds, threads, graph, degrees, layout) of its best thread count
    probes = []
    for layout in (4, 8, 16, 32):
        if layout > max(physical, 8):
            continue
        L.gmo_set_num_threads(min(max(threads), 64))
        t0 = time.time()
        og = ob.OracleGraph(nv, s, d, None, ref_threads=layout)
        deg = og.degree()
        build_s = time.time() - t0
        mine = None
        for t in threads:
            if t < layout or t > layout * 8:  # (layout threads..half the partitions)
                continue
            L.gmo_set_num_threads(t)
            og.pagerank(2, degree=deg)  # warm
            t0 = time.time()
            og.pagerank(10, degree=deg)
            probe = (time.time() - t0) / 10
            probes.append({"layout_threads": layout, "threads": t, "ms_per_iteration": round(probe * 1e3, 2)})
            log(rank, "cpu_baseline probe: layout %d (%d partitions), %d threads: %.1f ms/iteration (build %.1f s)" % (layout, layout * 16, t, probe * 1e3, build_s))
            if mine is None or probe < mine[0]:
                mine = (probe, t, og, deg, layout)
        if mine is not None:
            cands.append(mine)
        del og
    # the probes are 10 iterations each and the host is not quiet: the two best (layout, threads) pairs both run the timed
    # blocks, and the better median is the baseline
    if not cands:  # (a host with very few cores: no (layout, threads) pair of the grid applies -- one small layout on all of them)
        layout = max(1, min(4, logical))
        L.gmo_set_num_threads(logical)
        og = ob.OracleGraph(nv, s, d, None, ref_threads=layout)
        deg = og.degree()
        t0 = time.time()
        og.pagerank(2, degree=deg)
        cands.append(((time.time() - t0) / 2, logical, og, deg, layout))
    cands.sort(key=lambda c: c[0])
    per_block = max(1, iters // 3)
    ph = (C.c_double * 3)()
    best = None
    for _, t_c, og_c, deg_c, layout_c in cands[:2]:
        L.gmo_set_num_threads(t_c)
        blocks_c = []
        L.gmo_phase_seconds(ph, 1)
        for _ in range(3):
            t0 = time.time()
            og_c.pagerank(per_block, degree=deg_c)
            blocks_c.append(time.time() - t0)
        L.gmo_phase_seconds(ph, 1)
        med = sorted(blocks_c)[1]
        log(rank, "cpu_baseline: layout %d, %d threads: 3 x %d iterations %s s" % (layout_c, t_c, per_block, ["%.2f" % b for b in blocks_c]))
        if best is None or med < best[0]:
            best = (med, t_c, og_c, deg_c, layout_c, blocks_c, [ph[0], ph[1], ph[2]])
    _, t, og, deg, layout, blocks, phs = best
    ph[0], ph[1], ph[2] = phs
    del cands
    gteps = sorted(len(s) * per_block / b / 1e9 for b in blocks)
    tot_it = 3 * per_block
    log(rank, "cpu_baseline: RMAT-%d, 3 x %d iterations %s s on %d threads (layout %d): %s GTEPS" % (
        scale, per_block, ["%.2f" % b for b in blocks], t, layout, ["%.3f" % x for x in gteps]))
    # the same pair on a larger sample (the review asked for RMAT-24 beside RMAT-22: 16x the metric's graph does not fit the
    # reference layout's memory, this one does): a few iterations, enough for a rate
    second = None
    if scale2 > scale:
        try:
            del og
            best = None
            nv2, s2, d2, _ = api.rmat_on_device(scale2, 16, 1)
            s2 = s2.cpu().numpy()
            d2 = d2.cpu().numpy()
            L.gmo_set_num_threads(min(max(threads), 64))
            t0 = time.time()
            og2 = ob.OracleGraph(nv2, s2, d2, None, ref_threads=layout)
            deg2 = og2.degree()
            build2 = time.time() - t0
            L.gmo_set_num_threads(t)
            og2.pagerank(2, degree=deg2)
            t0 = time.time()
            og2.pagerank(15, degree=deg2)
            per = (time.time() - t0) / 15
            second = {"scale": scale2, "E": int(len(s2)), "ms_per_iteration": round(per * 1e3, 1), "gteps": round(len(s2) / per / 1e9, 3), "build_s": round(build2, 1)}
            log(rank, "cpu_baseline: RMAT-%d with the same pair: %.1f ms/iteration = %.3f GTEPS (build %.1f s)" % (scale2, per * 1e3, second["gteps"], build2))
            del og2, s2, d2
        except Exception as e:  # pragma: no cover
            second = {"scale": scale2, "error": repr(e)}
    interleave_memory(False)
    # bytes the port's multiply moves per iteration (row index + value per edge, a column entry of 12 bytes per distinct
    # (partition, column), x per column entry, y read+written per edge in cache): what its GTEPS means in GB/s
    return {"numa": "OMP_PROC_BIND=%s OMP_PLACES=%s, memory %s" % (os.environ.get("OMP_PROC_BIND"), os.environ.get("OMP_PLACES"),
                                                                  "interleaved over all NUMA nodes" if interleaved else "default policy"),
            "value": round(gteps[1], 4), "unit": "GTEPS", "cores": t, "layout_threads": layout, "kind": "port",
            "min": round(gteps[0], 4), "max": round(gteps[2], 4), "spread_rel": round((gteps[2] - gteps[0]) / gteps[1], 4),
            "host_cores": {"logical": logical, "physical": physical}, "thread_probe": probes, "stream_triad": triad, "larger_sample": second,
            "phase_ms_per_iteration": {"send": round(ph[0] / tot_it * 1e3, 3), "spmv": round(ph[1] / tot_it * 1e3, 3),
                                       "apply": round(ph[2] / tot_it * 1e3, 3)},
            "calibration": "none possible: the reference proper cannot be built in this image (include/GMDP/gmdp.h needs "
                           "boost/serialization, which is absent, and stand-ins are not allowed), so there is no measured ratio "
                           "between this port and GraphMat itself; the survey's own run of the reference (8 vCPU, RMAT-22) gave 0.99 GTEPS",
            "sample": "oracle (oracle/gm_oracle.hpp, OpenMP, %d threads on %d logical / %d physical host cores, layout threads=%d = %d row "
                      "partitions) PageRank, median of 3 blocks of %d iterations on RMAT-%d (V=%d, E=%d), graph build excluded"
                      % (t, logical, physical, layout, layout * 16, per_block, scale, nv, len(s))}


def kernels_fingerprint():
    """sha256 (16 hex digits) of the sources the multiply kernels are built from: a committed PMC traffic figure
    is only quoted while it was measured on exactly these kernels."""
    import hashlib
    h = hashlib.sha256()
    for rel in ("include/graphmat/kernels.hpp", "include/graphmat/engine.hpp", "graphmat_amd/csrc/gm_graph.hip",
                "graphmat_amd/csrc/gm_programs.hip"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def extra_bfs(scale, edge_factor, seed, ref_threads, local_rank, rank):
    """BASELINE config 3: BFS on RMAT-<scale>, whole gm_run_bfs call per source (host syncs included), with the
    independent torch check of depth and parent (tools/fullscale_checks.py: max-native-id parent rule)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fullscale_checks import check_bfs
    from graphmat_amd import api
    dev = torch.device("cuda", local_rank)
    nv, src, dst, _ = api.rmat_on_device(scale, edge_factor, seed, weights=False, device=local_rank)
    g = api.Graph(nv, src, dst, None, ref_threads=ref_threads, device=local_rank, keep_values=False)
    nat = torch.from_numpy(api.native_index(nv, ref_threads * 16)).to(dev)
    g.bfs(1)  # warm: kernels, scratch
    runs = []
    for source in (1, 12345, 777):
        r = check_bfs(g, nv, src, dst, nat, source, dev)
        # 4 B per traversable edge + per vertex (8 rowptr + 24 read + 24 written) + 2 bit vectors per level
        r["alg_bytes"] = 4 * r["traversable_edges"] + nv * 56 + 2 * (nv // 8) * r["levels"]
        r["gteps"] = round(r["traversable_edges"] / r["wall_ms"] / 1e6, 2)
        r["hbm_gbps"] = round(r["alg_bytes"] / r["wall_ms"] / 1e6, 1)
        r["hbm_frac"] = round(r["alg_bytes"] / r["wall_ms"] / 1e6 / HBM_PEAK_GBPS, 4)
        r["wall_ms"] = round(r["wall_ms"], 3)
        log(rank, "extra bfs: source %d: %d levels, %.2f ms, %.1f GTEPS, parents %s" % (source, r["levels"], r["wall_ms"], r["gteps"], "OK" if r["ok"] else "WRONG"))
        runs.append(r)
    g.close()
    del src, dst, nat
    torch.cuda.empty_cache()
    return {"workload": "BFS (src/BFS.cpp program) on RMAT scale-%d, whole gm_run_bfs call per source" % scale,
            "parents_bit_exact_vs_max_native_rule": all(r["ok"] for r in runs),
            "median_wall_ms": sorted(r["wall_ms"] for r in runs)[1], "median_gteps": sorted(r["gteps"] for r in runs)[1],
            "runs": runs}


def extra_uniform(scale, edge_factor, seed, local_rank, rank, iters=10):
    """Not a BASELINE configuration: PageRank on a graph WITHOUT skew -- 2^scale vertices with `edge_factor` out-edges each to uniformly
    drawn destinations, the shape of the reference's own random test graphs (test/generator.h:73-105) -- with the automatic policy
    (the short rows as a column-blocked stream, kernels.hpp: k_spmv_blocked) and with gm_set_option("blocked_rows", -1) (the row-block
    kernel, every gather of which misses on such a graph); the two runs' states are compared bit for bit."""
    from graphmat_amd import api, _lib
    L = _lib.lib()
    nv, src, dst, _ = api.uniform_on_device(scale, edge_factor, seed, device=local_rank)
    res = {}
    states = {}
    try:
        for name, mode in (("column_blocked_stream", 0), ("row_blocks", -1)):
            _lib.check(L.gm_set_option(b"blocked_rows", mode))
            g = api.Graph(nv, src, dst, None, device=local_rank, keep_values=False)
            st = g.new_pr_state()
            g.run_degree(st)
            g.run_pagerank(st, 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.run_pagerank(st, iters)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / iters
            res[name] = {"ms_per_iteration": round(ms, 4), "gteps": round(edge_factor * nv / ms / 1e6, 2)}
            states[name] = g.to_vertex_order(st[:, 0].contiguous()).clone()  # (the two graphs' device orders differ: slices of ~4 MiB against ~1.3 MiB)
            log(rank, "extra uniform 2^%d: %s %.3f ms/iteration = %.1f GTEPS" % (scale, name, ms, edge_factor * nv / ms / 1e6))
            g.close()
    finally:
        _lib.check(L.gm_set_option(b"blocked_rows", 0))
    same = bool((states["column_blocked_stream"] == states["row_blocks"]).all())
    del src, dst, states
    torch.cuda.empty_cache()
    return {"workload": "PageRank (fp32, %d + 2 iterations) on a uniform random graph WITHOUT skew, 2^%d vertices x %d out-edges (NOT the metric's input)" % (iters, scale, edge_factor),
            "V": nv, "E": edge_factor * nv, "bits_equal_between_the_two_paths": same,
            "speedup": round(res["row_blocks"]["ms_per_iteration"] / res["column_blocked_stream"]["ms_per_iteration"], 2), **res}


def sgd_sampled_rows_check(g, nv, src, dst, val, lat0, lat1, users, items, K, lam, step, nsample, dev):
    """One ALL_EDGES SGD iteration recomputed for `nsample` user rows and `nsample` item rows from the same initial
    state, independently of the kernels (torch elementwise ops only, nothing shared with the library or the oracle),
    with the reference's formulas AND evaluation order (the reference's src/SGD.cpp:77-120: sequential K-term dot,
    error = rating - estimate, res = message * error; include/GMDP/singlenode/spmspv3.h:38-90: a row's results
    folded one by one in ascending NATIVE column order, the first one assigned; apply: lv += step * (-lambda * lv +
    sum)).  Every op is a separate IEEE fp32 multiply or add, so the comparison is expected to be bit-exact; the
    bound north_star states is 1e-6 relative.  Returns rows checked, rows bit-identical, the largest relative error."""
    nparts = g.nparts
    h = nv // nparts
    vmax = h * nparts

    def native(v0):  # include/Graph.h:111-130 on 0-based ids
        return torch.where(v0 >= vmax, v0, v0 // nparts + (v0 % nparts) * h)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    dov = g.dev_of_vertex
    lam32 = torch.tensor(np.float32(lam), device=dev)
    step32 = torch.tensor(np.float32(step), device=dev)
    checked = exact = 0
    worst = 0.0
    for side in ("items", "users"):
        if side == "items":   # an item row receives from its raters (OUT pass: rows = destinations)
            R = users + 1 + torch.randperm(items, generator=gen, device=dev)[:nsample].long()
            rows_all, cols_all = dst, src
        else:                 # a user row receives from the items it rated (IN pass: rows = sources)
            R = 1 + torch.randperm(users, generator=gen, device=dev)[:nsample].long()
            rows_all, cols_all = src, dst
        R, _ = torch.sort(R)
        mark = torch.zeros(nv + 1, dtype=torch.bool, device=dev)
        mark[R] = True
        idx = torch.nonzero(mark[rows_all.long()]).squeeze(1)  # ascending = input order
        rows = rows_all[idx].long()
        cols = cols_all[idx].long()
        rating = val[idx].to(torch.float32)
        del mark, idx
        rank_of = torch.full((nv + 1,), -1, dtype=torch.int64, device=dev)
        rank_of[R] = torch.arange(R.numel(), device=dev)
        key = rank_of[rows] * (1 << 32) + native(cols - 1)
        del rank_of
        key, order = torch.sort(key, stable=True)       # (row, native column), duplicates in input order
        rr = key >> 32
        cols, rating = cols[order], rating[order]
        count = torch.bincount(rr, minlength=R.numel())
        start = torch.cumsum(count, 0) - count
        m = lat0[dov[cols - 1], :K]
        vp_e = lat0[dov[R - 1], :K][rr]
        est = torch.zeros(cols.numel(), dtype=torch.float32, device=dev)
        for k in range(K):
            est = est + m[:, k] * vp_e[:, k]
        err = rating - est
        terms = m * err[:, None]
        del m, vp_e, est
        acc = torch.zeros((R.numel(), K), dtype=torch.float32, device=dev)
        for j in range(int(count.max())):
            live = torch.nonzero(count > j).squeeze(1)
            t = terms[start[live] + j]
            if j == 0:
                acc[live] = t
            else:
                acc[live] = acc[live] + t
        vp = lat0[dov[R - 1], :K]
        t1 = (-lam32) * vp
        t2 = t1 + acc
        t3 = step32 * t2
        want = torch.where((count > 0)[:, None], vp + t3, vp)
        got = lat1[dov[R - 1], :K]
        same = (want.view(torch.int32) == got.view(torch.int32)).all(dim=1)
        rel = ((want - got).abs() / want.abs().clamp(min=1e-30)).max()
        checked += int(R.numel())
        exact += int(same.sum())
        worst = max(worst, float(rel))
        del terms, acc
    return checked, exact, worst


def extra_sgd(users, items, per_user, iters, local_rank, rank):
    """BASELINE config 5 shape on one GPU: SGD/CF, K=128 fp32 latent vectors, one ALL_EDGES iteration."""
    from graphmat_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", local_rank)
    K = 128
    nv = users + items
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    src = torch.arange(1, users + 1, dtype=torch.int32, device=dev).repeat_interleave(per_user)
    dst = (users + 1 + torch.randint(0, items, (src.numel(),), generator=gen, device=dev)).to(torch.int32)
    val = torch.randint(1, 6, (src.numel(),), generator=gen, device=dev).to(torch.int32)
    E = src.numel()
    g = api.Graph(nv, src, dst, val, device=local_rank, keep_values=True)
    lat = torch.rand((g.rows, K + 1), generator=gen, device=dev, dtype=torch.float32)
    lat0 = lat.clone()
    it = C.c_int(0)
    _lib.check(L.gm_run_sgd(g.h, lat.data_ptr(), K, 4, 0.001, 1e-5, 1, C.byref(it), None))  # warm, and the checked one
    torch.cuda.synchronize()
    nsample = min(1024, users, items)
    checked, exact, worst = sgd_sampled_rows_check(g, nv, src, dst, val, lat0, lat, users, items, K, 0.001, 1e-5, nsample, dev)
    log(rank, "extra sgd: %d sampled rows recomputed with torch in the reference's order: %d bit-identical, max rel err %.3g"
        % (checked, exact, worst))
    del src, dst, val, lat0
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    _lib.check(L.gm_run_sgd(g.h, lat.data_ptr(), K, 4, 0.001, 1e-5, iters, C.byref(it), None))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    finite = bool(torch.isfinite(lat).all())
    # the dot products on the matrix cores (gm_set_option("sgd_mfma"), k_sgd_multiply_mfma): one iteration of each form from the
    # same state -- time and largest difference; the vector form is the one that ships and the one `ms_per_iteration` times
    mfma = None
    try:
        a, b = lat.clone(), lat.clone()
        _lib.check(L.gm_run_sgd(g.h, a.data_ptr(), K, 4, 0.001, 1e-5, 1, C.byref(it), None))
        _lib.check(L.gm_set_option(b"sgd_mfma", 1))
        _lib.check(L.gm_run_sgd(g.h, b.data_ptr(), K, 4, 0.001, 1e-5, 1, C.byref(it), None))  # (first use of the kernel)
        b.copy_(lat)
        torch.cuda.synchronize()
        tm = time.perf_counter()
        _lib.check(L.gm_run_sgd(g.h, b.data_ptr(), K, 4, 0.001, 1e-5, 1, C.byref(it), None))
        torch.cuda.synchronize()
        tm = time.perf_counter() - tm
        _lib.check(L.gm_set_option(b"sgd_mfma", 0))
        big = a[:, :K].abs() > 1e-3
        rel = float(((a[:, :K] - b[:, :K]).abs()[big] / a[:, :K].abs()[big]).max().item())
        mfma = {"ms_per_iteration": round(tm * 1e3, 3), "vs_vector_form": round(tm / dt, 3), "max_rel_diff_vs_vector_form": rel,
                "values_differing_in_some_bit": int((a[:, :K] != b[:, :K]).sum().item()), "values": int(a[:, :K].numel()),
                "mfma_flops_per_iteration": 2 * E * K * 4 * 2, "useful_share_of_mfma_flops": 0.25,
                "note": "v_mfma_f32_4x4x1_16b_f32, 128 per 64-edge tile, lane = edge; not the default (profiles/r04_sgd_k128.md)"}
        log(rank, "extra sgd: matrix-core form of the dot products: %.2f ms/iteration (%.2fx the vector form), max relative difference %.2e" % (tm * 1e3, tm / dt, rel))
        del a, b
    except Exception as e:  # pragma: no cover
        mfma = {"error": repr(e)}
        L.gm_set_option(b"sgd_mfma", 0)
    balg = 2 * E * 8 + nv * K * 4 * 4          # index + rating per edge direction, x/vp read+write per vertex
    flops = 2 * E * 4 * K + 3 * K * nv
    g.close()
    del lat
    torch.cuda.empty_cache()
    log(rank, "extra sgd: %d x %d, %d ratings: %.2f ms/iteration" % (users, items, E, dt * 1e3))
    return {"workload": "SGD/CF (src/SGD.cpp program, K=128 fp32) on synthetic %d users x %d items, %d ratings, one ALL_EDGES iteration"
                        % (users, items, E), "ms_per_iteration": round(dt * 1e3, 3), "iterations_timed": iters,
            "edge_visits_per_s_e9": round(2 * E / dt / 1e9, 3), "alg_bytes": balg, "hbm_gbps": round(balg / dt / 1e9, 1),
            "hbm_frac": round(balg / dt / 1e9 / HBM_PEAK_GBPS, 4), "gather_inclusive_gbps": round(2 * E * K * 4 / dt / 1e9, 1),
            "tflops": round(flops / dt / 1e12, 2), "result_finite": finite, "mfma_form": mfma,
            "rows_checked": checked, "rows_bit_identical": exact, "max_rel_err": worst, "rel_tol": 1e-6,
            "rows_check": "first iteration, %d sampled item rows + %d sampled user rows recomputed from the same initial state by "
                          "an independent torch fp32 evaluation in the reference's order (bench.py sgd_sampled_rows_check)" % (nsample, nsample),
            "rows_ok": bool(checked >= 2 * nsample and worst <= 1e-6 and exact == checked)}


DUMP_SAMPLE = 1 << 21  # vertices written by --dump-outputs: 2^21 x (8 + 4 + 8) B = 40 MB at most
DUMP_SEED = 20250101


def dump_outputs(outdir, g, st, nv, rank, world, dev, on_host):
    """--dump-outputs: what a caller of the timed path receives (Graph.pagerank: pagerank float32 and out-degree per vertex,
    vertex order), for every vertex up to DUMP_SAMPLE vertices, else for a fixed seeded sample of vertex ids.  Sharded runs
    fold the shards' rows onto rank 0, which writes the files.  Collective: every rank calls it."""
    from graphmat_amd import api
    if nv <= DUMP_SAMPLE:
        idx = np.arange(nv, dtype=np.int64)
    else:
        idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, nv, DUMP_SAMPLE, dtype=np.int64))
    don, _ = g.maps_to_host()
    slots = torch.from_numpy(don[api.native_index(nv, g.nparts)[idx]].astype(np.int64)).to(dev)
    del don
    mine = (slots >= g.row_lo) & (slots < g.row_hi)
    vals = torch.zeros((idx.size, 2), dtype=torch.int32, device=dev)
    vals[mine] = st[slots[mine] - g.row_lo]
    if world > 1:  # every vertex is owned by one shard, the others add zeros
        import torch.distributed as dist
        vals = vals.cpu() if on_host else vals
        dist.all_reduce(vals, op=dist.ReduceOp.SUM)
    if rank != 0:
        return
    vals = vals.cpu()
    os.makedirs(outdir, exist_ok=True)
    np.save(os.path.join(outdir, "vertex.npy"), (idx + 1).astype(np.float64))
    np.save(os.path.join(outdir, "pagerank.npy"), vals[:, 0].contiguous().view(torch.float32).numpy())
    np.save(os.path.join(outdir, "out_degree.npy"), vals[:, 1].numpy().astype(np.float64))
    log(rank, "outputs of the last timed step (%d of %d vertices) written to %s" % (idx.size, nv, outdir))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=26, help="RMAT scale (26 = the metric's configuration, 22 = configs[1])")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ref-threads", type=int, default=1, help="layout parameter of the id permutation (oracle config)")
    ap.add_argument("--cpu-scale", type=int, default=22, help="RMAT scale of the cpu_baseline sample (0 = skip)")
    ap.add_argument("--cpu-scale2", type=int, default=24, help="a second, larger cpu_baseline sample with the tuned (layout, threads) pair: 15 iterations (0 = skip)")
    ap.add_argument("--cpu-iters", type=int, default=300, help="iterations of the cpu_baseline sample (~10-15 s of CPU work)")
    ap.add_argument("--no-extra", action="store_true", help="skip the BFS (config 3) and SGD (config 5) legs of the JSON line")
    ap.add_argument("--sgd-users", type=int, default=10_000_000)
    ap.add_argument("--sgd-items", type=int, default=1_000_000)
    ap.add_argument("--no-timing", action="store_true", help="do not bracket kernels with HIP events")
    ap.add_argument("--short-row", type=int, default=0, help="experiment: rows up to this many edges go to row-blocks")
    ap.add_argument("--giant-row", type=int, default=0, help="experiment: rows above this many edges get a workgroup")
    ap.add_argument("--rank-cap", type=int, default=0, help="experiment: rank only vertices of degree >= cap, others stay in native order")
    ap.add_argument("--rank-by", type=int, default=0, help="experiment: device order ranked by 0 total, 1 out-, 2 in-degree")
    ap.add_argument("--no-overlap", action="store_true", help="multi-GPU: plain exchange between send and multiply (no two-stage overlap)")
    ap.add_argument("--native-layout", action="store_true", help="device order = native order (single GPU; for A/B)")
    ap.add_argument("--tile-min-row", type=int, default=-1, help="experiment: rows of more than this many edges are tiled (0 = all rows)")
    ap.add_argument("--col-tiles", type=int, default=-1, help="column tiles of the OUT adjacency (-1 = default for the scale, 1 = none)")
    ap.add_argument("--graph", choices=("rmat", "uniform", "rmat-scrambled"), default="rmat", help="rmat = the metric's input; uniform = every vertex with edge-factor out-edges to uniformly drawn destinations (the reference's test/generator.h:73-105 shape): policy robustness runs")
    ap.add_argument("--lib-option", action="append", default=[], metavar="KEY=VALUE", help="gm_set_option(KEY, VALUE) before the graph is built (experiments)")
    ap.add_argument("--debug-flags", type=int, default=0, help="ablation only (results become invalid): 1 skip fold, 2 skip gathers")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed to DIR/<name>.npy (vertex ids, pagerank, out_degree; "
                         "a fixed seeded sample of %d vertices on larger graphs)" % DUMP_SAMPLE)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            print("bench.py: --gpus %d needs torch.distributed.run (WORLD_SIZE=%d)" % (args.gpus, world), file=sys.stderr)
            sys.exit(2)
    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    import torch.distributed as dist
    # GM_BENCH_BACKEND=gloo lets the sharded path be exercised on a 1-GPU box (all ranks on
    # cuda:0, collectives through the host); the driver's multi-GPU runs use nccl = RCCL.
    backend = os.environ.get("GM_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        dist.barrier()
    from graphmat_amd import _lib, api
    from graphmat_amd.dist import MessageExchange
    L = _lib.lib()
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    if args.short_row:
        _lib.check(L.gm_set_option(b"short_row", args.short_row))
    if args.giant_row:
        _lib.check(L.gm_set_option(b"giant_row", args.giant_row))
    if args.rank_cap:
        _lib.check(L.gm_set_option(b"rank_cap", args.rank_cap))
    if args.rank_by:
        _lib.check(L.gm_set_option(b"rank_by", args.rank_by))
    for kv in args.lib_option:
        k, v = kv.split("=", 1)
        _lib.check(L.gm_set_option(k.encode(), int(v)))
    if args.tile_min_row >= 0:
        _lib.check(L.gm_set_option(b"tile_min_row", args.tile_min_row))
    # ---- synthetic input, generated in HBM ------------------------------------------------
    t0 = time.time()
    # N > 1 with the library's own communicator: distributed build -- every rank generates 1/N of the edge list and
    # the library hands each edge to the shard that owns its row (gm_graph_desc_t.edges_local), so no rank ever
    # holds or sorts the whole graph.  Without the communicator (gloo, GM_BENCH_EXCHANGE=python): whole list per rank.
    want_native = world > 1 and (backend == "nccl" or os.environ.get("GRAPHMAT_RCCL_LIBRARY")) and \
        os.environ.get("GM_BENCH_EXCHANGE", "rccl") == "rccl"
    have_comm = False
    if want_native:
        from graphmat_amd import dist as gdist
        ok = 1
        try:
            gdist.init_native_rccl(device=dev)
        except Exception as e:  # pragma: no cover
            log(rank, "native RCCL communicator unavailable: %r" % (e,))
            ok = 0
        okt = torch.tensor([ok], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        have_comm = int(okt.item()) == 1
    local_build = have_comm and not args.native_layout and os.environ.get("GM_BENCH_BUILD", "local") == "local"
    E = args.edge_factor * (1 << args.scale)
    nparts = args.ref_threads * 16

    def build_graph(local):
        if args.graph == "uniform":
            nv_, src_, dst_, _ = api.uniform_on_device(args.scale, args.edge_factor, args.seed, device=local_rank, part=((rank, world) if local else None))
        else:
            nv_, src_, dst_, _ = api.rmat_on_device(args.scale, args.edge_factor, args.seed, weights=False, device=local_rank,
                                                    part=((rank, world) if local else None))
            if args.graph == "rmat-scrambled":
                # the same power-law graph with its vertex ids passed through a random permutation: degree rank and native id -- which the
                # slices of the device order are ranges of -- no longer have anything to do with each other (policy robustness runs)
                gen_ = torch.Generator(device=src_.device)
                gen_.manual_seed(1234567 + int(args.seed))
                perm_ = (torch.randperm(nv_, device=src_.device, generator=gen_) + 1).to(torch.int32)
                src_ = perm_[(src_ - 1).long()]
                dst_ = perm_[(dst_ - 1).long()]
                del perm_
        # device order chosen by the library: degree-ranked, dealt over the `world` shards
        g_ = api.Graph(nv_, src_, dst_, None, ref_threads=args.ref_threads, device=local_rank, keep_values=False,
                       layout=(_lib.GM_LAYOUT_NATIVE if args.native_layout else _lib.GM_LAYOUT_DEGREE), nshards=world, shard=rank,
                       col_tiles=(args.col_tiles if args.col_tiles >= 0 else 0), edges_local=local)
        return nv_, src_, dst_, g_
    g = None
    if local_build:
        # (a failed collective build must not take the run down: every rank then falls back to the whole edge list)
        ok, kept = 1, 0
        try:
            nv, src, dst, g = build_graph(True)
            kept = int(g.csr(api.GM_DIR_OUT).nnz)
        except Exception as e:  # pragma: no cover
            log(rank, "distributed graph build failed: %r" % (e,))
            ok = 0
        okt = torch.tensor([ok], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        tot = torch.tensor([kept], dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        if int(okt.item()) == 1 and int(tot.item()) != E:  # every edge must have arrived at exactly one shard
            log(rank, "distributed graph build kept %d of %d edges: not used" % (int(tot.item()), E))
            okt[0] = 0
        if int(okt.item()) != 1:
            local_build = False
            g = None
            torch.cuda.empty_cache()
    if g is None:
        nv, src, dst, g = build_graph(False)
    S = g.row_hi - g.row_lo
    ranges = [(r * S, (r + 1) * S) for r in range(world)] if world > 1 else [(0, g.ndevice)]
    del src, dst
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    build_s = time.time() - t0
    c_out = g.csr(api.GM_DIR_OUT)
    log(rank, "RMAT-%d V=%d E=%d built in %.1fs%s; rank0 rows [%d,%d) nnz=%d blocks=%d wave_rows=%d giant_rows=%d" % (
        args.scale, nv, E, build_s, " (distributed: each rank generated E/%d edges)" % world if local_build else "",
        ranges[rank][0], ranges[rank][1], c_out.nnz, c_out.nblk, c_out.nmid, c_out.ngiant))

    ex = None
    # N > 1.  The message buffers are torch tensors adopted by the library, so either exchange
    # implementation can serve them: the library's native RCCL exchange (gm_dist.hip: no Python per
    # iteration) or the torch.distributed callback (graphmat_amd/dist.py; the only one gloo can use, and
    # the cross-check of the native one below).  GM_BENCH_EXCHANGE=python forces the callback.
    native = False
    if world > 1:
        x_bytes = torch.zeros(g.ndevice * 4 + 64, dtype=torch.uint8, device=dev)
        x_bits = torch.zeros((g.ndevice + 31) // 32 + 2, dtype=torch.int32, device=dev)
        _lib.check(L.gm_graph_adopt_workspace(g.h, 1, x_bytes.data_ptr(), x_bytes.numel()))
        _lib.check(L.gm_graph_adopt_workspace(g.h, 2, x_bits.data_ptr(), x_bits.numel() * 4))
        # second message buffer: lets the library exchange one stage's messages while the other
        # stage computes (graphmat_hip.h GM_XCHG_PART); --no-overlap keeps the plain exchange
        x_bytes2 = None
        if not args.no_overlap:
            x_bytes2 = torch.zeros(g.ndevice * 4 + 64, dtype=torch.uint8, device=dev)
            _lib.check(L.gm_graph_adopt_workspace(g.h, 9, x_bytes2.data_ptr(), x_bytes2.numel()))
        ex = MessageExchange(ranges, rank, x_bytes, x_bits, live_rows=g.xchg_rows, x_bytes2=x_bytes2)
        cb = ex.callback()
        g._cb = cb
        _lib.check(L.gm_graph_set_exchange(g.h, cb, None))
        # (GRAPHMAT_RCCL_LIBRARY=tests/support/libgm_shm_transport.so: the test suite's shared-memory stand-in for
        # librccl, so that the native exchange code can be tried with several ranks on a 1-GPU box next to GM_BENCH_BACKEND=gloo)
        if have_comm:
            ok = 1
            try:
                # the two implementations must produce the same bits: a few iterations each from the same state
                st_a = g.new_pr_state()
                g.run_degree(st_a)
                st_b = st_a.clone()
                g.run_pagerank(st_b, 3)                      # callback exchange
                _lib.check(L.gm_graph_use_rccl(g.h))
                g.run_pagerank(st_a, 3)                      # native exchange
                ok = 1 if bool(torch.equal(st_a, st_b)) else 0
                del st_a, st_b
            except Exception as e:  # pragma: no cover
                log(rank, "native RCCL exchange unavailable: %r" % (e,))
                ok = 0
            okt = torch.tensor([ok], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            native = int(okt.item()) == 1
            if native:
                log(rank, "native RCCL exchange verified against the torch.distributed callback (3 iterations, same bits)")
            else:
                log(rank, "native RCCL exchange NOT used (unavailable or disagreeing): torch.distributed callback instead")
                _lib.check(L.gm_graph_set_exchange(g.h, cb, None))
                ex.parts = 0

    # edges handled by the long-row kernel (for per-kernel algorithmic bytes):
    # pull rowptr to the host once (8 bytes/row) and compute degrees
    rowptr = np.zeros(c_out.nrows + 1, np.int64)
    _lib.check(L.gm_graph_csr_to_host(g.h, api.GM_DIR_OUT, rowptr.ctypes.data, None, None))
    degs = np.diff(rowptr)
    # the library picked the giant threshold itself unless --giant-row was given: recover it
    thr = args.giant_row
    if not thr:
        thr = 4096
        while (degs > thr).sum() > 1024 and thr < (1 << 30):
            thr *= 2
    e_giant = int(degs[degs > thr].sum())
    e_mid = int(degs[degs > (args.short_row or 64)].sum()) - e_giant
    e_long = e_mid + e_giant
    max_deg = int(degs.max()) if degs.size else 0
    n_short_rows = int(((degs > 0) & (degs <= (args.short_row or 64))).sum())  # rows the row-block kernel folds (rank 0's shard)
    n_giant_rows = int(c_out.ngiant)
    del rowptr, degs

    from graphmat_amd import _lib as _gl0
    _sw0 = _gl0.Sweep()
    sharded_sweep = world > 1 and _gl0.lib().gm_graph_sweep(g.h, C.byref(_sw0)) == 0 and int(_sw0.nsub) == world and int(_sw0.nslices) > 1
    # ---- state, Degree pass, warm-up ---------------------------------------------------------
    st = g.new_pr_state()
    g.run_degree(st)
    overlapped = False
    forms_ms = None

    def parts_started():
        if native:
            return gdist.exchange_counters(g)[1]
        return ex.parts if ex is not None else 0
    if world > 1 and ex is not None and ex.x_bytes2 is not None:
        # the overlapped schedule must give the plain loop's bits; if it does not (or cannot run
        # here), say so and time the plain loop
        ok = 1
        t_two = t_plain = 0.0

        def timed(state, flags, iters=4):
            L.gm_set_option(b"debug_flags", flags)
            dist.barrier()
            torch.cuda.synchronize()
            t = time.perf_counter()
            g.run_pagerank(state, iters)
            torch.cuda.synchronize()
            t = time.perf_counter() - t
            L.gm_set_option(b"debug_flags", 0)
            tt = torch.tensor([t], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt.item())
        try:
            a, b = st.clone(), st.clone()
            timed(a, 0, 2)           # first use of each path (staging buffers, kernels)
            overlapped = parts_started() > 0
            timed(b, 128, 2)
            t_two = timed(a, 0)
            t_plain = timed(b, 128)
            ok = 1 if bool(torch.equal(a, b)) else 0
            del a, b
        except Exception as e:  # pragma: no cover
            log(rank, "overlapped exchange check failed: %r" % (e,))
            ok = 0
        okt = torch.tensor([ok], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        if int(okt.item()) != 1:
            log(rank, "overlapped two-stage schedule disagrees with the plain loop: using the plain loop")
            args.debug_flags |= 128
            overlapped = False
        elif overlapped and t_plain > 0 and t_two > t_plain * 1.02:
            # both schedules give the same bits; keep the faster one on this machine (max over ranks, 4 iterations each)
            log(rank, "%s schedule %.3f ms/iteration vs plain %.3f: using the plain exchange" % ("sharded swept" if sharded_sweep else "two-stage", t_two / 4 * 1e3, t_plain / 4 * 1e3))
            args.debug_flags |= 128
            overlapped = False
        else:
            log(rank, "%s schedule %.3f ms/iteration vs plain %.3f: using the %s" % ("sharded swept" if sharded_sweep else "two-stage", t_two / 4 * 1e3, t_plain / 4 * 1e3,
                                                                                      "overlapped schedule" if overlapped else "plain loop (no overlapped schedule applies)"))
        forms_ms = {"overlapped": round(t_two / 4 * 1e3, 4) if t_two > 0 else None, "plain": round(t_plain / 4 * 1e3, 4) if t_plain > 0 else None}
    if args.warmup > 0:
        if args.debug_flags & 128:
            L.gm_set_option(b"debug_flags", args.debug_flags)
        g.run_pagerank(st, args.warmup)
    cnt64 = (C.c_int64 * 4)()
    L.gm_debug_counters(cnt64)  # reset
    if args.debug_flags:
        L.gm_set_option(b"debug_flags", args.debug_flags)

    # ---- timed region: exactly K steps -------------------------------------------------------
    g.enable_timing(not args.no_timing)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps_done = g.run_pagerank(st, args.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    assert steps_done == args.steps, "timed %d PageRank steps instead of %d" % (steps_done, args.steps)
    stats = g.last_stats()
    L.gm_debug_counters(cnt64)
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, g, st, nv, rank, world, dev, backend != "nccl")
    # N > 1 diagnostics (after the timed region, not part of `value`): the same schedule once more with an exchange that
    # moves NOTHING -- what the shards' kernels alone take (results are garbage, a scratch state is used) -- so that
    # exchange_ms_exposed = measured iteration - compute-only iteration is what the collectives add on the critical
    # path; plus the bytes a rank contributes / receives per iteration and the per-phase times of this rank.
    multi_diag = None
    if world > 1 and ex is not None:
        try:
            xc0 = gdist.exchange_counters(g) if native else (ex.calls, ex.parts, 0)

            def nothing(ctx, kind, ptr, elt, bits, flag):
                return 0
            cb0 = _lib.EXCHANGE_FN(nothing)
            _lib.check(L.gm_graph_set_exchange(g.h, cb0, None))
            _lib.check(L.gm_graph_set_exchange_caps(g.h, _lib.GM_XCAP_SPARSE))  # (the sharded swept schedule asks for the list exchange; this one moves nothing either)
            scratch = st.clone()
            g.enable_timing(False)

            def compute_only(flags):
                L.gm_set_option(b"debug_flags", flags)
                g.run_pagerank(scratch, 2)
                dist.barrier()
                torch.cuda.synchronize()
                tc = time.perf_counter()
                g.run_pagerank(scratch, args.steps)
                torch.cuda.synchronize()
                tc = time.perf_counter() - tc
                tct = torch.tensor([tc], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
                dist.all_reduce(tct, op=dist.ReduceOp.MAX)
                return float(tct.item()) * 1e3 / args.steps
            compute_ms = compute_only(args.debug_flags)
            # ... and of the OTHER form (overlapped / plain), so that the line carries what the exchange exposes in each
            other_flags = (args.debug_flags & ~128) if (args.debug_flags & 128) else (args.debug_flags | 128)
            compute_other_ms = compute_only(other_flags) if forms_ms is not None else None
            L.gm_set_option(b"debug_flags", args.debug_flags)
            del scratch
            if native:
                _lib.check(L.gm_graph_use_rccl(g.h))
            else:
                _lib.check(L.gm_graph_set_exchange(g.h, cb, None))
            live = int(g.xchg_rows)
            multi_diag = {"compute_only_ms_per_step": round(compute_ms, 4),
                          "exchange_ms_exposed": round(dt * 1e3 / args.steps - compute_ms, 4),
                          "bytes_sent_per_rank_per_step": live * 4, "bytes_received_per_rank_per_step": live * 4 * (world - 1),
                          "exchange_calls_total": int(xc0[0]), "overlapped_parts_total": int(xc0[1]),
                          "native_bytes_contributed_total": int(xc0[2]) if native else None,
                          "phase_ms_per_step_rank0": {"send_and_exchange_enqueue": round(stats["send_ms"] / args.steps, 4),
                                                      "rowblock": round(stats["rowblock_ms"] / args.steps, 4), "wave": round(stats["wave_ms"] / args.steps, 4),
                                                      "giant_aux_stream": round(stats["giant_ms"] / args.steps, 4), "apply": round(stats["apply_ms"] / args.steps, 4)},
                          "note": "compute_only = the same schedule with an exchange callback that moves nothing (max over ranks); exposed = measured - compute_only"}
            if forms_ms is not None:
                # per form: measured (max over ranks; the chosen form over the timed region, the other one over the 4 iterations of the schedule check),
                # compute only, and the difference = what the exchange adds on the critical path in that form
                chosen = "plain" if (args.debug_flags & 128) else "overlapped"
                other = "overlapped" if chosen == "plain" else "plain"
                per_form = {chosen: {"ms_per_step": round(dt * 1e3 / args.steps, 4), "compute_only_ms_per_step": round(compute_ms, 4),
                                     "exchange_ms_exposed": round(dt * 1e3 / args.steps - compute_ms, 4)}}
                if forms_ms.get(other) is not None and compute_other_ms is not None:
                    per_form[other] = {"ms_per_step": forms_ms[other], "compute_only_ms_per_step": round(compute_other_ms, 4),
                                       "exchange_ms_exposed": round(forms_ms[other] - compute_other_ms, 4)}
                multi_diag["forms"] = per_form
                multi_diag["form_timed"] = chosen
                multi_diag["overlapped_form"] = ("sharded swept schedule: the all-gather starts before the giant rows are folded" if sharded_sweep else "two-stage schedule: tail rows' messages travel while the head rows are multiplied")
            log(rank, "N=%d diagnostics: %.3f ms/step measured, %.3f ms/step compute only => %.3f ms of exchange exposed; %d bytes sent and %d received per rank and step"
                % (world, dt * 1e3 / args.steps, compute_ms, dt * 1e3 / args.steps - compute_ms, live * 4, live * 4 * (world - 1)))
        except Exception as e:  # pragma: no cover
            multi_diag = {"error": repr(e)}

    ms_per_step = dt * 1e3 / args.steps
    gteps = E * args.steps / dt / 1e9
    # algorithmic bytes: whole iteration 4E + 48V; multiply+reduce kernels:
    #   row-block kernel: 4 B column id per edge it owns + per row (8 rowptr + 4 x + 4 y)
    #   wave / giant kernels: 4 B per edge they own
    rows0 = ranges[rank][1] - ranges[rank][0]
    e_short = int(c_out.nnz) - e_long
    # per-kernel algorithmic bytes per launch:
    #   row-block: 4 B column id per edge + per row 8 (rowptr) + 4 (y) ; x counted once per iteration in the wave line
    #   wave:      4 B per edge + per row 4 (row id) + 16 (rowptr pair) + 4 (y); the wave rows are handled by a pair of
    #              launches timed as one: k_spmv_wave (the few long rows) and k_spmv_wave16 (the rest, 16 rows to a wave)
    kern = {
        "k_spmv_rowblock": (stats["rowblock_ms"], stats["rowblock_launches"], 4 * e_short + 12 * rows0),
        "k_spmv_wave": (stats["wave_ms"], stats["wave_launches"], 4 * e_mid + 24 * int(c_out.nmid)),
    }
    # edges by the KERNEL that multiplies them (gm_csr_t.edges_*): with column tiles a wave row's short pieces are
    # row-block work, so this differs from the split by row class above
    def class_edges(c):
        blk, w16, w = int(c.edges_blk), int(c.edges_wave16), int(c.edges_wave)
        return [blk, w16, w, int(c.nnz) - blk - w16 - w]
    by_kernel = class_edges(c_out)
    if int(g.col_tiles) > 1:
        by_kernel = [by_kernel[0], 0, 0, 0]  # (the whole-graph CSR only multiplies its short rows: tile_min_row = short_row)
        for t in range(int(g.col_tiles)):
            ct, _ = g.tile(api.GM_DIR_OUT, t)
            by_kernel = [a + b for a, b in zip(by_kernel, class_edges(ct))]
    # the row-stationary sweep (graphmat_hip.h gm_sweep_t; kernels.hpp k_spmv_sell): every row of more than 64 edges that is not
    # giant goes through it, the short rows through the row-block kernel, the giant rows through their own passes on the auxiliary stream
    from graphmat_amd import _lib as _gl
    sweep = _gl.Sweep()
    if _gl.lib().gm_graph_sweep(g.h, C.byref(sweep)) != 0 or (world > 1 and int(sweep.nsub) != world):
        sweep.nrows = 0  # (N > 1: rank 0's shard, when its rows go through the sharded sweep -- gm_sweep_t.nsub)
    swept = int(sweep.nrows) > 0
    # (round 6, last session: the short rows' gathers ride the sweep as stream groups -- gm_sweep_t.nstream -- and k_short_fold folds their
    # products behind it; note 4 of the graph = multiplies of the last run that went that way)
    n4 = C.c_int64(0)
    streamed = swept and int(sweep.nstream) > 0 and _gl.lib().gm_graph_note_get(g.h, 4, C.byref(n4)) == 0 and n4.value > 0
    roof = None
    name = max(kern, key=lambda k: kern[k][0])
    ms, launches, alg_bytes = kern[name]
    tiled = int(g.col_tiles) > 1 and not swept
    if swept:
        # the dominant kernel: one launch per iteration (nsets launches timed as one unit when the rows do not fit one);
        # algorithmic bytes = 4 B column id per edge + 8 B per row (its y entry, its slot)
        name = "k_spmv_sell"
        ms, launches = stats["wave_ms"], stats["wave_launches"]
        swept_edges = int(sweep.nedges) + int(sweep.nedges_long)
        alg_bytes = 4 * swept_edges + 8 * int(sweep.nrows)
        if streamed:  # + the short rows' edges: 4 B column id read, 4 B product written
            alg_bytes += 8 * int(sweep.nstream)
        by_kernel = [int(c_out.edges_blk), swept_edges, 0, int(c_out.nnz) - int(c_out.edges_blk) - swept_edges]
    elif tiled:
        # column tiles: a row's pieces are spread over T launches of every kernel class (and per tile the long wave rows
        # overlap the other kernels on the auxiliary stream), so the unit is the whole multiply of one iteration: every
        # row-block and wave launch of its T tiles, its duration the span of the run's stream up to the join of the
        # auxiliary stream (HIP events on that stream; giant rows' bytes aside)
        name = "multiply"
        ms = stats["rowblock_ms"] + stats["wave_ms"]
        launches = stats["rowblock_launches"] + stats["wave_launches"]
        alg_bytes = kern["k_spmv_rowblock"][2] + kern["k_spmv_wave"][2]
    if launches > 0 and ms > 0:
        # the two-stage multi-GPU schedule launches every multiply kernel twice per iteration (tail rows,
        # head rows): the algorithmic bytes are per iteration, so is the time they are divided by
        per_step = max(1, round(launches / max(args.steps, 1)))
        avg_ms = ms / launches * per_step
        ach = alg_bytes / (avg_ms * 1e-3) / 1e9
        traffic = None
        traffic_raw = None
        # HBM/fabric bytes per launch from the committed rocprofv3 PMC passes -- quoted only while they were taken on
        # exactly the kernels that just ran (fingerprint of the kernel sources); otherwise null
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        traffic_note = "no PMC pass on record for these kernels"
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                per = tj.get("scale%d" % args.scale, {})
                if tj.get("kernels_fingerprint") == kernels_fingerprint() and tj.get("col_tiles", {}).get("scale%d" % args.scale) == int(g.col_tiles):
                    # (large graphs run the persistent forms k_spmv_rowwave / k_spmv_wave16p instead of, or next to, the plain ones)
                    names = {"k_spmv_rowblock": ["k_spmv_rowblock", "k_spmv_rowwave"], "k_spmv_wave": ["k_spmv_wave", "k_spmv_wave16", "k_spmv_wave16p"],
                             "k_spmv_sell": ["k_spmv_sell", "k_spmv_sell_sharded", "k_spmv_sell_stream"],
                             "multiply": ["k_spmv_rowblock", "k_spmv_rowwave", "k_spmv_wave", "k_spmv_wave16", "k_spmv_wave16p"]}.get(name, [name])
                    parts = [per.get(k + "_bytes_per_iteration") for k in names]
                    traffic = int(sum(v for v in parts if v is not None)) if any(v is not None for v in parts) else None
                    traffic_raw = traffic
                    # FETCH_SIZE counts a coalesced stream at half its bytes on this rocprofv3 / gfx950 (calibrated: tj["calibration"]):
                    # the kernel's coalesced streams are known by construction, their uncounted half is added
                    cal = tj.get("calibration", {}).get("FETCH_SIZE_reported_over_known_coalesced_stream")
                    if traffic is not None and cal and swept:
                        stream_bytes = 4 * (int(sweep.nentries) + int(sweep.nedges_long)) * (2 if int(sweep.val_bytes) else 1)
                        traffic = int(traffic + (1.0 - cal) * stream_bytes)
                    traffic_note = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same kernels (profiles/pmc_traffic.json); calibration of the counters "
                                    "on a pure coalesced stream and a pure random 4-byte gather: %s" % json.dumps(tj.get("calibration", "not recorded")))
                else:
                    traffic_note = "profiles/pmc_traffic.json was measured on other kernel sources: not quoted"
            except Exception:
                traffic = None
        # engine.hpp: persistent_forms_pay -- unsharded graphs from 48 M device ids on, tiled ones (row classes fixed per row) from 24 M on
        ndev = int(g.ndevice)
        big = world == 1 and (ndev >= (48 << 20) or (ndev >= (24 << 20) and int(g.col_tiles) > 1))
        kname = {"k_spmv_wave": "k_spmv_wave16+k_spmv_wave", "multiply": ("k_spmv_rowblock/k_spmv_rowwave+k_spmv_wave16p+k_spmv_wave" if big else "k_spmv_rowblock+k_spmv_wave16+k_spmv_wave") +
                 (" over %d column tiles" % int(g.col_tiles) if tiled else "")}.get(name, name)
        if swept:
            kname = "k_spmv_sell (row-stationary sweep over %d slices, %d launch(es) per iteration)" % (int(sweep.nslices), int(sweep.nsets))
            if streamed:
                kname = "k_spmv_sell_stream (row-stationary sweep over %d slices, %d launch(es) per iteration; also gathers for the rows of up to 64 edges and writes their products)" % (
                    int(sweep.nslices), int(sweep.nsets))
        # every multiply kernel of the iteration by itself: edges x 4 B / its average time / the HBM peak.  (The giant rows'
        # fold passes run on the auxiliary stream next to the row-block kernel: their time overlaps it; the sweep's time includes
        # the gathers it does for the giant rows.)
        steps_ = max(args.steps, 1)
        pmc_per = {}   # raw counter bytes per iteration and kernel, when the PMC passes on record were taken on these kernels
        pmc_cal = None
        if traffic_raw is not None:
            pmc_per = tj.get("scale%d" % args.scale, {})
            pmc_cal = tj.get("calibration", {}).get("FETCH_SIZE_reported_over_known_coalesced_stream")

        def kfrac(edges, ms_total, alg_bytes_k, pmc_names=(), stream_bytes=0):
            # frac: 4 B per edge (the column id / the gathered message: round 1-5's figure); frac_alg_bytes: DESIGN §4's algorithmic bytes of the
            # kernel (the row-block kernel also reads 8 B of row pointer and writes 4 B per row it folds, the sweep 8 B per row); traffic: the
            # counters' bytes of its launches + the uncounted half of its coalesced streams (FETCH_SIZE tallies those at half: calibration)
            t = ms_total / steps_
            raw = [pmc_per.get(k + "_bytes_per_iteration") for k in pmc_names]
            raw = int(sum(v for v in raw if v is not None)) if any(v is not None for v in raw) else None
            tr = int(raw + (1.0 - pmc_cal) * stream_bytes) if (raw is not None and pmc_cal) else raw
            return {"edges": int(edges), "avg_ms": round(t, 4), "gbps": round(4 * edges / (t * 1e-3) / 1e9, 1) if t > 0 else None,
                    "frac": round(4 * edges / (t * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if t > 0 else None,
                    "alg_bytes": int(alg_bytes_k), "frac_alg_bytes": round(alg_bytes_k / (t * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if t > 0 else None,
                    "traffic": tr, "traffic_raw_counters": raw, "traffic_over_alg_bytes": round(tr / alg_bytes_k, 2) if (tr and alg_bytes_k) else None}
        if swept:
            sweep_stream = 4 * (int(sweep.nentries) + int(sweep.nedges_long) + int(sweep.ngiant_edges) * 2) * (2 if int(sweep.val_bytes) else 1)
            if streamed:
                short_kernel = {"k_short_fold (rows of up to 64 edges, folded from the products stream the sweep wrote: 4 B product + 2 B place per edge, 12 B per row)":
                                    kfrac(by_kernel[0], stats["rowblock_ms"], 6 * by_kernel[0] + 12 * n_short_rows, ("k_short_fold",), 6 * by_kernel[0] + 8 * n_short_rows),
                                "k_spmv_sell_stream (rows of 65 .. giant-limit edges, and the gathers of the rows of up to 64 edges)":
                                    kfrac(by_kernel[1] + by_kernel[0], stats["wave_ms"], 4 * by_kernel[1] + 8 * int(sweep.nrows) + 8 * by_kernel[0],
                                          ("k_spmv_sell", "k_spmv_sell_sharded", "k_spmv_sell_stream"), sweep_stream)}
            else:
                short_kernel = {"k_spmv_rowblock (rows of up to 64 edges)": kfrac(by_kernel[0], stats["rowblock_ms"], 4 * by_kernel[0] + 12 * n_short_rows,
                                                                                   ("k_spmv_rowblock", "k_spmv_rowwave"), 4 * by_kernel[0] + 8 * n_short_rows),
                                "k_spmv_sell (rows of 65 .. giant-limit edges)": kfrac(by_kernel[1], stats["wave_ms"], 4 * by_kernel[1] + 8 * int(sweep.nrows), ("k_spmv_sell", "k_spmv_sell_sharded"), sweep_stream)}
            per_kernel = {**short_kernel,
                          "k_giant_sums + k_giant_maps + k_giant_replay_maps: the giant rows' fold passes (auxiliary stream, next to the row-block kernel; their gathers are done by the sweep, "
                          "they read the products stream twice and the replayed sub-pieces once more)":
                              # (behind k_short_fold the passes are hidden: the timer only sees the wait that is left, not their duration -- no rate is quoted then)
                              kfrac(by_kernel[3], 0.0 if streamed else stats["giant_ms"], 8 * by_kernel[3] + 8 * n_giant_rows, ("k_giant_sums", "k_giant_maps", "k_giant_replay_maps"), 8 * by_kernel[3])}
        else:
            per_kernel = {"k_spmv_rowblock": kfrac(by_kernel[0], stats["rowblock_ms"], 4 * by_kernel[0] + 12 * n_short_rows, ("k_spmv_rowblock", "k_spmv_rowwave"), 4 * by_kernel[0] + 8 * n_short_rows),
                          "k_spmv_wave16+k_spmv_wave": kfrac(by_kernel[1] + by_kernel[2], stats["wave_ms"], 4 * (by_kernel[1] + by_kernel[2]) + 12 * int(c_out.nmid),
                                                           ("k_spmv_wave", "k_spmv_wave16", "k_spmv_wave16p"), 4 * (by_kernel[1] + by_kernel[2])),
                          "k_giant_terms+k_spmv_giant (auxiliary stream, overlapped)": kfrac(by_kernel[3], stats["giant_ms"], 8 * by_kernel[3] + 8 * n_giant_rows,
                                                                                              ("k_giant_terms", "k_spmv_giant", "k_giant_sums", "k_giant_maps", "k_giant_replay_maps"), 8 * by_kernel[3])}
        roof = {"bound": "hbm", "kernel": kname + "<PageRank>", "achieved": round(ach, 1),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_raw_counters": traffic_raw, "traffic_source": traffic_note,
                "avg_launch_ms": round(avg_ms, 4), "alg_bytes_per_launch": alg_bytes,
                "unit_note": ("one launch unit = all %d launches of these kernels in one iteration" % per_step) if per_step > 1 else "one launch per iteration",
                "launches_per_iteration": per_step,
                "per_kernel": per_kernel,
                "rowblock_avg_ms": round(stats["rowblock_ms"] / max(args.steps, 1), 4),
                "wave_avg_ms": round(stats["wave_ms"] / max(args.steps, 1), 4),
                "aux_streams_avg_ms_overlapped": round(stats["giant_ms"] / max(args.steps, 1), 4),  # giant-row passes + long wave rows
                "edges_rowblock_wave_giant": [e_short, e_mid, e_giant],
                "edges_by_kernel": ({"k_spmv_sell_stream+k_short_fold" if streamed else "k_spmv_rowblock": by_kernel[0], "k_spmv_sell": by_kernel[1], "k_giant_terms+k_spmv_giant": by_kernel[3]} if swept else
                                    {"k_spmv_rowblock": by_kernel[0], "k_spmv_wave16": by_kernel[1], "k_spmv_wave": by_kernel[2],
                                     "k_giant_terms+k_spmv_giant": by_kernel[3]}),
                "send_avg_ms": round(stats["send_ms"] / args.steps, 4),
                "apply_avg_ms": round(stats["apply_ms"] / args.steps, 4),
                "bound_note": ("one 4-byte gather of x per edge is inherent to the path; what bounds the sweep is measured with its own phase clocks and "
                               "measurement forms (tools/sweep_lib_bench.hip, profiles/r05_sweep_phase_clocks.md): the L1-miss path of the CUs for the gathers "
                               "the LDS hot sets do not serve, and the per-slice latency chains")}
    iter_bytes = 4 * E + 48 * nv
    live_vertices = min(nv, int(g.xchg_rows) * world)
    out = {
        "metric": "GTEPS (edges/s) per iter + achieved HBM GB/s, PageRank %s-%d" % ({"rmat": "RMAT", "uniform": "uniform", "rmat-scrambled": "RMAT(scrambled ids)"}[args.graph], args.scale),
        "value": round(gteps, 3), "unit": "GTEPS", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("PageRank (alpha=0.3, fp32, fixed iteration count) on RMAT scale-%d, a/b/c=.57/.19/.19, "
                                "edge factor %d, seed %d, duplicates and self loops kept" % (args.scale, args.edge_factor, args.seed)) if args.graph == "rmat" else
                               ("PageRank (alpha=0.3, fp32, fixed iteration count) on RMAT scale-%d (a/b/c=.57/.19/.19, edge factor %d, seed %d) with the vertex ids SCRAMBLED by a "
                                "random permutation (NOT the metric's input: policy robustness run)" % (args.scale, args.edge_factor, args.seed)) if args.graph == "rmat-scrambled" else
                               ("PageRank (alpha=0.3, fp32, fixed iteration count) on a UNIFORM random graph (NOT the metric's input: policy robustness run), 2^%d "
                                "vertices with %d out-edges each to uniformly drawn destinations, seed %d" % (args.scale, args.edge_factor, args.seed)),
                   "V": nv, "E": E, "parallelism": "1d-rows x%d" % world, "exchange": ((("native exchange (gm_dist.hip) over %s, " % ("%s [GRAPHMAT_RCCL_LIBRARY, not RCCL]" % os.path.basename(os.environ["GRAPHMAT_RCCL_LIBRARY"]) if os.environ.get("GRAPHMAT_RCCL_LIBRARY") else "RCCL"))
                                                                              if native else "torch.distributed callback, ") if world > 1 else "") +
                                                                            (("all-gather started before the giant rows are folded, their messages following as lists (sharded swept schedule)"
                                                                              if sharded_sweep else "two-stage overlapped all-gather") if overlapped else
                                                                             (("all-gather between send and multiply" + (" (sharded sweep)" if sharded_sweep else "")) if world > 1 else "none")), "id_layout_nparts": nparts,
                   "exchange_fell_back_to_broadcasts": bool(ex is not None and ex.no_fast_path and not native),
                   "device_order": "native" if args.native_layout else "degree-ranked, dealt over shards",
                   "col_tiles": int(g.col_tiles),
                   "graph_build": ("distributed: each rank generates E/N edges, edges shuffled to the shard owning their row" if local_build
                                   else ("every rank sorts the whole edge list" if world > 1 else "single GPU")),
                   "graph_build_s": round(build_s, 2),
                   "rows_per_shard": S, "exchanged_rows_per_shard": int(g.xchg_rows),
                   "max_in_degree_rank0": max_deg,
                   "giant_row_groups_replayed": int(cnt64[0]), "giant_row_groups_serial": int(cnt64[1])},
        "iter_hbm_gbps": round(iter_bytes / (ms_per_step * 1e-3) / 1e9, 1),
        "iter_hbm_frac": round(iter_bytes / (ms_per_step * 1e-3) / 1e9 / (HBM_PEAK_GBPS * world), 4),
        # the same with the vertices that have an edge only (the degree-ranked device order puts the others behind every shard's live rows:
        # nothing of theirs is read or written): what the layout actually touches
        "iter_hbm_frac_live_vertices": round((4 * E + 48 * live_vertices) / (ms_per_step * 1e-3) / 1e9 / (HBM_PEAK_GBPS * world), 4),
        "live_vertices": live_vertices,
        "roofline": roof,
    }
    if multi_diag is not None:
        out["multi_gpu"] = multi_diag
    if args.debug_flags & ~(128 | 64 | 32 | 16):  # flags that only choose between exact strategies keep the result valid
        out["INVALID_ablation_debug_flags"] = args.debug_flags
    if rank == 0 and world == 1 and args.cpu_scale > 0:
        out["cpu_baseline"] = cpu_baseline(args.cpu_scale, args.cpu_iters, rank, args.cpu_scale2)
    elif rank == 0:
        out["cpu_baseline"] = None
    if rank == 0 and world == 1 and not args.no_extra:
        # the other single-GPU configurations of BASELINE.json, measured by the same run
        g.close()
        del st
        torch.cuda.empty_cache()
        extra = {}
        try:
            extra["bfs_rmat%d" % args.scale] = extra_bfs(args.scale, args.edge_factor, args.seed, args.ref_threads, local_rank, rank)
        except Exception as e:  # pragma: no cover
            extra["bfs_rmat%d" % args.scale] = {"error": repr(e)}
        try:
            extra["sgd_k128"] = extra_sgd(args.sgd_users, args.sgd_items, 100, 3, local_rank, rank)
        except Exception as e:  # pragma: no cover
            extra["sgd_k128"] = {"error": repr(e)}
        try:
            extra["pagerank_uniform25"] = extra_uniform(25, 16, 1, local_rank, rank)
        except Exception as e:  # pragma: no cover
            extra["pagerank_uniform25"] = {"error": repr(e)}
        out["extra"] = extra
    if rank == 0:
        r = roof or {}
        log(rank, "summary scale=%d gpus=%d dbg=%d ms/step=%.3f GTEPS=%.1f rowblock=%.3fms wave=%.3fms giant=%.3fms send=%.3f "
                  "apply=%.3f replayed=%d serial=%d edges(rb/wave/giant)=%d/%d/%d rows(blk/wave/giant)=%d/%d/%d" % (args.scale, world, args.debug_flags, ms_per_step, gteps,
                                                        r.get("rowblock_avg_ms", 0), r.get("wave_avg_ms", 0), r.get("aux_streams_avg_ms_overlapped", 0),
                                                        r.get("send_avg_ms", 0), r.get("apply_avg_ms", 0), int(cnt64[0]), int(cnt64[1]),
                                                        e_short, e_mid, e_giant, c_out.nblk, c_out.nmid, c_out.ngiant))
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

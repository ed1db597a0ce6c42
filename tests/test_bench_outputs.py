"""bench.py --dump-outputs: the files hold what the timed path computed (the PageRank state after warm-up + timed steps,
as Graph.pagerank returns it), the same bits from run to run, and --steps is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, STEPS, WARMUP = 12, 3, 2


def _bench(outdir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", str(SCALE), "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--cpu-scale", "0", "--no-extra", "--dump-outputs", str(outdir)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    return line, {n: np.load(os.path.join(str(outdir), n + ".npy")) for n in ("vertex", "pagerank", "out_degree")}


def test_bench_dumps_the_timed_path_outputs(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import api
    line, got = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert got["vertex"].dtype == np.float64 and got["pagerank"].dtype == np.float32 and got["out_degree"].dtype == np.float64
    nv = 1 << SCALE
    assert np.array_equal(got["vertex"], np.arange(1, nv + 1, dtype=np.float64))  # small graph: every vertex
    # the same graph and the same number of iterations through the library's caller-facing path
    nv_, s, d, _ = api.rmat_on_device(SCALE, 16, 1, weights=False, device=0)
    g = api.Graph(nv_, s, d, None, ref_threads=1, device=0, keep_values=False)
    pr, deg, it = g.pagerank(WARMUP + STEPS)
    g.close()
    assert nv_ == nv and it == WARMUP + STEPS
    assert np.array_equal(got["pagerank"].view(np.uint32), np.ascontiguousarray(pr, np.float32).view(np.uint32))
    assert np.array_equal(got["out_degree"], deg.astype(np.float64))
    # same arguments, same inputs, same bits
    _, again = _bench(tmp_path / "b")
    for n in got:
        assert np.array_equal(got[n].view(np.uint8), again[n].view(np.uint8)), n

"""bench.py's output contract on a small workload: one JSON line with the keys the driver reads, at N = 1 and in a
two-rank rehearsal (both ranks on the one GPU of the test box, barrier / MAX over gloo -- the driver's own multi-GPU
runs use nccl, one rank per GPU; the code path around the timed region is the same); a plain run carries none of the
--full legs, and --dump-outputs writes the same y from run to run -- the oracle's, on host-regenerated inputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line():
    _gpu()
    env = dict(os.environ, SPX_NO_BUILD="1")
    p = subprocess.run([sys.executable, "bench.py", "--steps", "5", "--warmup", "2", "--elements", "4000000", "--no-extra",
                        "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    assert KEYS <= set(d) and "cpu_baseline" in d
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert d["value"] > 0 and d["higher_is_better"] is True and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0
    assert "workload" in d["config"]


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    _gpu()
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle
    n, env = 4000000, dict(os.environ, SPX_NO_BUILD="1")
    ys = []
    for run in ("a", "b"):
        d = tmp_path / run
        p = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--elements", str(n), "--dump-outputs", str(d)],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        line = _line(p.stdout)
        assert KEYS <= set(line) and line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert not {"cpu_baseline", "other_operators", "solver_iteration_in_a_graph", "cpu_port_other_configs"} & set(line)
        assert sorted(os.listdir(d)) == ["y.npy", "y_index.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 2**20
        y, idx = np.load(d / "y.npy"), np.load(d / "y_index.npy")
        assert y.dtype == np.float64 and idx.dtype == np.float64 and y.shape == idx.shape
        assert 0 < y.size <= bench.DUMP_SAMPLE < n and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
        ys.append((y, idx))
    (ya, ia), (yb, ib) = ys
    assert np.array_equal(ia, ib) and np.array_equal(ya.view(np.int64), yb.view(np.int64))
    xh, sh, qh = (oracle.synth_fill(n, bench.SYNTH_SEED, stream, kind, 1.0, 4) for stream, kind in ((0, 1), (1, 0), (2, 1)))
    ref = oracle.prox_l1_box(qh, xh, sh, 1.0, 1.0, -1.0, 1.0)
    assert np.array_equal(ya.view(np.int64), ref[ia.astype(np.int64)].view(np.int64))


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_two_rank_rehearsal():
    _gpu()
    env = dict(os.environ, SPX_NO_BUILD="1", SPX_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "5",
                        "--warmup", "2", "--elements", "4000000", "--no-extra", "--no-cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    d = _line(p.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    # whole-job value = elements of BOTH ranks / max-over-ranks time
    assert d["value"] > 0 and abs(d["value"] - 2 * 4000000 * 5 / (d["ms_per_step"] * 5 * 1e-3) / 1e9) <= 0.02 * d["value"]

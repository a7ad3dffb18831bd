"""bench.py --master local[N]: BASELINE.json config 1 (the reference's own
CPU mode, ConfArguments.scala:54-56) -- the line vs_baseline is measured
against (profiles/r6/config1_local2.json).  CPU only."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_local_bench_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--master", "local[2]", "--steps", "2",
                        "--warmup", "1", "--batch", "3000", "--profile", "bench", "--features", "1000"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "p50_microbatch_latency_ms"):
        assert k in d, k
    assert d["n_gpus"] == 0 and d["dtype"] == "fp64" and d["steps"] == 2
    assert d["config"]["parallelism"] == "cpu local[2]" and d["config"]["global_batch"] == 3000
    assert d["value"] > 0 and d["p50_microbatch_latency_ms"] > 0 and d["host_threads"] == 1
    assert d["trained_tweets_per_step"] > 0


def test_cpu_local_bench_dumps_outputs(tmp_path):
    """--dump-outputs: the model and the last timed batch's results as float64
    .npy files, the same from run to run (seeded inputs, fp64 engine)."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--master", "local[2]", "--steps", "2",
                            "--warmup", "1", "--batch", "3000", "--profile", "bench", "--features", "1000",
                            "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        runs.append({f.stem: np.load(f) for f in sorted(out.glob("*.npy"))})
    a, b = runs
    assert set(a) == {"weights", "stats", "loss_history", "batch_results"}
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["weights"].shape == (1004,) and np.abs(a["weights"]).max() > 0
    assert a["batch_results"][0] == 3000 and a["stats"][0] == a["batch_results"][1] > 0
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_cpu_local_bench_rejects_other_masters():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--master", "yarn"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "local[N]" in p.stderr

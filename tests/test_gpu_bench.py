"""bench.py contract on one MI355X: one JSON line with the driver's fields,
the end-to-end default, the pre-packed device pipeline and the config-5 HBM
micro-batch sizing (``--batch hbm``, ops/sizing.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
          "scaling", "vs_baseline", "dtype", "data", "config"}


def _bench(*args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert FIELDS <= set(d), FIELDS - set(d)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["higher_is_better"] is True
    return d


@pytest.mark.parametrize("mode", [[], ["--prepacked"]], ids=["e2e", "prepacked"])
def test_bench_json_line(hip_module, mode):
    d = _bench("--batch", "100000", "--steps", "3", "--warmup", "1", "--pool", "2", "--full", *mode)
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["replicas_identical"] is True
    assert d["config"]["global_batch"] == 100000
    assert ("e2e" in d["ingest"]) == (not mode)
    # the timed window starts with an empty pipeline
    assert d["prestaged_at_t0"] == 0
    assert d["comm_world"] == 1 and len(d["per_rank_value"]) == 1
    assert d["per_rank_host"][0]["pinned_mb"] > 0
    # the window's H2D bytes (engine counter, ~150-200 B per wide tweet) and
    # the host-link floor they imply at this box's measured pinned bandwidth
    assert 100 < d["h2d_bytes_per_tweet"] < 400, d["h2d_bytes_per_tweet"]
    assert 20 < d["h2d_gbps"] < 200 and 0 < d["h2d_floor_ms_per_step"] <= d["ms_per_step"] * 1.05


def test_bench_plain_run_dumps_outputs(hip_module, tmp_path):
    """A plain run (no --full) measures nothing beside its steps, and
    --dump-outputs writes the last timed step's model and batch results as
    float64 .npy; the inputs are seeded, so a second run writes the same."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        d = _bench("--batch", "20000", "--features", "10000", "--steps", "2", "--warmup", "1",
                   "--dump-outputs", str(out))
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        assert not {"h2d_gbps", "h2d_floor_ms_per_step", "replicas_identical"} & set(d)
        arrs = {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}
        assert set(arrs) == {"weights", "stats", "loss_history", "batch_results"}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) < 64 << 20
        runs.append(arrs)
    a, b = runs
    assert a["weights"].shape == (10004,) and np.abs(a["weights"]).max() > 0
    # n_raw, n_kept of the last batch; its prequential count is the kept rows
    assert a["batch_results"][0] == 20000 and 0 < a["batch_results"][1] <= 20000
    assert a["stats"].shape == (6,) and a["stats"][0] == a["batch_results"][1]
    np.testing.assert_array_equal(a["batch_results"][:2], b["batch_results"][:2])
    # fp32 gradient sums may round differently from run to run: 1e-3 of the model's scale
    np.testing.assert_allclose(a["weights"], b["weights"], rtol=0, atol=1e-3 * np.abs(a["weights"]).max())


def test_bench_force_dp_reports_the_collective(hip_module):
    """--force-dp: the engine's DP path through a world-1 RCCL communicator;
    the JSON shows the gradient all-reduces per step and their time."""
    d = _bench("--batch", "100000", "--steps", "3", "--warmup", "1", "--pool", "2", "--force-dp")
    assert d["config"]["parallelism"] == "dp1-forced" and d["comm_kind"] == "rccl"
    assert d["comm_world"] == 1 and d["grad_allreduce_per_step"] >= 1
    assert d["grad_allreduce_us_per_iter"] > 0
    assert d["comm_counters"]["allgather_calls"] >= 3 + 1


def test_bench_hbm_batch_sizing(hip_module):
    d = _bench("--batch", "hbm", "--batch-cap", "131072", "--steps", "2", "--warmup", "1", "--pool", "2")
    s = d["config"]["batch_sizing"]
    assert s["hbm_max_rows"] >= 131072          # 288 GB holds far more than the cap
    assert d["config"]["global_batch"] == 131072

"""Streaming logistic regression on the MI355X engine (``loss="logistic"``).

The oracle is the fp64 CPU implementation
(``models/logistic_regression.py``: MLlib ``LogisticGradient`` inside
``GradientDescent.runMiniBatchSGD``).  The GPU path is the linear engine's
exact fixed-point GD with the logistic row epilogue (``csrc/hip/sgd.hip``,
``row_residual<kLossLogistic>``), 0/1 labels from the featurizer and the link
functions of ``csrc/hip/score.hip``.

Bounds against the oracle are the project's LR-vs-oracle bounds
(``test_gpu_lr_engine.py::test_sgd_matches_oracle_over_batches``): iterations
within +-1, ``|w_gpu - w| <= 1e-6 |w|`` at equal iteration counts and ``3e-3
|w|`` otherwise, elementwise ``rtol 2e-3, atol 2e-4 max|w|``.
"""
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.models.logistic_regression import (labels_of, logistic_gradient,
                                                              run_minibatch_sgd_logistic)
from twitter_stream_ml_amd.oracle import featurize_batch, featurize_batch_native
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000_000
STEP = 0.1
LABEL_THRESHOLD = 550


def _cfg(F, **kw):
    from twitter_stream_ml_amd.ops.lr_engine import LRDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, "step_size": STEP, "label_threshold": LABEL_THRESHOLD, **kw}
    return LRDeviceConfig(num_text_features=F, loss="logistic", **kw)


def _engine(F, **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression
    return DeviceLogisticRegression(_cfg(F, **kw), device=0)


def _assert_weights_close(wg, w, it_gpu, it_ref, what=""):
    """The LR-vs-oracle bounds (module docstring)."""
    assert abs(it_gpu - it_ref) <= 1, (what, it_gpu, it_ref)
    tol = 1e-6 if it_gpu == it_ref else 3e-3
    err = np.linalg.norm(wg - w)
    print(f"{what}: iterations {it_gpu} / {it_ref}, |dw| / |w| = {err / max(np.linalg.norm(w), 1e-30):.3e}")
    assert err <= tol * max(np.linalg.norm(w), 1e-30), (what, err, np.linalg.norm(w))
    np.testing.assert_allclose(wg, w, rtol=2e-3, atol=2e-4 * max(np.abs(w).max(), 1e-12))


def _mismatch_rate(res):
    return float(np.mean(np.asarray(res["pred"], np.float64) != np.asarray(res["real"], np.float64)))


# ---------------------------------------------------------------------------
# 1. oracle parity over warm-started batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol,want_iters", [(1e-3, [50, 50, 50]), (1e-2, [21, 23, 21])])
def test_matches_oracle_over_batches(hip_module, tol, want_iters):
    """twitter profile, seed 9, F = 1000, 3 x 3000 rows, step 0.1,
    labelThreshold 550; the oracle continues from its own weights.  At tol
    1e-3 every batch runs all 50 iterations, at 1e-2 the oracle converges
    after 21, 23 and 21 (the convergence path)."""
    F = 1000
    cfg = SynthConfig.profile("twitter", seed=9)
    eng = _engine(F, tol=tol, num_iterations=50)
    w = np.zeros(F + 4)
    for t in range(3):
        raw = generate_batch(cfg, t * 3000, 3000, batch_time_ms=NOW + t * 5000)
        fb = featurize_batch(raw, F, 100, 1000)
        y = labels_of(fb.y, LABEL_THRESHOLD)
        assert 0.47 <= y.mean() <= 0.49, y.mean()
        margin = np.asarray(fb.X @ w).reshape(-1)
        cls_o = (margin > 0.0).astype(np.float64)
        res = eng.train_batch(raw, want_pred=True)
        assert res["n_kept"] == fb.n and not res["diverged"]
        # prequential classes under the pre-training weights
        pred_g = np.asarray(res["pred"], np.float64)
        np.testing.assert_array_equal(np.asarray(res["real"], np.float64), y)
        diff = pred_g != cls_o
        print(f"batch {t}: {int(diff.sum())} of {fb.n} classes differ, max |margin| among them "
              f"{np.abs(margin[diff]).max() if diff.any() else 0.0:.3e}")
        assert diff.mean() < 0.01, diff.mean()
        assert np.all(np.abs(margin[diff]) <= 1e-3)
        n, sy, sy2, sp, sp2, se2 = res["stats"]
        assert n == fb.n and sy == y.sum()
        assert se2 / n == _mismatch_rate(res)
        assert sp == pred_g.sum() and sp2 == pred_g.sum() and sy2 == y.sum()
        # training
        r = run_minibatch_sgd_logistic(fb.X, y, w, STEP, 50, 1.0, tol)
        assert r.iterations == want_iters[t]
        w = r.weights
        _assert_weights_close(eng.get_weights(), w, res["iterations"], r.iterations, f"tol {tol} batch {t}")
        k = min(len(res["loss_history"]), len(r.loss_history))
        assert k >= want_iters[t] - 1
        np.testing.assert_allclose(res["loss_history"][:k], r.loss_history[:k], rtol=2e-3)
        if res["iterations"] < 50:
            assert res["converged"]


# ---------------------------------------------------------------------------
# 2. exact class predictions
# ---------------------------------------------------------------------------
def _dyadic_weights(F, seed=4):
    """Text weights k / 64, |k| <= 64, numeric weights 0: a row's fixed-point
    dot is then exact (and exact in fp64), so its sign is too."""
    w = np.zeros(F + 4)
    w[:F] = np.random.default_rng(seed).integers(-64, 65, F) / 64.0
    return w


@pytest.fixture(scope="module")
def exact_cases():
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    cases = [("classes-homogeneous", eb.length_class_batch(True)[0]),
             ("classes-straddling", eb.length_class_batch(False)[0]),
             ("empty-rows", eb.empty_rows_batch())]
    cases += [(f"tiny-{n}", raw) for raw, n in zip(eb.tiny_batches(synth), eb.TINY_SIZES)]
    cases.append(("none-kept", generate_batch(SynthConfig.profile("twitter", seed=1, retweet_fraction=0.0), 0, 500,
                                              batch_time_ms=NOW)))
    cases.append(("generator", generate_batch(synth, 0, 3000, batch_time_ms=NOW)))
    return cases


def test_class_predictions_exact(hip_module, exact_cases):
    """Every kept row's class equals the oracle's: no exclusions."""
    F = 1000
    w = _dyadic_weights(F)
    eng = _engine(F, num_iterations=1)
    total = ones = 0
    for name, raw in exact_cases:
        fb = featurize_batch_native(raw, F, 100, 1000, now_ms=raw.batch_time_ms)
        cls_o = (np.asarray(fb.X @ w).reshape(-1) > 0.0).astype(np.float32)
        eng.set_weights(w)
        res = eng.train_batch(raw, want_pred=True)
        assert res["n_kept"] == fb.n, name
        if fb.n == 0:
            assert res["pred"] is None or len(res["pred"]) == 0
            continue
        np.testing.assert_array_equal(np.asarray(res["pred"]), cls_o, err_msg=name)
        np.testing.assert_array_equal(np.asarray(res["real"]), labels_of(fb.y, LABEL_THRESHOLD).astype(np.float32),
                                      err_msg=name)
        total += fb.n
        ones += int(cls_o.sum())
    assert 0.2 * total < ones < 0.8 * total   # both classes are exercised


# ---------------------------------------------------------------------------
# 3. bitwise layout independence
# ---------------------------------------------------------------------------
def _run(profile, rows, nb, seed, monkeypatch=None, env=None, **kw):
    if monkeypatch is not None:
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
    eng = _engine(1 << 20, max_rows=rows, max_units=rows * 300, **kw)
    if monkeypatch is not None:
        for k in (env or {}):
            monkeypatch.delenv(k)
    synth = SynthConfig.profile(profile, seed=seed)
    meta = []
    for t in range(nb):
        raw = generate_batch(synth, t * rows, rows, batch_time_ms=NOW + t * 5000)
        r = eng.train_batch(raw, want_pred=True)
        assert not r["diverged"]
        meta.append((r["iterations"], bool(r["tiered"]), r["n_near"], list(r["stats"]), list(r["loss_history"]),
                     np.asarray(r["pred"]).copy()))
    w = eng.get_weights()
    del eng
    return w, meta


def _same(a, b):
    wa, ma = a
    wb, mb = b
    for (ia, _, _, sa, la, pa), (ib, _, _, sb, lb, pb) in zip(ma, mb):
        assert ia == ib
        assert sa == sb
        assert la == lb
        np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(wa, wb)


@pytest.fixture(scope="module")
def bench_default(hip_module):
    a = _run("bench", 20000, 2, seed=14)
    assert not a[1][0][1] and np.abs(a[0]).max() > 0
    return a


def test_hybrid_vs_plain_layout_bitwise(hip_module, bench_default):
    _same(bench_default, _run("bench", 20000, 2, seed=14, hybrid=False))


@pytest.mark.parametrize("grid", [1, 7])
def test_grid_split_bitwise(hip_module, bench_default, grid):
    _same(bench_default, _run("bench", 20000, 2, seed=14, sgd_grid=grid))


def test_forced_tiered_vs_hybrid_bitwise(hip_module, bench_default, monkeypatch):
    b = _run("bench", 20000, 2, seed=14, monkeypatch=monkeypatch,
             env={"TWTML_FORCE_TIERED": "1", "TWTML_NEAR_CAP": "256"})
    assert b[1][0][1]
    _same(bench_default, b)


def test_dedup_vs_off_bitwise(hip_module, bench_default):
    _same(bench_default, _run("bench", 20000, 2, seed=14, dedup=True))


def test_near_tier_size_bitwise(hip_module, monkeypatch):
    a = _run("wide", 20000, 2, seed=13)
    assert a[1][0][1]                       # tiered
    b = _run("wide", 20000, 2, seed=13, monkeypatch=monkeypatch, env={"TWTML_NEAR_CAP": "512"})
    assert b[1][0][2] == 512
    _same(a, b)


def test_fraction_sampling_matches_oracle(hip_module):
    F = 1000
    raw = generate_batch(SynthConfig.profile("twitter", seed=9), 0, 3000, batch_time_ms=NOW)
    fb = featurize_batch(raw, F, 100, 1000)
    y = labels_of(fb.y, LABEL_THRESHOLD)
    eng = _engine(F, fraction=0.5, num_iterations=10)
    res = eng.train_batch(raw)
    r = run_minibatch_sgd_logistic(fb.X, y, np.zeros(F + 4), STEP, 10, mini_batch_fraction=0.5)
    assert res["iterations"] == r.iterations
    _assert_weights_close(eng.get_weights(), r.weights, res["iterations"], r.iterations, "fraction 0.5")


# ---------------------------------------------------------------------------
# 4. DP
# ---------------------------------------------------------------------------
def test_dp_loopback_equals_single_engine(hip_module):
    """Two loopback engines on the shards of each batch == one engine on the
    whole batch, bit for bit (the logistic residual depends on the row alone)."""
    from test_gpu_dp_loopback import _run_dp
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression
    cfg = _cfg(1 << 20, num_iterations=20)
    synth = SynthConfig.profile("twitter", seed=33, unicode_fraction=0.2)
    batches = [generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(3)]
    engines, res = _run_dp(2, batches, cfg)
    single = DeviceLogisticRegression(cfg, device=0)
    for t, full in enumerate(batches):
        r1 = single.train_batch(full, want_pred=False)
        for r in range(2):
            assert res[r][t]["n_kept_global"] == r1["n_kept"]
            assert res[r][t]["iterations"] == r1["iterations"]
            assert list(res[r][t]["stats"]) == list(r1["stats"])
            assert list(res[r][t]["loss_history"]) == list(r1["loss_history"])
    w1 = single.get_weights()
    assert np.abs(w1).max() > 0
    for r in range(2):
        np.testing.assert_array_equal(engines[r].get_weights(), w1)


def test_forced_dp_rccl_equals_plain_engine(hip_module):
    """The DP branches over a world-1 RCCL communicator: bit-identical to the
    plain engine, one packed int64 all-reduce per GD iteration."""
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression
    h = hip_module
    comm = h.Comm(h.rccl_unique_id(), 0, 1, 0)
    synth = SynthConfig.profile("twitter", seed=70)
    nb = 3
    batches = [generate_batch(synth, t * 6000, 6000, batch_time_ms=NOW + t * 5000) for t in range(nb)]
    base = dict(num_iterations=20, tol=1e-2)
    dp = DeviceLogisticRegression(_cfg(1 << 20, force_dp=True, **base), device=0, comm=comm)
    plain = DeviceLogisticRegression(_cfg(1 << 20, **base), device=0)
    comm_iters = 0
    for b in batches:
        a, p = dp.train_batch(b, want_pred=True), plain.train_batch(b, want_pred=True)
        assert (a["iterations"], a["n_kept"], a["n_kept_global"]) == (p["iterations"], p["n_kept"], p["n_kept"])
        assert list(a["stats"]) == list(p["stats"])
        assert list(a["loss_history"]) == list(p["loss_history"])
        np.testing.assert_array_equal(np.asarray(a["pred"]), np.asarray(p["pred"]))
        # the host enqueues up to early_exit_depth iterations past the verdict;
        # those keep their (paired) collectives
        assert a["iterations"] <= a["comm_iters"] <= a["iterations"] + 4 and p["comm_iters"] == 0
        comm_iters += a["comm_iters"]
    np.testing.assert_array_equal(dp.get_weights(), plain.get_weights())
    c = comm.counters()
    # gradient all-reduces + two stats all-reduces per batch (+ the in-line
    # active-set size all-reduce of a batch not gathered ahead)
    assert comm_iters + 2 * nb <= c["allreduce_calls"] <= comm_iters + 3 * nb
    assert c["allgather_calls"] == nb


# ---------------------------------------------------------------------------
# 5. saturation and degenerate labels
# ---------------------------------------------------------------------------
def test_saturated_margins_stay_finite(hip_module):
    """Text weights of +-1024: margins reach +-1e5, far beyond exp's range."""
    F = 1000
    raw = generate_batch(SynthConfig.profile("twitter", seed=9), 0, 3000, batch_time_ms=NOW)
    fb = featurize_batch(raw, F, 100, 1000)
    y = labels_of(fb.y, LABEL_THRESHOLD)
    w = np.zeros(F + 4)
    w[:F] = np.where(np.random.default_rng(2).random(F) < 0.5, -1024.0, 1024.0)
    margin = np.asarray(fb.X @ w).reshape(-1)
    assert np.abs(margin).max() > 5e4 and (margin > 88).any() and (margin < -88).any()
    eng = _engine(F, num_iterations=5)
    eng.set_weights(w)
    res = eng.train_batch(raw, want_pred=True)
    # |w| ~ 3e4: the second update already moves w by less than tol |w| (the oracle stops there too)
    r = run_minibatch_sgd_logistic(fb.X, y, w, STEP, 5)
    assert not res["diverged"] and abs(res["iterations"] - r.iterations) <= 1 and res["iterations"] >= 2
    assert np.isfinite(eng.get_weights()).all() and np.isfinite(res["loss_history"]).all()
    _, loss0, m = logistic_gradient(fb.X, y, w)
    print(f"first loss: gpu {res['loss_history'][0]!r}, oracle {loss0 / m!r}")
    np.testing.assert_allclose(res["loss_history"][0], loss0 / m, rtol=1e-5)
    np.testing.assert_array_equal(np.asarray(res["pred"], np.float64), (margin > 0.0).astype(np.float64))


@pytest.mark.parametrize("label_threshold,label", [(1001, 0.0), (100, 1.0)], ids=["all-zero", "all-one"])
def test_degenerate_labels_match_oracle(hip_module, label_threshold, label):
    """labelThreshold above `end` (every label 0) and at `begin` (every label 1)."""
    F = 1000
    raw = generate_batch(SynthConfig.profile("twitter", seed=9), 0, 3000, batch_time_ms=NOW)
    fb = featurize_batch(raw, F, 100, 1000)
    y = labels_of(fb.y, label_threshold)
    assert np.all(y == label)
    eng = _engine(F, label_threshold=label_threshold, num_iterations=20)
    res = eng.train_batch(raw, want_pred=True)
    assert res["stats"][1] == y.sum() and not res["diverged"]
    r = run_minibatch_sgd_logistic(fb.X, y, np.zeros(F + 4), STEP, 20)
    _assert_weights_close(eng.get_weights(), r.weights, res["iterations"], r.iterations, f"labels {label}")
    k = min(len(res["loss_history"]), len(r.loss_history))
    np.testing.assert_allclose(res["loss_history"][:k], r.loss_history[:k], rtol=2e-3)


def test_tiny_and_empty_batches(hip_module):
    """0, 1, 2, 15, 16, 17, 63, 64 and 65 kept rows, warm-started one after
    the other; a fully filtered batch leaves the model bit-identical."""
    F = 1000
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    eng = _engine(F, num_iterations=20)
    w = np.zeros(F + 4)
    for raw, n in zip(eb.tiny_batches(synth), eb.TINY_SIZES):
        fb = featurize_batch(raw, F, 100, 1000)
        y = labels_of(fb.y, LABEL_THRESHOLD)
        assert fb.n == n
        eng.set_weights(w)                     # the oracle's weights: each size is checked on its own
        res = eng.train_batch(raw, want_pred=True)
        assert res["n_kept"] == n and res["stats"][0] == n and res["stats"][1] == y.sum()
        r = run_minibatch_sgd_logistic(fb.X, y, w, STEP, 20)
        w = r.weights
        _assert_weights_close(eng.get_weights(), w, res["iterations"], r.iterations, f"{n} rows")
    before = eng.get_weights()
    none = generate_batch(SynthConfig.profile("twitter", seed=1, retweet_fraction=0.0), 0, 500, batch_time_ms=NOW)
    res = eng.train_batch(none, want_pred=True)
    assert res["n_kept"] == 0 and res["iterations"] == 0 and res["stats"][0] == 0
    np.testing.assert_array_equal(eng.get_weights(), before)


# ---------------------------------------------------------------------------
# 6. scoring
# ---------------------------------------------------------------------------
def _ulp_diff(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.abs(ia - ib)


def test_scoring_links(hip_module):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    F = 1000
    rng = np.random.default_rng(7)
    w = rng.standard_normal(F + 4) * 0.3
    w[F:] = rng.standard_normal(4) * 1e7
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    raws = eb.tiny_batches(synth) + [generate_batch(synth, 0, 3000, batch_time_ms=NOW)]
    lin = DeviceLinearRegression(LRDeviceConfig(num_text_features=F, max_rows=8192, max_units=8192 * 300), device=0)
    lin.set_weights(w)
    engs = {tau: _engine(F, threshold=tau) for tau in (0.5, 0.2)}
    for e in engs.values():
        e.set_weights(w)
    for raw in raws:
        for flt in (False, True):
            m0 = lin.predict_batch(raw, apply_filter=flt)
            m = engs[0.5].predict_batch(raw, apply_filter=flt, output="margin")
            np.testing.assert_array_equal(m["rows"], m0["rows"])
            np.testing.assert_array_equal(m["pred"], m0["pred"])          # today's scores, bit for bit
            margins = np.asarray(m["pred"], np.float64)
            p = engs[0.5].predict_batch(raw, apply_filter=flt, output="probability")["pred"]
            with np.errstate(over="ignore"):
                want = 1.0 / (1.0 + np.exp(-margins))
            assert p.dtype == np.float64 and _ulp_diff(p, want).max(initial=0) <= 4
            for tau, e in engs.items():
                c = e.predict_batch(raw, apply_filter=flt)["pred"]       # default output: the class
                np.testing.assert_array_equal(c, (margins > math.log(tau / (1.0 - tau))).astype(np.float64))
    big = raws[-1]
    margins = engs[0.5].predict_batch(big, output="margin")["pred"]
    lo, hi = math.log(0.2 / 0.8), 0.0
    assert ((margins > lo) & (margins <= hi)).any()      # the two thresholds tell rows apart
    with pytest.raises(ValueError):
        engs[0.5].predict_batch(big, output="logit")


def test_scoring_between_batches_leaves_training_alone(hip_module):
    F = 1000
    synth = SynthConfig.profile("twitter", seed=21)
    raws = [generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t * 5000) for t in range(2)]
    a, b = _engine(F, num_iterations=20), _engine(F, num_iterations=20)
    ra = [a.train_batch(raws[0], want_pred=True)]
    for out in ("class", "probability", "margin"):
        a.predict_batch(raws[1], output=out)
    ra.append(a.train_batch(raws[1], want_pred=True))
    rb = [b.train_batch(r, want_pred=True) for r in raws]
    for x, y in zip(ra, rb):
        assert x["iterations"] == y["iterations"] and list(x["stats"]) == list(y["stats"])
        assert list(x["loss_history"]) == list(y["loss_history"])
        np.testing.assert_array_equal(np.asarray(x["pred"]), np.asarray(y["pred"]))
    np.testing.assert_array_equal(a.get_weights(), b.get_weights())


# ---------------------------------------------------------------------------
# 7. squared loss untouched
# ---------------------------------------------------------------------------
def test_squared_is_the_default_and_unchanged(hip_module):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    assert LRDeviceConfig().loss == "squared" and LRDeviceConfig().as_dict()["loss"] == 0
    base = dict(num_text_features=1 << 20, max_rows=8192, max_units=8192 * 300)
    a = DeviceLinearRegression(LRDeviceConfig(**base), device=0)
    b = DeviceLinearRegression(LRDeviceConfig(loss="squared", **base), device=0)
    synth = SynthConfig.profile("twitter", seed=5, unicode_fraction=0.1)
    for t in range(3):
        raw = generate_batch(synth, t * 2500, 2500, batch_time_ms=NOW + t * 5000)
        ra, rb = a.train_batch(raw, want_pred=True), b.train_batch(raw, want_pred=True)
        assert ra["iterations"] == rb["iterations"] and list(ra["stats"]) == list(rb["stats"])
        assert list(ra["loss_history"]) == list(rb["loss_history"])
        np.testing.assert_array_equal(np.asarray(ra["pred"]), np.asarray(rb["pred"]))
        assert np.asarray(ra["real"]).max() >= 100          # labels are retweet counts, not classes
    np.testing.assert_array_equal(a.get_weights(), b.get_weights())
    with pytest.raises(ValueError):
        DeviceLinearRegression(LRDeviceConfig(loss="hinge", **base), device=0)


# ---------------------------------------------------------------------------
# 8. driver
# ---------------------------------------------------------------------------
CLOCK = "manual:1700000000000:5000"


def _driver_args(master, ck, batches=4):
    return ["--master", master, "--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
            "--seconds", "0", "--batchSize", "3000", "--sourceRate", "0", "--numBatches", str(batches),
            "-f", "2048", "-i", "20", "-p", "0.1", "--labelThreshold", "550",
            "--checkpoint", str(ck), "--checkpointInterval", "2"]


def _metrics(path):
    import json
    return [r for r in (json.loads(l) for l in open(path)) if not r.get("summary")]


def test_driver_gpu_matches_cpu_and_resumes(hip_module, tmp_path, monkeypatch):
    from twitter_stream_ml_amd.apps import logistic_regression as app
    from twitter_stream_ml_amd.checkpoint import load_progress
    from twitter_stream_ml_amd.models.logistic_regression import LogisticRegressionModel
    monkeypatch.setenv("TWTML_STREAMING_CLOCK", CLOCK)
    monkeypatch.setenv("TWTML_METRICS", str(tmp_path / "cpu.jsonl"))
    assert app.main(_driver_args("local[2]", tmp_path / "cpu")) == 0
    monkeypatch.setenv("TWTML_METRICS", str(tmp_path / "gpu.jsonl"))
    assert app.main(_driver_args("rocm[1]", tmp_path / "gpu")) == 0
    mc, mg = _metrics(tmp_path / "cpu.jsonl"), _metrics(tmp_path / "gpu.jsonl")
    assert len(mc) == len(mg) == 4
    for a, b in zip(mc, mg):
        assert a["batch"] == b["batch"] and abs(a["iterations"] - b["iterations"]) <= 1, (a, b)
    m_cpu = LogisticRegressionModel.load(str(tmp_path / "cpu"))
    m_gpu = LogisticRegressionModel.load(str(tmp_path / "gpu"))
    assert m_gpu.threshold == 0.5 and m_gpu.weights.shape == (2052,)
    assert load_progress(str(tmp_path / "gpu"))["batches"] == 4
    same = all(a["iterations"] == b["iterations"] for a, b in zip(mc, mg))
    _assert_weights_close(m_gpu.weights, m_cpu.weights, 0 if same else 1, 0, "driver")
    # --resume auto: 2 batches, then on to 4 == the uninterrupted run
    monkeypatch.setenv("TWTML_METRICS", str(tmp_path / "res.jsonl"))
    ck = tmp_path / "res"
    assert app.main(_driver_args("rocm[1]", ck, batches=2)) == 0
    assert load_progress(str(ck))["batches"] == 2
    assert app.main(_driver_args("rocm[1]", ck, batches=4) + ["--resume", "auto"]) == 0
    assert load_progress(str(ck))["batches"] == 4
    w_res = LogisticRegressionModel.load(str(ck)).weights
    assert np.linalg.norm(w_res - m_gpu.weights) <= 1e-6 * np.linalg.norm(m_gpu.weights)

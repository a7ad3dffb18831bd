"""Streaming logistic regression on the CPU: the fp64 implementation
(``models/logistic_regression.py``) that is the oracle of the MI355X logistic
path, its MLlib API, checkpoints and the ``local[N]`` driver.

Reference semantics: MLlib 1.6 ``LogisticGradient`` (binary) --
``margin = -x.w``, multiplier ``1 / (1 + exp(margin)) - y``, loss
``log1pExp(margin)`` for y > 0 and ``log1pExp(margin) - margin`` otherwise --
inside ``GradientDescent.runMiniBatchSGD`` with ``SquaredL2Updater`` at
``regParam = 0`` (arithmetically ``SimpleUpdater``).
"""
import json
import math
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from twitter_stream_ml_amd.apps import logistic_regression as lg_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.checkpoint import (LOGISTIC_CLASS, load_linear_regression, load_logistic_regression,
                                              model_class, save_logistic_regression)
from twitter_stream_ml_amd.models.linear_regression import featurize_columnar
from twitter_stream_ml_amd.models.logistic_regression import (CpuLogisticConfig, CpuLogisticRegression,
                                                              LogisticRegressionModel,
                                                              StreamingLogisticRegressionWithSGD, labels_of,
                                                              logistic_gradient, run_minibatch_sgd_logistic)
from twitter_stream_ml_amd.runtime.streaming import StreamingContext
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = 1_700_000_000_000
F = 1000


def test_logistic_gradient_hand_computed():
    """3 rows, 2 features, w = (ln 2, -ln 3): dots ln 2, -ln 3, ln 2 - 2 ln 3 =
    ln(2/9); sigma = 2/3, 1/4, 2/11; labels 1, 0, 1."""
    X = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 2.0]]))
    y = np.array([1.0, 0.0, 1.0])
    w = np.array([math.log(2.0), -math.log(3.0)])
    g, loss, m = logistic_gradient(X, y, w)
    r = np.array([2 / 3 - 1, 1 / 4 - 0, 2 / 11 - 1])
    np.testing.assert_allclose(g, [r[0] + r[2], r[1] + 2 * r[2]], rtol=1e-14)
    # -ln sigma for y = 1, -ln(1 - sigma) for y = 0
    np.testing.assert_allclose(loss, -math.log(2 / 3) - math.log(3 / 4) - math.log(2 / 11), rtol=1e-14)
    assert m == 3
    # a mask samples rows
    g2, loss2, m2 = logistic_gradient(X, y, w, np.array([True, False, True]))
    np.testing.assert_allclose(g2, [r[0] + r[2], 2 * r[2]], rtol=1e-14)
    assert m2 == 2 and loss2 < loss


def test_logistic_gradient_saturates_cleanly():
    """Margins of +-1e4: exp would overflow; the residual is exactly -y or
    1 - y and the loss |dot| or 0, all finite."""
    X = sp.csr_matrix(np.array([[1e4], [1e4], [-1e4], [-1e4]]))
    y = np.array([1.0, 0.0, 1.0, 0.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):   # exp(-1e4) underflows to 0: intended
        g, loss, m = logistic_gradient(X, y, np.array([1.0]))
    mult = np.array([1.0 - 1.0, 1.0 - 0.0, 0.0 - 1.0, 0.0 - 0.0])     # sigma = 1, 1, 0, 0
    assert g[0] == float((X.T @ mult)[0]) and np.isfinite(g).all()
    assert loss == 0.0 + 1e4 + 1e4 + 0.0
    assert m == 4


def _threaded_allreduce(world):
    """A gloo-style sum over `world` threads: every rank gets the parts added
    in rank order (``parallel.dist.allreduce_fn``)."""
    parts = [None] * world
    bar = threading.Barrier(world)

    def make(rank):
        def red(v):
            parts[rank] = np.array(v, dtype=np.float64, copy=True)
            bar.wait()
            out = parts[0].copy()
            for p in parts[1:]:
                out += p
            bar.wait()
            return out
        return red
    return [make(r) for r in range(world)]


@pytest.mark.parametrize("world,fraction", [(2, 1.0), (3, 1.0), (3, 0.6)])
def test_sharded_sgd_equals_one_rank(world, fraction):
    raw = generate_batch(SynthConfig.profile("twitter", seed=17), 0, 1500, batch_time_ms=NOW)
    X, rt, _ = featurize_columnar(raw, F, 100, 1000)
    y = labels_of(rt, 550)
    assert 0.3 < y.mean() < 0.7
    one = run_minibatch_sgd_logistic(X, y, np.zeros(F + 4), 0.1, 15, fraction)
    n = y.shape[0]
    cuts = [n * r // world for r in range(world + 1)]
    reds = _threaded_allreduce(world)
    out = [None] * world

    def worker(r):
        lo, hi = cuts[r], cuts[r + 1]
        out[r] = run_minibatch_sgd_logistic(X[lo:hi], y[lo:hi], np.zeros(F + 4), 0.1, 15, fraction,
                                            allreduce=reds[r], row_offset=lo)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    for r in range(world):
        assert out[r] is not None and out[r].iterations == one.iterations and out[r].num_examples == n
        np.testing.assert_allclose(out[r].weights, one.weights, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(out[r].loss_history, one.loss_history, rtol=1e-12)
        np.testing.assert_array_equal(out[r].weights, out[0].weights)   # replicas hold the same bits


def test_training_lowers_the_loss_and_converges():
    raw = generate_batch(SynthConfig.profile("twitter", seed=9), 0, 3000, batch_time_ms=NOW)
    X, rt, _ = featurize_columnar(raw, F, 100, 1000)
    y = labels_of(rt, 550)
    r = run_minibatch_sgd_logistic(X, y, np.zeros(F + 4), 0.1, 50, convergence_tol=1e-2)
    assert r.loss_history[0] == pytest.approx(math.log(2.0))      # zero weights: ln 2 per row
    assert r.loss_history[-1] < r.loss_history[0]
    assert r.converged and r.iterations < 50


def test_saveable_round_trip_and_metadata(tmp_path):
    w = np.zeros(F + 4)
    w[[3, 17, F + 1]] = [0.5, -2.0, 1e7]
    for thr in (0.5, 0.2, None):
        path = str(tmp_path / f"m{thr}")
        LogisticRegressionModel(w, 0.0, thr).save(path, {"batches": 3})
        meta = json.loads(open(f"{path}/metadata/part-00000").readline())
        assert meta == {"class": "org.apache.spark.mllib.classification.LogisticRegressionModel",
                        "version": "1.0", "numFeatures": F + 4, "numClasses": 2}
        assert model_class(path) == LOGISTIC_CLASS
        w2, b, t2 = load_logistic_regression(path)
        np.testing.assert_array_equal(w2, w)
        assert b == 0.0 and t2 == thr
        m = LogisticRegressionModel.load(path)
        assert m.threshold == thr and m.numFeatures == F + 4 and m.numClasses == 2
        import pyarrow.parquet as pq
        t = pq.read_table(f"{path}/data/part-00000.parquet")
        assert t.column_names == ["weights", "intercept", "threshold"] and t.num_rows == 1
        assert t.schema.field("threshold").nullable
    with pytest.raises(ValueError, match="expected class"):
        load_linear_regression(path)      # a logistic directory is not a LinearRegressionModel
    from twitter_stream_ml_amd.checkpoint import SparseWeights
    save_logistic_regression(str(tmp_path / "s"), SparseWeights(F + 4, [3, 17, F + 1], [0.5, -2.0, 1e7]))
    np.testing.assert_array_equal(load_logistic_regression(str(tmp_path / "s"))[0], w)


def test_model_predict_and_thresholds():
    m = LogisticRegressionModel(np.array([1.0, -1.0]))
    X = np.array([[2.0, 0.0], [0.0, 2.0], [0.0, 0.0], [1e4, 0.0], [0.0, 1e4]])
    np.testing.assert_array_equal(m.predict(X), [1.0, 0.0, 0.0, 1.0, 0.0])   # p > 0.5; p == 0.5 is class 0
    m.setThreshold(0.1)
    np.testing.assert_array_equal(m.predict(X), [1.0, 1.0, 1.0, 1.0, 0.0])
    m.clearThreshold()
    np.testing.assert_allclose(m.predict(X), [1 / (1 + math.exp(-2)), 1 / (1 + math.exp(2)), 0.5, 1.0, 0.0])
    from twitter_stream_ml_amd.models.vectors import Vectors
    assert m.predict(Vectors.dense([0.0, 0.0])) == 0.5


def test_predict_on_raw_stream():
    """predictOn over a raw DStream: one engine call per batch, unfiltered
    classes in record order; probabilities after clearThreshold."""
    synth = SynthConfig.profile("twitter", seed=3)
    raws = [generate_batch(synth, t * 300, 300, batch_time_ms=NOW + t) for t in range(2)]
    eng = CpuLogisticRegression(CpuLogisticConfig(num_text_features=F, num_iterations=5))
    w = np.random.default_rng(1).standard_normal(F + 4) * 0.1
    model = StreamingLogisticRegressionWithSGD(engine=eng).setInitialWeights(w)
    ssc = StreamingContext(batch_seconds=1.0)
    stream = ssc.receiverStream(None)
    got = []
    model.predictOn(stream).foreachRDD(lambda rdd: got.append(rdd.collect()))
    ssc.run_batch(raws[0])
    X, _, rows = featurize_columnar(raws[0], F, 100, 1000, apply_filter=False)
    margins = np.asarray(X @ w).reshape(-1)
    assert len(got[0]) == raws[0].n
    np.testing.assert_array_equal(got[0], (margins > 0.0).astype(np.float64))
    assert 0 < sum(got[0]) < raws[0].n
    model.latestModel().clearThreshold()
    ssc.run_batch(raws[1])
    X, _, _ = featurize_columnar(raws[1], F, 100, 1000, now_ms=NOW + 1, apply_filter=False)
    np.testing.assert_allclose(got[1], 1.0 / (1.0 + np.exp(-np.asarray(X @ w).reshape(-1))), rtol=1e-14)


def test_cpu_engine_batch_contract():
    """Prequential classes under the weights before training, 0/1 labels at
    labelThreshold (default: the middle of the filter range), then training."""
    cfg = CpuLogisticConfig(num_text_features=F, num_iterations=10)
    assert cfg.label_threshold == 550 and cfg.step_size == 0.1
    eng = CpuLogisticRegression(cfg)
    raw = generate_batch(SynthConfig.profile("twitter", seed=5), 0, 2000, batch_time_ms=NOW)
    res = eng.train_batch(raw, want_pred=True)
    X, rt, _ = featurize_columnar(raw, F, 100, 1000)
    y = labels_of(rt, 550)
    n, sy, sy2, sp_, sp2, se2 = res["stats"]
    assert (n, sy, sy2) == (y.shape[0], y.sum(), y.sum())
    assert sp_ == 0.0 and se2 == y.sum()                # zero weights: every row class 0
    np.testing.assert_array_equal(res["real"], y.astype(np.float32))
    assert res["iterations"] == 10 and res["loss_history"][0] == pytest.approx(math.log(2.0))
    w1 = eng.get_weights()
    res2 = eng.train_batch(raw, want_pred=True)
    cls = (np.asarray(X @ w1).reshape(-1) > 0.0).astype(np.float64)   # the classes under the first batch's model
    assert res2["stats"][3] == cls.sum() and res2["stats"][5] == np.sum((y - cls) ** 2)
    assert cls.sum() > 0                                # the model moved: no longer the all-zero guess
    for out in ("class", "probability", "margin"):
        p = eng.predict_batch(raw, output=out)["pred"]
        assert p.shape == (raw.n,)
    with pytest.raises(ValueError):
        eng.predict_batch(raw, output="logit")


def test_nonzero_reg_param_raises():
    with pytest.raises(ValueError, match="regParam"):
        StreamingLogisticRegressionWithSGD(regParam=0.01)
    m = StreamingLogisticRegressionWithSGD()
    assert (m.stepSize, m.numIterations, m.miniBatchFraction, m.regParam) == (0.1, 50, 1.0, 0.0)
    with pytest.raises(ValueError, match="regParam"):
        m.setRegParam(1e-6)
    assert m.setRegParam(0.0) is m


def test_logistic_driver_local2_checkpoint_resume_and_score(tmp_path, monkeypatch):
    metrics = tmp_path / "m.jsonl"
    monkeypatch.setenv("TWTML_METRICS", str(metrics))
    ck = tmp_path / "model"
    common = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
              "--seconds", "0.2", "--sourceRate", "4000", "-f", "1000", "-p", "0.1"]
    args = ["--master", "local[2]", "--numBatches", "3", "--checkpoint", str(ck), "--checkpointInterval", "2",
            "--labelThreshold", "400", "--threshold", "0.4"] + common
    assert lg_app.main(args) == 0
    recs = [json.loads(l) for l in open(metrics)]
    recs = [r for r in recs if not r.get("summary")]
    assert len(recs) == 3 and all(r["batch"] > 0 for r in recs)
    # percent: the misclassification rate and the stdevs of 0/1 values
    assert all(0 <= r["mse"] <= 100 and 0 <= r["realStdev"] <= 50 and 0 <= r["predStdev"] <= 50 for r in recs)
    assert recs[0]["predStdev"] == 0                     # zero weights: one class
    m = LogisticRegressionModel.load(str(ck))
    assert m.weights.shape == (1004,) and m.threshold == 0.4 and np.abs(m.weights).max() > 0
    w1 = m.weights
    assert lg_app.main(args + ["--resume", str(ck)]) == 0
    assert not np.array_equal(LogisticRegressionModel.load(str(ck)).weights, w1)
    # twtml-score picks the output by the model class: 0/1 classes under the saved threshold
    out = tmp_path / "pred"
    assert score_app.main(["--master", "local[1]", "--numBatches", "2", "--model", str(ck),
                           "--predictOut", str(out)] + common) == 0
    for seq in range(2):
        pred = np.load(out / f"pred_{seq}.npy")
        assert pred.size > 0 and set(np.unique(pred)) <= {0.0, 1.0}

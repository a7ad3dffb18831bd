"""Inference-only scoring on the CPU engine, ``predictOn`` over a raw tweet
stream and the ``apps.score`` driver (``local[N]``).

The reference for every prediction is the fp64 oracle
``featurize_batch_native(...).X @ w``.
"""
import json
import os

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.apps import linear_regression as lr_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.checkpoint import load_linear_regression
from twitter_stream_ml_amd.models.linear_regression import (CpuLinearRegression, CpuLRConfig,
                                                            StreamingLinearRegressionWithSGD)
from twitter_stream_ml_amd.oracle import featurize_batch_native
from twitter_stream_ml_amd.runtime.streaming import StreamingContext
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = eb.NOW
F = 1000


def _weights(seed=7):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(F + 4)
    w[F:] = rng.standard_normal(4) * 1e7   # the numeric features are ~1e-7: both parts matter
    return w


def _oracle(raw, w, apply_filter, hash="java", now=NOW):
    fb = featurize_batch_native(raw, F, 100, 1000, now_ms=now, hash=hash, apply_filter=apply_filter)
    return fb.rows, np.asarray(fb.X @ w).reshape(-1)


def _batches():
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    tiny = eb.tiny_batches(synth)
    return tiny + [eb.with_junk_rows(tiny[-1])]


@pytest.mark.parametrize("hash", ["java", "murmur3"])
@pytest.mark.parametrize("apply_filter", [False, True])
def test_cpu_predict_batch_equals_oracle(apply_filter, hash):
    eng = CpuLinearRegression(CpuLRConfig(num_text_features=F, hash=hash))
    w = _weights()
    eng.set_weights(w)
    for raw in _batches():
        res = eng.predict_batch(raw, apply_filter=apply_filter)
        rows, pred = _oracle(raw, w, apply_filter, hash)
        assert res["n_raw"] == raw.n and res["n_scored"] == rows.shape[0]
        assert res["rows"].dtype == np.int64 and res["pred"].dtype == np.float64
        np.testing.assert_array_equal(res["rows"], rows)
        # the same CSR product up to the order scipy sums a row in
        np.testing.assert_allclose(res["pred"], pred, rtol=1e-12, atol=1e-9)
        if not apply_filter:
            np.testing.assert_array_equal(res["rows"], np.arange(raw.n))
    np.testing.assert_array_equal(eng.get_weights(), w)   # scoring leaves the model alone
    # now_ms moves the age feature only
    raw = _batches()[3]
    a = eng.predict_batch(raw, now_ms=NOW)["pred"]
    b = eng.predict_batch(raw, now_ms=NOW + 10 ** 9)["pred"]
    np.testing.assert_allclose(b - a, 10 ** 9 * 1e-14 * w[F + 3], rtol=1e-6)


def test_cpu_predict_batch_empty():
    eng = CpuLinearRegression(CpuLRConfig(num_text_features=F))
    raw = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    res = eng.predict_batch(raw)
    assert res["n_raw"] == 0 and res["n_scored"] == 0
    assert res["rows"].shape == (0,) and res["pred"].shape == (0,)


def test_predict_on_raw_stream_uses_current_weights():
    """predictOn over a raw DStream: one engine call per batch, unfiltered, in
    record order, evaluated lazily with the weights current at that point."""
    synth = SynthConfig.profile("twitter", seed=3)
    raws = [generate_batch(synth, t * 300, 300, batch_time_ms=NOW + t) for t in range(3)]
    eng = CpuLinearRegression(CpuLRConfig(num_text_features=F, num_iterations=5))
    model = StreamingLinearRegressionWithSGD(engine=eng).setInitialWeights(_weights(1) * 1e-3)
    calls = []
    inner = eng.predict_batch
    eng.predict_batch = lambda raw, **kw: (calls.append(raw.n), inner(raw, **kw))[1]

    ssc = StreamingContext(batch_seconds=1.0)
    stream = ssc.receiverStream(None)
    got = []
    model.predictOn(stream).foreachRDD(lambda rdd: got.append(rdd.collect()))

    w0 = eng.get_weights()
    ssc.run_batch(raws[0])
    assert calls == [300]                      # one engine call for the batch
    np.testing.assert_allclose(got[0], _oracle(raws[0], w0, False, now=NOW)[1], rtol=1e-12, atol=1e-12)
    assert len(got[0]) == raws[0].n            # unfiltered: every record

    eng.train_batch(raws[1], want_pred=False)  # the model moves between two predictions
    w1 = eng.get_weights()
    assert not np.array_equal(w0, w1)
    ssc.run_batch(raws[1])
    want_new = _oracle(raws[1], w1, False, now=NOW + 1)[1]
    want_old = _oracle(raws[1], w0, False, now=NOW + 1)[1]
    np.testing.assert_allclose(got[1], want_new, rtol=1e-12, atol=1e-12)
    assert np.abs(np.asarray(got[1]) - want_old).max() > 1e-6

    # lazy: the RDD of batch 2 is built first, the model then changes, and the
    # predictions are those of the weights at evaluation time
    rdd = model.predictOn(stream).compute(raws[2])
    eng.set_weights(w0)
    np.testing.assert_allclose(rdd.collect(), _oracle(raws[2], w0, False, now=NOW + 2)[1], rtol=1e-12, atol=1e-12)


def test_predict_on_without_raw_is_unchanged():
    from twitter_stream_ml_amd.models.vectors import LabeledPoint, Vectors
    from twitter_stream_ml_amd.runtime.rdd import RDD
    from twitter_stream_ml_amd.runtime.streaming import DStream
    model = StreamingLinearRegressionWithSGD().setInitialWeights(np.array([1.0, 2.0, 3.0]))
    ssc = StreamingContext(batch_seconds=1.0)
    pts = [LabeledPoint(0.0, Vectors.dense([1.0, 0.0, 1.0])), LabeledPoint(1.0, Vectors.dense([0.0, 1.0, 0.0]))]
    src = DStream(ssc, None, lambda r: RDD(pts))
    assert model.predictOn(src).compute(None).collect() == [4.0, 2.0]


def test_score_driver_local(tmp_path):
    ck = tmp_path / "model"
    common = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
              "--seconds", "0.2", "--sourceRate", "3000", "-f", "1000"]
    assert lr_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(ck)] + common) == 0
    w, _ = load_linear_regression(str(ck))
    out = tmp_path / "pred"
    rc = score_app.main(["--master", "local[2]", "--numBatches", "3", "--model", str(ck),
                         "--predictOut", str(out)] + common)
    assert rc == 0
    recs = [json.loads(l) for l in open(out / "predictions.jsonl")]
    assert [r["seq"] for r in recs] == [0, 1, 2]
    for r in recs:
        pred = np.load(out / f"pred_{r['seq']}.npy")
        rows = np.load(out / f"rows_{r['seq']}.npy")
        assert pred.dtype == np.float64 and rows.dtype == np.int64
        assert pred.shape == rows.shape == (r["count"],) and r["count"] > 0
        np.testing.assert_array_equal(rows, np.arange(r["count"]))   # unfiltered, record order
        assert r["min"] <= r["mean"] <= r["max"] and r["ms"] >= 0 and "batch_time_ms" in r
        assert r["mean"] == pytest.approx(float(pred.mean()))
    # the model on disk is the one that was loaded: scoring never writes it
    w2, _ = load_linear_regression(str(ck))
    np.testing.assert_array_equal(w, w2)
    assert sorted(os.listdir(out)) == sorted(["predictions.jsonl"] + [f"{k}_{i}.npy" for k in ("pred", "rows")
                                                                    for i in range(3)])


def test_score_driver_rejects_feature_mismatch(tmp_path, capsys):
    ck = tmp_path / "model"
    common = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
              "--seconds", "0.2", "--sourceRate", "3000"]
    assert lr_app.main(["--master", "local[1]", "--numBatches", "1", "--checkpoint", str(ck), "-f", "1000"]
                       + common) == 0
    rc = score_app.main(["--master", "local[2]", "--numBatches", "1", "--model", str(ck), "-f", "2000",
                         "--predictOut", str(tmp_path / "p")] + common)
    assert rc != 0
    assert "1004" in capsys.readouterr().err
    assert not (tmp_path / "p").exists()
    assert score_app.main(["--master", "local[2]"] + common) != 0   # no --model

"""K-means scoring on the CPU engine and the ``apps.score`` driver with a
KMeansModel directory (``local[N]``).

``CpuKMeans.predict_batch`` is the fp64 oracle of the GPU scoring tests; here
it is held to its own parts: ``kmeans_features``, ``standard_scaler_fit`` /
``standard_scaler_transform``, ``find_closest`` and direct squared differences.
"""
import json
import os

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.apps import kmeans as km_app
from twitter_stream_ml_amd.apps import linear_regression as lr_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.models.kmeans import CpuKMeans, StreamingKMeansModel, kmeans_features
from twitter_stream_ml_amd.oracle.mllib import (KMeansState, find_closest, standard_scaler_fit,
                                                standard_scaler_transform)
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = eb.NOW
SERVICES = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]


def _raw(rows=600, seed=21):
    return generate_batch(SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.2), 0, rows,
                          batch_time_ms=NOW)


def _engine(k, text_dims, seed=5, **kw):
    eng = CpuKMeans(k, 2 + text_dims, seed=seed, **kw)
    st = KMeansState.random(k, 2 + text_dims, 0.0, seed=seed)
    eng.set_state(st.centers, st.weights)
    return eng


@pytest.mark.parametrize("k,text_dims", [(1, 0), (3, 0), (7, 5), (40, 14)])
@pytest.mark.parametrize("apply_filter", [True, False])
def test_predict_batch_oracle_identities(k, text_dims, apply_filter):
    raw = _raw()
    eng = _engine(k, text_dims)
    c0, w0 = eng.get_state()
    res = eng.predict_batch(raw, text_dims, apply_filter=apply_filter)
    X, rows = kmeans_features(raw, text_dims, apply_filter=apply_filter)
    if apply_filter:
        np.testing.assert_array_equal(rows, np.nonzero(raw.is_retweet != 0)[0])
        Xd, rd = kmeans_features(raw, text_dims)   # the default keeps today's result
        np.testing.assert_array_equal(Xd, X)
        np.testing.assert_array_equal(rd, rows)
    else:
        np.testing.assert_array_equal(rows, np.arange(raw.n))
    assert res["n_raw"] == raw.n and res["n_scored"] == rows.shape[0] > 0
    np.testing.assert_array_equal(res["rows"], rows)
    std = standard_scaler_fit(X)
    np.testing.assert_array_equal(res["std"], std)
    Xs = standard_scaler_transform(X, std)
    want = find_closest(c0, Xs)
    np.testing.assert_array_equal(res["pred"], want)
    np.testing.assert_array_equal(res["dist2"], ((Xs - c0[want]) ** 2).sum(axis=1))
    assert res["cost"] == res["dist2"].sum()
    np.testing.assert_array_equal(res["sizes"], np.bincount(res["pred"], minlength=k))
    assert res["rows"].dtype == np.int64 and res["pred"].dtype == np.int32
    assert res["dist2"].dtype == np.float64 and res["sizes"].dtype == np.int64
    assert res["sizes"].shape == (k,) and res["sizes"].sum() == res["n_scored"]
    c1, w1 = eng.get_state()   # scoring leaves the model alone
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(w0, w1)


def test_predict_batch_scaler_modes():
    k, td = 5, 3
    raw = _raw()
    eng = _engine(k, td)
    c = eng.get_state()[0]
    X, _ = kmeans_features(raw, td)
    # none: the unscaled features
    r = eng.predict_batch(raw, td, scaler="none")
    assert r["std"] is None
    want = find_closest(c, X)
    np.testing.assert_array_equal(r["pred"], want)
    np.testing.assert_array_equal(r["dist2"], ((X - c[want]) ** 2).sum(axis=1))
    # an engine that does not scale: "batch" means "none"
    r2 = _engine(k, td, scale=False).predict_batch(raw, td)
    assert r2["std"] is None
    np.testing.assert_array_equal(r2["dist2"], r["dist2"])
    # given, with a zero entry: factor 0, the column contributes c_j^2
    std = np.array([3.0, 0.0, 2.0, 0.5, 7.0])
    r = eng.predict_batch(raw, td, scaler=std)
    np.testing.assert_array_equal(r["std"], std)
    Xs = X / np.array([3.0, 1.0, 2.0, 0.5, 7.0])
    Xs[:, 1] = 0.0
    want = find_closest(c, Xs)
    np.testing.assert_array_equal(r["pred"], want)
    np.testing.assert_allclose(r["dist2"], ((Xs - c[want]) ** 2).sum(axis=1), rtol=1e-13)
    keep = [0, 2, 3, 4]
    # (a difference of two sums of dist2's size: absolute error ~1e-16 of them)
    np.testing.assert_allclose(r["dist2"] - ((Xs[:, keep] - c[want][:, keep]) ** 2).sum(axis=1),
                               c[want, 1] ** 2, rtol=0, atol=1e-13 * r["dist2"].max())
    # a frozen scaler makes a row's result depend on the row alone
    half = eng.predict_batch(raw.shard(0, 2), td, scaler=std)
    np.testing.assert_array_equal(half["dist2"], r["dist2"][:half["n_scored"]])
    np.testing.assert_array_equal(half["pred"], r["pred"][:half["n_scored"]])
    with pytest.raises(ValueError):
        eng.predict_batch(raw, td, scaler=np.ones(4))
    with pytest.raises(ValueError):
        eng.predict_batch(raw, td, scaler="frozen")
    with pytest.raises(ValueError):
        eng.predict_batch(raw, td + 1)


def test_predict_batch_one_row_and_empty():
    k, td = 6, 4
    eng = _engine(k, td)
    c = eng.get_state()[0]
    synth = SynthConfig.profile("twitter", seed=27, unicode_fraction=0.2)
    one = eb.kmeans_tiny_batch(synth, 1, 10000)
    r = eng.predict_batch(one, td)
    assert r["n_scored"] == 1 and not np.any(r["std"])   # one row: every std is 0, every factor 0
    best = int(np.argmin((c ** 2).sum(axis=1)))
    np.testing.assert_array_equal(r["pred"], [best])
    np.testing.assert_array_equal(r["dist2"], [(c[best] ** 2).sum()])
    # unfiltered, the same batch has 5 rows
    assert eng.predict_batch(one, td, apply_filter=False)["n_scored"] == one.n == 5
    # no retweets / no rows: empty arrays, cost 0, sizes all zero
    none_rt = eb.texts_to_raw([one.text_of(i) for i in range(one.n)], np.zeros(one.n, np.uint8), one.scalars, NOW)
    empty = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    for raw, n_raw in ((none_rt, 5), (empty, 0)):
        r = eng.predict_batch(raw, td)
        assert r["n_raw"] == n_raw and r["n_scored"] == 0 and r["cost"] == 0.0 and r["std"] is None
        assert r["rows"].shape == r["pred"].shape == r["dist2"].shape == (0,)
        assert r["pred"].dtype == np.int32 and r["rows"].dtype == np.int64
        np.testing.assert_array_equal(r["sizes"], np.zeros(k, np.int64))


def _train_kmeans(ck, k=4, text_dims=6):
    args = ["--master", "local[2]", "--k", str(k), "--textDims", str(text_dims), "--numBatches", "3",
            "--seconds", "0.2", "--sourceRate", "3000", "--checkpoint", str(ck), "--checkpointInterval", "1"]
    assert km_app.main(args) == 0
    return StreamingKMeansModel.load(str(ck))


def test_score_driver_kmeans_local(tmp_path):
    from twitter_stream_ml_amd.sources import write_jsonl
    k, td = 4, 6
    ck = tmp_path / "km"
    model = _train_kmeans(ck, k, td)
    assert model.clusterCenters.shape == (k, 2 + td)
    # a recorded stream: the driver's batches are these, 500 tweets each
    synth = SynthConfig.profile("twitter", seed=13, unicode_fraction=0.2)
    raws = [generate_batch(synth, t * 500, 500, batch_time_ms=NOW + t) for t in range(3)]
    write_jsonl(str(tmp_path / "stream.jsonl"), [s for raw in raws for s in raw.to_statuses()])
    common = SERVICES + ["--source", f"replay:{tmp_path / 'stream.jsonl'}", "--seconds", "0", "--batchSize", "500",
                         "--sourceRate", "0", "--numBatches", "3", "--master", "local[2]", "--model", str(ck)]
    oracle = CpuKMeans(k, 2 + td)
    oracle.set_state(model.clusterCenters, model.clusterWeights)
    std = np.array([50.0, 2e4, 0.0, 1.0, 2.0, 1.5, 1.0, 3.0])
    np.save(tmp_path / "std.npy", std)
    for name, extra, scaler in (("batch", [], "batch"), ("frozen", ["--scalerStd", str(tmp_path / "std.npy")], std)):
        out = tmp_path / name
        assert score_app.main(common + ["--predictOut", str(out)] + extra) == 0
        recs = [json.loads(l) for l in open(out / "predictions.jsonl")]
        assert [r["seq"] for r in recs] == [0, 1, 2]
        for r, raw in zip(recs, raws):
            pred = np.load(out / f"pred_{r['seq']}.npy")
            dist2 = np.load(out / f"dist2_{r['seq']}.npy")
            rows = np.load(out / f"rows_{r['seq']}.npy")
            assert pred.dtype == np.int32 and dist2.dtype == np.float64 and rows.dtype == np.int64
            assert pred.shape == dist2.shape == rows.shape == (r["count"],) and r["count"] > 0
            assert r["cost"] == dist2.sum()                      # the jsonl cost is the saved distances' sum
            assert r["mean_cost"] == pytest.approx(r["cost"] / r["count"])
            assert r["clusters_used"] == np.unique(pred).size
            assert r["ms"] >= 0 and "batch_time_ms" in r and "score_ms" in r
            want = oracle.predict_batch(raw, td, apply_filter=True, scaler=scaler)   # the isRetweet filter is on
            np.testing.assert_array_equal(rows, want["rows"])
            np.testing.assert_array_equal(pred, want["pred"])
            np.testing.assert_array_equal(dist2, want["dist2"])
        assert sorted(os.listdir(out)) == sorted(["predictions.jsonl"] + [f"{n}_{i}.npy" for i in range(3)
                                                                        for n in ("pred", "dist2", "rows")])
    # the model on disk is the one that was loaded: scoring never writes it
    again = StreamingKMeansModel.load(str(ck))
    np.testing.assert_array_equal(again.clusterCenters, model.clusterCenters)
    np.testing.assert_array_equal(again.clusterWeights, model.clusterWeights)


def test_score_driver_kmeans_usage_errors(tmp_path, capsys):
    common = SERVICES + ["--seconds", "0.2", "--sourceRate", "3000", "--numBatches", "1", "--master", "local[2]"]
    # an unreadable directory is still the usage error
    assert score_app.main(common + ["--model", str(tmp_path / "missing")]) == 2
    # a width the engine does not take
    wide = tmp_path / "wide"
    StreamingKMeansModel(np.zeros((2, 4003)), np.ones(2)).save(str(wide))
    assert score_app.main(common + ["--model", str(wide), "--predictOut", str(tmp_path / "p")]) == 2
    assert "4000" in capsys.readouterr().err
    narrow = tmp_path / "narrow"
    StreamingKMeansModel(np.zeros((2, 1)), np.ones(2)).save(str(narrow))
    assert score_app.main(common + ["--model", str(narrow)]) == 2
    # a scaler of the wrong length
    ok = tmp_path / "ok"
    StreamingKMeansModel(np.zeros((2, 2)), np.ones(2)).save(str(ok))
    np.save(tmp_path / "std3.npy", np.ones(3))
    assert score_app.main(common + ["--model", str(ok), "--scalerStd", str(tmp_path / "std3.npy")]) == 2
    assert score_app.main(common + ["--model", str(ok), "--scalerStd", str(tmp_path / "none.npy")]) == 2
    assert not (tmp_path / "p").exists()


def test_score_driver_linear_model_unchanged(tmp_path):
    """A linear-regression checkpoint still scores as before."""
    ck = tmp_path / "lr"
    common = SERVICES + ["--seconds", "0.2", "--sourceRate", "3000", "-f", "1000"]
    assert lr_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(ck)] + common) == 0
    out = tmp_path / "pred"
    assert score_app.main(["--master", "local[2]", "--numBatches", "2", "--model", str(ck),
                           "--predictOut", str(out)] + common) == 0
    recs = [json.loads(l) for l in open(out / "predictions.jsonl")]
    assert [r["seq"] for r in recs] == [0, 1] and set(recs[0]) >= {"mean", "min", "max", "count"}
    assert "cost" not in recs[0]
    for r in recs:
        pred = np.load(out / f"pred_{r['seq']}.npy")
        rows = np.load(out / f"rows_{r['seq']}.npy")
        assert pred.dtype == np.float64 and pred.shape == rows.shape == (r["count"],)
        np.testing.assert_array_equal(rows, np.arange(r["count"]))   # unfiltered, record order
    assert not [f for f in os.listdir(out) if f.startswith("dist2_")]

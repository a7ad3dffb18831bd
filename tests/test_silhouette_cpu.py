"""The silhouette contract (``models/silhouette.py``) on the CPU: the formulas
against the brute-force definition (pairwise squared distances), the
degenerate batches, the integer accumulator, the CPU engine and the
``local[1]`` driver.

Bound of the definition test.  ``D(x, G) = |x - mu_G|^2 + V_G`` equals the
mean of ``|x - y|^2`` over G exactly in real arithmetic; in fp64 both sides are
sums of at most n d non-negative terms of size <= max D, each rounded to
2^-53 relative, plus the mean's own rounding: far below ``1e-10 max D`` for
n <= 300, the bound asserted.
"""
import json

import numpy as np
import pytest

from twitter_stream_ml_amd.models import silhouette as S
from twitter_stream_ml_amd.models.kmeans import CpuKMeans, StreamingKMeansModel, kmeans_features
from twitter_stream_ml_amd.oracle.mllib import KMeansState, standard_scaler_transform
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

SERVICES = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]
NOW = 1_700_000_000_000


def _brute(X, pred, k):
    """a, b, s, neighbor by the definition: means of pairwise |x - y|^2."""
    n = X.shape[0]
    P = ((X[:, None, :] - X[None]) ** 2).sum(axis=2)
    N = np.bincount(pred, minlength=k)
    a, b, s = np.zeros(n), np.zeros(n), np.zeros(n)
    nb = np.full(n, -1)
    for p in range(n):
        own = pred[p]
        if N[own] > 1:
            a[p] = P[p, pred == own].sum() / (N[own] - 1)
        best = np.inf
        for g in range(k):
            if g == own or N[g] == 0:
                continue
            D = P[p, pred == g].mean()
            if D < best:
                best, nb[p] = D, g
        b[p] = best
        if N[own] == 1:
            s[p] = 0.0
        elif a[p] < b[p]:
            s[p] = 1.0 - a[p] / b[p]
        elif a[p] > b[p]:
            s[p] = b[p] / a[p] - 1.0
    return a, b, s, nb, P


def _case(n, k, d, seed):
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(k, d)) * 3.0
    pred = rng.integers(0, k, size=n)
    X = C[pred] + rng.normal(size=(n, d))
    return X, pred


@pytest.mark.parametrize("n,k,d,seed", [(300, 2, 3, 1), (257, 3, 5, 2), (300, 7, 16, 3), (40, 7, 2, 4)])
def test_formulas_match_the_pairwise_definition(n, k, d, seed):
    X, pred = _case(n, k, d, seed)
    # duplicated rows in one cluster (a = 0 for a pair), a singleton cluster, and labels
    # that are not the closest centre (a > b)
    X[pred == 0] = X[pred == 0][0] if k > 2 else X[pred == 0]
    lone = int(np.nonzero(pred == 1)[0][0])
    if k > 2:
        pred[(pred == 1) & (np.arange(n) != lone)] = 2
    pred[-5:] = (pred[-5:] + 1) % k if k == 2 else np.where(pred[-5:] == 1, 2, pred[-5:])
    r = S.batch_silhouette(X, pred, k)
    a, b, s, nb, P = _brute(X, pred, k)
    tol = 1e-10 * P.max()
    assert r["defined"]
    np.testing.assert_array_equal(r["neighbor"], nb)
    assert np.abs(r["a"] - a).max() <= tol and np.abs(r["b"] - b).max() <= tol
    # s: the quotient's sensitivity to a and b is 1 / max(a, b)
    safe = np.maximum(np.maximum(a, b), 1e-300)
    assert np.all(np.abs(r["s"] - s) <= 4 * tol / safe + 1e-15)
    np.testing.assert_array_equal(r["s"], S.point_silhouette(r["a"], r["b"]) * (r["N"][pred] != 1))
    if k > 2:
        assert r["N"][1] == 1 and r["s"][lone] == 0.0 and r["a"][lone] == 0.0 and r["neighbor"][lone] >= 0
        # duplicates: a = 0 up to the rounding of their mean
        assert np.all(a[pred == 0] == 0.0) and np.all(r["a"][pred == 0] <= tol)
        assert np.all(r["s"][pred == 0] >= 1.0 - tol / b[pred == 0])
    assert np.any(r["a"] > r["b"]) and np.any(r["a"] < r["b"])


def test_point_silhouette_branches():
    a = np.array([0.0, 1.0, 2.0, 3.0, 0.0])
    b = np.array([2.0, 2.0, 2.0, 2.0, 0.0])
    np.testing.assert_array_equal(S.point_silhouette(a, b), [1.0, 0.5, 0.0, 2.0 / 3.0 - 1.0, 0.0])
    # a == b: row 0 is as far from its only cluster mate as from both rows of the other cluster
    X = np.array([[0.0], [2.0], [2.0], [2.0]])
    r = S.batch_silhouette(X, np.array([0, 0, 1, 1]), 2)
    assert r["a"][0] == r["b"][0] == 4.0 and r["s"][0] == 0.0
    np.testing.assert_array_equal(r["a"], [4.0, 4.0, 0.0, 0.0])
    np.testing.assert_array_equal(r["b"], [4.0, 0.0, 2.0, 2.0])
    np.testing.assert_array_equal(r["s"], [0.0, -1.0, 1.0, 1.0])


def test_degenerate_batches():
    X, _ = _case(50, 3, 4, 7)
    r = S.batch_silhouette(X, np.full(50, 2), 3)
    assert not r["defined"] and np.all(r["neighbor"] == -1) and not r["s"].any()
    acc = S.SilhouetteAccumulator(3).add_undefined(50)
    assert acc.n_undefined == 50 and acc.silhouette is None and acc.n == [0, 0, 0] and acc.batches == 1
    assert acc.cluster_silhouette == [None, None, None]
    r = S.batch_silhouette(np.zeros((0, 4)), np.zeros(0, np.int64), 3)
    assert not r["defined"] and r["s"].shape == (0,)
    e = S.empty_silhouette(0, 3, per_row=True)
    assert e["silhouette"] is None and e["accumulator"].to_dict() == S.SilhouetteAccumulator(3).to_dict()
    assert e["neighbor"].dtype == np.int32 and e["s"].shape == (0,)
    # two non-empty clusters, one a singleton: defined
    r = S.batch_silhouette(X, np.r_[np.zeros(49, np.int64), 2], 3)
    assert r["defined"] and r["s"][-1] == 0.0 and np.all(r["neighbor"][:-1] == 2) and r["neighbor"][-1] == 0


def test_accumulator_is_exact_and_merges_in_any_order():
    k = 7
    parts = []
    for i in range(5):
        X, pred = _case(120 + i, k, 6, 20 + i)
        r = S.batch_silhouette(X, pred, k)
        parts.append((pred, r["s"]))
    whole = S.SilhouetteAccumulator(k)
    for pred, s in parts:
        whole.add_rows(pred, s)
    # s_fix is the sum of rint(s 2^36) per own cluster
    for g in range(k):
        want = sum(int(v) for pred, s in parts for v in np.rint(s[pred == g] * 2.0 ** 36))
        assert whole.s_fix[g] == want
        assert whole.n[g] == sum(int(np.count_nonzero(pred == g)) for pred, _ in parts)
    accs = [S.SilhouetteAccumulator(k).add_rows(pred, s) for pred, s in parts]
    accs.append(S.SilhouetteAccumulator(k).add_undefined(11))
    whole.add_undefined(11)
    for order in (accs, accs[::-1]):
        m = S.SilhouetteAccumulator(k)
        for a in order:
            m.merge(a)
        assert m == whole and m.to_dict() == whole.to_dict()
    n = sum(len(p) for p, _ in parts)
    mean = sum(float(s.sum()) for _, s in parts) / n
    assert abs(whole.silhouette - mean) <= 2.0 ** -36
    cs = whole.cluster_silhouette
    assert abs(sum(c * m for c, m in zip(cs, whole.n)) / n - whole.silhouette) <= 1e-15
    # JSON round trip, and totals beyond 2^63 stay exact
    back = S.SilhouetteAccumulator.from_dict(json.loads(json.dumps(whole.to_dict())))
    assert back == whole
    big = S.SilhouetteAccumulator(2)
    big.n, big.s_fix = [1 << 62, 3], [(1 << 62) * (1 << 36) - 5, -(3 << 36)]
    tot = S.SilhouetteAccumulator(2)
    for _ in range(4):
        tot.merge(big)
    assert tot.n[0] == 1 << 64 and tot.s_fix[0] == 4 * ((1 << 98) - 5) and tot.s_fix[0] > 1 << 63
    again = S.SilhouetteAccumulator.from_dict(json.loads(json.dumps(tot.to_dict())))
    assert again.s_fix == tot.s_fix and again.n == tot.n
    assert tot.cluster_silhouette[1] == -1.0 and abs(tot.silhouette - 1.0) < 1e-15
    with pytest.raises(ValueError):
        tot.merge(S.SilhouetteAccumulator(3))


def _raw(n=600, seed=11):
    return generate_batch(SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.2), 0, n, batch_time_ms=NOW)


@pytest.mark.parametrize("scaler", ["batch", "none", "given"])
def test_cpu_engine_equals_the_module_on_its_own_labels(scaler):
    k, td = 5, 6
    raw = _raw()
    cpu = CpuKMeans(k, 2 + td, seed=5)
    X, rows = kmeans_features(raw, td)
    if scaler == "given":
        scaler = X.std(axis=0, ddof=1)
    # centres at the scaled data's own scale, so several clusters are used
    pb = cpu.predict_batch(raw, td, scaler=scaler)
    Xs = X if pb["std"] is None else standard_scaler_transform(X, pb["std"])
    cpu.set_state(Xs[:: max(1, len(Xs) // k)][:k], np.ones(k))
    pb = cpu.predict_batch(raw, td, scaler=scaler)
    assert np.count_nonzero(pb["sizes"]) >= 2
    c0 = cpu.get_state()[0]
    res = cpu.silhouette_batch(raw, td, scaler=scaler, per_row=True)
    np.testing.assert_array_equal(cpu.get_state()[0], c0)
    want = S.batch_silhouette(Xs, pb["pred"], k)
    for key in ("a", "b", "s", "neighbor"):
        np.testing.assert_array_equal(res[key], want[key])
    np.testing.assert_array_equal(res["pred"], pb["pred"])
    np.testing.assert_array_equal(res["rows"], rows)
    np.testing.assert_array_equal(res["sizes"], pb["sizes"])
    assert res["cost"] == pb["cost"] and res["n_scored"] == X.shape[0] and res["n_raw"] == raw.n
    assert res["neighbor"].dtype == np.int32
    acc = res["accumulator"]
    assert acc == S.SilhouetteAccumulator(k).add_rows(pb["pred"], want["s"])
    assert acc.n == [int(v) for v in pb["sizes"]]
    assert res["silhouette"] == acc.silhouette and abs(res["silhouette"] - want["s"].mean()) <= 2.0 ** -36
    plain = cpu.silhouette_batch(raw, td, scaler=scaler)
    assert "s" not in plain and plain["accumulator"] == acc
    # one cluster holds everything: undefined
    cpu.set_state(np.r_[Xs[:1], np.full((k - 1, 2 + td), 1e9)], np.ones(k))
    res = cpu.silhouette_batch(raw, td, scaler=scaler, per_row=True)
    assert res["silhouette"] is None and res["accumulator"].n_undefined == X.shape[0]
    assert np.all(res["neighbor"] == -1) and not res["s"].any()
    # nothing kept, and no rows
    none = raw.slice(0, 0)
    res = cpu.silhouette_batch(none, td, scaler=scaler, per_row=True)
    assert res["n_scored"] == 0 and res["silhouette"] is None and res["accumulator"].batches == 0


def test_sklearn_cross_check():
    metrics = pytest.importorskip("sklearn.metrics")
    X, pred = _case(200, 4, 5, 9)
    r = S.batch_silhouette(X, pred, 4)
    np.testing.assert_allclose(r["s"], metrics.silhouette_samples(X, pred, metric="sqeuclidean"), atol=1e-10)


def test_score_driver_silhouette_out_local(tmp_path, capsys):
    from twitter_stream_ml_amd.apps import linear_regression as lr_app
    from twitter_stream_ml_amd.apps import score as score_app
    k, td = 4, 6
    st = KMeansState.random(k, 2 + td, 0.0, seed=5)
    ck = tmp_path / "km"
    StreamingKMeansModel(st.centers, np.ones(k)).save(str(ck))
    common = SERVICES + ["--seconds", "0.2", "--sourceRate", "3000", "--master", "local[1]"]
    out, pout = tmp_path / "sil", tmp_path / "pred"
    assert score_app.main(["--numBatches", "3", "--model", str(ck), "--silhouetteOut", str(out),
                           "--predictOut", str(pout)] + common) == 0
    lines = [json.loads(l) for l in open(out / "silhouette.jsonl")]
    assert len(lines) == 3 and [l["seq"] for l in lines] == [0, 1, 2]
    total = S.SilhouetteAccumulator(k)
    for l in lines:
        acc = S.SilhouetteAccumulator.from_dict(l["accumulator"])
        assert l["silhouette"] == acc.silhouette and l["n_single"] == acc.n_single
        assert l["n_undefined"] == acc.n_undefined and l["n_scored"] == acc.n_total + acc.n_undefined
        assert l["n_raw"] >= l["n_scored"] > 0 and l["cost"] > 0 and l["clusters_used"] >= 1
        total.merge(acc)
    summary = json.load(open(out / "summary.json"))
    assert summary["batches"] == 3 and summary["accumulator"] == total.to_dict()
    assert summary["silhouette"] == total.silhouette and summary["cluster_silhouette"] == total.cluster_silhouette
    preds = [json.loads(l) for l in open(pout / "predictions.jsonl")]
    assert [p["count"] for p in preds] == [l["n_scored"] for l in lines]
    assert [p["cost"] for p in preds] == [l["cost"] for l in lines]
    # alone (no predictions are written), with a frozen scaler
    std = tmp_path / "std.npy"
    np.save(std, np.r_[50.0, 4000.0, np.ones(td)])
    out2 = tmp_path / "sil_std"
    assert score_app.main(["--numBatches", "2", "--model", str(ck), "--silhouetteOut", str(out2),
                           "--scalerStd", str(std)] + common) == 0
    assert len(open(out2 / "silhouette.jsonl").readlines()) == 2
    assert json.load(open(out2 / "summary.json"))["batches"] == 2
    assert not (out2 / "predictions.jsonl").exists()
    # usage errors: a linear model, and --evalOut with a k-means model stays refused
    lin = tmp_path / "lin"
    assert lr_app.main(["--numBatches", "1", "--checkpoint", str(lin), "-f", "100"] + common) == 0
    capsys.readouterr()
    rc = score_app.main(["--numBatches", "1", "--model", str(lin), "-f", "100", "--silhouetteOut",
                         str(tmp_path / "no")] + common)
    assert rc == 2 and "--silhouetteOut" in capsys.readouterr().err and not (tmp_path / "no").exists()
    rc = score_app.main(["--numBatches", "1", "--model", str(ck), "--evalOut", str(tmp_path / "no2")] + common)
    assert rc == 2 and "--evalOut" in capsys.readouterr().err and not (tmp_path / "no2").exists()

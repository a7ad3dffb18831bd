"""Held-out evaluation on the host: the accumulator contract of
``models/metrics.py`` (margin bins, the basic-operation ``log1p(exp(-a))``,
merge), MLlib's metrics from it against exact references in numpy, the CPU
engines' ``evaluate_batch`` and ``twtml-score --evalOut`` on ``local[1]``.
"""
import json
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.apps import kmeans as km_app
from twitter_stream_ml_amd.apps import linear_regression as lr_app
from twitter_stream_ml_amd.apps import logistic_regression as lg_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.models import metrics as M
from twitter_stream_ml_amd.models.linear_regression import CpuLinearRegression, CpuLRConfig
from twitter_stream_ml_amd.models.logistic_regression import CpuLogisticConfig, CpuLogisticRegression
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = eb.NOW
F = 1000
SERVICES = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]


# ---- margin bins ---------------------------------------------------------------

BIN_TABLE = [(0.0, 2048), (-0.0, 2048), (2.0 ** -21, 2048), (2.0 ** -20, 2049), (-2.0 ** -20, 2047), (1.0, 3329),
             (np.nextafter(1.0, 0.0), 3328), (-1.0, 767), (4095.9, 4096), (1e300, 4096), (np.inf, 4096),
             (-np.inf, 0)]


def test_margin_bin_table():
    m = np.array([v for v, _ in BIN_TABLE])
    np.testing.assert_array_equal(M.margin_bin(m), [b for _, b in BIN_TABLE])
    assert M.margin_bin(np.array([np.nan, -np.nan, 1.0])).tolist() == [-1, -1, 3329]
    assert M.margin_bin(5e-324) == 2048 and M.margin_bin(-5e-324) == 2048      # subnormals
    assert M.EVAL_BINS == 4097


def test_margin_bin_is_monotone_and_edges_decode():
    rng = np.random.default_rng(1)
    # every scale from far below 2^-20 to far above 2^12, both signs
    rnd = rng.standard_normal(70_000) * np.exp2(rng.uniform(-40, 20, 70_000))
    # neighbours around every power of two (and around every bin edge of two octaves)
    p2 = np.exp2(np.arange(-30, 20, dtype=np.float64))
    edges = np.concatenate([p2, (1.0 + np.arange(64) / 64.0), 2.0 ** -20 * (1.0 + np.arange(64) / 64.0)])
    adv = np.concatenate([np.nextafter(edges, 0.0), edges, np.nextafter(edges, np.inf)])
    adv = np.concatenate([adv, -adv, [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324], rng.uniform(-1, 1, 30_000)])
    m = np.sort(np.concatenate([rnd, adv]))
    assert m.size >= 100_000
    b = M.margin_bin(m)
    assert b.min() == 0 and b.max() == 4096
    assert (np.diff(b) >= 0).all()
    # a bin's lower edge is the smallest margin of a bin above zero, and is
    # excluded from the zero bin and the bins below it
    for k in (2049, 2050, 3329, 3330, 4095, 4096):
        e = M.bin_lower_edge(k)
        assert M.margin_bin(e) == k and M.margin_bin(np.nextafter(e, -np.inf)) == k - 1
    for k in (1, 2, 767, 2047, 2048):
        e = M.bin_lower_edge(k)
        assert M.margin_bin(e) == k - 1 and M.margin_bin(np.nextafter(e, np.inf)) == k
    assert M.bin_lower_edge(0) == -math.inf and M.bin_lower_edge(3329) == 1.0
    assert M.bin_lower_edge(4096) == 4064.0 and M.bin_lower_edge(2048) == -2.0 ** -20


def test_log1p_exp_neg_accuracy():
    """~20 roundings of 2^-53 with weight <= 1 each (``log1p_exp_neg``'s
    docstring): 2e-15 relative; the reference is evaluated in extended
    precision where numpy has it, else by libm (1 ulp of its own)."""
    rng = np.random.default_rng(2)
    a = np.concatenate([[0.0, 2.0 ** -30, 0.5 * math.log(2), math.log(2), 36.0, 37.0, 699.9, 700.0],
                        rng.uniform(0, 1, 20000), rng.uniform(0, 50, 20000), rng.uniform(0, 700, 20000),
                        np.exp2(rng.uniform(-40, 0, 5000))])
    got = M.log1p_exp_neg(a)
    ld = a.astype(np.longdouble)
    ref = np.log1p(np.exp(-ld)).astype(np.float64)
    rel = np.abs(got - ref) / ref
    print("log1p_exp_neg: max relative error", rel.max())
    assert rel.max() <= 2e-15
    assert M.log1p_exp_neg(np.array([700.5, 1e300, np.inf])).tolist() == [0.0, 0.0, 0.0]
    # the row loss: MLUtils.log1pExp on either side
    m = np.array([-3.0, 0.0, 2.5])
    ref1 = np.log1p(np.exp(-m))
    np.testing.assert_allclose(M.row_logloss(m, np.ones(3)), ref1, rtol=4e-15)
    np.testing.assert_allclose(M.row_logloss(m, np.zeros(3)), ref1 + m, rtol=4e-15)


# ---- metrics against exact references -------------------------------------------

def _exact_auc2(scores, labels):
    """2 P N times the exact (midrank) AUC, in integers: a (positive,
    negative) pair counts 2 if the positive scores higher, 1 on a tie."""
    pos, neg = np.sort(scores[labels]), np.sort(scores[~labels])
    below = np.searchsorted(neg, pos, side="left")
    upto = np.searchsorted(neg, pos, side="right")
    return int(below.sum()) + int(upto.sum()), int(pos.size), int(neg.size)


def _trapezoid(pts):
    return sum((x1 - x0) * (y0 + y1) / 2.0 for (x0, y0), (x1, y1) in zip(pts, pts[1:]))


def _fake_counts(labels):
    """retweet counts whose label at threshold 10 is ``labels``"""
    return np.where(labels, 10, 9)


def test_binned_auc_within_tie_bound_of_exact():
    rng = np.random.default_rng(3)
    for trial, (n, scale, levels) in enumerate([(4000, 1.0, 40), (4000, 1e-3, 0), (3000, 30.0, 7), (500, 1e3, 0)]):
        s = rng.standard_normal(n) * scale
        if levels:      # heavy ties: few distinct scores
            s = np.round(s * levels / (4 * scale)) * (4 * scale / levels)
        lab = (s + 0.8 * scale * rng.standard_normal(n)) > 0.3 * scale
        acc = M.binary_accumulator(s, _fake_counts(lab), 10)
        bm = M.BinaryClassificationMetrics.from_accumulator(acc)
        auc2, P, N = _exact_auc2(s, lab)
        assert (bm.numPositives, bm.numNegatives) == (P, N) and P and N
        exact = auc2 / (2 * P * N)
        print(f"trial {trial}: exact {exact:.6f} binned {bm.areaUnderROC:.6f} tie bound {bm.auc_tie_bound:.3g}")
        assert abs(exact - bm.areaUnderROC) <= bm.auc_tie_bound
        assert 0.5 < bm.areaUnderROC < 1.0 and 0.0 < bm.auc_tie_bound < 0.5
        # the curves: MLlib's end points, monotone, and the trapezoid areas
        roc, pr = bm.roc(), bm.pr()
        assert roc[0] == (0.0, 0.0) and roc[-1] == (1.0, 1.0) and roc[-2] == (1.0, 1.0) and pr[0] == (0.0, 1.0)
        assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(roc, roc[1:]))
        assert bm.areaUnderROC == pytest.approx(_trapezoid(roc), abs=1e-12)
        assert bm.areaUnderPR == pytest.approx(_trapezoid(pr), abs=1e-12)
        th = bm.thresholds()
        assert all(a[0] > b[0] and a[1] >= b[1] for a, b in zip(th, th[1:])) and len(th) == len(roc) - 2


def test_binned_auc_equals_exact_when_no_bin_is_mixed():
    rng = np.random.default_rng(4)
    # one score per bin (the bins' own lower edges), so ties are ties of equal scores
    bins = rng.choice(np.arange(2049, 4097), 300, replace=False)
    lab_of_bin = rng.random(300) < 0.4
    idx = rng.integers(0, 300, 5000)
    s = np.array([M.bin_lower_edge(b) for b in bins])[idx]
    lab = lab_of_bin[idx]
    acc = M.binary_accumulator(s, _fake_counts(lab), 10)
    bm = M.BinaryClassificationMetrics.from_accumulator(acc)
    auc2, P, N = _exact_auc2(s, lab)
    assert bm.auc_tie_bound == 0.0
    assert bm.areaUnderROC == auc2 / (2 * P * N)


def test_confusion_metrics_logloss_and_single_class():
    m = np.array([-2.0, -0.5, 0.25, 3.0, 0.0, np.nan, 1.0])
    rc = np.array([0, 20, 20, 20, 0, 20, 10])
    acc = M.binary_accumulator(m, rc, 10, threshold=0.5)
    assert (acc["n"], acc["n_nan"]) == (6, 1)
    assert acc["confusion"] == [2, 0, 1, 3]          # margin > 0 predicts 1; 0.0 does not; count == threshold is 1
    bm = M.BinaryClassificationMetrics.from_accumulator(acc)
    assert bm.accuracy == 5 / 6 and bm.precision == 1.0 and bm.recall == 0.75 and bm.f1 == 6 / 7
    ok = ~np.isnan(m)
    y = (rc >= 10)[ok]
    p = 1.0 / (1.0 + np.exp(-m[ok]))
    ref = -(np.log(p[y]).sum() + np.log1p(-p[~y]).sum()) / 6
    assert bm.logLoss == pytest.approx(ref, rel=1e-14)
    assert acc["hist"].sum() == 6 and acc["hist"][1].sum() == 4
    # a threshold other than 0.5 moves the predicate to logit(threshold)
    assert M.binary_accumulator(m, rc, 10, threshold=0.6)["confusion"] == [2, 0, 2, 2]
    # one class only
    one = M.BinaryClassificationMetrics.from_accumulator(M.binary_accumulator(m, rc, 1000))
    assert one.areaUnderROC is None and one.areaUnderPR is None and one.auc_tie_bound is None
    assert one.confusion[2:] == [0, 0] and one.recall is None and one.accuracy == 0.5
    # all in one bin: AUC 1/2, tie bound 1/2
    z = M.BinaryClassificationMetrics.from_accumulator(M.binary_accumulator(np.zeros(4), [0, 20, 0, 20], 10))
    assert z.areaUnderROC == 0.5 and z.auc_tie_bound == 0.5
    # nothing at all
    e = M.metrics_of(M.empty_result("binary", 10))
    assert e.logLoss is None and e.accuracy is None and e.areaUnderROC is None
    json.dumps(e.to_dict())


def test_regression_metrics_are_mllibs():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 2000, 500)
    p = y + 40.0 * rng.standard_normal(500)
    p[7] = np.nan
    acc = M.regression_accumulator(p, y)
    assert (acc["n"], acc["n_nan"]) == (499, 1)
    rm = M.RegressionMetrics.from_accumulator(acc)
    ok = ~np.isnan(p)
    yy, pp = y[ok].astype(float), p[ok]
    e = yy - pp
    assert rm.meanSquaredError == pytest.approx((e * e).mean(), rel=1e-12)
    assert rm.rootMeanSquaredError == pytest.approx(math.sqrt((e * e).mean()), rel=1e-12)
    assert rm.meanAbsoluteError == pytest.approx(np.abs(e).mean(), rel=1e-12)
    assert rm.r2 == pytest.approx(1.0 - (e * e).sum() / ((yy - yy.mean()) ** 2).sum(), rel=1e-9)
    assert rm.explainedVariance == pytest.approx(((pp - yy.mean()) ** 2).mean(), rel=1e-9)
    assert M.metrics_of(M.empty_result("regression")).meanSquaredError is None


def test_merge_of_a_split_equals_the_whole():
    rng = np.random.default_rng(6)
    n = 3000
    m = rng.standard_normal(n) * np.exp2(rng.uniform(-12, 6, n))
    m[::97] = np.nan
    rc = rng.integers(0, 1200, n)
    whole = M.binary_accumulator(m, rc, 550, 0.3)
    parts = [M.binary_accumulator(m[a:b], rc[a:b], 550, 0.3) for a, b in ((0, 1), (1, 1700), (1700, 1700), (1700, n))]
    acc = M.EvalAccumulator.like(parts[0])
    for part in parts[:2]:
        acc.add(part)
    other = M.EvalAccumulator.like(parts[0])
    for part in parts[2:]:
        other.add(part)
    acc = M.EvalAccumulator.from_dict(json.loads(json.dumps(acc.to_dict()))).merge(other)
    got = acc.result()
    assert (got["n"], got["n_nan"], got["confusion"]) == (whole["n"], whole["n_nan"], whole["confusion"])
    np.testing.assert_array_equal(got["hist"], whole["hist"])
    assert acc.batches == 4
    assert got["logloss_sum"] == pytest.approx(whole["logloss_sum"], rel=1e-12)
    assert M.EvalAccumulator.from_dict(json.loads(json.dumps(acc.to_dict()))) == acc
    # regression, and a mismatch is refused
    rw = M.regression_accumulator(m, rc)
    ra = M.EvalAccumulator("regression").add(M.regression_accumulator(m[:1000], rc[:1000]))
    ra.merge(M.EvalAccumulator("regression").add(M.regression_accumulator(m[1000:], rc[1000:])))
    assert (ra.n, ra.n_nan) == (rw["n"], rw["n_nan"])
    for k in M.REGRESSION_SUMS:
        assert ra.result()[k] == pytest.approx(rw[k], rel=1e-12)
    assert M.EvalAccumulator.from_dict(json.loads(json.dumps(ra.to_dict()))) == ra
    with pytest.raises(ValueError):
        acc.merge(ra)
    with pytest.raises(ValueError):
        acc.add(M.binary_accumulator(m, rc, 551, 0.3))


# ---- the CPU engines --------------------------------------------------------------

def _raw(n=600, seed=11):
    return generate_batch(SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.3), 0, n, batch_time_ms=NOW)


@pytest.mark.parametrize("apply_filter", [False, True])
def test_cpu_evaluate_batch_equals_accumulator_of_its_margins(apply_filter):
    raw = _raw()
    rng = np.random.default_rng(7)
    w = rng.standard_normal(F + 4) * 0.05
    lin = CpuLinearRegression(CpuLRConfig(num_text_features=F))
    lin.set_weights(w)
    res = lin.evaluate_batch(raw, apply_filter=apply_filter)
    pr = lin.predict_batch(raw, apply_filter=apply_filter)
    want = M.regression_accumulator(pr["pred"], raw.scalars[0][pr["rows"]])
    assert res["kind"] == "regression" and res["n_raw"] == raw.n and res["n_scored"] == pr["n_scored"] == res["n"]
    assert (apply_filter and 0 < res["n"] < raw.n) or (not apply_filter and res["n"] == raw.n)
    for k in M.REGRESSION_SUMS:
        assert res[k] == want[k]
    np.testing.assert_array_equal(lin.get_weights(), w)

    lt = int(np.median(raw.scalars[0][pr["rows"]]))
    log = CpuLogisticRegression(CpuLogisticConfig(num_text_features=F, label_threshold=lt, threshold=0.4))
    log.set_weights(w)
    res = log.evaluate_batch(raw, apply_filter=apply_filter)
    pm = log.predict_batch(raw, apply_filter=apply_filter, output="margin")
    want = M.binary_accumulator(pm["pred"], raw.scalars[0][pm["rows"]], lt, 0.4)
    assert res["kind"] == "binary" and res["label_threshold"] == lt and res["threshold"] == 0.4
    assert (res["n"], res["n_nan"], res["confusion"]) == (want["n"], 0, want["confusion"])
    np.testing.assert_array_equal(res["hist"], want["hist"])
    assert res["logloss_sum"] == want["logloss_sum"]
    # the confusion counts are predict_batch's classes against the labels
    cls = log.predict_batch(raw, apply_filter=apply_filter, output="class")["pred"]
    lab = raw.scalars[0][pm["rows"]] >= lt
    assert res["confusion"] == [int((~lab & (cls == 0)).sum()), int((~lab & (cls == 1)).sum()),
                                int((lab & (cls == 0)).sum()), int((lab & (cls == 1)).sum())]
    assert 0 < lab.sum() < lab.size and M.metrics_of(res).areaUnderROC is not None


def test_cpu_evaluate_batch_empty():
    empty = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    res = CpuLogisticRegression(CpuLogisticConfig(num_text_features=F)).evaluate_batch(empty)
    assert res["n"] == res["n_scored"] == 0 and res["hist"].sum() == 0 and res["label_threshold"] == 550
    assert CpuLinearRegression(CpuLRConfig(num_text_features=F)).evaluate_batch(empty)["sum_e2"] == 0.0


# ---- the driver -------------------------------------------------------------------

def _check_eval_dir(out, kind, n_batches):
    recs = [json.loads(l) for l in open(out / "metrics.jsonl")]
    assert [r["seq"] for r in recs] == list(range(n_batches))
    total = None
    for r in recs:
        assert r["count"] > 0 and r["ms"] >= 0 and r["batch_time_ms"] > 0
        acc = M.EvalAccumulator.from_dict(r["accumulator"])
        assert acc.kind == kind and acc.n + acc.n_nan == r["count"]
        assert acc.metrics().to_dict() == r["metrics"]
        if kind == "binary":
            assert "auc_tie_bound" in r["metrics"] and "areaUnderROC" in r["metrics"]
        total = acc if total is None else total.merge(acc)
    summary = json.load(open(out / "summary.json"))
    assert summary["batches"] == n_batches
    assert summary["metrics"] == total.metrics().to_dict()
    assert M.EvalAccumulator.from_dict(summary["accumulator"]).result()["n"] == total.n
    return summary


def test_score_driver_eval_out_local(tmp_path, capsys):
    common = SERVICES + ["--seconds", "0.2", "--sourceRate", "3000", "-f", "1000"]
    lin_ck, log_ck, km_ck = tmp_path / "lin", tmp_path / "log", tmp_path / "km"
    assert lr_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(lin_ck)] + common) == 0
    assert lg_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(log_ck),
                        "--labelThreshold", "300"] + common) == 0
    out = tmp_path / "lin_eval"
    assert score_app.main(["--master", "local[1]", "--numBatches", "3", "--model", str(lin_ck),
                           "--evalOut", str(out)] + common) == 0
    s = _check_eval_dir(out, "regression", 3)
    assert s["metrics"]["meanSquaredError"] > 0
    assert not (out / "predictions.jsonl").exists()
    # logistic, together with --predictOut: both passes run
    out, pout = tmp_path / "log_eval", tmp_path / "log_pred"
    assert score_app.main(["--master", "local[1]", "--numBatches", "3", "--model", str(log_ck), "--evalOut", str(out),
                           "--predictOut", str(pout), "--labelThreshold", "300"] + common) == 0
    s = _check_eval_dir(out, "binary", 3)
    assert s["accumulator"]["label_threshold"] == 300
    assert s["metrics"]["numPositives"] > 0 and s["metrics"]["numNegatives"] > 0
    assert s["metrics"]["auc_tie_bound"] is not None and 0.0 <= s["metrics"]["areaUnderROC"] <= 1.0
    assert len(open(pout / "predictions.jsonl").readlines()) == 3
    # the default label threshold is the middle of -B..-E
    out = tmp_path / "log_eval_default"
    assert score_app.main(["--master", "local[1]", "--numBatches", "1", "--model", str(log_ck),
                           "--evalOut", str(out)] + common) == 0
    assert json.load(open(out / "summary.json"))["accumulator"]["label_threshold"] == 550
    # k-means: cost is its metric
    assert km_app.main(["--master", "local[1]", "--k", "3", "--textDims", "4", "--numBatches", "2", "--seconds", "0.2",
                        "--sourceRate", "3000", "--checkpoint", str(km_ck), "--checkpointInterval", "1"]) == 0
    capsys.readouterr()
    rc = score_app.main(["--master", "local[1]", "--numBatches", "1", "--model", str(km_ck),
                         "--evalOut", str(tmp_path / "km_eval")] + common)
    assert rc == 2 and "--evalOut" in capsys.readouterr().err
    assert not (tmp_path / "km_eval").exists()

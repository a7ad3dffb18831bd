"""Top-N on the host: the contract of ``models/topn.py`` (``top_n`` against a
plain Python sort, ``TopNMerger``), the CPU engines' ``top_batch`` and
``twtml-score --top`` on ``local[1]``.
"""
import functools
import json
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.apps import kmeans as km_app
from twitter_stream_ml_amd.apps import linear_regression as lr_app
from twitter_stream_ml_amd.apps import logistic_regression as lg_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.models.kmeans import CpuKMeans
from twitter_stream_ml_amd.models.linear_regression import CpuLinearRegression, CpuLRConfig
from twitter_stream_ml_amd.models.logistic_regression import CpuLogisticConfig, CpuLogisticRegression, sigmoid
from twitter_stream_ml_amd.models.topn import TOPN_MAX, TopNMerger, top_n
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = eb.NOW
F = 1000
SERVICES = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _python_top(values, rows, n, largest):
    """The contract with Python's sort: (value, row) pairs of the non-NaN
    entries ordered by a comparison of the values as numbers, then the row."""
    rows = list(range(len(values))) if rows is None else [int(r) for r in rows]
    pairs = [(float(v), r) for v, r in zip(values, rows) if not math.isnan(v)]

    def cmp(a, b):
        if a[0] != b[0]:   # IEEE comparison: -0.0 == +0.0
            better = a[0] > b[0] if largest else a[0] < b[0]
            return -1 if better else 1
        return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)

    pairs.sort(key=functools.cmp_to_key(cmp))
    return pairs[:n], len(values) - len(pairs)


def _check(values, rows, n, what):
    values = np.asarray(values, np.float64)
    for largest in (True, False):
        v, r, n_nan = top_n(values, rows, n, largest)
        want, want_nan = _python_top(values.tolist(), rows, n, largest)
        assert n_nan == want_nan and v.size == r.size == len(want) == min(n, values.size - n_nan), (what, largest)
        assert r.tolist() == [p[1] for p in want], (what, largest)
        assert _bits(v).tolist() == _bits(np.array([p[0] for p in want], np.float64)).tolist(), (what, largest)
        assert v.dtype == np.float64 and r.dtype == np.int64


def test_top_n_against_python_sort():
    rng = np.random.default_rng(1)
    rand = rng.standard_normal(500) * np.exp2(rng.integers(-40, 40, 500))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.2250738585072014e-308,
                        1e-310, -1e-310, 1.0, -1.0])
    ulp = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)] * 9)
    rows = np.cumsum(rng.integers(1, 6, 500)).astype(np.int64)
    cases = {"random": rand, "all equal": np.full(77, 2.5), "all zero": np.zeros(40),
             "special": special[rng.integers(0, special.size, 300)], "one ulp apart": ulp,
             "all NaN": np.full(9, np.nan), "one": np.array([3.0]), "none": np.zeros(0)}
    for what, values in cases.items():
        ln = values.size
        for n in sorted({1, 2, 10, max(1, ln - 1), max(1, ln), ln + 1, TOPN_MAX}):
            _check(values, None, n, (what, n))
    for n in (1, 64, 499, 500, 501):
        _check(np.round(rand[:500]), rows, n, ("rows", n))
    # the bits of a selected -0.0 are kept, and it ties with +0.0 on the row
    v, r, _ = top_n([0.0, -0.0, -0.0, 0.0], None, 3)
    assert r.tolist() == [0, 1, 2] and np.signbit(v).tolist() == [False, True, True]


def test_top_n_rejects_bad_n_and_shapes():
    for n in (0, -3, TOPN_MAX + 1, 2.5, True):
        with pytest.raises(ValueError, match="predict_batch"):
            top_n(np.zeros(4), None, n)
    with pytest.raises(ValueError):
        top_n(np.zeros(4), np.arange(3), 1)
    with pytest.raises(ValueError):
        TopNMerger(0)


def _merged(m):
    return [(e["value"], e["seq"], e["row"]) for e in m.result()]


@pytest.mark.parametrize("largest", [True, False])
def test_merger_split_equals_whole_and_order_independent(largest):
    rng = np.random.default_rng(5)
    n = 25
    batches = []
    for seq in range(7):
        v = np.round(rng.standard_normal(40 + 13 * seq) * 4.0) / 2.0   # heavy ties, across batches too
        v[::11] = np.nan
        v[3] = -0.0 if seq % 2 else 0.0
        batches.append(top_n(v, None, n, largest))
    # the whole: every batch's selection added to one merger
    whole = TopNMerger(n, largest)
    for seq, (v, r, nn) in enumerate(batches):
        whole.add(seq, v, r, nn)
    # reference: the same rule over all entries with Python's sort
    entries = [(float(x) + 0.0, seq, int(row)) for seq, (v, r, _) in enumerate(batches) for x, row in zip(v, r)]
    entries.sort(key=lambda e: (-e[0] if largest else e[0], e[1], e[2]))
    assert [(a + 0.0, b, c) for a, b, c in _merged(whole)] == entries[:n]
    assert whole.n_nan == sum(b[2] for b in batches) and whole.batches == 7
    # a split, merged either way round, and batches added in any order
    for order in (list(range(7)), [6, 2, 4, 0, 5, 1, 3]):
        a, b = TopNMerger(n, largest), TopNMerger(n, largest)
        for i, seq in enumerate(order):
            (a if i % 2 else b).add(seq, *batches[seq])
        ab = TopNMerger(n, largest).merge(a).merge(b)
        ba = TopNMerger(n, largest).merge(b).merge(a)
        assert _merged(ab) == _merged(ba) == _merged(whole)
        assert ab.n_nan == whole.n_nan and ab.batches == 7
    with pytest.raises(ValueError):
        whole.merge(TopNMerger(n + 1, largest))
    with pytest.raises(ValueError):
        whole.add(9, [np.nan], [0])
    # extras ride along
    m = TopNMerger(2).add(0, [1.0, 3.0], [4, 9], extras=[{"text": "a"}, {"text": "b"}])
    assert m.result() == [{"text": "b", "seq": 0, "row": 9, "value": 3.0}, {"text": "a", "seq": 0, "row": 4, "value": 1.0}]


# ---- the CPU engines -------------------------------------------------------------

def _raw(n=600, seed=11):
    return generate_batch(SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.3), 0, n, batch_time_ms=NOW)


@pytest.mark.parametrize("apply_filter", [False, True])
def test_cpu_top_batch_equals_top_n_of_its_predict_batch(apply_filter):
    raw = _raw()
    rng = np.random.default_rng(7)
    w = np.round(rng.standard_normal(F + 4) * 4.0) / 64.0
    lin = CpuLinearRegression(CpuLRConfig(num_text_features=F))
    lin.set_weights(w)
    log = CpuLogisticRegression(CpuLogisticConfig(num_text_features=F))
    log.set_weights(w)
    for eng, kw in ((lin, {}), (log, {"output": "margin"})):
        pr = eng.predict_batch(raw, apply_filter=apply_filter, **kw)
        for n, largest in ((1, True), (10, False), (TOPN_MAX, True)):
            res = eng.top_batch(raw, n, largest=largest, apply_filter=apply_filter)
            v, r, n_nan = top_n(pr["pred"], pr["rows"], n, largest)
            np.testing.assert_array_equal(res["rows"], r)
            np.testing.assert_array_equal(_bits(res["values"]), _bits(v))
            assert (res["n_top"], res["n_nan"], res["n_raw"], res["n_scored"]) == (v.size, n_nan, raw.n, pr["n_scored"])
        np.testing.assert_array_equal(eng.get_weights(), w)
        with pytest.raises(ValueError):
            eng.top_batch(raw, TOPN_MAX + 1)
    km = CpuKMeans(5, 2 + 6, seed=3)
    pr = km.predict_batch(raw, 6, apply_filter=apply_filter, scaler="none")
    for n, largest in ((1, True), (10, False), (TOPN_MAX, True)):
        res = km.top_batch(raw, n, 6, largest=largest, apply_filter=apply_filter, scaler="none")
        v, r, n_nan = top_n(pr["dist2"], pr["rows"], n, largest)
        np.testing.assert_array_equal(res["rows"], r)
        np.testing.assert_array_equal(_bits(res["dist2"]), _bits(v))
        np.testing.assert_array_equal(res["labels"], pr["pred"][np.searchsorted(pr["rows"], r)])
        assert res["cost"] == pr["cost"] and res["n_scored"] == pr["n_scored"] and res["n_nan"] == 0
        np.testing.assert_array_equal(res["sizes"], pr["sizes"])
    empty = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    assert lin.top_batch(empty, 5)["n_top"] == 0 and km.top_batch(empty, 5, 6)["n_top"] == 0


# ---- the driver --------------------------------------------------------------------

def check_top_dir(out, n, largest, n_batches, kind):
    """The files of ``--topOut``: ``summary.json`` equals a merge of ``top.jsonl``."""
    recs = [json.loads(l) for l in open(out / "top.jsonl")]
    assert [r["seq"] for r in recs] == list(range(n_batches))
    merger = TopNMerger(n, largest)
    for r in recs:
        es = r["entries"]
        assert r["count"] > 0 and r["ms"] >= 0 and r["batch_time_ms"] > 0 and r["n_nan"] == 0
        assert len(es) == min(n, r["count"])
        vals = [e["value"] for e in es]
        assert vals == sorted(vals, reverse=largest)
        assert all(a["value"] != b["value"] or a["row"] < b["row"] for a, b in zip(es, es[1:]))
        for e in es:
            assert isinstance(e["text"], str) and e["retweetCount"] >= 0 and 0 <= e["row"]
            if kind == "logistic":
                assert e["probability"] == float(sigmoid(np.float64(e["value"])))
            if kind == "kmeans":
                assert e["dist2"] == e["value"] >= 0 and e["label"] >= 0
        merger.add(r["seq"], vals, [e["row"] for e in es], r["n_nan"],
                   [{k: v for k, v in e.items() if k not in ("row", "value")} for e in es])
    summary = json.load(open(out / "summary.json"))
    assert summary["batches"] == n_batches and summary["n"] == n and summary["largest"] == largest
    assert summary["entries"] == merger.result()
    assert all("seq" in e and "text" in e for e in summary["entries"]) and len(summary["entries"]) == n
    return recs, summary


def test_score_driver_top_local(tmp_path, capsys):
    common = SERVICES + ["--seconds", "0.2", "--sourceRate", "3000", "-f", "1000"]
    lin_ck, log_ck, km_ck = tmp_path / "lin", tmp_path / "log", tmp_path / "km"
    assert lr_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(lin_ck)] + common) == 0
    assert lg_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(log_ck),
                        "--labelThreshold", "300"] + common) == 0
    assert km_app.main(["--master", "local[1]", "--k", "3", "--textDims", "4", "--numBatches", "2", "--seconds", "0.2",
                        "--sourceRate", "3000", "--checkpoint", str(km_ck), "--checkpointInterval", "1"]) == 0
    # scored on a recorded stream: the same three batches for every model
    score = ["--master", "local[1]", "--numBatches", "3", "--source", "replay:synthetic:twitter:3", "--batchSize", "500",
             "--seconds", "0", "--sourceRate", "0", "-f", "1000"] + SERVICES
    out = tmp_path / "lin_top"
    assert score_app.main(score + ["--model", str(lin_ck), "--top", "7", "--topOut", str(out)]) == 0
    check_top_dir(out, 7, True, 3, "linear")
    assert not (out / "predictions.jsonl").exists()
    # logistic, the lowest margins, together with --predictOut and --evalOut: every pass runs
    out, pout, eout = tmp_path / "log_top", tmp_path / "log_pred", tmp_path / "log_eval"
    assert score_app.main(score + ["--model", str(log_ck), "--top", "5", "--topSmallest", "--topOut", str(out),
                                   "--predictOut", str(pout), "--evalOut", str(eout)]) == 0
    check_top_dir(out, 5, False, 3, "logistic")
    assert len(open(pout / "predictions.jsonl").readlines()) == 3
    assert json.load(open(eout / "summary.json"))["batches"] == 3
    # k-means: the rows farthest from their centres
    out = tmp_path / "km_top"
    assert score_app.main(score + ["--model", str(km_ck), "--top", "4", "--topOut", str(out)]) == 0
    recs, _ = check_top_dir(out, 4, True, 3, "kmeans")
    assert all("cost" in r for r in recs)
    # usage errors: exit code 2, nothing written
    capsys.readouterr()
    for bad in (["--top", "5"], ["--top", "0", "--topOut", str(tmp_path / "bad")],
                ["--top", str(TOPN_MAX + 1), "--topOut", str(tmp_path / "bad")], ["--topOut", str(tmp_path / "bad")]):
        assert score_app.main(score + ["--model", str(lin_ck)] + bad) == 2
        assert "--top" in capsys.readouterr().err
    assert not (tmp_path / "bad").exists()

"""Per-cluster exemplars on the host: the contract of ``models/exemplars.py``
(``cluster_top`` against a plain Python sort per cluster, ``ExemplarMerger``),
``CpuKMeans.exemplars_batch`` and ``twtml-score --exemplars`` on ``local[1]``.
"""
import functools
import json
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.apps import kmeans as km_app
from twitter_stream_ml_amd.apps import linear_regression as lr_app
from twitter_stream_ml_amd.apps import score as score_app
from twitter_stream_ml_amd.config.arguments import ConfArguments
from twitter_stream_ml_amd.models.exemplars import (EXEMPLARS_MAX, EXEMPLARS_MAX_CELLS, ExemplarMerger, check_m,
                                                    cluster_top, empty_exemplars, exemplars_result)
from twitter_stream_ml_amd.models.kmeans import CpuKMeans
from twitter_stream_ml_amd.sources import make_source
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

NOW = eb.NOW
SERVICES = ["--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _python_cluster_top(values, labels, rows, k, m, largest):
    """The contract with Python's sort, one cluster at a time: (value, row)
    pairs of the cluster's non-NaN entries ordered by a comparison of the
    values as numbers, then the row."""
    rows = list(range(len(values))) if rows is None else [int(r) for r in rows]

    def cmp(a, b):
        if a[0] != b[0]:   # IEEE comparison: -0.0 == +0.0
            better = a[0] > b[0] if largest else a[0] < b[0]
            return -1 if better else 1
        return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)

    out = []
    for c in range(k):
        pairs = [(float(v), r) for v, l, r in zip(values, labels, rows) if l == c and not math.isnan(v)]
        pairs.sort(key=functools.cmp_to_key(cmp))
        out.append(pairs[:m])
    return out, sum(1 for v in values if math.isnan(v))


def _check(values, labels, rows, k, m, what):
    values = np.asarray(values, np.float64)
    labels = np.asarray(labels)
    for largest in (False, True):
        counts, r, v, n_nan = cluster_top(values, labels, rows, k=k, m=m, largest=largest)
        want, want_nan = _python_cluster_top(values.tolist(), labels.tolist(), rows, k, m, largest)
        assert n_nan == want_nan, (what, largest)
        assert counts.dtype == np.int64 and r.dtype == np.int64 and v.dtype == np.float64
        assert counts.shape == (k,) and r.shape == v.shape == (k, m)
        for c in range(k):
            n = len(want[c])
            assert counts[c] == n, (what, largest, c)
            assert r[c, :n].tolist() == [p[1] for p in want[c]], (what, largest, c)
            assert _bits(v[c, :n]).tolist() == _bits(np.array([p[0] for p in want[c]], np.float64)).tolist(), (what, c)
            assert (r[c, n:] == -1).all() and (_bits(v[c, n:]) == 0).all()


def test_cluster_top_against_python_sort():
    rng = np.random.default_rng(1)
    nans = np.array([0x7FF8000000000000, -0x0008000000000000, 0x7FF0000000000001], np.int64).view(np.float64)
    for n, k in ((0, 1), (1, 1), (1, 2), (40, 1), (40, 2), (300, 33), (20, 50)):   # k > n as well
        labels = rng.integers(0, k, n)
        size0 = int(np.count_nonzero(labels == 0))
        kinds = {
            "random": rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n)),
            "all equal": np.full(n, 0.75),
            "+-0": np.array([0.0, -0.0, 1.0, -1.0])[rng.integers(0, 4, n)],
            "+-inf": np.array([np.inf, -np.inf, 0.0, 1e308, -1e308])[rng.integers(0, 5, n)],
            "subnormals": np.array([5e-324, -5e-324, 2.2250738585072014e-308, 0.0, 1e-310, -1e-310])[rng.integers(0, 6, n)],
            "one ulp": np.array([1.5, np.nextafter(1.5, 2.0), np.nextafter(1.5, 1.0)])[rng.integers(0, 3, n)],
        }
        v = rng.standard_normal(n)
        hit = rng.random(n) < 0.3
        v[hit] = nans[rng.integers(0, 3, int(hit.sum()))]
        v[labels == k - 1] = np.nan                    # a cluster that is all NaN: count 0
        kinds["NaNs"] = v
        for name, values in kinds.items():
            for m in sorted({1, 2, 64, size0 - 1, size0, size0 + 1}):
                if 1 <= m <= EXEMPLARS_MAX:
                    _check(values, labels, None, k, m, (name, n, k, m))
        rows = np.cumsum(rng.integers(1, 5, n)).astype(np.int64) + 11   # given row ids; ties, so they decide
        _check(np.round(rng.standard_normal(n) * 2.0), labels, rows, k, 3, ("rows", n, k))
    counts, r, v, n_nan = cluster_top(np.full(9, np.nan), np.zeros(9, np.int32), k=2, m=4)
    assert n_nan == 9 and not counts.any() and (r == -1).all()


def test_cluster_top_rejects_bad_arguments():
    v, l = np.zeros(4), np.zeros(4, np.int32)
    for bad in (np.array([0, 1, 2, 3]), np.array([0, -1, 0, 0])):
        with pytest.raises(ValueError, match="labels"):
            cluster_top(v, bad, k=3, m=1)
    with pytest.raises(ValueError, match="labels"):
        cluster_top(v, np.zeros(4), k=3, m=1)          # not integers
    for k, m in ((1, 0), (1, -1), (1, EXEMPLARS_MAX + 1), (1, 1.5), (1, True), (EXEMPLARS_MAX_CELLS + 1, 1),
                 (EXEMPLARS_MAX_CELLS // 64 + 1, 64), (0, 1)):
        with pytest.raises(ValueError) as e:
            cluster_top(v, l, k=k, m=m)
        if k > 0:
            assert "predict_batch" in str(e.value)
    assert check_m(EXEMPLARS_MAX_CELLS // 64, 64) == 64 and check_m(EXEMPLARS_MAX_CELLS, 1) == 1
    with pytest.raises(ValueError):
        cluster_top(v, l[:3], k=1, m=1)
    with pytest.raises(ValueError):
        cluster_top(v, l, np.arange(3), k=1, m=1)
    e = empty_exemplars(3, 2)
    assert e["rows"].shape == (3, 2) and (e["rows"] == -1).all() and not e["counts"].any() and e["n_nan"] == 0
    res = exemplars_result([2.0, 1.0], [0, 0], None, 1, 1)
    assert res["rows"].tolist() == [[1]] and res["values"].tolist() == [[1.0]] and res["counts"].tolist() == [1]


@pytest.mark.parametrize("largest", [False, True])
def test_merger_split_equals_whole_and_order_independent(largest):
    rng = np.random.default_rng(5)
    k, m, n = 7, 4, 600
    values = np.round(rng.standard_normal(n) * 3.0) / 2.0      # many ties, across batches too
    values[rng.random(n) < 0.05] = np.nan
    values[::97] = -0.0
    labels = rng.integers(0, k - 1, n)                          # cluster k - 1 stays empty
    cuts = [0, 100, 101, 350, 600]
    parts = []
    for seq, (a, b) in enumerate(zip(cuts, cuts[1:])):
        c, r, v, n_nan = cluster_top(values[a:b], labels[a:b], k=k, m=m, largest=largest)
        parts.append((seq, c, r, v, n_nan, a))
    whole = ExemplarMerger(k, m, largest)
    for seq, c, r, v, n_nan, _ in parts:
        whole.add(seq, c, r, v, n_nan=n_nan)
    # the whole stream, keyed by (value, seq, row in batch): what a sort of everything gives
    want = []
    for c in range(k):
        es = [(float(values[i]) + 0.0, s, i - a) for s, (a, b) in enumerate(zip(cuts, cuts[1:])) for i in range(a, b)
              if labels[i] == c and not math.isnan(values[i])]
        es.sort(key=lambda e: (-e[0] if largest else e[0], e[1], e[2]))
        if es:
            want.append((c, es[:m]))
    got = [(c["label"], [(e["value"] + 0.0, e["seq"], e["row"]) for e in c["entries"]]) for c in whole.result()]
    assert got == want
    assert whole.n_nan == int(np.isnan(values).sum()) and whole.batches == 4
    # both orders, and merged halves
    rev = ExemplarMerger(k, m, largest)
    for seq, c, r, v, n_nan, _ in reversed(parts):
        rev.add(seq, c, r, v, n_nan=n_nan)
    assert rev.result() == whole.result()
    a, b = ExemplarMerger(k, m, largest), ExemplarMerger(k, m, largest)
    for seq, c, r, v, n_nan, _ in parts[:2]:
        a.add(seq, c, r, v, n_nan=n_nan)
    for seq, c, r, v, n_nan, _ in parts[2:]:
        b.add(seq, c, r, v, n_nan=n_nan)
    ab = ExemplarMerger.from_dict(a.to_dict()).merge(b)
    ba = ExemplarMerger.from_dict(b.to_dict()).merge(a)
    assert ab.result() == ba.result() == whole.result() and ab.n_nan == ba.n_nan == whole.n_nan and ab.batches == 4
    with pytest.raises(ValueError):
        a.merge(ExemplarMerger(k, m + 1, largest))
    with pytest.raises(ValueError):
        a.add(9, np.ones(k, np.int64), np.zeros((k, 1), np.int64), np.full((k, 1), np.nan))


def test_merger_ties_extras_and_json_round_trip():
    mg = ExemplarMerger(2, 3)
    one = np.array([[5, 9, -1], [-1, -1, -1]])
    mg.add(1, [2, 0], one, [[1.0, 1.0, 0.0], [0, 0, 0]], {(0, 5): {"text": "b5"}, (0, 9): {"text": "b9"}})
    mg.add(0, [2, 0], np.array([[7, 8, -1], [-1, -1, -1]]), [[1.0, 2.0, 0.0], [0, 0, 0]], {(0, 7): {"text": "a7"}})
    res = mg.result()
    assert [c["label"] for c in res] == [0]
    # equal values: the earlier batch first, then the row
    assert [(e["seq"], e["row"]) for e in res[0]["entries"]] == [(0, 7), (1, 5), (1, 9)]
    assert [e.get("text") for e in res[0]["entries"]] == ["a7", "b5", "b9"]
    mg.add(2, [0, 1], np.array([[-1], [3]]), [[0.0], [-np.inf]])
    back = ExemplarMerger.from_dict(json.loads(json.dumps(mg.to_dict())))
    assert back.result() == mg.result() and (back.k, back.m, back.largest, back.n_nan, back.batches) == (2, 3, False, 0, 3)
    assert back.result()[1]["entries"][0]["value"] == -np.inf
    # a line's clusters, as the scoring driver writes them
    again = ExemplarMerger(2, 3)
    again.add_clusters(0, [{"label": 0, "entries": [{"row": 7, "dist2": 1.0, "text": "a7"}, {"row": 8, "dist2": 2.0}]}])
    again.add_clusters(1, [{"label": 0, "entries": [{"row": 5, "dist2": 1.0, "text": "b5"},
                                                    {"row": 9, "dist2": 1.0, "text": "b9"}]}])
    again.add_clusters(2, [{"label": 1, "entries": [{"row": 3, "dist2": -np.inf}]}])
    assert again.result() == mg.result()
    # two ranks' files: the same seq, row and value for one cluster -- the result must not depend on the order
    a = [{"label": 0, "entries": [{"row": 4, "dist2": 1.0, "text": "rank 0"}, {"row": 6, "dist2": 2.0, "text": "x"}]}]
    b = [{"label": 0, "entries": [{"row": 4, "dist2": 1.0, "text": "rank 1"}, {"row": 5, "dist2": -0.0, "text": "y"}]}]
    c = [{"label": 0, "entries": [{"row": 5, "dist2": 0.0, "text": "y"}]}]
    results = []
    for order in ((a, b, c), (c, b, a), (b, a, c), (b, c, a)):
        mm = ExemplarMerger(2, 3)
        for part in order:
            mm.add_clusters(0, part)
        results.append(json.dumps(mm.result()))
    assert len(set(results)) == 1
    assert [e["text"] for e in json.loads(results[0])[0]["entries"]] == ["y", "y", "rank 0"]


@functools.lru_cache(maxsize=None)
def _raw(rows=3000):
    return generate_batch(SynthConfig.profile("twitter", seed=31, unicode_fraction=0.3), 0, rows, batch_time_ms=NOW)


@pytest.mark.parametrize("apply_filter", [False, True])
def test_cpu_exemplars_batch_equals_cluster_top_of_its_predict_batch(apply_filter):
    raw = _raw()
    k, td = 9, 6
    km = CpuKMeans(k, 2 + td, seed=3)
    for scaler in ("none", "batch"):
        pr = km.predict_batch(raw, td, apply_filter=apply_filter, scaler=scaler)
        assert pr["n_scored"] > 100
        for m, largest in ((1, False), (10, True), (64, False)):
            res = km.exemplars_batch(raw, m, td, largest=largest, apply_filter=apply_filter, scaler=scaler)
            c, r, v, n_nan = cluster_top(pr["dist2"], pr["pred"], pr["rows"], k=k, m=m, largest=largest)
            np.testing.assert_array_equal(res["counts"], c)
            np.testing.assert_array_equal(res["rows"], r)
            np.testing.assert_array_equal(_bits(res["dist2"]), _bits(v))
            assert res["cost"] == pr["cost"] and res["n_scored"] == pr["n_scored"] and res["n_nan"] == 0
            assert res["n_raw"] == raw.n and res["dist2"] is res["values"]
            np.testing.assert_array_equal(res["sizes"], pr["sizes"])
            np.testing.assert_array_equal(res["counts"], np.minimum(pr["sizes"], m))
    # one row, and no rows
    one = km.exemplars_batch(raw.slice(0, 1), 3, td, apply_filter=False)
    assert one["counts"].sum() == 1 and one["rows"][one["counts"] == 1, 0].tolist() == [0]
    empty = km.exemplars_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)), 3, td)
    assert empty["n_scored"] == 0 and not empty["counts"].any() and empty["rows"].shape == (k, 3)
    with pytest.raises(ValueError, match="predict_batch"):
        km.exemplars_batch(raw, EXEMPLARS_MAX + 1, td)


# ---- the driver --------------------------------------------------------------------

def check_exemplars_dir(out, k, m, largest, raws):
    """The files of ``--exemplarsOut``: ``summary.json`` equals a merge of
    ``exemplars.jsonl``; every entry's text is the raw row's."""
    recs = [json.loads(l) for l in open(out / "exemplars.jsonl")]
    assert [r["seq"] for r in recs] == list(range(len(raws)))
    merger = ExemplarMerger(k, m, largest)
    for r, raw in zip(recs, raws):
        assert r["n_raw"] == raw.n and 0 < r["n_scored"] <= raw.n and r["n_nan"] == 0
        assert r["ms"] >= 0 and r["ex_ms"] >= 0 and r["batch_time_ms"] > 0 and r["cost"] > 0
        assert r["clusters_used"] == len(r["clusters"]) > 0
        assert sum(c["size"] for c in r["clusters"]) == r["n_scored"]
        assert [c["label"] for c in r["clusters"]] == sorted(c["label"] for c in r["clusters"])
        for c in r["clusters"]:
            es = c["entries"]
            assert len(es) == min(m, c["size"]) and 0 <= c["label"] < k
            vals = [e["dist2"] for e in es]
            assert vals == sorted(vals, reverse=largest)
            assert all(a["dist2"] != b["dist2"] or a["row"] < b["row"] for a, b in zip(es, es[1:]))
            for e in es:
                assert e["text"] == raw.text_of(e["row"]) and e["dist2"] >= 0
                assert e["retweetCount"] == int(raw.scalars[0][e["row"]]) >= 0
                assert raw.is_retweet[e["row"]] == 1   # the training filter: retweets only
        merger.add_clusters(r["seq"], r["clusters"], r["n_nan"])
    summary = json.load(open(out / "summary.json"))
    assert (summary["batches"], summary["k"], summary["m"], summary["largest"]) == (len(raws), k, m, largest)
    want = [{"label": c["label"], "entries": [{**{kk: v for kk, v in e.items() if kk != "value"}, "dist2": e["value"]}
                                              for e in c["entries"]]} for c in merger.result()]
    assert summary["clusters"] == want and summary["n_nan"] == 0
    assert all("seq" in e and "text" in e for c in summary["clusters"] for e in c["entries"])
    return recs, summary


def test_score_driver_exemplars_local(tmp_path, capsys):
    lin_ck, km_ck = tmp_path / "lin", tmp_path / "km"
    assert lr_app.main(["--master", "local[1]", "--numBatches", "2", "--checkpoint", str(lin_ck), "--seconds", "0.2",
                        "--sourceRate", "3000", "-f", "1000"] + SERVICES) == 0
    assert km_app.main(["--master", "local[1]", "--k", "3", "--textDims", "4", "--numBatches", "2", "--seconds", "0.2",
                        "--sourceRate", "3000", "--checkpoint", str(km_ck), "--checkpointInterval", "1"]) == 0
    spec = "replay:synthetic:twitter:3"
    score = ["--master", "local[1]", "--numBatches", "3", "--source", spec, "--batchSize", "500", "--seconds", "0",
             "--sourceRate", "0", "-f", "1000"] + SERVICES
    src = make_source(spec, rate=0, seed=ConfArguments().seed, shard=0, num_shards=1, start=0, batch_size=500)
    raws = [src.poll(500) for _ in range(3)]
    out = tmp_path / "ex"
    assert score_app.main(score + ["--model", str(km_ck), "--exemplars", "4", "--exemplarsOut", str(out)]) == 0
    _, summary = check_exemplars_dir(out, 3, 4, False, raws)
    assert summary["scaler"] == "batch" and not (out / "predictions.jsonl").exists()
    # the farthest, a frozen scaler, together with the other passes: each runs
    std = tmp_path / "std.npy"
    np.save(std, np.linspace(0.5, 2.0, 6))
    out, pout, tout, sout = (tmp_path / n for n in ("ex2", "pred", "top", "sil"))
    assert score_app.main(score + ["--model", str(km_ck), "--exemplars", "64", "--exemplarsFarthest", "--exemplarsOut",
                                   str(out), "--scalerStd", str(std), "--predictOut", str(pout), "--top", "3",
                                   "--topOut", str(tout), "--silhouetteOut", str(sout)]) == 0
    recs, summary = check_exemplars_dir(out, 3, 64, True, raws)
    assert summary["scaler"] == "given"
    assert len(open(pout / "predictions.jsonl").readlines()) == 3 and (tout / "summary.json").exists()
    assert json.load(open(sout / "summary.json"))["batches"] == 3
    for t, r in enumerate(recs):   # the selection is cluster_top of what --predictOut wrote
        c, rows, v, _ = cluster_top(np.load(pout / f"dist2_{t}.npy"), np.load(pout / f"pred_{t}.npy"),
                                    np.load(pout / f"rows_{t}.npy"), k=3, m=64, largest=True)
        for cl in r["clusters"]:
            n = int(c[cl["label"]])
            assert [e["row"] for e in cl["entries"]] == rows[cl["label"], :n].tolist()
            assert [e["dist2"] for e in cl["entries"]] == v[cl["label"], :n].tolist()
    # usage errors: exit code 2, nothing written
    capsys.readouterr()
    bad_dir = str(tmp_path / "bad")
    big = tmp_path / "big"
    from twitter_stream_ml_amd.models.kmeans import StreamingKMeansModel
    StreamingKMeansModel(np.zeros((EXEMPLARS_MAX_CELLS // 64 + 1, 2)), np.ones(EXEMPLARS_MAX_CELLS // 64 + 1)).save(str(big))
    for model, bad in ((km_ck, ["--exemplars", "5"]), (km_ck, ["--exemplarsOut", bad_dir]),
                       (km_ck, ["--exemplars", "0", "--exemplarsOut", bad_dir]),
                       (km_ck, ["--exemplars", str(EXEMPLARS_MAX + 1), "--exemplarsOut", bad_dir]),
                       (km_ck, ["--exemplarsFarthest"]),
                       (big, ["--exemplars", "64", "--exemplarsOut", bad_dir]),
                       (lin_ck, ["--exemplars", "5", "--exemplarsOut", bad_dir])):
        assert score_app.main(score + ["--model", str(model)] + bad) == 2
        assert "--exemplars" in capsys.readouterr().err
    assert not (tmp_path / "bad").exists()

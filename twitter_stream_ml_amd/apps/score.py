"""twtml-score: score a tweet stream with a trained model, without training.

Loads an MLlib ``Saveable`` LinearRegressionModel directory -- what the
LinearRegression driver's ``--checkpoint`` writes -- and scores every
micro-batch of ``--source synthetic|replay:FILE|twitter`` with it:
``engine.predict_batch(raw)``, the unfiltered fp64 predictions ``x . w`` of
every tweet in record order (on ``rocm[N]`` one pass of ``csrc/hip/score.hip``
per batch, on ``local[N]`` the fp64 CPU engine).  The model is never updated.
A LogisticRegressionModel directory (the logistic driver's ``--checkpoint``) is
scored as such: the output is chosen by the model class found in ``--model`` --
the class (1.0 / 0.0) under the model's saved threshold, or the probability if
the model was saved with its threshold cleared.
A KMeansModel directory (the k-means driver's ``--checkpoint``) is the third
model class: every batch's retweets (the training filter) are assigned to the
saved centres -- k and ``text_dims = d - 2`` come from the centres, ``-f`` does
not apply -- after the per-batch StandardScaler of the training driver
(``KMeans.scala:103``) or the frozen one of ``--scalerStd``; the outputs are
the labels, each row's squared distance to its centre and the batch's cost
(their sum, ``KMeansModel.computeCost``).

``--model DIR``       the model directory; its weight count must be
                      ``numTextFeatures + 4`` (``-f`` / ``--hash`` as trained)
``--predictOut DIR``  per batch ``pred_<seq>.npy`` (float64), ``rows_<seq>.npy``
                      (int64 raw row ids) and one line of ``predictions.jsonl``
                      (batch time, count, mean / min / max prediction, ms)
                      k-means: ``pred`` is int32 labels, plus ``dist2_<seq>.npy``
                      (float64); the line holds count, cost, mean_cost,
                      clusters_used, ms
``--evalOut DIR``     held-out evaluation of a linear or logistic model against the
                      stream's own ``retweetCount`` (``engine.evaluate_batch``; on
                      ``rocm[N]`` the reduction of ``csrc/hip/eval.hip`` behind the
                      scoring kernels, ~66 KB per batch back to the host): per batch
                      one line of ``metrics.jsonl`` -- seq, batch time, count, the
                      batch's metrics (``models/metrics.py``: MLlib's
                      ``BinaryClassificationMetrics`` with ``auc_tie_bound`` next to
                      the AUC, or ``RegressionMetrics``), the accumulator itself and
                      ms -- and at the end ``summary.json``, the metrics of the
                      accumulator merged over all batches.  Logistic models: class 1
                      is ``retweetCount >= --labelThreshold`` (default: the middle of
                      ``-B..-E``, as in the training driver).  May be combined with
                      ``--predictOut`` (both passes run).  A k-means model with
                      ``--evalOut`` is a usage error (exit code 2): ``cost`` is its
                      metric already.  Nothing is posted to twtml-web.
``--top N``           with ``--topOut DIR``: the N (1..4096) highest-scored tweets of every
                      batch (``engine.top_batch``; on ``rocm[N]`` the exact radix select
                      of ``csrc/hip/topn.hip`` behind the scoring kernels: N entries come
                      back, not the predictions), ``--topSmallest``: the lowest.  Per
                      batch one line of ``top.jsonl`` -- seq, batch time, count, n_nan, ms
                      and ``entries``, best first, ties by row: ``row``, ``value``, the
                      row's ``retweetCount`` and ``text``; logistic models select on the
                      margin (``value``) and add ``probability``; k-means models select
                      the rows farthest from their centres (``dist2``, ``label``) -- and
                      at the end ``summary.json``, the best N of the stream
                      (``models/topn.TopNMerger``; entries carry ``seq``).  May be
                      combined with ``--predictOut`` and ``--evalOut`` (each runs its own
                      pass; give each its own directory).  ``--top`` without ``--topOut``
                      or N outside 1..4096 is a usage error (exit code 2).
``--silhouetteOut DIR``  k-means models: the silhouette of every batch's retweets under the
                      saved centres (``engine.silhouette_batch``: MLlib's
                      ``ClusteringEvaluator``, squared Euclidean, ``models/silhouette.py``; on
                      ``rocm[N]`` the neighbour pass of ``csrc/hip/silhouette.hip`` behind the
                      scoring kernels, 2k + 4 words per batch back to the host).  Per batch
                      one line of ``silhouette.jsonl`` -- seq, n_raw, n_scored, silhouette
                      (null when fewer than two clusters are non-empty), n_single,
                      n_undefined, clusters_used, cost, the accumulator, ms, sil_ms -- and at
                      the end ``summary.json``: the merged accumulator, ``silhouette`` and
                      ``cluster_silhouette``.  Every batch is measured against its own
                      cluster means: the stream's figure is the row-weighted mean of its
                      batches' silhouettes, not a silhouette over the whole stream.  May be
                      combined with ``--predictOut``, ``--top`` and ``--scalerStd`` (each runs
                      its own pass).  With a linear or logistic model it is a usage error
                      (exit code 2).
``--exemplars M``     with ``--exemplarsOut DIR``, k-means models: what each cluster is about --
                      per cluster, the M (1..64, k M <= 2^18) retweets of every batch nearest
                      its centre (``engine.exemplars_batch``, ``models/exemplars.py``; on
                      ``rocm[N]`` the segmented selection of ``csrc/hip/exemplars.hip`` behind
                      the scoring kernels: k x M entries come back, not the labels and
                      distances of every row); ``--exemplarsFarthest``: each cluster's own
                      outliers.  Per batch one line of ``exemplars.jsonl`` -- seq, batch time,
                      n_raw, n_scored, n_nan, clusters_used, cost, ms, ex_ms and ``clusters``:
                      for each non-empty cluster ``label``, ``size`` and ``entries``, best
                      first, ties by row: ``row``, ``dist2``, the row's ``retweetCount`` and
                      ``text`` -- and at the end ``summary.json``: the best M per cluster of
                      the stream (``models/exemplars.ExemplarMerger``; entries carry ``seq``)
                      and ``"scaler"``: ``"batch"``, ``"given"`` or ``"none"``.  Distances of
                      different batches are on one scale only with ``--scalerStd`` or no
                      scaler: under the per-batch scaler the summary merges distances
                      measured in each batch's own units.  May be combined with
                      ``--predictOut``, ``--top``, ``--silhouetteOut`` and ``--scalerStd``
                      (each runs its own pass).  ``--exemplars`` without ``--exemplarsOut`` or
                      the reverse, M outside 1..64, k M > 2^18 or a linear or logistic model
                      is a usage error (exit code 2).
``--scalerStd FILE``  k-means: ``.npy`` of d column stds, the frozen scaler
``--numBatches N``    stop after N batches

With more than one rank (``rocm[N>1]``, one process per GPU) every rank
scores its own shard of the stream and writes its own files, suffixed
``_r<rank>``; scoring needs no collective.  The ranks' ``metrics_r<rank>.jsonl``
accumulators combine exactly with ``EvalAccumulator.from_dict`` + ``merge``,
the lines of their ``top_r<rank>.jsonl`` with ``TopNMerger.add`` and those of
their ``exemplars_r<rank>.jsonl`` with ``ExemplarMerger.add``.
"""
from __future__ import annotations

import json
import logging
import os
import sys
import time
from typing import List, Optional

import numpy as np

from ..config.arguments import ConfArguments
from ..config.hocon import load_java_opts
from ..models.linear_regression import LinearRegressionModel
from ..models.mllib_helper import MllibHelper
from ..runtime.streaming import StreamingContext
from ..sources import make_source
from ..utils.logging import setup_logging
from ._common import exit_on_sigterm
from .linear_regression import build_engine

__all__ = ["main", "ScoreJob", "KMeansScoreJob", "EvalJob", "TopJob", "SilhouetteJob", "ExemplarsJob",
           "build_kmeans_scorer"]

log = logging.getLogger("com.giorgioinf.twtml.spark.Score")
APP_NAME = "twitter-stream-ml-score"


class ScoreJob:
    """Per-batch logic of the scoring driver."""

    def __init__(self, engine, out_dir: str = "", rank: int = 0, world: int = 1, output: Optional[str] = None):
        self.engine = engine
        self.output = output   # logistic models: "class" / "probability"; None: the engine's margin
        self.out_dir = out_dir
        self.suffix = f"_r{rank}" if world > 1 else ""
        self.batches = 0
        self.scored = 0
        self._jsonl = None
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            self._jsonl = open(os.path.join(out_dir, f"predictions{self.suffix}.jsonl"), "a", encoding="utf-8")

    def on_batch(self, rdd, time_ms: int) -> None:
        raw = rdd.raw
        t0 = time.perf_counter()
        kw = {} if self.output is None else {"output": self.output}
        res = self.engine.predict_batch(raw, apply_filter=False, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        pred = np.asarray(res["pred"], np.float64)
        seq = self.batches
        self.batches += 1
        self.scored += int(res["n_scored"])
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "count": int(res["n_scored"]),
               "mean": float(pred.mean()) if pred.size else None,
               "min": float(pred.min()) if pred.size else None,
               "max": float(pred.max()) if pred.size else None,
               "ms": round(ms, 3), "score_ms": round(float(res.get("score_ms", 0.0)), 3)}
        log.debug("batch %d: %d tweets scored in %.3f ms", seq, rec["count"], ms)
        if self.out_dir:
            np.save(os.path.join(self.out_dir, f"pred_{seq}{self.suffix}.npy"), pred)
            np.save(os.path.join(self.out_dir, f"rows_{seq}{self.suffix}.npy"), np.asarray(res["rows"], np.int64))
            self._jsonl.write(json.dumps(rec) + "\n")
            self._jsonl.flush()

    def close(self) -> None:
        if self._jsonl is not None:
            self._jsonl.close()
            self._jsonl = None


class KMeansScoreJob(ScoreJob):
    """Per-batch logic of the scoring driver with a k-means model: the
    retweets' clusters, squared distances and the batch's cost."""

    def __init__(self, engine, text_dims: int, scaler="batch", out_dir: str = "", rank: int = 0, world: int = 1):
        super().__init__(engine, out_dir, rank, world)
        self.scaler = scaler
        # the CPU engine takes the feature width per call (it holds no config)
        self._kw = {} if hasattr(engine, "cfg") else {"text_dims": int(text_dims)}

    def on_batch(self, rdd, time_ms: int) -> None:
        raw = rdd.raw
        t0 = time.perf_counter()
        res = self.engine.predict_batch(raw, apply_filter=True, scaler=self.scaler, **self._kw)
        ms = (time.perf_counter() - t0) * 1e3
        n = int(res["n_scored"])
        seq = self.batches
        self.batches += 1
        self.scored += n
        cost = float(res["cost"])
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "count": n, "cost": cost,
               "mean_cost": cost / n if n else None,
               "clusters_used": int(np.count_nonzero(res["sizes"])),
               "ms": round(ms, 3), "score_ms": round(float(res.get("score_ms", 0.0)), 3)}
        log.debug("batch %d: %d tweets clustered in %.3f ms, cost %g", seq, n, ms, cost)
        if self.out_dir:
            for name, arr, dt in (("pred", res["pred"], np.int32), ("dist2", res["dist2"], np.float64),
                                  ("rows", res["rows"], np.int64)):
                np.save(os.path.join(self.out_dir, f"{name}_{seq}{self.suffix}.npy"), np.asarray(arr, dt))
            self._jsonl.write(json.dumps(rec) + "\n")
            self._jsonl.flush()


class EvalJob:
    """Per-batch logic of ``--evalOut``: the batch's accumulator and metrics
    as one line of ``metrics.jsonl``, the merged accumulator's metrics in
    ``summary.json`` at the end."""

    def __init__(self, engine, out_dir: str, rank: int = 0, world: int = 1):
        self.engine = engine
        self.out_dir = out_dir
        self.suffix = f"_r{rank}" if world > 1 else ""
        self.batches = 0
        self.total = None
        os.makedirs(out_dir, exist_ok=True)
        self._jsonl = open(os.path.join(out_dir, f"metrics{self.suffix}.jsonl"), "a", encoding="utf-8")

    def on_batch(self, rdd, time_ms: int) -> None:
        from ..models.metrics import EvalAccumulator
        t0 = time.perf_counter()
        res = self.engine.evaluate_batch(rdd.raw, apply_filter=False)
        ms = (time.perf_counter() - t0) * 1e3
        acc = EvalAccumulator.like(res).add(res)
        if self.total is None:
            self.total = EvalAccumulator.like(res)
        self.total.merge(acc)
        seq = self.batches
        self.batches += 1
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "count": int(res["n_scored"]),
               "metrics": acc.metrics().to_dict(), "accumulator": acc.to_dict(),
               "ms": round(ms, 3), "eval_ms": round(float(res.get("eval_ms", 0.0)), 3)}
        self._jsonl.write(json.dumps(rec) + "\n")
        self._jsonl.flush()

    def close(self) -> None:
        if self._jsonl is None:
            return
        self._jsonl.close()
        self._jsonl = None
        summary = {"batches": self.batches}
        if self.total is not None:
            summary.update(metrics=self.total.metrics().to_dict(), accumulator=self.total.to_dict())
        with open(os.path.join(self.out_dir, f"summary{self.suffix}.json"), "w", encoding="utf-8") as f:
            json.dump(summary, f)
            f.write("\n")


class TopJob:
    """Per-batch logic of ``--top N``: the batch's N best rows
    (``engine.top_batch``) as one line of ``top.jsonl``, the best N of the
    whole stream (``models/topn.TopNMerger``) in ``summary.json`` at the end.
    ``kind``: ``"linear"`` (value = prediction), ``"logistic"`` (value =
    margin; ``probability`` added on the host with the model class's link) or
    ``"kmeans"`` (value = ``dist2``, with ``label``)."""

    def __init__(self, engine, n: int, largest: bool, out_dir: str, kind: str = "linear", rank: int = 0,
                 world: int = 1, **engine_kw):
        from ..models.topn import TopNMerger
        self.engine = engine
        self.n, self.largest, self.kind = int(n), bool(largest), kind
        self.kw = engine_kw
        self.out_dir = out_dir
        self.suffix = f"_r{rank}" if world > 1 else ""
        self.batches = 0
        self.merger = TopNMerger(self.n, self.largest)
        os.makedirs(out_dir, exist_ok=True)
        self._jsonl = open(os.path.join(out_dir, f"top{self.suffix}.jsonl"), "a", encoding="utf-8")

    def _entries(self, raw, res) -> List[dict]:
        from ..records.batch import RETWEET_COUNT
        rows = [int(r) for r in res["rows"]]
        out = [{"row": r, "value": float(v), "retweetCount": int(raw.scalars[RETWEET_COUNT][r]),
                "text": raw.text_of(r)} for r, v in zip(rows, res["values"])]
        if self.kind == "logistic":
            from ..models.logistic_regression import sigmoid
            for e, p in zip(out, sigmoid(np.asarray(res["values"], np.float64))):
                e["probability"] = float(p)
        elif self.kind == "kmeans":
            for e, lab in zip(out, res["labels"]):
                e["dist2"] = e["value"]
                e["label"] = int(lab)
        return out

    def on_batch(self, rdd, time_ms: int) -> None:
        raw = rdd.raw
        t0 = time.perf_counter()
        res = self.engine.top_batch(raw, self.n, largest=self.largest, **self.kw)
        ms = (time.perf_counter() - t0) * 1e3
        entries = self._entries(raw, res)
        seq = self.batches
        self.batches += 1
        self.merger.add(seq, [e["value"] for e in entries], [e["row"] for e in entries], int(res["n_nan"]),
                        [{k: v for k, v in e.items() if k not in ("row", "value")} for e in entries])
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "count": int(res["n_scored"]), "n_nan": int(res["n_nan"]),
               "ms": round(ms, 3), "top_ms": round(float(res.get("top_ms", 0.0)), 3), "entries": entries}
        if self.kind == "kmeans":
            rec["cost"] = float(res["cost"])
        self._jsonl.write(json.dumps(rec) + "\n")
        self._jsonl.flush()

    def close(self) -> None:
        if self._jsonl is None:
            return
        self._jsonl.close()
        self._jsonl = None
        summary = {"batches": self.batches, "n": self.n, "largest": self.largest, "n_nan": self.merger.n_nan,
                   "entries": self.merger.result()}
        with open(os.path.join(self.out_dir, f"summary{self.suffix}.json"), "w", encoding="utf-8") as f:
            json.dump(summary, f)
            f.write("\n")


class SilhouetteJob:
    """Per-batch logic of ``--silhouetteOut``: the batch's silhouette
    (``engine.silhouette_batch``) as one line of ``silhouette.jsonl``, the
    merged accumulator with the stream's ``silhouette`` and
    ``cluster_silhouette`` in ``summary.json`` at the end."""

    def __init__(self, engine, k: int, out_dir: str, rank: int = 0, world: int = 1, **engine_kw):
        from ..models.silhouette import SilhouetteAccumulator
        self.engine = engine
        self.kw = engine_kw
        self.out_dir = out_dir
        self.suffix = f"_r{rank}" if world > 1 else ""
        self.batches = 0
        self.total = SilhouetteAccumulator(k)
        os.makedirs(out_dir, exist_ok=True)
        self._jsonl = open(os.path.join(out_dir, f"silhouette{self.suffix}.jsonl"), "a", encoding="utf-8")

    def on_batch(self, rdd, time_ms: int) -> None:
        t0 = time.perf_counter()
        res = self.engine.silhouette_batch(rdd.raw, apply_filter=True, **self.kw)
        ms = (time.perf_counter() - t0) * 1e3
        acc = res["accumulator"]
        self.total.merge(acc)
        seq = self.batches
        self.batches += 1
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "n_raw": int(res["n_raw"]), "n_scored": int(res["n_scored"]),
               "silhouette": res["silhouette"], "n_single": acc.n_single, "n_undefined": acc.n_undefined,
               "clusters_used": int(np.count_nonzero(res["sizes"])), "cost": float(res["cost"]),
               "accumulator": acc.to_dict(), "ms": round(ms, 3), "sil_ms": round(float(res.get("sil_ms", 0.0)), 3)}
        self._jsonl.write(json.dumps(rec) + "\n")
        self._jsonl.flush()

    def close(self) -> None:
        if self._jsonl is None:
            return
        self._jsonl.close()
        self._jsonl = None
        summary = {"batches": self.batches, **self.total.summary()}
        with open(os.path.join(self.out_dir, f"summary{self.suffix}.json"), "w", encoding="utf-8") as f:
            json.dump(summary, f)
            f.write("\n")


class ExemplarsJob:
    """Per-batch logic of ``--exemplars M``: per cluster the batch's M rows
    nearest the centre (``engine.exemplars_batch``; ``largest``: the farthest)
    as one line of ``exemplars.jsonl``, the best M per cluster of the whole
    stream (``models/exemplars.ExemplarMerger``) in ``summary.json`` at the end.
    The scaler the engine is called with is recorded there by name (an array of
    stds: ``"given"``; else ``"batch"`` or ``"none"`` as passed; the driver
    passes the first two): distances of different batches are on one scale only
    with a given scaler or none -- under the per-batch scaler the summary merges
    distances measured in each batch's own units."""

    def __init__(self, engine, k: int, m: int, largest: bool, out_dir: str, rank: int = 0, world: int = 1,
                 **engine_kw):
        from ..models.exemplars import ExemplarMerger
        self.engine = engine
        self.k, self.m, self.largest = int(k), int(m), bool(largest)
        scaler = engine_kw.get("scaler", "batch")
        self.scaler_name = scaler if isinstance(scaler, str) else "given"
        self.kw = engine_kw
        self.out_dir = out_dir
        self.suffix = f"_r{rank}" if world > 1 else ""
        self.batches = 0
        self.merger = ExemplarMerger(self.k, self.m, self.largest)
        os.makedirs(out_dir, exist_ok=True)
        self._jsonl = open(os.path.join(out_dir, f"exemplars{self.suffix}.jsonl"), "a", encoding="utf-8")

    def _clusters(self, raw, res) -> List[dict]:
        from ..records.batch import RETWEET_COUNT
        out = []
        for c in np.flatnonzero(np.asarray(res["sizes"]) > 0):
            n = int(res["counts"][c])
            entries = [{"row": int(r), "dist2": float(v), "retweetCount": int(raw.scalars[RETWEET_COUNT][int(r)]),
                        "text": raw.text_of(int(r))} for r, v in zip(res["rows"][c, :n], res["values"][c, :n])]
            out.append({"label": int(c), "size": int(res["sizes"][c]), "entries": entries})
        return out

    def on_batch(self, rdd, time_ms: int) -> None:
        raw = rdd.raw
        t0 = time.perf_counter()
        res = self.engine.exemplars_batch(raw, self.m, largest=self.largest, **self.kw)
        ms = (time.perf_counter() - t0) * 1e3
        clusters = self._clusters(raw, res)
        seq = self.batches
        self.batches += 1
        extras = {(c["label"], e["row"]): {"retweetCount": e["retweetCount"], "text": e["text"]}
                  for c in clusters for e in c["entries"]}
        self.merger.add(seq, res["counts"], res["rows"], res["values"], extras, int(res["n_nan"]))
        rec = {"seq": seq, "batch_time_ms": int(time_ms), "n_raw": int(res["n_raw"]), "n_scored": int(res["n_scored"]),
               "n_nan": int(res["n_nan"]), "clusters_used": int(np.count_nonzero(res["sizes"])),
               "cost": float(res["cost"]), "ms": round(ms, 3), "ex_ms": round(float(res.get("ex_ms", 0.0)), 3),
               "clusters": clusters}
        self._jsonl.write(json.dumps(rec) + "\n")
        self._jsonl.flush()

    def close(self) -> None:
        if self._jsonl is None:
            return
        self._jsonl.close()
        self._jsonl = None
        clusters = [{"label": c["label"], "entries": [{**{k: v for k, v in e.items() if k != "value"},
                                                       "dist2": e["value"]} for e in c["entries"]]}
                    for c in self.merger.result()]
        summary = {"batches": self.batches, "k": self.k, "m": self.m, "largest": self.largest,
                   "scaler": self.scaler_name, "n_nan": self.merger.n_nan, "clusters": clusters}
        with open(os.path.join(self.out_dir, f"summary{self.suffix}.json"), "w", encoding="utf-8") as f:
            json.dump(summary, f)
            f.write("\n")


def build_kmeans_scorer(conf, centers: np.ndarray, weights: np.ndarray, device: Optional[int]):
    """The engine that scores with a loaded k-means model: a DeviceKMeans on
    ``device`` (no communicator: every rank scores its own shard) or, with
    ``device`` None, the fp64 CpuKMeans."""
    k, dim = centers.shape
    if device is not None:
        from ..ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
        rows = max(65536, conf.batchSize)
        engine = DeviceKMeans(KMDeviceConfig(k=k, text_dims=dim - 2, max_rows=rows, max_units=rows * 290,
                                             seed=conf.seed), device=device)
    else:
        from ..models.kmeans import CpuKMeans
        engine = CpuKMeans(k, dim, seed=conf.seed)
    engine.set_state(centers, weights)
    return engine


def main(argv: Optional[List[str]] = None) -> int:
    setup_logging()
    exit_on_sigterm()
    from ..runtime.clock import streaming_clock
    args = load_java_opts(list(sys.argv[1:] if argv is None else argv))
    conf = ConfArguments().setAppName(APP_NAME).parse(args)
    if not conf.model:
        print("twtml-score: --model <MLlib model directory> is required", file=sys.stderr)
        return 2
    output = None
    km = None
    try:
        from ..checkpoint.saveable import KMEANS_CLASS, LOGISTIC_CLASS, model_class
        cls = model_class(conf.model)
        logistic = cls == LOGISTIC_CLASS
        if cls == KMEANS_CLASS:
            from ..models.kmeans import StreamingKMeansModel
            km = StreamingKMeansModel.load(conf.model)
            w = km.clusterCenters
        elif logistic:
            from ..models.logistic_regression import LogisticRegressionModel
            m = LogisticRegressionModel.load(conf.model)
            w = m.weights
            output = "probability" if m.threshold is None else "class"
            if m.threshold is not None:
                conf.threshold = m.threshold   # the model's own threshold decides the class
        else:
            w = LinearRegressionModel.load(conf.model).weights
    except Exception as e:   # noqa: BLE001 -- any unreadable model is the same usage error
        print(f"twtml-score: cannot load the model at {conf.model}: {e}", file=sys.stderr)
        return 2
    if km is not None and conf.evalOut:
        print("twtml-score: --evalOut does not apply to a k-means model: its metric is the cost that "
              "--predictOut already reports (--silhouetteOut measures the clustering itself)", file=sys.stderr)
        return 2
    if km is None and conf.silhouetteOut:
        print("twtml-score: --silhouetteOut needs a k-means model; --evalOut evaluates a linear or logistic one",
              file=sys.stderr)
        return 2
    if conf.top or conf.topOut or conf.topSmallest:
        from ..models.topn import TOPN_MAX
        if not conf.topOut or not 1 <= conf.top <= TOPN_MAX:
            print(f"twtml-score: --top N needs N in 1..{TOPN_MAX} and --topOut <dir> (got --top {conf.top}, "
                  f"--topOut {conf.topOut!r}); --predictOut writes every row", file=sys.stderr)
            return 2
    if conf.exemplars or conf.exemplarsOut or conf.exemplarsFarthest:
        from ..models.exemplars import EXEMPLARS_MAX, check_m
        if km is None:
            print("twtml-score: --exemplars needs a k-means model; --top selects the best rows of a linear or "
                  "logistic one", file=sys.stderr)
            return 2
        if not conf.exemplarsOut or not 1 <= conf.exemplars <= EXEMPLARS_MAX:
            print(f"twtml-score: --exemplars M needs M in 1..{EXEMPLARS_MAX} and --exemplarsOut <dir> (got --exemplars "
                  f"{conf.exemplars}, --exemplarsOut {conf.exemplarsOut!r}); --predictOut writes every row",
                  file=sys.stderr)
            return 2
        try:
            check_m(int(w.shape[0]), conf.exemplars)
        except ValueError as e:
            print(f"twtml-score: --exemplars {conf.exemplars} with the {w.shape[0]} centres of {conf.model}: {e}",
                  file=sys.stderr)
            return 2
    scaler = "batch"
    if km is not None:
        text_dims = (w.shape[1] if w.ndim == 2 else 0) - 2
        if w.shape[0] < 1 or text_dims < 0 or text_dims > 4000:
            print(f"twtml-score: the k-means model at {conf.model} has centres of shape {w.shape}; the engine takes "
                  f"k >= 1 centres of 2 + text_dims columns, text_dims in [0, 4000]", file=sys.stderr)
            return 2
        if conf.scalerStd:
            try:
                scaler = np.asarray(np.load(conf.scalerStd), np.float64)
                if scaler.shape != (w.shape[1],):
                    raise ValueError(f"{scaler.shape[0] if scaler.ndim == 1 else scaler.shape} stds for "
                                     f"{w.shape[1]} columns")
            except Exception as e:   # noqa: BLE001 -- unreadable or misshapen: the same usage error
                print(f"twtml-score: cannot use --scalerStd {conf.scalerStd}: {e}", file=sys.stderr)
                return 2
    want = conf.effectiveNumTextFeatures + 4
    if km is None and w.shape[0] != want:
        print(f"twtml-score: the model at {conf.model} has {w.shape[0]} weights, but numTextFeatures + 4 = {want} "
              f"(give the -f / --numTextFeatures the model was trained with)", file=sys.stderr)
        return 2

    spec = conf.master_spec()
    # one process per GPU under the launcher; no process group: scoring has no collective
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    MllibHelper.reset(conf)
    # every rank scores alone: an engine without a communicator, on its GPU
    dev = (spec.devices[rank] if spec.devices else rank) if spec.is_gpu else None
    if km is not None:
        engine = build_kmeans_scorer(conf, km.clusterCenters, km.clusterWeights, dev)
        log.info("scoring with %d centres of %d columns from %s", w.shape[0], w.shape[1], conf.model)
    else:
        engine = build_engine(conf, 0, 1, device=dev, loss="logistic" if logistic else "squared")
        engine.set_weights(w)
        log.info("scoring with %d weights from %s", w.shape[0], conf.model)

    cap = getattr(engine, "cfg", None)
    ssc = StreamingContext(conf.seconds, batch_size=conf.batchSize, num_batches=conf.numBatches,
                           app_name=conf.appName(),
                           max_batch_rows=int(getattr(cap, "max_rows", 0) or 0),
                           max_batch_units=int(getattr(cap, "max_units", 0) or 0),
                           clock=streaming_clock())
    stream = ssc.twitterStream(make_source(conf.source, rate=conf.sourceRate, seed=conf.seed,
                                           shard=rank, num_shards=world, start=0, batch_size=conf.batchSize)).cache()
    if km is not None:
        job = KMeansScoreJob(engine, text_dims, scaler, conf.predictOut, rank, world)
    else:
        job = ScoreJob(engine, conf.predictOut, rank, world, output)
    ev = EvalJob(engine, conf.evalOut, rank, world) if conf.evalOut else None
    top = None
    if conf.top:
        if km is not None:
            top = TopJob(engine, conf.top, not conf.topSmallest, conf.topOut, "kmeans", rank, world,
                         apply_filter=True, scaler=scaler, **job._kw)
        else:
            top = TopJob(engine, conf.top, not conf.topSmallest, conf.topOut, "logistic" if logistic else "linear",
                         rank, world, apply_filter=False)
    sil = None
    if conf.silhouetteOut:
        sil = SilhouetteJob(engine, int(w.shape[0]), conf.silhouetteOut, rank, world, scaler=scaler, **job._kw)
    ex = None
    if conf.exemplars:
        ex = ExemplarsJob(engine, int(w.shape[0]), conf.exemplars, conf.exemplarsFarthest, conf.exemplarsOut,
                          rank, world, apply_filter=True, scaler=scaler, **job._kw)
    score = (ev is None and top is None and sil is None and ex is None) or bool(conf.predictOut)
    if score:
        stream.foreachRDD(job.on_batch)
    if ev is not None:
        stream.foreachRDD(ev.on_batch)
    if top is not None:
        stream.foreachRDD(top.on_batch)
    if sil is not None:
        stream.foreachRDD(sil.on_batch)
    if ex is not None:
        stream.foreachRDD(ex.on_batch)
    ssc.start()
    try:
        ssc.awaitTermination()
    except KeyboardInterrupt:
        pass
    finally:
        ssc.stop()
        job.close()
        if ev is not None:
            ev.close()
        if top is not None:
            top.close()
        if sil is not None:
            sil.close()
        if ex is not None:
            ex.close()
    if sil is not None:
        log.info("silhouette %s over %d batches", sil.total.silhouette, sil.batches)
    if ex is not None:
        log.info("selected %d exemplars per cluster of %d batches", ex.m, ex.batches)
    if ev is not None:
        log.info("evaluated %d batches", ev.batches)
    if top is not None:
        log.info("selected the top %d of %d batches", top.n, top.batches)
    if score:
        log.info("scored %d tweets in %d batches", job.scored, job.batches)
    return 0


if __name__ == "__main__":
    sys.exit(main())

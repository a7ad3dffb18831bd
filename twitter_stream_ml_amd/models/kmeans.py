"""Streaming k-means and the standard scaler: MLlib API + CPU engine (C2, U8-U10).

* :class:`StreamingKMeans` — builder (``setK``, ``setDecayFactor``,
  ``setHalfLife(h, "batches"|"points")``, ``setRandomCenters(dim, weight,
  seed)``, ``setInitialCenters``), ``latestModel``, ``trainOn``,
  ``predictOn`` (``KMeans.scala:69-73``).
* :class:`StreamingKMeansModel` — ``update(data, decayFactor, timeUnit)``,
  ``predict``, ``clusterCenters`` / ``clusterWeights``, checkpoint save/load.
* :class:`StandardScaler` / :class:`StandardScalerModel` —
  ``StandardScaler(withMean=false, withStd=true).fit(rdd).transform(rdd)``
  re-fitted every batch (``KMeans.scala:103``).
* :func:`kmeans_features` — the KMeans job's featurization of a raw batch:
  retweets only (``KMeans.scala:77-80``), ``[retweetCount, followersCount]``
  of the original (``:19-29``), optionally followed by ``text_dims`` hashed
  bigram counts (engine extension for the k=1024 configuration).
* :class:`CpuKMeans` — the ``local[N]`` engine with the batch contract of the
  MI355X k-means engine (``ops/kmeans_engine.py``).
"""
from __future__ import annotations

import math
import time
from typing import Callable, Dict, Optional

import numpy as np

from ..oracle.mllib import (KMeansState, decay_factor_from_half_life, find_closest, kmeans_update,
                            standard_scaler_fit, standard_scaler_transform)
from ..records.batch import FOLLOWERS, RETWEET_COUNT, RawBatch
from .vectors import DenseVector, Vector

__all__ = ["StreamingKMeans", "StreamingKMeansModel", "StandardScaler", "StandardScalerModel",
           "kmeans_features", "CpuKMeans", "scaler_mode", "empty_score"]

BATCHES = "batches"
POINTS = "points"


def kmeans_features(raw: RawBatch, text_dims: int = 0, hash: str = "java", apply_filter: bool = True):
    """Dense (n_retweets, 2 + text_dims) fp64 features and the kept row ids
    (``apply_filter`` off: every row, for scoring)."""
    rows = (np.nonzero(raw.is_retweet != 0)[0] if apply_filter else np.arange(raw.n)).astype(np.int64)
    n = rows.shape[0]
    X = np.zeros((n, 2 + text_dims))
    X[:, 0] = raw.scalars[RETWEET_COUNT, rows]
    X[:, 1] = raw.scalars[FOLLOWERS, rows]
    if text_dims > 0 and n:
        from ..ops._native import host
        raw.ensure_text()   # a replayed batch may carry only its UTF-8 bytes
        indptr, idx = host().featurize_rows(raw.text, raw.offsets, rows, text_dims, hash, 0)
        r = np.repeat(np.arange(n), np.diff(indptr))
        np.add.at(X, (r, 2 + idx), 1.0)
    return X, rows


# predict_batch's scaler modes, as KMEngine::score numbers them
SCALER_BATCH, SCALER_GIVEN, SCALER_NONE = 0, 1, 2


def scaler_mode(scaler, dim: int, scale: bool = True):
    """``predict_batch``'s ``scaler`` argument -> (mode, std or None): "batch"
    (per-batch fit; "none" for an engine that does not scale), "none", or an
    array of ``dim`` stds (frozen)."""
    if isinstance(scaler, str):
        if scaler not in ("batch", "none"):
            raise ValueError(f"unknown scaler {scaler!r} (batch, none or an array of {dim} stds)")
        return (SCALER_BATCH if scaler == "batch" and scale else SCALER_NONE), None
    std = np.ascontiguousarray(scaler, dtype=np.float64)
    if std.shape != (dim,):
        raise ValueError(f"the scaler needs {dim} stds, got shape {std.shape}")
    return SCALER_GIVEN, std


def empty_score(n_raw: int, k: int, std=None) -> Dict[str, object]:
    """``predict_batch`` of a batch with nothing to score."""
    return {"n_raw": int(n_raw), "n_scored": 0, "rows": np.zeros(0, np.int64), "pred": np.zeros(0, np.int32),
            "dist2": np.zeros(0, np.float64), "cost": 0.0, "sizes": np.zeros(int(k), np.int64),
            "std": None if std is None else std.copy(), "score_ms": 0.0, "wall_ms": 0.0}


class StandardScalerModel:
    def __init__(self, std: np.ndarray, mean: Optional[np.ndarray] = None,
                 withStd: bool = True, withMean: bool = False):
        self.std = np.asarray(std, np.float64)
        self.mean = mean
        self.withStd, self.withMean = withStd, withMean

    def transform(self, data):
        from ..runtime.rdd import RDD
        if isinstance(data, RDD):
            return data.map(lambda v: DenseVector(self.transform(v.toArray() if isinstance(v, Vector) else v)))
        X = np.asarray(data, np.float64)
        if self.withMean and self.mean is not None:
            X = X - self.mean
        return standard_scaler_transform(X, self.std) if self.withStd else X


class StandardScaler:
    def __init__(self, withMean: bool = False, withStd: bool = True):
        self.withMean, self.withStd = withMean, withStd

    def fit(self, data, allreduce=None) -> StandardScalerModel:
        from ..runtime.rdd import RDD
        if isinstance(data, RDD):
            X = np.stack([v.toArray() if isinstance(v, Vector) else np.asarray(v) for v in data.collect()])
        else:
            X = np.asarray(data, np.float64)
        std = standard_scaler_fit(X, allreduce)
        mean = X.mean(axis=0) if self.withMean and X.shape[0] else None
        return StandardScalerModel(std, mean, self.withStd, self.withMean)


class StreamingKMeansModel:
    def __init__(self, clusterCenters: np.ndarray, clusterWeights: np.ndarray):
        self.state = KMeansState(np.asarray(clusterCenters, np.float64).copy(),
                                 np.asarray(clusterWeights, np.float64).copy())

    @property
    def clusterCenters(self) -> np.ndarray:
        return self.state.centers

    @property
    def clusterWeights(self) -> np.ndarray:
        return self.state.weights

    @property
    def k(self) -> int:
        return int(self.state.centers.shape[0])

    def predict(self, x):
        from ..runtime.rdd import RDD
        if isinstance(x, RDD):
            return x.map(self.predict)
        if isinstance(x, Vector):
            return int(find_closest(self.state.centers, x.toArray()[None, :])[0])
        X = np.asarray(x, np.float64)
        if X.ndim == 1:
            return int(find_closest(self.state.centers, X[None, :])[0])
        return find_closest(self.state.centers, X)

    def update(self, data, decayFactor: float, timeUnit: str = BATCHES, allreduce=None):
        from ..runtime.rdd import RDD
        if isinstance(data, RDD):
            pts = data.collect()
            X = np.stack([p.toArray() if isinstance(p, Vector) else np.asarray(p) for p in pts]) \
                if pts else np.zeros((0, self.state.centers.shape[1]))
        else:
            X = np.asarray(data, np.float64)
        self.state, labels = kmeans_update(self.state, X, decayFactor, timeUnit, allreduce)
        return self

    def save(self, path: str, progress: Optional[dict] = None) -> None:
        from ..checkpoint.saveable import save_kmeans
        save_kmeans(path, self.state.centers, self.state.weights, progress)

    @classmethod
    def load(cls, path: str) -> "StreamingKMeansModel":
        from ..checkpoint.saveable import load_kmeans
        c, w = load_kmeans(path)
        return cls(c, w if w is not None else np.ones(c.shape[0]))


class StreamingKMeans:
    def __init__(self, k: int = 2, decayFactor: float = 1.0, timeUnit: str = BATCHES):
        self.k = int(k)
        self.decayFactor = float(decayFactor)
        self.timeUnit = timeUnit
        self.model: Optional[StreamingKMeansModel] = None
        self.allreduce = None

    def setK(self, k: int) -> "StreamingKMeans":
        self.k = int(k)
        return self

    def setDecayFactor(self, a: float) -> "StreamingKMeans":
        self.decayFactor = float(a)
        return self

    def setHalfLife(self, halfLife: float, timeUnit: str) -> "StreamingKMeans":
        if timeUnit not in (BATCHES, POINTS):
            raise ValueError(f"Invalid time unit for decay: {timeUnit}")
        self.decayFactor = decay_factor_from_half_life(halfLife)
        self.timeUnit = timeUnit
        return self

    def setRandomCenters(self, dim: int, weight: float, seed: Optional[int] = None) -> "StreamingKMeans":
        seed = int(np.random.SeedSequence().entropy % (1 << 63)) if seed is None else int(seed)
        st = KMeansState.random(self.k, dim, weight, seed)
        self.model = StreamingKMeansModel(st.centers, st.weights)
        return self

    def setInitialCenters(self, centers, weights) -> "StreamingKMeans":
        self.model = StreamingKMeansModel(np.asarray(centers), np.asarray(weights))
        self.k = self.model.k
        return self

    def latestModel(self) -> StreamingKMeansModel:
        if self.model is None:
            raise ValueError("Initial cluster centers must be set before starting predictions")
        return self.model

    def trainOn(self, stream) -> None:
        def op(rdd):
            self.latestModel().update(rdd, self.decayFactor, self.timeUnit, self.allreduce)
        stream.foreachRDD(op)

    def predictOn(self, stream):
        return stream.map(lambda v: self.latestModel().predict(v))

    def predictOnValues(self, stream):
        return stream.map(lambda kv: (kv[0], self.latestModel().predict(kv[1])))


class CpuKMeans:
    """fp64 engine: per batch scaler fit + transform, then the streaming update."""

    def __init__(self, k: int, dim: int, half_life: float = 5.0, time_unit: str = BATCHES,
                 init_weight: float = 0.0, seed: int = 42, scale: bool = True,
                 allreduce: Optional[Callable[[np.ndarray], np.ndarray]] = None):
        st = KMeansState.random(k, dim, init_weight, seed)
        self.state = st
        self.decay = decay_factor_from_half_life(half_life)
        self.time_unit = time_unit
        self.scale = scale
        self.allreduce = allreduce

    def set_state(self, centers, weights) -> None:
        self.state = KMeansState(np.asarray(centers, np.float64).copy(), np.asarray(weights, np.float64).copy())

    def get_state(self):
        return self.state.centers.copy(), self.state.weights.copy()

    def update_batch(self, X: np.ndarray) -> Dict[str, object]:
        n_local = np.array([float(X.shape[0])])
        n = self.allreduce(n_local)[0] if self.allreduce else n_local[0]
        if n == 0:
            return {"n": 0, "labels": np.zeros(0, np.int64), "std": None}
        std = standard_scaler_fit(X, self.allreduce) if self.scale else np.ones(X.shape[1])
        Xs = standard_scaler_transform(X, std) if self.scale else X
        self.state, labels = kmeans_update(self.state, Xs, self.decay, self.time_unit, self.allreduce)
        # KMeans.scala:113 predicts with the *updated* model
        pred = find_closest(self.state.centers, Xs) if Xs.shape[0] else np.zeros(0, np.int64)
        return {"n": int(n), "labels": labels, "pred": pred, "std": std, "scaled": Xs}

    def predict_batch(self, raw: RawBatch, text_dims: int, apply_filter: bool = True,
                      scaler="batch") -> Dict[str, object]:
        """The contract of ``DeviceKMeans.predict_batch`` in fp64 (its oracle):
        closest centre, squared distance to it in the scaled space, their sum
        (``KMeansModel.computeCost``) and the rows per cluster of a raw batch
        under the current model, which is left as it is.  The per-batch scaler
        is fitted on the scored rows of this process alone."""
        t0 = time.perf_counter()
        k, dim = self.state.centers.shape
        if dim != 2 + text_dims:
            raise ValueError(f"the model has {dim} columns, text_dims + 2 = {2 + text_dims}")
        mode, std = scaler_mode(scaler, dim, self.scale)
        X, rows = kmeans_features(raw, text_dims, apply_filter=apply_filter)
        if X.shape[0] == 0:
            return empty_score(raw.n, k, std)
        if mode == SCALER_BATCH:
            std = standard_scaler_fit(X)
        Xs = X if std is None else standard_scaler_transform(X, std)
        pred = find_closest(self.state.centers, Xs)
        dist2 = ((Xs - self.state.centers[pred]) ** 2).sum(axis=1)
        ms = (time.perf_counter() - t0) * 1e3
        return {"n_raw": int(raw.n), "n_scored": int(X.shape[0]), "rows": rows, "pred": pred.astype(np.int32),
                "dist2": dist2, "cost": float(dist2.sum()), "sizes": np.bincount(pred, minlength=k).astype(np.int64),
                "std": std, "score_ms": ms, "wall_ms": ms}

    def silhouette_batch(self, raw: RawBatch, text_dims: int, apply_filter: bool = True, scaler="batch",
                         per_row: bool = False) -> Dict[str, object]:
        """The silhouette of the current model on one raw batch (MLlib's
        ``ClusteringEvaluator``, squared Euclidean), the contract of
        ``DeviceKMeans.silhouette_batch``: ``models/silhouette.py`` applied in
        fp64 to this engine's own ``predict_batch`` labels.  ``silhouette``
        (None when fewer than two clusters are non-empty), ``accumulator``
        (a ``SilhouetteAccumulator`` of this batch), ``sizes``, ``cost``,
        ``std``, ``n_raw``, ``n_scored``; ``per_row``: also ``rows``, ``pred``,
        ``neighbor`` (int32, -1 where undefined), ``a``, ``b``, ``s``.  Every
        batch is measured against its own cluster means; the model is left as
        it is."""
        from .silhouette import SilhouetteAccumulator, batch_silhouette, empty_silhouette
        t0 = time.perf_counter()
        k = self.state.centers.shape[0]
        res = self.predict_batch(raw, text_dims, apply_filter=apply_filter, scaler=scaler)
        n = int(res["n_scored"])
        if n == 0:
            return empty_silhouette(raw.n, k, res["std"], per_row)
        X, rows = kmeans_features(raw, text_dims, apply_filter=apply_filter)
        Xs = X if res["std"] is None else standard_scaler_transform(X, res["std"])
        b = batch_silhouette(Xs, res["pred"], k)
        acc = SilhouetteAccumulator(k)
        if b["defined"]:
            acc.add_rows(res["pred"], b["s"])
        else:
            acc.add_undefined(n)
        ms = (time.perf_counter() - t0) * 1e3
        out = {"n_raw": int(raw.n), "n_scored": n, "silhouette": acc.silhouette, "accumulator": acc,
               "sizes": res["sizes"], "cost": res["cost"], "std": res["std"], "sil_ms": ms, "wall_ms": ms}
        if per_row:
            out.update(rows=rows, pred=res["pred"], neighbor=b["neighbor"], a=b["a"], b=b["b"], s=b["s"])
        return out

    def top_batch(self, raw: RawBatch, n: int, text_dims: int, largest: bool = True, apply_filter: bool = True,
                  scaler="batch") -> Dict[str, object]:
        """The n rows farthest from their centres (``largest``: the batch's
        outliers; else the closest), the contract of ``DeviceKMeans.top_batch``:
        ``models/topn.top_n`` of this engine's own ``predict_batch`` ``dist2``,
        with the rows' labels and the batch's ``cost``, ``sizes`` and ``std``."""
        from .topn import check_n, top_result
        check_n(n)
        t0 = time.perf_counter()
        res = self.predict_batch(raw, text_dims, apply_filter=apply_filter, scaler=scaler)
        out = top_result(res["dist2"], res["rows"], n, largest)
        labels = np.asarray(res["pred"], np.int32)[np.searchsorted(res["rows"], out["rows"])]
        ms = (time.perf_counter() - t0) * 1e3
        out.update(dist2=out["values"], labels=labels, cost=res["cost"], sizes=res["sizes"], std=res["std"],
                   n_raw=res["n_raw"], n_scored=res["n_scored"], top_ms=ms, wall_ms=ms)
        return out

    def exemplars_batch(self, raw: RawBatch, m: int, text_dims: int, largest: bool = False,
                        apply_filter: bool = True, scaler="batch") -> Dict[str, object]:
        """Per cluster, the m rows nearest their centre (``largest``: the
        cluster's own outliers), the contract of
        ``DeviceKMeans.exemplars_batch``: ``models/exemplars.cluster_top`` of
        this engine's own ``predict_batch`` ``dist2`` and ``pred``, with the
        batch's ``cost``, ``sizes`` and ``std``."""
        from .exemplars import check_m, exemplars_result
        k = self.state.centers.shape[0]
        check_m(k, m)
        t0 = time.perf_counter()
        res = self.predict_batch(raw, text_dims, apply_filter=apply_filter, scaler=scaler)
        out = exemplars_result(res["dist2"], res["pred"], res["rows"], k, m, largest)
        ms = (time.perf_counter() - t0) * 1e3
        out.update(dist2=out["values"], cost=res["cost"], sizes=res["sizes"], std=res["std"],
                   n_raw=res["n_raw"], n_scored=res["n_scored"], ex_ms=ms, wall_ms=ms)
        return out

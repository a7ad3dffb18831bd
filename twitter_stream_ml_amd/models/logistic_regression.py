"""Streaming logistic regression: MLlib API + the fp64 CPU engine.

``StreamingLogisticRegressionWithSGD`` is MLlib's third streaming learner: the
GD loop of the linear model (``GradientDescent.runMiniBatchSGD``, same
sampling, same convergence rule) with the binary ``LogisticGradient``

    margin = -x.w
    r      = 1 / (1 + exp(margin)) - y              (the gradient multiplier)
    loss   = log1pExp(margin)            if y > 0
             log1pExp(margin) - margin   otherwise

and ``SquaredL2Updater``, which at the streaming class's default ``regParam =
0.0`` is arithmetically ``SimpleUpdater``.  A non-zero ``regParam`` is not
supported: L2 shrinkage touches every weight each iteration, which the
engines' compact active space (only the batch's features move) cannot express.

Here the label of a tweet is ``retweetCount >= labelThreshold`` -- "will this
tweet pass N retweets" -- on the rows the usual filter keeps.

* :func:`logistic_gradient`, :func:`run_minibatch_sgd_logistic` -- the oracle
  of the MI355X logistic path (``csrc/hip/sgd.hip``, ``LOSS = logistic``).
* :class:`LogisticRegressionModel` -- weights, threshold (``setThreshold`` /
  ``clearThreshold``), ``predict``, MLlib-layout ``save`` / ``load``.
* :class:`CpuLogisticRegression` -- the ``local[N]`` engine with the batch
  contract of ``ops/lr_engine.DeviceLogisticRegression``.
* :class:`StreamingLogisticRegressionWithSGD` -- the MLlib builder.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import scipy.sparse as sp

from ..oracle.mllib import CONVERGENCE_TOL, SGDResult, sgd_uniform
from ..records.batch import RawBatch
from .linear_regression import (StreamingLinearRegressionWithSGD, featurize_columnar,
                                stats_from_predictions)
from .vectors import DenseVector, Vector

__all__ = ["logistic_gradient", "run_minibatch_sgd_logistic", "LogisticRegressionModel",
           "StreamingLogisticRegressionWithSGD", "CpuLogisticRegression", "CpuLogisticConfig",
           "default_label_threshold", "logit", "sigmoid", "labels_of"]

log = logging.getLogger("org.apache.spark.mllib.classification.StreamingLogisticRegressionWithSGD")
AllReduce = Optional[Callable[[np.ndarray], np.ndarray]]


def default_label_threshold(begin: int, end: int) -> int:
    """Middle of the retweet filter's range (550 at the reference's 100..1000)."""
    return (int(begin) + int(end)) // 2


def logit(p: float) -> float:
    return math.log(p / (1.0 - p))


def sigmoid(m: np.ndarray) -> np.ndarray:
    """``1 / (1 + exp(-m))`` without overflow warnings (exp -> inf gives exactly 0)."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(m, dtype=np.float64)))


def labels_of(retweets: np.ndarray, label_threshold: int) -> np.ndarray:
    return (np.asarray(retweets) >= label_threshold).astype(np.float64)


def _log1p_exp(x: np.ndarray) -> np.ndarray:
    """``MLUtils.log1pExp``: x + log1p(exp(-x)) for x > 0, log1p(exp(x)) otherwise."""
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def logistic_gradient(X: sp.csr_matrix, y: np.ndarray, w: np.ndarray,
                      mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, float, int]:
    """Sum of the binary ``LogisticGradient`` over (sampled) rows: (g, loss, m)."""
    if mask is not None:
        X = X[mask]
        y = y[mask]
    dot = np.asarray(X @ w, dtype=np.float64).reshape(-1)
    margin = -dot
    e = np.exp(-np.abs(dot))                       # in (0, 1]: nothing overflows
    mult = np.where(dot >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e)) - y
    l1p = _log1p_exp(margin)
    loss = np.where(y > 0.0, l1p, l1p - margin)
    g = X.T @ mult
    return np.asarray(g, dtype=np.float64).reshape(-1), float(loss.sum()), int(y.shape[0])


def run_minibatch_sgd_logistic(X: sp.csr_matrix, y: np.ndarray, w0: np.ndarray, step_size: float,
                               num_iterations: int, mini_batch_fraction: float = 1.0,
                               convergence_tol: float = CONVERGENCE_TOL, allreduce: AllReduce = None,
                               row_offset: int = 0) -> SGDResult:
    """``oracle.mllib.run_minibatch_sgd`` with :func:`logistic_gradient`: the
    same loop, sampling, DP ``allreduce`` hook and convergence rule."""
    if mini_batch_fraction > 1.0 + 1e-12 or mini_batch_fraction <= 0:
        raise ValueError(f"miniBatchFraction must be in (0, 1], got {mini_batch_fraction}")
    red = allreduce if allreduce is not None else (lambda v: v)
    n_local = int(y.shape[0])
    num_examples = int(round(red(np.array([float(n_local)]))[0]))
    w = np.array(w0, dtype=np.float64, copy=True)
    res = SGDResult(w, num_examples=num_examples)
    if num_examples == 0:
        return res
    prev: Optional[np.ndarray] = None
    cur: Optional[np.ndarray] = None
    converged = False
    i = 1
    rows = np.arange(row_offset, row_offset + n_local, dtype=np.uint64)
    while not converged and i <= num_iterations:
        mask = None
        if mini_batch_fraction < 1.0:
            mask = sgd_uniform(42 + i, rows) < mini_batch_fraction
        g, loss, m = logistic_gradient(X, y, w, mask)
        packed = red(np.concatenate([g, [loss, float(m)]]))
        g, loss, m = packed[:-2], packed[-2], int(round(packed[-1]))
        if m > 0:
            res.loss_history.append(loss / m)
            w = w - (step_size / math.sqrt(i)) * (g / m)
            prev, cur = cur, w
            if prev is not None and cur is not None:
                diff = float(np.linalg.norm(prev - cur))
                converged = diff < convergence_tol * max(float(np.linalg.norm(cur)), 1.0)
        i += 1
    res.weights = w
    res.iterations = i - 1
    res.converged = converged
    return res


# ---------------------------------------------------------------------------
class LogisticRegressionModel:
    """Binary ``LogisticRegressionModel``: class 1 when the probability
    exceeds ``threshold``; after ``clearThreshold`` ``predict`` returns the
    probability itself."""

    def __init__(self, weights, intercept: float = 0.0, threshold: Optional[float] = 0.5):
        self.weights = np.asarray(weights.toArray() if isinstance(weights, Vector) else weights,
                                  dtype=np.float64).copy()
        self.intercept = float(intercept)
        self.threshold = None if threshold is None else float(threshold)
        self.numClasses = 2

    @property
    def numFeatures(self) -> int:
        return int(self.weights.shape[0])

    def setThreshold(self, threshold: float) -> "LogisticRegressionModel":
        self.threshold = float(threshold)
        return self

    def clearThreshold(self) -> "LogisticRegressionModel":
        self.threshold = None
        return self

    def margin(self, x):
        if isinstance(x, Vector):
            return float(x.dot(DenseVector(self.weights))) + self.intercept
        if sp.issparse(x):
            return np.asarray(x @ self.weights).reshape(-1) + self.intercept
        return np.asarray(x, dtype=np.float64) @ self.weights + self.intercept

    def predict(self, x):
        from ..runtime.rdd import RDD
        if isinstance(x, RDD):
            return x.map(self.predict)
        score = sigmoid(self.margin(x))
        if self.threshold is not None:
            score = (score > self.threshold).astype(np.float64)
        return float(score) if np.ndim(score) == 0 else score

    def save(self, path: str, progress: Optional[dict] = None) -> None:
        from ..checkpoint.saveable import save_logistic_regression
        save_logistic_regression(path, self.weights, self.intercept, self.threshold, progress)

    @staticmethod
    def save_sparse(path: str, weights, intercept: float = 0.0, threshold: Optional[float] = 0.5,
                    progress: Optional[dict] = None) -> None:
        """Save weights given as ``checkpoint.SparseWeights`` (non-zeros only)."""
        from ..checkpoint.saveable import save_logistic_regression
        save_logistic_regression(path, weights, intercept, threshold, progress)

    @classmethod
    def load(cls, path: str) -> "LogisticRegressionModel":
        from ..checkpoint.saveable import load_logistic_regression
        w, b, thr = load_logistic_regression(path)
        return cls(w, b, thr)


# ---------------------------------------------------------------------------
@dataclass
class CpuLogisticConfig:
    num_text_features: int = 1000
    hash: str = "java"
    step_size: float = 0.1
    num_iterations: int = 50
    fraction: float = 1.0
    tol: float = CONVERGENCE_TOL
    begin: int = 100
    end: int = 1000
    label_threshold: int = -1     # < 0: (begin + end) // 2
    threshold: float = 0.5

    def __post_init__(self):
        if self.label_threshold < 0:
            self.label_threshold = default_label_threshold(self.begin, self.end)


def _link(margins: np.ndarray, output: str, threshold: float) -> np.ndarray:
    if output == "margin":
        return margins
    if output == "probability":
        return sigmoid(margins)
    if output == "class":
        return (margins > logit(threshold)).astype(np.float64)
    raise ValueError(f"unknown output {output!r} (class, probability or margin)")


class CpuLogisticRegression:
    """fp64 CPU engine with the DeviceLogisticRegression batch contract."""

    def __init__(self, cfg: CpuLogisticConfig, allreduce: AllReduce = None, rank: int = 0, world: int = 1):
        self.cfg = cfg
        self.allreduce = allreduce
        self.rank, self.world = rank, world
        self.w = np.zeros(cfg.num_text_features + 4)

    @property
    def num_weights(self) -> int:
        return int(self.w.shape[0])

    def get_weights(self) -> np.ndarray:
        return self.w.copy()

    def set_weights(self, w) -> None:
        w = np.asarray(w, dtype=np.float64)
        if w.shape != self.w.shape:
            raise ValueError(f"expected {self.w.shape[0]} weights, got {w.shape}")
        self.w = w.copy()

    def train_batch(self, raw: RawBatch, want_pred: bool = True, plot_points: int = 0,
                    slot: int = 0) -> Dict[str, object]:
        c = self.cfg
        X, rt, rows = featurize_columnar(raw, c.num_text_features, c.begin, c.end, hash=c.hash)
        y = labels_of(rt, c.label_threshold)
        red = self.allreduce
        counts = np.zeros(self.world)
        counts[self.rank] = y.shape[0]
        if red is not None:
            counts = red(counts)
        n_glob = int(round(counts.sum()))
        row_offset = int(round(counts[:self.rank].sum()))
        # prequential class under the weights before training on the batch
        pred = _link(np.asarray(X @ self.w).reshape(-1), "class", c.threshold) if y.shape[0] else np.zeros(0)
        stats = np.array(stats_from_predictions(y, pred))
        if red is not None:
            stats = red(stats)
        res: Dict[str, object] = {"n_raw": raw.n, "n_kept": int(y.shape[0]),
                                  "n_kept_global": n_glob, "iterations": 0, "converged": False,
                                  "loss_history": [], "stats": stats.tolist(),
                                  "pred": None, "real": None,
                                  "n_unique": int(np.unique(X.indices).shape[0]) if X.nnz else 0,
                                  "prep_ms": 0.0, "train_ms": 0.0, "diverged": False}
        if want_pred:
            P = y.shape[0] if plot_points <= 0 else min(int(plot_points), y.shape[0])
            idx = (np.arange(P, dtype=np.int64) * max(y.shape[0] - 1, 0)) // max(P - 1, 1)
            res["pred"], res["real"] = pred[idx].astype(np.float32), y[idx].astype(np.float32)
        if n_glob == 0:
            return res
        r = run_minibatch_sgd_logistic(X, y, self.w, c.step_size, c.num_iterations, c.fraction, c.tol,
                                       allreduce=red, row_offset=row_offset)
        self.w = r.weights
        res.update(iterations=r.iterations, converged=r.converged, loss_history=r.loss_history)
        return res

    def predict_batch(self, raw: RawBatch, apply_filter: bool = False, now_ms: Optional[int] = None,
                      output: str = "class") -> Dict[str, object]:
        """Score a raw batch without training on it: the class (margin >
        logit(threshold)), the probability or the margin of every row, or of
        the rows the filter keeps."""
        import time
        t0 = time.perf_counter()
        c = self.cfg
        X, _, rows = featurize_columnar(raw, c.num_text_features, c.begin, c.end, now_ms=now_ms, hash=c.hash,
                                        apply_filter=apply_filter)
        m = np.asarray(X @ self.w, dtype=np.float64).reshape(-1) if rows.shape[0] else np.zeros(0)
        return {"n_raw": raw.n, "n_scored": int(rows.shape[0]), "rows": rows.astype(np.int64),
                "pred": _link(m, output, c.threshold), "score_ms": (time.perf_counter() - t0) * 1e3}

    def evaluate_batch(self, raw: RawBatch, apply_filter: bool = False,
                       now_ms: Optional[int] = None) -> Dict[str, object]:
        """Held-out evaluation (the contract of
        ``DeviceLogisticRegression.evaluate_batch``): the binary accumulator of
        ``models/metrics.py`` from this engine's own ``predict_batch`` margins
        and the labels ``retweetCount >= label_threshold``."""
        import time
        from ..records.batch import RETWEET_COUNT
        from .metrics import binary_accumulator
        t0 = time.perf_counter()
        c = self.cfg
        res = self.predict_batch(raw, apply_filter=apply_filter, now_ms=now_ms, output="margin")
        out = binary_accumulator(res["pred"], raw.scalars[RETWEET_COUNT][res["rows"]], c.label_threshold, c.threshold)
        ms = (time.perf_counter() - t0) * 1e3
        out.update(n_raw=raw.n, n_scored=int(res["n_scored"]), eval_ms=ms, wall_ms=ms)
        return out

    def top_batch(self, raw: RawBatch, n: int, largest: bool = True, apply_filter: bool = False,
                  now_ms: Optional[int] = None) -> Dict[str, object]:
        """The n best rows of a raw batch by margin (the contract of
        ``DeviceLogisticRegression.top_batch``): ``models/topn.top_n`` of this
        engine's own ``predict_batch(output="margin")``.  ``values`` are
        margins; ``link`` maps them to probabilities."""
        import time
        from .topn import check_n, top_result
        check_n(n)
        t0 = time.perf_counter()
        res = self.predict_batch(raw, apply_filter=apply_filter, now_ms=now_ms, output="margin")
        out = top_result(res["pred"], res["rows"], n, largest)
        ms = (time.perf_counter() - t0) * 1e3
        out.update(n_raw=raw.n, n_scored=int(res["n_scored"]), top_ms=ms, wall_ms=ms)
        return out

    def synchronize(self) -> None:
        pass


# ---------------------------------------------------------------------------
class StreamingLogisticRegressionWithSGD(StreamingLinearRegressionWithSGD):
    """``StreamingLogisticRegressionWithSGD`` (MLlib 1.6 builder API)."""

    def __init__(self, stepSize: float = 0.1, numIterations: int = 50, miniBatchFraction: float = 1.0,
                 regParam: float = 0.0, engine=None):
        super().__init__(stepSize, numIterations, miniBatchFraction, engine)
        self.threshold: Optional[float] = 0.5
        self.setRegParam(regParam)

    def setRegParam(self, v: float) -> "StreamingLogisticRegressionWithSGD":
        if float(v) != 0.0:
            raise ValueError("regParam != 0 is not supported: L2 shrinkage moves every weight each iteration, "
                             "outside the batch's active features")
        self.regParam = 0.0
        return self

    def setInitialWeights(self, w) -> "StreamingLogisticRegressionWithSGD":
        self.model = LogisticRegressionModel(w, 0.0, self.threshold)
        if self.engine is not None:
            self.engine.set_weights(self.model.weights)
        return self

    def latestModel(self) -> LogisticRegressionModel:
        if self.model is None:
            raise ValueError("Model must be initialized before starting training.")
        if self.engine is not None:
            self.model = LogisticRegressionModel(self.engine.get_weights(), 0.0, self.model.threshold)
        return self.model

    def train_rdd(self, rdd) -> None:
        """One ``algorithm.run(rdd, model.weights)`` on a LabeledPoint RDD."""
        if self.model is None:
            raise ValueError("Model must be initialized before starting training.")
        pts = rdd.collect()
        if not pts:
            return
        n = self.model.numFeatures
        X = sp.lil_matrix((len(pts), n))
        y = np.empty(len(pts))
        for i, lp in enumerate(pts):
            a = lp.features.toArray()
            nz = np.nonzero(a)[0]
            X[i, nz] = a[nz]
            y[i] = lp.label
        r = run_minibatch_sgd_logistic(X.tocsr(), y, self.model.weights, self.stepSize, self.numIterations,
                                       self.miniBatchFraction, self.convergenceTol, allreduce=self.allreduce)
        self.model = LogisticRegressionModel(r.weights, 0.0, self.model.threshold)
        log.info("Model updated")

    def predictOn(self, stream):
        """Class predictions (or probabilities after ``clearThreshold``) of
        every record.  A raw tweet stream with an engine attached is one
        ``predict_batch(raw)`` per batch, unfiltered, in record order."""
        from ..runtime.rdd import RDD
        from .vectors import LabeledPoint

        def per_record(lp):
            return self.latestModel().predict(lp.features if isinstance(lp, LabeledPoint) else lp)

        def op(rdd):
            raw = getattr(rdd, "raw", None)
            eng = self.engine
            if eng is not None and isinstance(raw, RawBatch) and hasattr(eng, "predict_batch"):
                out = "class" if self.model is None or self.model.threshold is not None else "probability"
                return RDD(lambda: eng.predict_batch(raw, apply_filter=False, output=out)["pred"].tolist(),
                           raw, rdd.num_slices)
            return rdd.map(per_record)
        return stream.transform(op)

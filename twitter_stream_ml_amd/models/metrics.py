"""Held-out evaluation of the linear / logistic models: the accumulator
contract, and MLlib's ``BinaryClassificationMetrics`` / ``RegressionMetrics``
computed from it.

An engine's ``evaluate_batch(raw)`` reduces the (margin, label) pairs of a
batch -- the margin is ``predict_batch(output="margin")``'s, the label comes
from ``retweetCount`` -- into a small accumulator.  This module is the single
definition of that accumulator: the CPU engines form it with
:func:`binary_accumulator` / :func:`regression_accumulator`, the device forms
it in ``csrc/hip/eval.hip``, and both must agree to the bit in every integer.

**Margin bins.**  A margin is binned by its bit pattern: sign, exponent and
the top 6 mantissa bits, i.e. 64 bins per octave from 2^-20 to 2^12 on either
side of zero (:data:`EVAL_BINS` = 4097 bins, relative resolution 1/64 at every
scale, so a young model whose margins are all ~1e-3 is resolved as well as a
mature one).  The index is non-decreasing in the margin.  NaN margins are not
binned: they are counted in ``n_nan`` and enter nothing else.

**Binary accumulator** (logistic engines): ``n``, ``n_nan``, ``hist[2][4097]``
(label, bin), ``confusion = [tn, fp, fn, tp]`` under ``margin >
logit(threshold)``, all int64, and the fp64 ``logloss_sum``.  The row loss is
``max(-m, 0) + log1p(exp(-|m|))`` for label 1 and ``max(m, 0) +
log1p(exp(-|m|))`` for label 0; ``log1p(exp(-a))`` is evaluated by
:func:`log1p_exp_neg`, a fixed sequence of IEEE additions, multiplications
and one division, so that the host and the device form the same bits of every
row's loss (a libm call would differ by an ulp between the two).

**Regression accumulator** (squared-loss engines): ``n``, ``n_nan`` and the
fp64 sums of ``y, y^2, p, p^2, (y - p)^2, |y - p|`` with ``y =
float(retweetCount)`` and ``p`` the unrounded margin.

Integer words add exactly across batches and ranks (:meth:`EvalAccumulator.merge`);
the fp64 sums are added in call order.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

__all__ = ["EVAL_BINS", "ZERO_BIN", "REGRESSION_SUMS", "margin_bin", "bin_lower_edge", "log1p_exp_neg",
           "row_logloss", "binary_accumulator", "regression_accumulator", "empty_result", "EvalAccumulator",
           "BinaryClassificationMetrics", "RegressionMetrics", "metrics_of"]

EVAL_BINS = 4097            # kEvalBins (csrc/hip/kernels.h)
ZERO_BIN = 2048             # |m| < 2^-20
_MIN_EXP, _MAX_EXP = -20, 12
REGRESSION_SUMS = ("sum_y", "sum_y2", "sum_p", "sum_p2", "sum_e2", "sum_abs_e")


def margin_bin(m) -> np.ndarray:
    """Bin index (0 .. 4096) of fp64 margins, from their bit patterns; -1 for NaN."""
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    u = a.reshape(-1).view(np.uint64)
    E = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    f = ((u >> np.uint64(46)) & np.uint64(0x3F)).astype(np.int64)
    e = E - 1023
    mag = np.where(e < _MIN_EXP, 0, np.where(e >= _MAX_EXP, 2048, (e - _MIN_EXP) * 64 + f + 1))
    neg = (u >> np.uint64(63)) != 0
    out = np.where(neg, ZERO_BIN - mag, ZERO_BIN + mag)
    nan = (E == 0x7FF) & ((u & np.uint64((1 << 52) - 1)) != 0)
    return np.where(nan, -1, out).reshape(a.shape)


def _mag_lo(mag: int) -> float:
    """Smallest |m| of magnitude class ``mag`` (1 .. 2048), exactly."""
    q = mag - 1
    return math.ldexp(1.0 + (q % 64) / 64.0, q // 64 + _MIN_EXP)


def bin_lower_edge(b: int) -> float:
    """Lower edge of bin ``b``, decoded exactly from the index: a bin above
    the zero bin holds ``edge <= m``, the zero bin and the bins below it hold
    ``edge < m`` (bin 0 reaches down to -inf)."""
    b = int(b)
    if not 0 <= b < EVAL_BINS:
        raise ValueError(f"bin {b} out of range")
    if b > ZERO_BIN:
        return _mag_lo(b - ZERO_BIN)
    mag = ZERO_BIN - b + 1            # the class below this bin's
    return -math.inf if mag > 2048 else -_mag_lo(mag)


# ---- log1p(exp(-a)) in IEEE basic operations --------------------------------
_LOG2E = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = float.fromhex("0x1.62e42fee00000p-1")    # 32 significant bits: k * LN2_HI is exact for k < 2^21
_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
_EXP_TERMS = 14            # exp(r), |r| <= ln(2) / 2: r^15 / 15! < 2^-62
_ATANH_LAST = 37           # 2 atanh(s), s <= 1 / 3: s^38 / 39 < 2^-65
_EXP_CUT = 700.0           # exp(-a) < 2^-1009 beyond: the term is taken as 0


def log1p_exp_neg(a) -> np.ndarray:
    """``log1p(exp(-a))`` for ``a >= 0`` as a fixed sequence of correctly
    rounded fp64 operations (no fused multiply-add, no libm), identical to
    ``eval_log1p_exp_neg`` in ``csrc/hip/eval.hip``.  About 20 roundings of
    relative size 2^-53 enter the result, each with weight <= 1: within
    2e-15 of the real value, relatively.  0 for ``a > 700``.

    ``exp(-a) = 2^-k exp(r)`` with ``k = floor(a log2(e) + 1/2)`` and ``r = k
    ln(2) - a`` (Cody-Waite, ln(2) in two parts), ``exp(r)`` by its nested
    Taylor polynomial; ``log1p(t) = 2 atanh(t / (2 + t))`` by the nested odd
    series in ``s^2``."""
    a = np.asarray(a, dtype=np.float64)
    big = a > _EXP_CUT
    ac = np.where(big, _EXP_CUT, a)
    k = np.floor(ac * _LOG2E + 0.5)
    r = (k * _LN2_HI - ac) + k * _LN2_LO
    p = 1.0 + r * (1.0 / _EXP_TERMS)
    for j in range(_EXP_TERMS - 1, 1, -1):
        p = 1.0 + (r * (1.0 / j)) * p
    p = 1.0 + r * p
    t = np.ldexp(p, -k.astype(np.int64))      # exact: p in [0.7, 1.42], k <= 1010
    s = t / (2.0 + t)
    s2 = s * s
    q = np.full_like(s2, 1.0 / _ATANH_LAST)
    for d in range(_ATANH_LAST - 2, 1, -2):
        q = 1.0 / d + s2 * q
    q = 1.0 + s2 * q
    return np.where(big, 0.0, 2.0 * (s * q))


def row_logloss(m, label) -> np.ndarray:
    """Per-row logistic loss of margins ``m`` (no NaN) under 0/1 ``label``."""
    m = np.asarray(m, dtype=np.float64)
    pos = np.asarray(label) != 0
    return np.maximum(np.where(pos, -m, m), 0.0) + log1p_exp_neg(np.abs(m))


def _logit(p: float) -> float:
    return math.log(p / (1.0 - p))


def binary_accumulator(margins, retweets, label_threshold: int, threshold: float = 0.5) -> Dict[str, object]:
    """The binary accumulator of (margin, retweetCount) pairs, in numpy."""
    m = np.asarray(margins, dtype=np.float64).reshape(-1)
    lab = (np.asarray(retweets).reshape(-1) >= int(label_threshold))
    nan = np.isnan(m)
    ok = ~nan
    mv, lv = m[ok], lab[ok]
    hist = np.zeros((2, EVAL_BINS), np.int64)
    np.add.at(hist, (lv.astype(np.int64), margin_bin(mv).astype(np.int64)), 1)
    pos = mv > _logit(float(threshold))
    confusion = [int(np.count_nonzero(~lv & ~pos)), int(np.count_nonzero(~lv & pos)),
                 int(np.count_nonzero(lv & ~pos)), int(np.count_nonzero(lv & pos))]
    loss = 0.0
    for t in row_logloss(mv, lv).tolist():    # in row order
        loss += t
    return {"kind": "binary", "n": int(mv.shape[0]), "n_nan": int(np.count_nonzero(nan)), "hist": hist,
            "confusion": confusion, "logloss_sum": float(loss), "label_threshold": int(label_threshold),
            "threshold": float(threshold)}


def regression_terms(margins, retweets) -> np.ndarray:
    """The six per-row terms [6][n] of the regression sums (no NaN margins)."""
    p = np.asarray(margins, dtype=np.float64).reshape(-1)
    y = np.asarray(retweets).reshape(-1).astype(np.float64)
    e = y - p
    return np.stack([y, y * y, p, p * p, e * e, np.abs(e)])


def regression_accumulator(margins, retweets) -> Dict[str, object]:
    """The regression accumulator of (margin, retweetCount) pairs, in numpy."""
    p = np.asarray(margins, dtype=np.float64).reshape(-1)
    nan = np.isnan(p)
    terms = regression_terms(p[~nan], np.asarray(retweets).reshape(-1)[~nan])
    out: Dict[str, object] = {"kind": "regression", "n": int(terms.shape[1]), "n_nan": int(np.count_nonzero(nan)),
                              "label_threshold": -1, "threshold": 0.5}
    for name, col in zip(REGRESSION_SUMS, terms):
        s = 0.0
        for t in col.tolist():
            s += t
        out[name] = float(s)
    return out


def empty_result(kind: str, label_threshold: int = -1, threshold: float = 0.5) -> Dict[str, object]:
    """Zeroed accumulator words of an engine's ``evaluate_batch``."""
    out: Dict[str, object] = {"kind": kind, "n": 0, "n_nan": 0, "label_threshold": int(label_threshold),
                              "threshold": float(threshold)}
    if kind == "binary":
        out.update(hist=np.zeros((2, EVAL_BINS), np.int64), confusion=[0, 0, 0, 0], logloss_sum=0.0)
    elif kind == "regression":
        out.update({k: 0.0 for k in REGRESSION_SUMS})
    else:
        raise ValueError(f"unknown accumulator kind {kind!r}")
    return out


class EvalAccumulator:
    """Sum of ``evaluate_batch`` results: integer words exactly, fp64 sums in
    call order."""

    def __init__(self, kind: str, label_threshold: int = -1, threshold: float = 0.5):
        z = empty_result(kind, label_threshold, threshold)
        self.kind = kind
        self.label_threshold = int(label_threshold)
        self.threshold = float(threshold)
        self.n = 0
        self.n_nan = 0
        self.batches = 0
        self.hist: Optional[np.ndarray] = z.get("hist")
        self.confusion: List[int] = [0, 0, 0, 0]
        self.logloss_sum = 0.0
        self.sums: Dict[str, float] = {k: 0.0 for k in REGRESSION_SUMS}

    @classmethod
    def like(cls, result: Dict[str, object]) -> "EvalAccumulator":
        return cls(str(result["kind"]), int(result["label_threshold"]), float(result["threshold"]))

    def _check(self, kind, label_threshold, threshold) -> None:
        if (kind, int(label_threshold), float(threshold)) != (self.kind, self.label_threshold, self.threshold):
            raise ValueError(f"accumulators differ: {kind} / {label_threshold} / {threshold} against "
                             f"{self.kind} / {self.label_threshold} / {self.threshold}")

    def add(self, result: Dict[str, object]) -> "EvalAccumulator":
        self._check(result["kind"], result["label_threshold"], result["threshold"])
        self.n += int(result["n"])
        self.n_nan += int(result["n_nan"])
        self.batches += 1
        if self.kind == "binary":
            self.hist = self.hist + np.asarray(result["hist"], np.int64).reshape(2, EVAL_BINS)
            self.confusion = [a + int(b) for a, b in zip(self.confusion, result["confusion"])]
            self.logloss_sum += float(result["logloss_sum"])
        else:
            for k in REGRESSION_SUMS:
                self.sums[k] += float(result[k])
        return self

    def merge(self, other: "EvalAccumulator") -> "EvalAccumulator":
        self._check(other.kind, other.label_threshold, other.threshold)
        b = self.batches + other.batches
        self.add(other.result())
        self.batches = b
        return self

    def result(self) -> Dict[str, object]:
        """The accumulator in the layout of an ``evaluate_batch`` result."""
        out: Dict[str, object] = {"kind": self.kind, "n": self.n, "n_nan": self.n_nan,
                                  "label_threshold": self.label_threshold, "threshold": self.threshold}
        if self.kind == "binary":
            out.update(hist=self.hist.copy(), confusion=list(self.confusion), logloss_sum=self.logloss_sum)
        else:
            out.update(self.sums)
        return out

    def to_dict(self) -> Dict[str, object]:
        """JSON form; the histogram as ``[label, bin, count]`` of its non-zero bins."""
        out = self.result()
        out["batches"] = self.batches
        if self.kind == "binary":
            lab, bins = np.nonzero(self.hist)
            out["hist"] = [[int(a), int(b), int(self.hist[a, b])] for a, b in zip(lab, bins)]
        return out

    @classmethod
    def from_dict(cls, d: Dict[str, object]) -> "EvalAccumulator":
        acc = cls(str(d["kind"]), int(d["label_threshold"]), float(d["threshold"]))
        acc.n, acc.n_nan, acc.batches = int(d["n"]), int(d["n_nan"]), int(d.get("batches", 1))
        if acc.kind == "binary":
            for a, b, c in d["hist"]:
                acc.hist[int(a), int(b)] += int(c)
            acc.confusion = [int(v) for v in d["confusion"]]
            acc.logloss_sum = float(d["logloss_sum"])
        else:
            acc.sums = {k: float(d[k]) for k in REGRESSION_SUMS}
        return acc

    def __eq__(self, other) -> bool:
        if not isinstance(other, EvalAccumulator):
            return NotImplemented
        a, b = self.to_dict(), other.to_dict()
        return a == b

    def metrics(self):
        return metrics_of(self)


def _ratio(a: float, b: float) -> Optional[float]:
    return a / b if b else None


class BinaryClassificationMetrics:
    """MLlib's ``BinaryClassificationMetrics`` over the margin bins (one
    threshold per non-empty bin, descending), plus the fixed-threshold
    confusion counts and the log-loss."""

    def __init__(self, hist: np.ndarray, confusion, logloss_sum: float, n: int, n_nan: int = 0):
        self.hist = np.asarray(hist, np.int64).reshape(2, EVAL_BINS)
        self.confusion = [int(v) for v in confusion]
        self.n, self.n_nan = int(n), int(n_nan)
        self.logloss_sum = float(logloss_sum)
        self.numNegatives = int(self.hist[0].sum())
        self.numPositives = int(self.hist[1].sum())
        # non-empty bins from the highest down, with cumulative counts
        tot = self.hist[0] + self.hist[1]
        self._bins = [int(b) for b in np.nonzero(tot)[0][::-1]]
        self._tp: List[int] = []
        self._fp: List[int] = []
        tp = fp = 0
        for b in self._bins:
            tp += int(self.hist[1, b])
            fp += int(self.hist[0, b])
            self._tp.append(tp)
            self._fp.append(fp)

    @classmethod
    def from_accumulator(cls, acc) -> "BinaryClassificationMetrics":
        r = acc.result() if isinstance(acc, EvalAccumulator) else acc
        if r["kind"] != "binary":
            raise ValueError("not a binary accumulator")
        return cls(r["hist"], r["confusion"], r["logloss_sum"], r["n"], r["n_nan"])

    # ---- curves -------------------------------------------------------------
    def thresholds(self) -> List[Tuple[float, float]]:
        """(margin edge, probability) of every non-empty bin, descending."""
        out = []
        for b in self._bins:
            e = bin_lower_edge(b)
            out.append((e, 1.0 / (1.0 + math.exp(-e)) if e >= 0 else math.exp(e) / (1.0 + math.exp(e))))
        return out

    def _both(self) -> bool:
        return self.numPositives > 0 and self.numNegatives > 0

    def roc(self) -> List[Tuple[float, float]]:
        """(false positive rate, true positive rate), (0, 0) first and (1, 1) last."""
        P, N = self.numPositives, self.numNegatives
        pts = [(0.0, 0.0)]
        pts += [(fp / N if N else 0.0, tp / P if P else 0.0) for tp, fp in zip(self._tp, self._fp)]
        return pts + [(1.0, 1.0)]

    def pr(self) -> List[Tuple[float, float]]:
        """(recall, precision), (0, 1.0) first (MLlib 1.6)."""
        P = self.numPositives
        return [(0.0, 1.0)] + [(tp / P if P else 0.0, tp / (tp + fp)) for tp, fp in zip(self._tp, self._fp)]

    @property
    def areaUnderROC(self) -> Optional[float]:
        """Trapezoid rule over :meth:`roc`, summed in integers (2 P N times
        the area) and divided once."""
        if not self._both():
            return None
        area2, tp0, fp0 = 0, 0, 0
        for tp, fp in zip(self._tp, self._fp):
            area2 += (fp - fp0) * (tp + tp0)
            tp0, fp0 = tp, fp
        return area2 / (2 * self.numPositives * self.numNegatives)

    @property
    def areaUnderPR(self) -> Optional[float]:
        if not self._both():
            return None
        pts = self.pr()
        return float(sum((x1 - x0) * (y1 + y0) / 2.0 for (x0, y0), (x1, y1) in zip(pts, pts[1:])))

    @property
    def auc_tie_bound(self) -> Optional[float]:
        """``sum_b P_b N_b / (2 P N)``: pairs of a positive and a negative in
        one bin are all that tells this AUC from the exact one, which lies
        within ``areaUnderROC +- auc_tie_bound``."""
        if not self._both():
            return None
        ties = sum(int(self.hist[0, b]) * int(self.hist[1, b]) for b in self._bins)
        return ties / (2 * self.numPositives * self.numNegatives)

    # ---- at the model's threshold ----------------------------------------------
    @property
    def accuracy(self) -> Optional[float]:
        tn, fp, fn, tp = self.confusion
        return _ratio(tn + tp, tn + fp + fn + tp)

    @property
    def precision(self) -> Optional[float]:
        tn, fp, fn, tp = self.confusion
        return _ratio(tp, tp + fp)

    @property
    def recall(self) -> Optional[float]:
        tn, fp, fn, tp = self.confusion
        return _ratio(tp, tp + fn)

    @property
    def f1(self) -> Optional[float]:
        tn, fp, fn, tp = self.confusion
        return _ratio(2 * tp, 2 * tp + fp + fn)

    @property
    def logLoss(self) -> Optional[float]:
        return _ratio(self.logloss_sum, self.n)

    def to_dict(self) -> Dict[str, object]:
        return {"kind": "binary", "n": self.n, "n_nan": self.n_nan, "numPositives": self.numPositives,
                "numNegatives": self.numNegatives, "areaUnderROC": self.areaUnderROC,
                "auc_tie_bound": self.auc_tie_bound, "areaUnderPR": self.areaUnderPR, "accuracy": self.accuracy,
                "precision": self.precision, "recall": self.recall, "f1": self.f1, "logLoss": self.logLoss,
                "confusion": list(self.confusion)}


class RegressionMetrics:
    """MLlib's ``RegressionMetrics`` from the six sums."""

    def __init__(self, n: int, sums: Dict[str, float], n_nan: int = 0):
        self.n, self.n_nan = int(n), int(n_nan)
        self.sums = {k: float(sums[k]) for k in REGRESSION_SUMS}

    @classmethod
    def from_accumulator(cls, acc) -> "RegressionMetrics":
        r = acc.result() if isinstance(acc, EvalAccumulator) else acc
        if r["kind"] != "regression":
            raise ValueError("not a regression accumulator")
        return cls(r["n"], r, r["n_nan"])

    @property
    def meanSquaredError(self) -> Optional[float]:
        return _ratio(self.sums["sum_e2"], self.n)

    @property
    def rootMeanSquaredError(self) -> Optional[float]:
        m = self.meanSquaredError
        return None if m is None else math.sqrt(m)

    @property
    def meanAbsoluteError(self) -> Optional[float]:
        return _ratio(self.sums["sum_abs_e"], self.n)

    def _ss_tot(self) -> float:
        """sum (y - mean y)^2"""
        return self.sums["sum_y2"] - self.sums["sum_y"] * self.sums["sum_y"] / self.n

    @property
    def r2(self) -> Optional[float]:
        """``1 - SSerr / SStot``"""
        if not self.n:
            return None
        tot = self._ss_tot()
        return 1.0 - self.sums["sum_e2"] / tot if tot else None

    @property
    def explainedVariance(self) -> Optional[float]:
        """``sum (p - mean y)^2 / n`` (MLlib's ``SSreg / n``)."""
        if not self.n:
            return None
        s, n = self.sums, self.n
        my = s["sum_y"] / n
        return (s["sum_p2"] - 2.0 * my * s["sum_p"] + n * my * my) / n

    def to_dict(self) -> Dict[str, object]:
        return {"kind": "regression", "n": self.n, "n_nan": self.n_nan, "meanSquaredError": self.meanSquaredError,
                "rootMeanSquaredError": self.rootMeanSquaredError, "meanAbsoluteError": self.meanAbsoluteError,
                "r2": self.r2, "explainedVariance": self.explainedVariance}


def metrics_of(acc):
    """The metrics class that fits an accumulator (or an ``evaluate_batch`` result)."""
    kind = acc.kind if isinstance(acc, EvalAccumulator) else acc["kind"]
    return (BinaryClassificationMetrics if kind == "binary" else RegressionMetrics).from_accumulator(acc)

"""The silhouette of a k-means model on a batch: one contract for the CPU engine
and the device (MLlib's ``ClusteringEvaluator``, squared Euclidean distance).

Everything is in the model's scaled space, the space ``predict_batch`` reports
``dist2`` in.  For one batch with the model's labels ``A(p)`` (``predict_batch``'s
``pred``), per cluster G:

* ``N_G`` the rows labelled G, ``mu_G`` their mean, ``dev2_p = |x_p - mu_A(p)|^2``,
  ``W_G = sum_{p in G} dev2_p``, ``V_G = W_G / N_G``.
* The mean squared distance from x to all rows of G is ``D(x, G) = |x - mu_G|^2
  + V_G`` -- algebraically MLlib's ``xi_x + Psi_G / N_G - 2 x.Y_G / N_G``, but
  every term is non-negative and nothing cancels.

Per row:

* ``a_p = (N_A dev2_p + W_A) / (N_A - 1)``, the mean squared distance to the
  other rows of its own cluster;
* ``b_p = min over G != A(p), N_G > 0 of D(x_p, G)``; ``neighbor_p`` that G, the
  lowest index on an exact fp64 tie;
* ``s_p = 1 - a / b`` if ``a < b``, ``b / a - 1`` if ``a > b``, else 0 (MLlib's
  ``pointSilhouetteCoefficient``);
* ``N_A == 1``: ``s_p = 0`` and ``a_p = 0``, as in MLlib.

A batch with fewer than two non-empty clusters is undefined (MLlib asserts): its
rows are counted in ``n_undefined`` and nothing else is added.

:class:`SilhouetteAccumulator` holds integers only -- per own cluster the rows
``n`` and ``s_fix = sum rint(s_p 2^36)`` -- so batches and ranks merge exactly in
any order.  The stream's figure, ``sum s_fix / 2^36 / sum n``, is therefore the
row-weighted mean of its batches' silhouettes: every batch is measured against
its own cluster means.  A silhouette over the whole stream would need two
passes over it and is not computed here.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

__all__ = ["S_FIX_BITS", "S_FIX_ONE", "point_silhouette", "cluster_stats", "batch_silhouette",
           "SilhouetteAccumulator", "empty_silhouette"]

S_FIX_BITS = 36
S_FIX_ONE = 1 << S_FIX_BITS


def point_silhouette(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """MLlib's three branches, each a single IEEE division and subtraction."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    s = np.zeros(np.broadcast(a, b).shape, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lt, gt = a < b, a > b
        np.putmask(s, lt, 1.0 - a / b)
        np.putmask(s, gt, b / a - 1.0)
    return s


def s_fixed(s: np.ndarray) -> np.ndarray:
    """``rint(s 2^36)`` as int64 (|s| <= 1: exact in fp64)."""
    return np.rint(np.asarray(s, np.float64) * float(S_FIX_ONE)).astype(np.int64)


def cluster_stats(Xs: np.ndarray, pred: np.ndarray, k: int) -> Dict[str, np.ndarray]:
    """``N``, ``mu`` (zero rows for empty clusters), ``dev2`` per row, ``W`` and
    ``V`` (0 for empty clusters) of a labelled batch."""
    Xs = np.asarray(Xs, np.float64)
    pred = np.asarray(pred, np.int64)
    n, d = Xs.shape
    N = np.bincount(pred, minlength=k).astype(np.int64)
    mu = np.zeros((k, d))
    np.add.at(mu, pred, Xs)
    nz = N > 0
    mu[nz] /= N[nz, None]
    dev2 = ((Xs - mu[pred]) ** 2).sum(axis=1) if n else np.zeros(0)
    W = np.bincount(pred, weights=dev2, minlength=k).astype(np.float64)
    V = np.zeros(k)
    V[nz] = W[nz] / N[nz]
    return {"N": N, "mu": mu, "dev2": dev2, "W": W, "V": V}


def mean_dist2(Xs: np.ndarray, mu: np.ndarray, V: np.ndarray, N: np.ndarray, chunk_elems: int = 1 << 22) -> np.ndarray:
    """``D(x_p, G)`` for every row and cluster, ``+inf`` for empty clusters."""
    n, d = Xs.shape
    k = mu.shape[0]
    D = np.empty((n, k))
    step = max(1, chunk_elems // max(1, k * d))
    for s in range(0, n, step):
        D[s:s + step] = ((Xs[s:s + step, None, :] - mu[None]) ** 2).sum(axis=2) + V[None]
    D[:, N == 0] = np.inf
    return D


def batch_silhouette(Xs: np.ndarray, pred: np.ndarray, k: int) -> Dict[str, object]:
    """The definitions of the module docstring applied to the scaled rows
    ``Xs`` with labels ``pred``: ``defined``, ``N``, ``a``, ``b``, ``s`` (fp64),
    ``neighbor`` (int32, -1 where undefined) and the cluster statistics."""
    Xs = np.asarray(Xs, np.float64)
    pred = np.asarray(pred, np.int64)
    n = Xs.shape[0]
    st = cluster_stats(Xs, pred, k)
    N = st["N"]
    out = dict(st)
    out["defined"] = bool(np.count_nonzero(N) >= 2)
    out["a"] = np.zeros(n)
    out["b"] = np.zeros(n)
    out["s"] = np.zeros(n)
    out["neighbor"] = np.full(n, -1, np.int32)
    if not out["defined"]:
        return out
    D = mean_dist2(Xs, st["mu"], st["V"], N)
    D[np.arange(n), pred] = np.inf
    nb = np.argmin(D, axis=1)             # the first (lowest) index on exact ties
    b = D[np.arange(n), nb]
    Na = N[pred]
    single = Na == 1
    a = np.zeros(n)
    m = ~single
    a[m] = (Na[m] * st["dev2"][m] + st["W"][pred[m]]) / (Na[m] - 1)
    s = point_silhouette(a, b)
    s[single] = 0.0
    out.update(a=a, b=b, s=s, neighbor=nb.astype(np.int32))
    return out


class SilhouetteAccumulator:
    """Integer sums of a stream's per-row silhouettes, per own cluster.

    ``n[G]`` the rows with a defined ``s`` (singletons included), ``s_fix[G] =
    sum rint(s_p 2^36)``, ``n_single``, ``n_undefined``, ``batches``.  All
    Python integers: a long stream outgrows int64 at this scale, and JSON
    carries them exactly."""

    def __init__(self, k: int):
        self.k = int(k)
        self.n: List[int] = [0] * self.k
        self.s_fix: List[int] = [0] * self.k
        self.n_single = 0
        self.n_undefined = 0
        self.batches = 0

    # ---- building ----------------------------------------------------------
    def add_rows(self, pred, s, n_single: Optional[int] = None, sizes=None) -> "SilhouetteAccumulator":
        """One defined batch from its per-row labels and silhouettes."""
        pred = np.asarray(pred, np.int64)
        fix = s_fixed(s)
        cnt = np.bincount(pred, minlength=self.k)
        if n_single is None:
            n_single = int(np.count_nonzero(cnt == 1))
        for g in np.nonzero(cnt)[0]:
            self.n[g] += int(cnt[g])
            self.s_fix[g] += int(fix[pred == g].sum(dtype=np.int64))
        self.n_single += int(n_single)
        self.batches += 1
        return self

    def add_undefined(self, n: int) -> "SilhouetteAccumulator":
        self.n_undefined += int(n)
        self.batches += 1
        return self

    def add_words(self, n, s_fix, n_single: int, n_undefined: int) -> "SilhouetteAccumulator":
        """One batch from the device's result words."""
        for g in range(self.k):
            self.n[g] += int(n[g])
            self.s_fix[g] += int(s_fix[g])
        self.n_single += int(n_single)
        self.n_undefined += int(n_undefined)
        self.batches += 1
        return self

    def merge(self, other: "SilhouetteAccumulator") -> "SilhouetteAccumulator":
        if other.k != self.k:
            raise ValueError(f"accumulators of {self.k} and {other.k} clusters do not merge")
        self.n = [x + y for x, y in zip(self.n, other.n)]
        self.s_fix = [x + y for x, y in zip(self.s_fix, other.s_fix)]
        self.n_single += other.n_single
        self.n_undefined += other.n_undefined
        self.batches += other.batches
        return self

    # ---- reading -----------------------------------------------------------
    @property
    def n_total(self) -> int:
        return sum(self.n)

    @property
    def silhouette(self) -> Optional[float]:
        nt = self.n_total
        if nt == 0:
            return None
        return float((_frac(sum(self.s_fix), nt)))

    @property
    def cluster_silhouette(self) -> List[Optional[float]]:
        return [None if c == 0 else float(_frac(f, c)) for f, c in zip(self.s_fix, self.n)]

    def to_dict(self) -> Dict[str, object]:
        return {"k": self.k, "n": list(self.n), "s_fix": list(self.s_fix), "n_single": self.n_single,
                "n_undefined": self.n_undefined, "batches": self.batches}

    @classmethod
    def from_dict(cls, d: Dict[str, object]) -> "SilhouetteAccumulator":
        acc = cls(int(d["k"]))
        acc.n = [int(x) for x in d["n"]]
        acc.s_fix = [int(x) for x in d["s_fix"]]
        if len(acc.n) != acc.k or len(acc.s_fix) != acc.k:
            raise ValueError("accumulator arrays do not have k entries")
        acc.n_single = int(d["n_single"])
        acc.n_undefined = int(d["n_undefined"])
        acc.batches = int(d["batches"])
        return acc

    def summary(self) -> Dict[str, object]:
        return {"silhouette": self.silhouette, "cluster_silhouette": self.cluster_silhouette,
                "accumulator": self.to_dict()}

    def __eq__(self, other) -> bool:
        return isinstance(other, SilhouetteAccumulator) and self.to_dict() == other.to_dict()


def _frac(fix: int, n: int):
    """``fix / 2^36 / n`` of Python integers, correctly rounded to fp64."""
    from fractions import Fraction
    return Fraction(fix, S_FIX_ONE * n)


def empty_silhouette(n_raw: int, k: int, std=None, per_row: bool = False) -> Dict[str, object]:
    """``silhouette_batch`` of a batch with nothing to score."""
    out = {"n_raw": int(n_raw), "n_scored": 0, "silhouette": None, "accumulator": SilhouetteAccumulator(k),
           "sizes": np.zeros(int(k), np.int64), "cost": 0.0, "std": None if std is None else std.copy(),
           "sil_ms": 0.0, "wall_ms": 0.0}
    if per_row:
        out.update(rows=np.zeros(0, np.int64), pred=np.zeros(0, np.int32), neighbor=np.zeros(0, np.int32),
                   a=np.zeros(0), b=np.zeros(0), s=np.zeros(0))
    return out

"""Per-cluster exemplars: the m rows nearest (or farthest from) each k-means
centre.  The one contract of the host and the device
(``csrc/hip/exemplars.hip``), the engines' ``exemplars_batch`` and the
stream-wide merge of ``twtml-score --exemplars``.  It extends ``models/topn.py``
from one group to k groups.

``cluster_top(values, labels, rows=None, k=..., m=1, largest=False)``

* ``values``: fp64, one per scored row, in scored order; ``labels``: int32 in
  ``[0, k)`` (anything else is a ``ValueError``); ``rows``: the raw row ids,
  ascending (``None``: row i is i).
* Within a cluster, best value first -- ascending by default (nearest the
  centre), descending with ``largest`` (the cluster's own outliers).  Values
  compare as IEEE numbers, so ``-0.0 == +0.0``; equal values by ascending raw
  row id.
* NaN values are never selected; they are counted as ``n_nan``, a batch total.
* The result is ``counts`` int64[k] = ``min(m, rows of c that are not NaN)``,
  ``rows`` int64[k, m] (``-1`` in unused entries), ``values`` fp64[k, m] (the
  selected values' original bits, ``+0.0`` in unused entries) and ``n_nan``.
* ``1 <= m <= EXEMPLARS_MAX`` and ``k * m <= EXEMPLARS_MAX_CELLS``; anything
  else is a ``ValueError`` (``predict_batch`` returns every row).

``ExemplarMerger(k, m, largest)`` keeps, per cluster, the best m entries over
all batches added so far, ordered by value, then batch sequence number, then
row (then, for the files of several ranks, whose ``seq`` and ``row`` repeat, by
the value's sign and the serialised ``extra``); merging two mergers equals
adding their batches to one, in any order.
"""
from __future__ import annotations

import json
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["EXEMPLARS_MAX", "EXEMPLARS_MAX_CELLS", "check_m", "cluster_top", "exemplars_result", "empty_exemplars",
           "ExemplarMerger"]

EXEMPLARS_MAX = 64
EXEMPLARS_MAX_CELLS = 1 << 18


def check_m(k, m) -> int:
    """m as an int, after the limits on m and on k * m."""
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= EXEMPLARS_MAX:
        raise ValueError(f"exemplars: m must be an integer in 1..{EXEMPLARS_MAX}, got {m!r}; "
                         f"predict_batch returns every row")
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError(f"exemplars: k must be a positive integer, got {k!r}")
    if int(k) * int(m) > EXEMPLARS_MAX_CELLS:
        raise ValueError(f"exemplars: k * m must be at most {EXEMPLARS_MAX_CELLS}, got {int(k)} * {int(m)}; "
                         f"predict_batch returns every row")
    return int(m)


def cluster_top(values, labels, rows=None, k: int = 1, m: int = 1,
                largest: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """``(counts[k], rows[k, m], values[k, m], n_nan)`` (module docstring).
    The values keep their bits (a selected ``-0.0`` stays one)."""
    m = check_m(k, m)
    k = int(k)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    if lab.size and lab.dtype.kind not in "iu":
        raise ValueError(f"exemplars: labels must be integers, got {lab.dtype}")
    lab = lab.astype(np.int64)
    r = np.arange(v.size, dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    if r.shape != v.shape or lab.shape != v.shape:
        raise ValueError(f"exemplars: {v.size} values, {lab.size} labels, {r.size} rows")
    if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= k):
        raise ValueError(f"exemplars: labels must lie in [0, {k})")
    ok = ~np.isnan(v)
    n_nan = int(v.size - np.count_nonzero(ok))
    v, lab, r = v[ok], lab[ok], r[ok]
    # lexsort: last key first; -0.0 and +0.0 compare equal, so they tie on the row
    o = np.lexsort((r, -v if largest else v, lab))
    v, lab, r = v[o], lab[o], r[o]
    size = np.bincount(lab, minlength=k).astype(np.int64)
    start = np.cumsum(size) - size
    rank = np.arange(v.size, dtype=np.int64) - start[lab]
    keep = rank < m
    counts = np.minimum(size, m)
    out_rows = np.full((k, m), -1, np.int64)
    out_vals = np.zeros((k, m), np.float64)
    out_rows[lab[keep], rank[keep]] = r[keep]
    out_vals[lab[keep], rank[keep]] = v[keep]
    return counts, out_rows, out_vals, n_nan


def empty_exemplars(k: int, m: int) -> Dict[str, object]:
    m = check_m(k, m)
    return {"counts": np.zeros(int(k), np.int64), "rows": np.full((int(k), m), -1, np.int64),
            "values": np.zeros((int(k), m), np.float64), "n_nan": 0}


def exemplars_result(values, labels, rows, k: int, m: int, largest: bool = False) -> Dict[str, object]:
    """``cluster_top`` as the dict the engines' ``exemplars_batch`` return:
    ``counts``, ``rows``, ``values``, ``n_nan``."""
    c, r, v, n_nan = cluster_top(values, labels, rows, k=k, m=m, largest=largest)
    return {"counts": c, "rows": r, "values": v, "n_nan": n_nan}


class ExemplarMerger:
    """Per cluster, the best m entries of a stream of per-batch selections.
    An entry is ``(value, seq, row, extra)``; the order is by value
    (``-0.0 == +0.0``), then ``seq``, then ``row``.  ``extra`` (a dict, or
    None) rides along."""

    def __init__(self, k: int, m: int, largest: bool = False):
        self.m = check_m(k, m)
        self.k = int(k)
        self.largest = bool(largest)
        self.clusters: Dict[int, List[Tuple[float, int, int, Optional[dict]]]] = {}
        self.n_nan = 0
        self.batches = 0

    def _key(self, e):
        v = e[0] + 0.0   # -0.0 + 0.0 == +0.0: one key for both zeros
        # Files of different ranks can hold the same (seq, row) with equal
        # values: the value's sign bit and the extra, serialised, settle those,
        # so the order never depends on the order of insertion (entries equal
        # in all of these are interchangeable).
        return (-v if self.largest else v, e[1], e[2], math.copysign(1.0, e[0]),
                json.dumps(e[3], sort_keys=True, default=str))

    def _trim(self, c: int) -> None:
        es = self.clusters[c]
        es.sort(key=self._key)
        del es[self.m:]

    def add(self, seq: int, counts, rows, values, extras=None, n_nan: int = 0) -> "ExemplarMerger":
        """One batch's selection: ``counts[k]``, ``rows[k, m']``,
        ``values[k, m']`` (only the first ``counts[c]`` entries of a cluster are
        read); ``extras``: ``{(label, row): dict}`` or None."""
        counts = np.asarray(counts).reshape(-1)
        if counts.size != self.k:
            raise ValueError(f"ExemplarMerger.add: {counts.size} counts for k = {self.k}")
        rows = np.asarray(rows).reshape(self.k, -1) if self.k else np.zeros((0, 0), np.int64)
        values = np.asarray(values, dtype=np.float64).reshape(self.k, -1)
        if rows.shape != values.shape or (counts.size and int(counts.max(initial=0)) > rows.shape[1]):
            raise ValueError("ExemplarMerger.add: counts, rows and values differ in shape")
        for c in np.flatnonzero(counts > 0):
            c = int(c)
            n = int(counts[c])
            vals = [float(x) for x in values[c, :n]]
            if any(x != x for x in vals):
                raise ValueError("ExemplarMerger.add: NaN values are never selected")
            es = self.clusters.setdefault(c, [])
            for v, r in zip(vals, rows[c, :n]):
                r = int(r)
                es.append((v, int(seq), r, None if extras is None else extras.get((c, r))))
            self._trim(c)
        self.n_nan += int(n_nan)
        self.batches += 1
        return self

    def add_clusters(self, seq: int, clusters: Sequence[dict], n_nan: int = 0,
                     value_key: str = "dist2") -> "ExemplarMerger":
        """One batch's selection as the ``clusters`` list of a line of the
        scoring driver's ``exemplars.jsonl``: ``{"label", "entries": [{"row",
        value_key, ...}]}``; an entry's other keys become its ``extra``."""
        m = max([len(c["entries"]) for c in clusters] + [1])
        counts = np.zeros(self.k, np.int64)
        rows = np.full((self.k, m), -1, np.int64)
        values = np.zeros((self.k, m), np.float64)
        extras = {}
        for c in clusters:
            lab = int(c["label"])
            counts[lab] = len(c["entries"])
            for j, e in enumerate(c["entries"]):
                rows[lab, j], values[lab, j] = int(e["row"]), float(e[value_key])
                extras[(lab, int(e["row"]))] = {k: v for k, v in e.items() if k not in ("row", value_key)}
        return self.add(seq, counts, rows, values, extras, n_nan)

    def merge(self, other: "ExemplarMerger") -> "ExemplarMerger":
        if (other.k, other.m, other.largest) != (self.k, self.m, self.largest):
            raise ValueError("ExemplarMerger.merge: k, m or direction differ")
        for c, es in other.clusters.items():
            self.clusters.setdefault(c, []).extend(es)
            self._trim(c)
        self.n_nan += other.n_nan
        self.batches += other.batches
        return self

    def result(self) -> List[dict]:
        """The non-empty clusters by label: ``{"label", "entries": [{"seq",
        "row", "value", **extra}]}``, best first."""
        return [{"label": c, "entries": [{**(x or {}), "seq": s, "row": r, "value": v} for v, s, r, x in es]}
                for c, es in sorted(self.clusters.items()) if es]

    def to_dict(self) -> dict:
        return {"k": self.k, "m": self.m, "largest": self.largest, "n_nan": self.n_nan, "batches": self.batches,
                "clusters": [{"label": c, "entries": [[v, s, r, x] for v, s, r, x in es]}
                             for c, es in sorted(self.clusters.items()) if es]}

    @classmethod
    def from_dict(cls, d: dict) -> "ExemplarMerger":
        me = cls(d["k"], d["m"], d["largest"])
        me.n_nan = int(d["n_nan"])
        me.batches = int(d["batches"])
        for c in d["clusters"]:
            me.clusters[int(c["label"])] = [(float(v), int(s), int(r), x) for v, s, r, x in c["entries"]]
        return me

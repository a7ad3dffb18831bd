"""Top-N selection of scored rows: the one contract of the host and the device
(``csrc/hip/topn.hip``), the CPU engines' ``top_batch`` and the stream-wide
merge of ``twtml-score --top``.

``top_n(values, rows, n, largest=True)``

* ``values``: fp64, one per scored row, in scored order; ``rows``: their raw row
  ids, ascending (``None``: row k is k).
* NaN values are never selected; they are counted as ``n_nan``.
* Values compare as IEEE numbers, so ``-0.0 == +0.0``.
* Best value first -- descending when ``largest``, ascending otherwise; equal
  values by ascending raw row id.
* The result is the first ``min(n, len(values) - n_nan)`` entries of that order,
  each ``(value with its original bits, raw row id)``.
* ``1 <= n <= TOPN_MAX``; anything else is a ``ValueError`` (``predict_batch``
  returns every row).

``TopNMerger(n, largest)`` keeps the best n entries over all batches added so
far, ordered by value, then batch sequence number, then row; merging two
mergers equals adding their batches to one.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["TOPN_MAX", "check_n", "top_n", "top_result", "empty_top", "TopNMerger"]

TOPN_MAX = 4096


def check_n(n) -> int:
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= TOPN_MAX:
        raise ValueError(f"top-N: n must be an integer in 1..{TOPN_MAX}, got {n!r}; "
                         f"predict_batch returns every row")
    return int(n)


def top_n(values, rows=None, n: int = 1, largest: bool = True) -> Tuple[np.ndarray, np.ndarray, int]:
    """``(values, rows, n_nan)`` of the n best entries, best first (module
    docstring).  The values keep their bits (a selected ``-0.0`` stays one)."""
    n = check_n(n)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    r = np.arange(v.size, dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    if r.shape != v.shape:
        raise ValueError(f"top-N: {v.size} values but {r.size} rows")
    ok = ~np.isnan(v)
    n_nan = int(v.size - np.count_nonzero(ok))
    v, r = v[ok], r[ok]
    # lexsort: last key first; -0.0 and +0.0 compare equal, so they tie on the row
    o = np.lexsort((r, -v if largest else v))[:n]
    return v[o], r[o], n_nan


def empty_top() -> Dict[str, object]:
    return {"rows": np.zeros(0, np.int64), "values": np.zeros(0, np.float64), "n_top": 0, "n_nan": 0}


def top_result(values, rows, n: int, largest: bool = True) -> Dict[str, object]:
    """``top_n`` as the dict the engines' ``top_batch`` return: ``rows``,
    ``values``, ``n_top``, ``n_nan``."""
    v, r, n_nan = top_n(values, rows, n, largest)
    return {"rows": r, "values": v, "n_top": int(v.size), "n_nan": n_nan}


class TopNMerger:
    """The best n entries of a stream of per-batch selections.  An entry is
    ``(value, seq, row, extra)``; the order is by value (``-0.0 == +0.0``),
    then ``seq``, then ``row``.  ``extra`` (a dict, or None) rides along."""

    def __init__(self, n: int, largest: bool = True):
        self.n = check_n(n)
        self.largest = bool(largest)
        self.entries: List[Tuple[float, int, int, Optional[dict]]] = []
        self.n_nan = 0
        self.batches = 0

    def _key(self, e):
        v = e[0] + 0.0   # -0.0 + 0.0 == +0.0: one key for both zeros
        return (-v if self.largest else v, e[1], e[2])

    def _trim(self) -> None:
        self.entries.sort(key=self._key)
        del self.entries[self.n:]

    def add(self, seq: int, values: Sequence[float], rows: Sequence[int], n_nan: int = 0,
            extras: Optional[Sequence[Optional[dict]]] = None) -> "TopNMerger":
        """One batch's selection (its values must not be NaN)."""
        vals = [float(x) for x in values]
        if any(x != x for x in vals):
            raise ValueError("TopNMerger.add: NaN values are never selected")
        ex = list(extras) if extras is not None else [None] * len(vals)
        if not len(vals) == len(rows) == len(ex):
            raise ValueError("TopNMerger.add: values, rows and extras differ in length")
        self.entries.extend((v, int(seq), int(r), x) for v, r, x in zip(vals, rows, ex))
        self.n_nan += int(n_nan)
        self.batches += 1
        self._trim()
        return self

    def merge(self, other: "TopNMerger") -> "TopNMerger":
        if (other.n, other.largest) != (self.n, self.largest):
            raise ValueError("TopNMerger.merge: n or direction differ")
        self.entries.extend(other.entries)
        self.n_nan += other.n_nan
        self.batches += other.batches
        self._trim()
        return self

    def result(self) -> List[dict]:
        """The entries, best first: ``{"seq", "row", "value", **extra}``."""
        return [{**(x or {}), "seq": s, "row": r, "value": v} for v, s, r, x in self.entries]

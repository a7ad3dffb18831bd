"""Python face of the MI355X streaming-LR engine (``csrc/hip/engine.cpp``).

The engine executes, per micro-batch and entirely on the GPU, what the
reference runs as ~60 Spark jobs: filter (K3), featurize
(K1+K2), prequential predict + stats (K4+K7, output op #1 of
``LinearRegression.scala:53-81``) and ``numIterations`` steps of
``GradientDescent`` (K5+K6, output op #2 ``model.trainOn`` at ``:86``).

Host-side contract: raw batches live in pinned :class:`HostBatch` buffers,
either in the packed wire format (narrow/cesu/wide ``text`` bytes, row
words, packed scalars; ``csrc/host/wire.h``) or as plain UTF-16 (``ingest
="utf16"``: no per-unit host work at all, the text can even be DMA'd
straight from the receiver's registered buffer).  Lower-casing -- including
the rows whose full case mapping is not one unit per unit (U+0130, Final
Sigma, astral cased letters, ``MllibHelper.scala:45``) -- happens on the
device (``csrc/hip/rows.hip``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import os
import weakref

import numpy as np

from ..records.batch import RETWEET_COUNT, RawBatch, Utf8Text
from ._native import hip, host
from .ingest import SlotPipeline

__all__ = ["LRDeviceConfig", "DeviceLinearRegression", "DeviceLogisticRegression", "prelower", "HostBatchView", "register_host",
           "unregister_host", "Utf8Text", "encode_utf8"]


def prelower(raw: RawBatch) -> RawBatch:
    """Host full case mapping of the special rows (reference / tests only:
    the device does this itself, ``csrc/hip/rows.hip``)."""
    h = host()
    if h.count_special_rows(raw.text, raw.offsets) == 0:
        return raw
    text, offsets, _ = h.prelower_special_rows(raw.text, raw.offsets)
    return RawBatch(text, offsets, raw.is_retweet, raw.scalars, raw.batch_time_ms)


def encode_utf8(raw: RawBatch, threads: int = 0) -> Utf8Text:
    """UTF-16 rows -> UTF-8 (astral pairs as 4 bytes, lone surrogates as 3:
    exact round trip through the device decoder)."""
    data, off = host().utf8_encode(raw.text, raw.offsets, int(threads))
    return Utf8Text(np.asarray(data), np.asarray(off))


@dataclass
class LRDeviceConfig:
    num_text_features: int = 1000
    hash: str = "java"
    step_size: float = 0.005
    num_iterations: int = 50
    fraction: float = 1.0
    tol: float = 1e-3
    begin: int = 100
    end: int = 1000
    require_retweet: bool = True
    range_filter: bool = True
    max_rows: int = 1 << 16
    max_units: int = (1 << 16) * 281
    sgd_grid: int = 0
    ablate: int = 0          # perf diagnostics only (1: no scatter, 2: no gather/scatter)
    # merge a row's repeated bigrams into term counts before the GD loop.
    # Measured on MI355X (1M-tweet batches, 35 iterations): -7% per iteration
    # but the merge pass costs more than it saves, so it is off by default.
    dedup: bool = False
    # dense 4-bit counts for the batch's 128 hottest bigrams (csrc/hip/hot_split.hip)
    hybrid: bool = True
    # hybrid layout only: the featurizer materialises hashed ids just for the
    # chunks the hot-slot histogram samples; the remap re-derives the rest
    # from the raw text (csrc/hip/narrow_text.h).  False keeps every id
    # (debug_prepared() inspection).
    lazy_idx: bool = True
    # host staging: "wire" packs rows on the host (Latin-1 / cesu / UTF-16,
    # ~166 B per tweet on PCIe); "utf16" ships plain UTF-16 (~300 B per
    # tweet) with no per-unit host work -- the device narrows Latin-1 rows;
    # "utf8" ships the receiver's UTF-8 bytes (~155 B per tweet) -- the
    # device decodes non-ASCII rows and narrows the Latin-1 ones
    ingest: str = "wire"
    # prepare batch t+1 (featurize .. layout, on a prep stream and the
    # engine's prep thread) while batch t trains; DP ranks all-gather their
    # prep packets between two of t's GD iterations (engine.cpp issue_c1)
    overlap: bool = True
    # take the DP path with a world-1 communicator (the packet all-gather,
    # the packed int64 gradient all-reduce per GD iteration and the stats
    # all-reduce all go through it): RCCL carries the DP traffic on one GPU
    force_dp: bool = False
    # DP: time each gradient all-reduce on the compute stream (result
    # "comm_ms"; events around the collective)
    comm_timing: bool = False
    # device raw-batch slots: the copy engine runs up to raw_slots - 1
    # batches ahead of the one training (0: TWTML_RAW_SLOTS or the engine
    # default, 6).  Deeper buffering lets the H2D of later batches proceed
    # while young-model batches (many GD iterations) keep the GPU busy, at
    # the cost of queueing latency (profiles/r6/raw_slots_sweep.txt: 6 is
    # the knee of tweets/s vs p50 on the headline bench).
    raw_slots: int = 0
    # GD loss: "squared" (StreamingLinearRegressionWithSGD, LeastSquaresGradient)
    # or "logistic" (StreamingLogisticRegressionWithSGD, binary LogisticGradient;
    # csrc/hip/sgd.hip LOSS).  Logistic: the label is retweetCount >=
    # label_threshold (< 0: the middle of begin..end), the prequential
    # prediction the class probability > threshold.
    loss: str = "squared"
    label_threshold: int = -1
    threshold: float = 0.5

    def effective_label_threshold(self) -> int:
        if self.loss == "logistic" and self.label_threshold < 0:
            return (int(self.begin) + int(self.end)) // 2
        return int(self.label_threshold)

    def as_dict(self) -> Dict[str, object]:
        return {
            "num_text_features": int(self.num_text_features),
            "hash_kind": 0 if self.hash == "java" else 1,
            "step_size": float(self.step_size),
            "num_iterations": int(self.num_iterations),
            "fraction": float(self.fraction),
            "tol": float(self.tol),
            "begin": int(self.begin),
            "end": int(self.end),
            "require_retweet": int(bool(self.require_retweet)),
            "range_filter": int(bool(self.range_filter)),
            "max_rows": int(self.max_rows),
            "max_units": int(self.max_units),
            "sgd_grid": int(self.sgd_grid),
            "ablate": int(self.ablate),
            "dedup": int(bool(self.dedup)),
            "hybrid": int(bool(self.hybrid)),
            "lazy_idx": int(bool(self.lazy_idx)),
            "overlap": int(bool(self.overlap)),
            "force_dp": int(bool(self.force_dp)),
            "comm_timing": int(bool(self.comm_timing)),
            "loss": _LOSSES[self.loss],
            "label_threshold": self.effective_label_threshold(),
            "threshold": float(self.threshold),
            **raw_slots_entry(self.raw_slots),
        }


_LOSSES = {"squared": 0, "logistic": 1}      # kLossSquared / kLossLogistic (csrc/hip/kernels.h)
_LINKS = {"margin": 0, "probability": 1, "class": 2}   # kLink* (csrc/hip/kernels.h)


def raw_slots_entry(n: int) -> Dict[str, int]:
    """The engine config's raw_slots (explicit, TWTML_RAW_SLOTS, else the
    engine's default)."""
    n = int(n) or int(os.environ.get("TWTML_RAW_SLOTS", "0") or 0)
    return {"raw_slots": n} if n > 0 else {}


class HostBatchView:
    """Pinned host staging buffer of one raw batch, with numpy views.

    ``load`` packs the UTF-16 batch into narrow (Latin-1, 1 byte/unit) /
    cesu / wide rows with the native multi-threaded packer
    (``csrc/host/wire.cpp``): typical tweet text crosses PCIe at half the
    UTF-16 size.  The five int64 scalar columns ship as bit-packed offsets
    from a per-batch base when their range fits (exact), and a row's byte
    length + flags as one u16 that the device scans back into offsets.
    ``load_utf16`` stages only the row words and scalars and leaves the
    text as UTF-16 (copied, or DMA'd from the caller's buffer by ``submit``).
    No lower-casing happens on the host in either mode.
    """

    def __init__(self, max_rows: int, max_units: int, text: bool = True):
        """text=False: no text buffer (row words and scalars only), for batches
        whose text is DMA'd from the receiver's registered buffer
        (``load_utf8(copy_text=False)``): the pinned footprint of a staging
        slot drops from ~3 bytes per unit to ~60 bytes per row."""
        self.max_units = int(max_units)
        self.has_text = bool(text)
        cap = max(int(host().wire_bound(self.max_units, int(max_rows))), int(host().utf8_bound(self.max_units)))
        if not self.has_text:
            cap = 256
        self._hb = hip().HostBatch(int(max_rows), cap)
        self.text = self._hb.text
        self.offsets = self._hb.offsets
        self.flags = self._hb.flags
        self.scalars_flat = self._hb.scalars_flat
        self.n = 0
        self.units = 0
        self.bytes = 0
        self.batch_time_ms = 0
        self.rows_packed = False
        self.ext_text = 0      # address of an external text buffer (load_utf16(copy_text=False))
        self._ext_owner = None

    @property
    def max_rows(self) -> int:
        return self._hb.max_rows

    def scalars(self) -> np.ndarray:
        return self.scalars_flat[:5 * self.n].reshape(5, self.n)

    def _check(self, raw: RawBatch) -> None:
        n, u = raw.n, raw.total_units
        if n > self.max_rows or u > self.max_units:
            raise ValueError(f"batch ({n} rows, {u} units) exceeds staging capacity "
                             f"({self.max_rows}, {self.max_units})")

    def load(self, raw: RawBatch, ingest: str = "wire") -> "HostBatchView":
        if not self.has_text and not (ingest == "utf8" and raw.utf8 is not None and raw.utf8.pinned):
            raise ValueError("this staging view has no text buffer (HostBatchView(text=False))")
        if ingest == "utf8" and raw.utf8 is not None:
            # the receiver's own UTF-8 bytes: DMA'd from its page-locked
            # buffer (no host copy), or copied into the staging buffer
            return self.load_utf8(raw, raw.utf8, copy_text=not raw.utf8.pinned)
        raw.ensure_text()
        if ingest == "utf16":
            return self.load_utf16(raw, copy_text=True)
        if ingest == "utf8":
            return self.load_utf8(raw, encode_utf8(raw), copy_text=True)
        if ingest != "wire":
            raise ValueError(f"unknown ingest mode {ingest!r}")
        self._check(raw)
        n, u = raw.n, raw.total_units
        self.bytes = int(host().wire_pack(raw.text, raw.offsets, raw.is_retweet, self.text,
                                          self.offsets, self.flags))
        self.scalars_flat[:5 * n] = raw.scalars.reshape(-1)
        self._hb.pack_scalars(n)   # bit-packed offsets from a per-batch base where a column's range fits
        self.rows_packed = bool(self._hb.pack_rows(n))   # offsets + flags as 2 B per row
        self.n, self.units, self.batch_time_ms = n, u, raw.batch_time_ms
        self.ext_text, self._ext_owner = 0, None
        return self

    def load_utf16(self, raw: RawBatch, copy_text: bool = True) -> "HostBatchView":
        """Raw UTF-16 staging (row words + scalars only; O(rows) host work
        plus the text copy, which copy_text=False skips: ``submit`` then DMAs
        the text from ``raw.text`` -- register it with :func:`register_host`)."""
        self._check(raw)
        if copy_text and not self.has_text:
            raise ValueError("this staging view has no text buffer (HostBatchView(text=False))")
        text = np.ascontiguousarray(raw.text, dtype=np.uint16)
        sc = np.ascontiguousarray(raw.scalars, dtype=np.int64)
        self.bytes = int(self._hb.load_utf16(text, np.ascontiguousarray(raw.offsets, dtype=np.int64),
                                             np.ascontiguousarray(raw.is_retweet, dtype=np.uint8), sc,
                                             bool(copy_text), range=raw.scalar_range))
        self.n, self.units, self.batch_time_ms = raw.n, raw.total_units, raw.batch_time_ms
        self.rows_packed = int(self._hb.rowpacked_n) == raw.n
        self.ext_text = 0 if copy_text else int(text.ctypes.data)
        self._ext_owner = None if copy_text else text   # keeps the DMA source alive
        return self

    def load_utf8(self, raw: RawBatch, u8: Utf8Text, copy_text: bool = True) -> "HostBatchView":
        """Raw UTF-8 staging: row words (byte lengths) + scalars; the text is
        copied, or (copy_text=False) DMA'd by ``submit`` straight from
        ``u8.data`` -- register it with :func:`register_host`.  ``raw``
        supplies the scalar columns, retweet flags and unit count."""
        self._check(raw)
        if copy_text and not self.has_text:
            raise ValueError("this staging view has no text buffer (HostBatchView(text=False))")
        if u8.offsets.shape[0] != raw.n + 1:
            raise ValueError("UTF-8 offsets do not match the batch")
        sc = np.ascontiguousarray(raw.scalars, dtype=np.int64)
        self.bytes = int(self._hb.load_utf8(u8.data, np.ascontiguousarray(u8.offsets, dtype=np.int64),
                                            np.ascontiguousarray(raw.is_retweet, dtype=np.uint8), sc,
                                            bool(copy_text), range=raw.scalar_range))
        self.n, self.units, self.batch_time_ms = raw.n, raw.total_units, raw.batch_time_ms
        self.rows_packed = int(self._hb.rowpacked_n) == raw.n
        self.ext_text = 0 if copy_text else int(u8.data.ctypes.data)
        self._ext_owner = None if copy_text else u8.data
        return self

    def as_raw(self) -> RawBatch:
        if self.ext_text:
            raise ValueError("text was not staged (load_utf16(copy_text=False))")
        text, offsets, is_rt = host().wire_unpack(self.text[:self.bytes], self.offsets[:self.n + 1],
                                                  self.flags[:self.n])
        return RawBatch(text, offsets, is_rt, self.scalars().copy(), self.batch_time_ms)


# ptr -> weakref.finalize of a live registration (register_host)
_REGISTERED: Dict[int, "weakref.finalize"] = {}


def _drop_registration(ptr: int) -> None:
    """Finalizer of a registered array: unregister before its memory is freed
    (the runtime would otherwise keep the stale range in its host-pointer map
    and resolve later buffers mapped there to it -- round 5's ``invalid
    argument`` H2D and illegal memory access, profiles/README.md round 6)."""
    _REGISTERED.pop(ptr, None)
    try:
        hip().host_unregister(ptr)
    except BaseException:   # noqa: BLE001 -- interpreter teardown: the runtime may be gone
        import sys
        if not sys.is_finalizing():
            raise


def register_host(arr) -> None:
    """Page-lock a host array (or a :class:`Utf8Text`'s bytes) so ``submit``
    can DMA from it asynchronously.  The registration lives as long as the
    array object: it is undone (after the device drained) when the array is
    freed, or by :func:`unregister_host`."""
    if isinstance(arr, Utf8Text):
        register_host(arr.data)
        arr.pinned = True
        return
    if not arr.nbytes:
        return
    # a view: the registration must not outlive the memory, so it is tied to
    # the outermost array of the chain (it dies only after every view)
    owner = arr
    while isinstance(owner.base, np.ndarray):
        owner = owner.base
    ptr = int(arr.ctypes.data)
    hip().host_register(ptr, int(arr.nbytes))
    try:
        fin = weakref.finalize(owner, _drop_registration, ptr)
    except TypeError:   # an owner that takes no weak reference: tie it to the array itself
        fin = weakref.finalize(arr, _drop_registration, ptr)
    fin.atexit = False
    _REGISTERED[ptr] = fin


def unregister_host(arr) -> None:
    if isinstance(arr, Utf8Text):
        unregister_host(arr.data)
        arr.pinned = False
        return
    if not arr.nbytes:
        return
    ptr = int(arr.ctypes.data)
    fin = _REGISTERED.pop(ptr, None)
    if fin is not None:
        fin.detach()
    hip().host_unregister(ptr)


def registered_host_ranges():
    """Live host registrations ``[(ptr, bytes)]`` (native registry)."""
    return list(hip().host_registrations())


class DeviceLinearRegression:
    """StreamingLinearRegressionWithSGD state + pipeline on one GPU."""

    def __init__(self, cfg: LRDeviceConfig, device: int = 0, comm=None):
        if cfg.loss not in _LOSSES:
            raise ValueError(f"unknown loss {cfg.loss!r} (squared or logistic)")
        self.cfg = cfg
        self.device = int(device)
        self.comm = comm
        self._eng = hip().LREngine(self.device, cfg.as_dict(), comm)
        self._staging: List[HostBatchView] = []
        self.raw_slots = int(self._eng.raw_slots)
        # callbacks through a weak proxy: no reference cycle, so dropping the
        # last reference frees the engine's device memory at once
        me = weakref.proxy(self)
        self._pipe = SlotPipeline(self.raw_slots, lambda s, raw: me.staging(s).load(raw, cfg.ingest),
                                  lambda hb, slot: me.submit(hb, slot), lambda: me.synchronize(),
                                  discard=lambda slot: me._eng.discard(int(slot)))

    # ---- weights (MLlib setInitialWeights / latestModel.weights) ---------
    @property
    def num_weights(self) -> int:
        return int(self._eng.num_weights)

    def get_weights(self) -> np.ndarray:
        return np.asarray(self._eng.get_weights())

    def snapshot_begin(self) -> None:
        """Non-blocking checkpoint, part 1 (training thread, between batches):
        the device compacts the non-zero weights behind the last batch
        (``csrc/hip/snapshot.hip``); nothing is copied yet."""
        self._eng.snapshot_begin()

    def snapshot_fetch(self, reuse: bool = False):
        """Part 2 (any thread, e.g. a checkpoint writer): ``(size, indices,
        values)`` of the begun snapshot -- only the non-zero weights cross
        PCIe, on the engine's snapshot stream, while training goes on.
        ``reuse=True`` (the checkpoint writer): the arrays view host buffers
        the engine keeps across snapshots (no fresh pages per checkpoint);
        they are overwritten by the next fetch."""
        idx, val = self._eng.snapshot_fetch(reuse)
        return self.num_weights, np.asarray(idx), np.asarray(val)

    def set_weights(self, w: np.ndarray) -> None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (self.num_weights,):
            raise ValueError(f"expected {self.num_weights} weights, got {w.shape}")
        self._eng.set_weights(w)

    # ---- staging / pipeline ----------------------------------------------
    def staging(self, i: int = 0) -> HostBatchView:
        while len(self._staging) <= i:
            self._staging.append(HostBatchView(self.cfg.max_rows, self.cfg.max_units))
        return self._staging[i]

    def submit(self, hb: HostBatchView, slot: int) -> None:
        self._eng.submit(hb._hb, int(hb.n), int(hb.bytes), int(slot), int(hb.ext_text), int(hb.batch_time_ms))

    def process(self, slot: int, now_ms: int, want_pred: bool = False, plot_points: int = 0) -> Dict[str, object]:
        """``want_pred``: ``pred`` / ``real`` hold this rank's kept rows'
        rounded predictions and labels (kept order) -- all of them, or
        ``plot_points`` evenly spaced ones sampled on the device."""
        return self._eng.process(int(slot), int(now_ms), bool(want_pred), int(plot_points))

    def prefetch(self, raw: RawBatch) -> bool:
        """Stage + async H2D of a queued future batch (overlaps the current one)."""
        return self._pipe.prefetch(raw)

    def train_batch(self, raw: RawBatch, want_pred: bool = True, plot_points: int = 0) -> Dict[str, object]:
        """Train on one micro-batch: uses its prefetched slot, else stages + H2D now."""
        return self.process(self._pipe.take(raw), raw.batch_time_ms, want_pred, plot_points)

    # ---- inference (csrc/hip/score.hip) -----------------------------------
    def predict_batch(self, raw: RawBatch, apply_filter: bool = False,
                      now_ms: Optional[int] = None, output: str = "margin") -> Dict[str, object]:
        """Score one raw micro-batch with the current weights, without
        training on it: ``rows`` (int64 raw row ids, ascending) and ``pred``
        (their fp64 predictions ``x . w``, nothing rounded; arrays owned by the
        caller), ``n_raw``, ``n_scored``, ``score_ms`` (device time of the
        scoring kernels).  ``apply_filter``: only the rows the training filter
        keeps.  ``output``: ``"margin"`` (``x . w``), ``"probability"`` (``1 /
        (1 + exp(-margin))``) or ``"class"`` (margin > logit(``cfg.threshold``)
        as 1.0 / 0.0), applied per row on the device in fp64.  The batch is staged into a raw slot the training pipeline
        holds no batch in and never enters the engine's prepare-ahead queue;
        the model, the prefetched batches and a pending snapshot are left as
        they are.  Call it from the thread that calls ``train_batch``."""
        if output not in _LINKS:
            raise ValueError(f"unknown output {output!r} (class, probability or margin)")
        self.staging(0)._check(raw)   # the ValueError of training, before a slot is touched
        if raw.n == 0:                # nothing is staged or launched
            return {"n_raw": 0, "n_scored": 0, "rows": np.zeros(0, np.int64), "pred": np.zeros(0, np.float64),
                    "score_ms": 0.0, "wall_ms": 0.0}
        slot = self._pipe.free_slot()
        try:
            hb = self.staging(slot).load(raw, self.cfg.ingest)
            self._eng.submit(hb._hb, int(hb.n), int(hb.bytes), int(slot), int(hb.ext_text),
                             int(hb.batch_time_ms), False)
            return self._eng.score(int(slot), int(raw.batch_time_ms if now_ms is None else now_ms),
                                   bool(apply_filter), _LINKS[output])
        finally:
            self._pipe.score_done(slot)

    # ---- held-out evaluation (csrc/hip/eval.hip) ---------------------------
    def evaluate_batch(self, raw: RawBatch, apply_filter: bool = False,
                       now_ms: Optional[int] = None) -> Dict[str, object]:
        """Evaluate the current model on one labelled raw micro-batch, without
        training on it: ``predict_batch``'s margins and the rows'
        ``retweetCount`` reduced on the device into the accumulator of
        ``models/metrics.py`` -- ``kind`` ``"binary"`` (logistic loss: ``hist``
        2 x 4097 int64, ``confusion`` [tn, fp, fn, tp], ``logloss_sum``) or
        ``"regression"`` (the six ``sum_*``), with ``n``, ``n_nan``, ``n_raw``,
        ``n_scored``, ``label_threshold``, ``threshold``, ``eval_ms`` (device
        time, filter through the reduction) and ``wall_ms``.  Only the
        accumulator (~66 KB) leaves the device.  Feed the result to
        ``metrics.EvalAccumulator.add`` / ``metrics.metrics_of``.  Staging and
        guarantees are ``predict_batch``'s."""
        from ..models import metrics
        kind = "binary" if self.cfg.loss == "logistic" else "regression"
        lt = self.cfg.effective_label_threshold() if kind == "binary" else -1
        self.staging(0)._check(raw)
        if raw.n == 0:                # nothing is staged or launched
            out = metrics.empty_result(kind, lt, float(self.cfg.threshold))
            out.update(n_raw=0, n_scored=0, eval_ms=0.0, wall_ms=0.0)
            return out
        slot = self._pipe.free_slot()
        try:
            hb = self.staging(slot).load(raw, self.cfg.ingest)
            self._eng.submit(hb._hb, int(hb.n), int(hb.bytes), int(slot), int(hb.ext_text),
                             int(hb.batch_time_ms), False)
            r = self._eng.evaluate(int(slot), int(raw.batch_time_ms if now_ms is None else now_ms),
                                   bool(apply_filter))
        finally:
            self._pipe.score_done(slot)
        iw, dw = np.asarray(r["iw"]), np.asarray(r["dw"])
        out = {"kind": kind, "n_raw": int(r["n_raw"]), "n_scored": int(r["n_scored"]), "n": int(iw[0]),
               "n_nan": int(iw[1]), "label_threshold": lt, "threshold": float(self.cfg.threshold),
               "eval_ms": float(r["eval_ms"]), "wall_ms": float(r["wall_ms"])}
        if kind == "binary":
            out.update(hist=iw[8:8 + 2 * metrics.EVAL_BINS].reshape(2, metrics.EVAL_BINS).copy(),
                       confusion=[int(v) for v in iw[2:6]], logloss_sum=float(dw[0]))
        else:
            out.update({k: float(dw[j]) for j, k in enumerate(metrics.REGRESSION_SUMS)})
        return out

    # ---- top-N (csrc/hip/topn.hip) -----------------------------------------
    def top_batch(self, raw: RawBatch, n: int, largest: bool = True, apply_filter: bool = False,
                  now_ms: Optional[int] = None) -> Dict[str, object]:
        """The n best rows of one raw micro-batch under the current weights,
        selected on the device (the contract of ``models/topn.py``):
        ``predict_batch``'s margins ``x . w``, then an exact radix select and
        sort behind them -- ``rows`` (int64 raw row ids) and ``values`` (their
        fp64 margins), best first (``largest``: descending), equal margins by
        ascending row, NaN margins never; ``n_top`` = ``min(n, n_scored -
        n_nan)``, ``n_nan``, ``n_raw``, ``n_scored``, ``top_ms`` (device time,
        filter through the selection) and ``wall_ms``.  Only the n entries
        leave the device.  The logistic engine selects on the margin too: it
        is monotone in the probability and still separates rows whose
        probability has saturated.  ``1 <= n <= 4096``.  Staging and
        guarantees are ``predict_batch``'s."""
        from ..models.topn import check_n, empty_top
        n = check_n(n)
        self.staging(0)._check(raw)
        if raw.n == 0:                # nothing is staged or launched
            return {**empty_top(), "n_raw": 0, "n_scored": 0, "top_ms": 0.0, "wall_ms": 0.0}
        slot = self._pipe.free_slot()
        try:
            hb = self.staging(slot).load(raw, self.cfg.ingest)
            self._eng.submit(hb._hb, int(hb.n), int(hb.bytes), int(slot), int(hb.ext_text),
                             int(hb.batch_time_ms), False)
            r = self._eng.top(int(slot), int(raw.batch_time_ms if now_ms is None else now_ms),
                              bool(apply_filter), n, bool(largest))
        finally:
            self._pipe.score_done(slot)
        return {"rows": np.asarray(r["rows"]), "values": np.asarray(r["values"]), "n_top": int(r["n_top"]),
                "n_nan": int(r["n_nan"]), "n_raw": int(r["n_raw"]), "n_scored": int(r["n_scored"]),
                "top_ms": float(r["top_ms"]), "wall_ms": float(r["wall_ms"])}

    @property
    def h2d_bytes(self) -> int:
        """Host-to-device bytes submitted so far (every copy of every batch)."""
        return int(self._eng.h2d_bytes)

    def synchronize(self) -> None:
        self._eng.synchronize()


class DeviceLogisticRegression(DeviceLinearRegression):
    """StreamingLogisticRegressionWithSGD on one GPU: the LR engine with
    ``loss="logistic"`` -- 0/1 labels (``retweetCount >= label_threshold``),
    the logistic row epilogue in the iteration kernels, class predictions in
    the prequential statistics -- and ``predict_batch`` defaulting to the
    class."""

    def __init__(self, cfg: LRDeviceConfig, device: int = 0, comm=None):
        if cfg.loss != "logistic":
            raise ValueError('DeviceLogisticRegression needs LRDeviceConfig(loss="logistic")')
        super().__init__(cfg, device, comm)

    def predict_batch(self, raw: RawBatch, apply_filter: bool = False,
                      now_ms: Optional[int] = None, output: str = "class") -> Dict[str, object]:
        return super().predict_batch(raw, apply_filter, now_ms, output)


def batch_report(res: Dict[str, object]) -> Dict[str, float]:
    """Population stdevs / MSE from the fused stats (``LinearRegression.scala:59-65``)."""
    n, sy, sy2, sp, sp2, se2 = res["stats"]
    if n <= 0:
        return {"count": 0, "mse": float("nan"), "realStdev": float("nan"),
                "predStdev": float("nan")}
    my, mp = sy / n, sp / n
    return {
        "count": int(round(n)),
        "mse": se2 / n,
        "realStdev": float(np.sqrt(max(sy2 / n - my * my, 0.0))),
        "predStdev": float(np.sqrt(max(sp2 / n - mp * mp, 0.0))),
    }

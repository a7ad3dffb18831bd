#!/usr/bin/env python
"""Throughput of held-out evaluation, end to end (one GPU).

``tools/score_bench.py``'s loop with ``LREngine::evaluate`` in place of
``score``: the flagship stream of ``bench.py`` -- wide profile, 1M tweets per
batch, UTF-8 ingest from a pool of distinct batches whose text is DMA'd from
the receiver's page-locked buffers -- evaluated against its own retweet
counts: per batch the host staging, the H2D, the scoring pass
(``csrc/hip/score.hip``), the reduction of ``csrc/hip/eval.hip`` and the D2H
of the ~66 KB accumulator (instead of 8 MB of predictions).  The weights come
from training the first 5 pool batches with the chosen loss.

Prints one JSON line: tweets/s evaluated, ms per batch (wall / steps, and the
p50 of the per-batch ``evaluate()`` calls), device ms filter through the
reduction (events), H2D bytes per tweet, and the metrics of the accumulator
merged over the last window (logistic: the AUC with its ``auc_tie_bound``).
``--repeat N`` times the window N times in one process and reports the median
window.

    python tools/eval_bench.py [--loss logistic] [--features 1000000] [--repeat 3]
"""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import score_bench  # noqa: E402  (the stream, the pool and the staging thread are its)


def run_window(eng, raws, u8s, views, first, n, now_ms, apply_filter, record, total=None):
    """score_bench.run_window with evaluate(): the engine binding is wrapped so
    that the loop, the staging thread and the slot hand-over stay one code."""

    class _Evaluating:
        def __init__(self, e):
            self._e = e
            self.submit = e.submit

        def score(self, slot, now, filt):
            r = self._e.evaluate(slot, now, filt)
            if total is not None:
                total.append(r)
            return {"n_scored": r["n_scored"], "score_ms": r["eval_ms"], "wall_ms": r["wall_ms"]}

    return score_bench.run_window(types.SimpleNamespace(_eng=_Evaluating(eng._eng)), raws, u8s, views, first, n, now_ms, apply_filter, record)


def _merged(eng, results):
    """The window's accumulator words as one EvalAccumulator."""
    from twitter_stream_ml_amd.models import metrics
    kind = "binary" if eng.cfg.loss == "logistic" else "regression"
    lt = eng.cfg.effective_label_threshold() if kind == "binary" else -1
    acc = metrics.EvalAccumulator(kind, lt, float(eng.cfg.threshold))
    for r in results:
        iw, dw = np.asarray(r["iw"]), np.asarray(r["dw"])
        res = {"kind": kind, "n": int(iw[0]), "n_nan": int(iw[1]), "label_threshold": lt,
               "threshold": float(eng.cfg.threshold)}
        if kind == "binary":
            res.update(hist=iw[8:8 + 2 * metrics.EVAL_BINS].reshape(2, metrics.EVAL_BINS),
                       confusion=[int(v) for v in iw[2:6]], logloss_sum=float(dw[0]))
        else:
            res.update({k: float(dw[j]) for j, k in enumerate(metrics.REGRESSION_SUMS)})
        acc.add(res)
    return acc


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    loss = "logistic"
    if "--loss" in argv:
        i = argv.index("--loss")
        loss = argv[i + 1]
        del argv[i:i + 2]
    if loss not in ("logistic", "squared"):
        print("eval_bench: --loss logistic|squared", file=sys.stderr)
        return 2
    args = score_bench.parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.ops.lr_engine import (DeviceLinearRegression, DeviceLogisticRegression, HostBatchView,
                                                     LRDeviceConfig)
    from twitter_stream_ml_amd.sources.synthetic import SynthConfig

    device = 0
    torch.cuda.set_device(device)
    synth = SynthConfig.profile(args.profile, seed=args.seed)
    now_ms = synth.now_ms
    B = int(args.batch)
    n_pool = args.pool if args.pool > 0 else args.warmup + args.steps
    n_pool = max(args.train, 1, min(n_pool, int(os.environ.get("TWTML_BENCH_POOL_TWEETS", "64000000")) // max(1, B)))
    t_gen = time.time()
    raws, u8s, pinned = bench.utf8_pool(synth, B, n_pool, now_ms)
    for r in raws:
        r.with_scalar_range()
    t_gen = time.time() - t_gen
    max_units = max(r.total_units for r in raws) + 1024
    cfg = LRDeviceConfig(num_text_features=args.features, hash=args.hash, num_iterations=args.iters, max_rows=B,
                         max_units=max_units, ingest="utf8", loss=loss)
    eng = (DeviceLogisticRegression if loss == "logistic" else DeviceLinearRegression)(cfg, device=device)
    views = [HostBatchView(B, max_units, text=False) for _ in range(eng.raw_slots)]

    # the model: the first pool batches, trained
    for i in range(min(args.train, len(raws))):
        hb = views[0].load_utf8(raws[i], u8s[i], copy_text=False)
        eng.submit(hb, 0)
        eng.process(0, now_ms)
    eng.synchronize()
    nz = int(np.count_nonzero(eng.get_weights()))

    run_window(eng, raws, u8s, views, 0, args.warmup, now_ms, args.filter, None)
    windows, results = [], []
    for k in range(max(1, args.repeat)):
        eng.synchronize()
        torch.cuda.synchronize()
        rec, results = [], []
        b0 = eng.h2d_bytes
        t0 = time.perf_counter()
        n_eval = run_window(eng, raws, u8s, views, args.warmup + k * args.steps, args.steps, now_ms, args.filter, rec,
                            results)
        eng.synchronize()
        t1 = time.perf_counter()
        windows.append({
            "tweets_per_s": n_eval / (t1 - t0),
            "ms_per_batch": (t1 - t0) / args.steps * 1e3,
            "call_ms_p50": float(np.median([r[0] for r in rec])),
            "device_ms_p50": float(np.median([r[1] for r in rec])),
            "device_ms_mean": float(np.mean([r[1] for r in rec])),
            "h2d_bytes_per_tweet": (eng.h2d_bytes - b0) / (args.steps * B),
            "evaluated_per_batch": n_eval / args.steps,
        })
    order = sorted(range(len(windows)), key=lambda i: windows[i]["ms_per_batch"])
    med = windows[order[len(order) // 2]]
    gbps = bench._h2d_gbps(device)
    floor_ms = med["h2d_bytes_per_tweet"] * B / (gbps * 1e9) * 1e3
    acc = _merged(eng, results)
    out = {
        "metric": "tweets/sec evaluated (one GPU, end to end)",
        "value": round(med["tweets_per_s"], 1),
        "unit": "tweets/s",
        "higher_is_better": True,
        "steps": args.steps, "warmup": args.warmup, "repeat": len(windows),
        "ms_per_batch": round(med["ms_per_batch"], 3),
        "ms_per_batch_windows": [round(w["ms_per_batch"], 3) for w in windows],
        "evaluate_call_ms_p50": round(med["call_ms_p50"], 3),
        "device_ms_filter_to_reduction_p50": round(med["device_ms_p50"], 3),
        "device_ms_filter_to_reduction_mean": round(med["device_ms_mean"], 3),
        "d2h_bytes_per_batch": 8 * (8 + 2 * 4097 + 8),
        "h2d_bytes_per_tweet": round(med["h2d_bytes_per_tweet"], 2),
        "h2d_gbps_pinned": round(gbps, 2),
        "host_link_floor_ms_per_batch": round(floor_ms, 3),
        "ratio_to_host_link_floor": round(med["ms_per_batch"] / floor_ms, 3) if floor_ms > 0 else None,
        "evaluated_tweets_per_batch": round(med["evaluated_per_batch"], 1),
        "metrics_last_window": acc.metrics().to_dict(),
        "config": {"batch": B, "features": args.features, "hash": args.hash, "profile": args.profile, "loss": loss,
                   "label_threshold": acc.label_threshold, "ingest": "e2e-utf8", "apply_filter": bool(args.filter),
                   "pool_batches": n_pool, "trained_batches": min(args.train, len(raws)), "nonzero_weights": nz,
                   "raw_slots": eng.raw_slots},
        "pool_gen_s": round(t_gen, 1),
    }
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

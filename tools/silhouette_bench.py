#!/usr/bin/env python
"""Cost of the silhouette next to k-means scoring, end to end (one GPU).

The stream of ``tools/km_score_bench.py`` -- wide profile, 1M tweets per batch,
k = 1024, 62 hashed bigram dims + 2 numeric, UTF-8 ingest from page-locked
buffers, the model trained on the first pool batches -- run through two timed
windows in one process: ``KMEngine::score`` (what ``predict_batch`` runs) and
``KMEngine::silhouette`` (the same passes, then the batch's cluster means,
``dev2``, ``W`` and the neighbour pass of ``csrc/hip/silhouette.hip``).  A
staging thread keeps up to ``raw_slots - 1`` batches submitted ahead.

Prints one JSON line: ms per batch of either call (wall / steps), the device
times ``score_ms`` and ``sil_ms`` (events around the kernels), and the bytes
that leave the device per batch.  ``--repeat N`` times each window N times and
reports the medians.  For the per-kernel split run it once more under
``rocprofv3 --kernel-trace --stats -- python tools/silhouette_bench.py --steps 5``.

    python tools/silhouette_bench.py [--k 1024] [--text-dims 62] [--repeat 3]
"""
import json
import os
import queue
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import km_score_bench as ksb   # noqa: E402  (the arguments and the stream are its own)


def run_window(eng, raws, u8s, views, first, n, call, record):
    """Batches first .. first + n - 1 of the stream through ``call(slot)``; a
    staging thread stages + submits up to len(views) - 1 batches ahead."""
    free, ready, err = queue.Queue(), queue.Queue(), []
    for s in range(max(1, len(views) - 1)):
        free.put(s)

    def stager():
        try:
            for i in range(first, first + n):
                slot = free.get()
                hb = views[slot].load_utf8(raws[i % len(raws)], u8s[i % len(raws)], copy_text=False)
                eng.submit(hb, slot)
                ready.put(slot)
        except BaseException as ex:   # surfaced by the main thread
            err.append(ex)
            ready.put(None)

    th = threading.Thread(target=stager, name="stager", daemon=True)
    th.start()
    scored = 0
    last = None
    for _ in range(n):
        slot = ready.get()
        if slot is None:
            raise err[0]
        t = time.perf_counter()
        last = call(slot)
        dt = (time.perf_counter() - t) * 1e3
        free.put(slot)
        scored += int(last["n_scored"])
        if record is not None:
            record.append((dt, float(last.get("sil_ms", last.get("score_ms", 0.0)))))
    th.join(timeout=60)
    return scored, last


def main(argv=None) -> int:
    args = ksb.parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.models.silhouette import SilhouetteAccumulator
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    from twitter_stream_ml_amd.ops.lr_engine import HostBatchView
    from twitter_stream_ml_amd.sources.synthetic import SynthConfig

    device = 0
    torch.cuda.set_device(device)
    synth = SynthConfig.profile(args.profile, seed=args.seed)
    B = int(args.batch)
    n_pool = args.pool if args.pool > 0 else args.warmup + args.steps
    n_pool = max(args.train, 1, min(n_pool, int(os.environ.get("TWTML_BENCH_POOL_TWEETS", "64000000")) // max(1, B)))
    raws, u8s, pinned = bench.utf8_pool(synth, B, n_pool, synth.now_ms)
    for r in raws:
        r.with_scalar_range()
    max_units = max(r.total_units for r in raws) + 1024
    eng = DeviceKMeans(KMDeviceConfig(k=args.k, text_dims=args.text_dims, half_life=5.0, max_rows=B,
                                      max_units=max_units, seed=args.seed), device=device)
    views = [HostBatchView(B, max_units, text=False) for _ in range(eng.raw_slots)]
    for v in views:
        v._hb.scalar_cols = 2   # k-means reads retweetCount and followersCount only
    for i in range(min(args.train, len(raws))):
        eng.submit(views[0].load_utf8(raws[i], u8s[i], copy_text=False), 0)
        eng.process(0, want_pred=False)
    eng.synchronize()

    apply_filter, scaler = not args.no_filter, ksb.SCALERS[args.scaler]
    e = eng._eng
    calls = {"score": lambda slot: e.score(slot, bool(apply_filter), scaler),
             "silhouette": lambda slot: e.silhouette(slot, bool(apply_filter), scaler)}
    out = {"metric": "ms per k-means batch with the silhouette (one GPU, end to end)", "unit": "ms",
           "higher_is_better": False, "steps": args.steps, "warmup": args.warmup, "repeat": max(1, args.repeat)}
    acc = SilhouetteAccumulator(args.k)
    for name, call in calls.items():
        run_window(eng, raws, u8s, views, 0, args.warmup, call, None)
        wall, dev, scored = [], [], 0
        for w in range(max(1, args.repeat)):
            eng.synchronize()
            torch.cuda.synchronize()
            rec = []
            t0 = time.perf_counter()
            scored, last = run_window(eng, raws, u8s, views, args.warmup + w * args.steps, args.steps, call, rec)
            eng.synchronize()
            wall.append((time.perf_counter() - t0) / args.steps * 1e3)
            dev.append(float(np.median([r[1] for r in rec])))
        out[f"{name}_ms_per_batch"] = round(float(np.median(wall)), 3)
        out[f"{name}_ms_per_batch_windows"] = [round(v, 3) for v in wall]
        out[f"{name}_device_ms_p50"] = round(float(np.median(dev)), 3)
        out[f"{name}_device_ms_p50_windows"] = [round(v, 3) for v in dev]
        out[f"{name}_scored_per_batch"] = round(scored / args.steps, 1)
        if name == "silhouette":
            acc.add_words(last["n"], last["s_fix"], int(last["n_single"]), int(last["n_undefined"]))
            out["last_batch_silhouette"] = acc.silhouette
            out["last_batch_clusters_used"] = int(last["nonempty"])
    n_scored = out["score_scored_per_batch"]
    d = 2 + args.text_dims
    out["value"] = out["silhouette_ms_per_batch"]
    out["sil_minus_score_device_ms"] = round(out["silhouette_device_ms_p50"] - out["score_device_ms_p50"], 3)
    out["d2h_bytes_per_batch"] = {"score": int(20 * n_scored + 8 + 8 * args.k),
                                  "silhouette": int(8 * (2 * args.k + 4) + 8 + 8 * args.k + 8 * d)}
    out["config"] = {"batch": B, "k": args.k, "text_dims": args.text_dims, "profile": args.profile,
                     "apply_filter": apply_filter, "scaler": args.scaler, "pool_batches": n_pool,
                     "raw_slots": eng.raw_slots}
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

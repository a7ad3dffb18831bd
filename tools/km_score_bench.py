#!/usr/bin/env python
"""Throughput of k-means scoring, end to end (one GPU).

The k-means stream of ``bench.py --model kmeans`` -- wide profile, 1M tweets
per batch, k = 1024, 62 hashed bigram dims + 2 numeric, UTF-8 ingest from a
pool of batches whose text is DMA'd from the receiver's page-locked buffers --
scored instead of trained: per batch the host staging (row words + the two
scalar columns), the H2D, ``KMEngine::score`` (decode, isRetweet filter,
features, the per-batch scaler, matrix-core assignment with its fp64 refine,
the fp64 cost pass ``k_km_cost``) and the D2H of rows, labels and squared
distances.  A staging thread keeps up to ``raw_slots - 1`` batches submitted
ahead of the one being scored, as ``bench.py``'s e2e loop does for training.
The model comes from training the first pool batches.

Prints one JSON line: ms per scored batch (wall / steps), the device
``score_ms`` (events around the kernels), tweets/s scored.  ``--repeat N``
times the window N times in one process and reports the median window.

    python tools/km_score_bench.py [--k 1024] [--text-dims 62] [--repeat 3]
"""
import argparse
import json
import os
import queue
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALERS = {"batch": 0, "none": 2}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--text-dims", type=int, default=62)
    ap.add_argument("--profile", default="wide", choices=["bench", "wide"])
    ap.add_argument("--pool", type=int, default=0, help="distinct batches (default: warmup + steps)")
    ap.add_argument("--train", type=int, default=3, help="pool batches trained for the model")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeat", type=int, default=1, help="timed windows in this process (median reported)")
    ap.add_argument("--scaler", default="batch", choices=sorted(SCALERS))
    ap.add_argument("--no-filter", action="store_true", help="score every row, not only the retweets")
    ap.add_argument("--json-out", default="")
    return ap.parse_args(argv)


def run_window(eng, raws, u8s, views, first, n, apply_filter, scaler, record):
    """Score batches first .. first + n - 1 of the stream; a staging thread
    stages + submits up to len(views) - 1 batches ahead."""
    e = eng._eng
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
    scored, cost = 0, 0.0
    for _ in range(n):
        slot = ready.get()
        if slot is None:
            raise err[0]
        t = time.perf_counter()
        res = e.score(slot, bool(apply_filter), scaler)
        dt = (time.perf_counter() - t) * 1e3
        free.put(slot)
        scored += int(res["n_scored"])
        cost += float(res["cost"])
        if record is not None:
            record.append((dt, float(res["score_ms"])))
    th.join(timeout=60)
    return scored, cost


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    from twitter_stream_ml_amd.ops.lr_engine import HostBatchView
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
    cfg = KMDeviceConfig(k=args.k, text_dims=args.text_dims, half_life=5.0, max_rows=B, max_units=max_units,
                         seed=args.seed)
    eng = DeviceKMeans(cfg, device=device)
    views = [HostBatchView(B, max_units, text=False) for _ in range(eng.raw_slots)]
    for v in views:
        v._hb.scalar_cols = 2   # k-means reads retweetCount and followersCount only

    # the model: the first pool batches, trained
    train_ms = []
    for i in range(min(args.train, len(raws))):
        hb = views[0].load_utf8(raws[i], u8s[i], copy_text=False)
        eng.submit(hb, 0)
        train_ms.append(float(eng.process(0, want_pred=False)["ms"]))
    eng.synchronize()

    apply_filter, scaler = not args.no_filter, SCALERS[args.scaler]
    run_window(eng, raws, u8s, views, 0, args.warmup, apply_filter, scaler, None)
    windows = []
    for k in range(max(1, args.repeat)):
        eng.synchronize()
        torch.cuda.synchronize()
        rec = []
        b0 = eng.h2d_bytes
        t0 = time.perf_counter()
        scored, cost = run_window(eng, raws, u8s, views, args.warmup + k * args.steps, args.steps, apply_filter,
                                  scaler, rec)
        eng.synchronize()
        t1 = time.perf_counter()
        windows.append({
            "tweets_per_s": scored / (t1 - t0),
            "ms_per_batch": (t1 - t0) / args.steps * 1e3,
            "score_call_ms_p50": float(np.median([r[0] for r in rec])),
            "score_ms_p50": float(np.median([r[1] for r in rec])),
            "score_ms_mean": float(np.mean([r[1] for r in rec])),
            "h2d_bytes_per_tweet": (eng.h2d_bytes - b0) / (args.steps * B),
            "scored_per_batch": scored / args.steps,
            "mean_cost": cost / max(1, scored),
        })
    order = sorted(range(len(windows)), key=lambda i: windows[i]["ms_per_batch"])
    med = windows[order[len(order) // 2]]
    out = {
        "metric": "ms per scored k-means batch (one GPU, end to end)",
        "value": round(med["ms_per_batch"], 3),
        "unit": "ms",
        "higher_is_better": False,
        "steps": args.steps, "warmup": args.warmup, "repeat": len(windows),
        "ms_per_batch": round(med["ms_per_batch"], 3),
        "ms_per_batch_windows": [round(w["ms_per_batch"], 3) for w in windows],
        "score_call_ms_p50": round(med["score_call_ms_p50"], 3),
        "score_ms_p50": round(med["score_ms_p50"], 3),
        "score_ms_mean": round(med["score_ms_mean"], 3),
        "score_ms_p50_windows": [round(w["score_ms_p50"], 3) for w in windows],
        "tweets_per_s": round(med["tweets_per_s"], 1),
        "h2d_bytes_per_tweet": round(med["h2d_bytes_per_tweet"], 2),
        "scored_tweets_per_batch": round(med["scored_per_batch"], 1),
        "d2h_bytes_per_scored_tweet": 20,
        "mean_cost": med["mean_cost"],
        "train_ms_of_model_batches": [round(m, 3) for m in train_ms],
        "config": {"batch": B, "k": args.k, "text_dims": args.text_dims, "profile": args.profile,
                   "ingest": "e2e-utf8", "apply_filter": apply_filter, "scaler": args.scaler,
                   "pool_batches": n_pool, "trained_batches": min(args.train, len(raws)),
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

#!/usr/bin/env python
"""Throughput of inference-only scoring, end to end (one GPU).

The flagship stream of ``bench.py`` -- wide profile, 1M tweets per batch,
UTF-8 ingest from a pool of distinct batches whose text is DMA'd from the
receiver's page-locked buffers -- scored instead of trained: per batch the
host staging (row words + packed scalars), the H2D, ``LREngine::score``
(decode / lower-casing, filter, sort, chunk layout, ``csrc/hip/score.hip``)
and the D2H of the fp64 predictions.  A staging thread keeps up to
``raw_slots - 1`` batches submitted ahead of the one being scored, as
``bench.py``'s e2e loop does for training.  The weights come from training
the first 5 pool batches.

Prints one JSON line: tweets/s scored, ms per batch (wall / steps, and the
p50 of the per-batch ``score()`` calls), device ms of the scoring kernels
(events), H2D bytes per tweet.  ``--repeat N`` times the window N times in
one process and reports the median window.

    python tools/score_bench.py [--features 1000000] [--hash java] [--repeat 3]
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=1_000_000, help="numTextFeatures")
    ap.add_argument("--hash", default="java")
    ap.add_argument("--profile", default="wide", choices=["bench", "wide"])
    ap.add_argument("--pool", type=int, default=0, help="distinct batches (default: warmup + steps)")
    ap.add_argument("--train", type=int, default=5, help="pool batches trained for the weights")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeat", type=int, default=1, help="timed windows in this process (median reported)")
    ap.add_argument("--filter", action="store_true", help="score only the rows the training filter keeps")
    ap.add_argument("--json-out", default="")
    return ap.parse_args(argv)


def run_window(eng, raws, u8s, views, first, n, now_ms, apply_filter, record):
    """Score batches first .. first + n - 1 of the stream; a staging thread
    stages + submits (train=False) up to len(views) - 1 batches ahead."""
    e = eng._eng
    free, ready, err = queue.Queue(), queue.Queue(), []
    for s in range(max(1, len(views) - 1)):
        free.put(s)

    def stager():
        try:
            for i in range(first, first + n):
                slot = free.get()
                hb = views[slot].load_utf8(raws[i % len(raws)], u8s[i % len(raws)], copy_text=False)
                e.submit(hb._hb, int(hb.n), int(hb.bytes), slot, int(hb.ext_text), int(now_ms), False)
                ready.put(slot)
        except BaseException as ex:   # surfaced by the main thread
            err.append(ex)
            ready.put(None)

    th = threading.Thread(target=stager, name="stager", daemon=True)
    th.start()
    scored = 0
    for _ in range(n):
        slot = ready.get()
        if slot is None:
            raise err[0]
        t = time.perf_counter()
        res = e.score(slot, int(now_ms), bool(apply_filter))
        dt = (time.perf_counter() - t) * 1e3
        free.put(slot)
        scored += int(res["n_scored"])
        if record is not None:
            record.append((dt, float(res["score_ms"]), float(res["wall_ms"])))
    th.join(timeout=60)
    return scored


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, HostBatchView, LRDeviceConfig
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
                         max_units=max_units, ingest="utf8")
    eng = DeviceLinearRegression(cfg, device=device)
    views = [HostBatchView(B, max_units, text=False) for _ in range(eng.raw_slots)]

    # the model: the first pool batches, trained
    for i in range(min(args.train, len(raws))):
        hb = views[0].load_utf8(raws[i], u8s[i], copy_text=False)
        eng.submit(hb, 0)
        eng.process(0, now_ms)
    eng.synchronize()
    nz = int(np.count_nonzero(eng.get_weights()))

    run_window(eng, raws, u8s, views, 0, args.warmup, now_ms, args.filter, None)
    windows = []
    for k in range(max(1, args.repeat)):
        eng.synchronize()
        torch.cuda.synchronize()
        rec = []
        b0 = eng.h2d_bytes
        t0 = time.perf_counter()
        scored = run_window(eng, raws, u8s, views, args.warmup + k * args.steps, args.steps, now_ms, args.filter, rec)
        eng.synchronize()
        t1 = time.perf_counter()
        raw_rows = args.steps * B
        windows.append({
            "tweets_per_s": scored / (t1 - t0),
            "ms_per_batch": (t1 - t0) / args.steps * 1e3,
            "score_call_ms_p50": float(np.median([r[0] for r in rec])),
            "device_ms_p50": float(np.median([r[1] for r in rec])),
            "device_ms_mean": float(np.mean([r[1] for r in rec])),
            "h2d_bytes_per_tweet": (eng.h2d_bytes - b0) / raw_rows,
            "scored_per_batch": scored / args.steps,
        })
    order = sorted(range(len(windows)), key=lambda i: windows[i]["ms_per_batch"])
    med = windows[order[len(order) // 2]]
    gbps = bench._h2d_gbps(device)
    floor_ms = med["h2d_bytes_per_tweet"] * B / (gbps * 1e9) * 1e3
    out = {
        "metric": "tweets/sec scored (one GPU, end to end)",
        "value": round(med["tweets_per_s"], 1),
        "unit": "tweets/s",
        "higher_is_better": True,
        "steps": args.steps, "warmup": args.warmup, "repeat": len(windows),
        "ms_per_batch": round(med["ms_per_batch"], 3),
        "ms_per_batch_windows": [round(w["ms_per_batch"], 3) for w in windows],
        "score_call_ms_p50": round(med["score_call_ms_p50"], 3),
        "device_ms_scoring_kernels_p50": round(med["device_ms_p50"], 3),
        "device_ms_scoring_kernels_mean": round(med["device_ms_mean"], 3),
        "h2d_bytes_per_tweet": round(med["h2d_bytes_per_tweet"], 2),
        "h2d_gbps_pinned": round(gbps, 2),
        "host_link_floor_ms_per_batch": round(floor_ms, 3),
        "ratio_to_host_link_floor": round(med["ms_per_batch"] / floor_ms, 3) if floor_ms > 0 else None,
        "scored_tweets_per_batch": round(med["scored_per_batch"], 1),
        "config": {"batch": B, "features": args.features, "hash": args.hash, "profile": args.profile,
                   "ingest": "e2e-utf8", "apply_filter": bool(args.filter), "pool_batches": n_pool,
                   "trained_batches": min(args.train, len(raws)), "nonzero_weights": nz,
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

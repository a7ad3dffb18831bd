#!/usr/bin/env python
"""Top-N selection on the device against ``predict_batch`` + a host sort (one GPU).

The pooled batches of ``tools/score_bench.py`` / ``tools/km_score_bench.py`` --
wide profile, 1M tweets per batch, UTF-8 ingest -- under a trained LR model
and a k = 1024 k-means model.  Per batch, already submitted to a raw slot, two
ways to the 100 best rows are timed:

* ``top``: ``engine.top(n)`` -- the scoring kernels, the radix select and sort
  of ``csrc/hip/topn.hip`` behind them, the D2H of the result block;
* ``sort``: ``engine.score()`` (the D2H of every prediction and its copy out of
  the pinned buffer included) and the ``np.lexsort`` of
  ``twitter_stream_ml_amd/models/topn.top_n`` that it replaces.

For both: the call's wall ms (p50), the device ms (events) and the bytes
brought back; the selection's own device time is ``top``'s device ms less
``sort``'s (the same kernels run before it).  One more line of ``top`` with
zero LR weights: every margin 0.0, every lane in one histogram bin, the
selection decided by the index digits alone.

    python tools/top_bench.py [--steps 5] [--n 100] [--json-out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--features", type=int, default=1_000_000, help="numTextFeatures")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--text-dims", type=int, default=62)
    ap.add_argument("--profile", default="wide", choices=["bench", "wide"])
    ap.add_argument("--pool", type=int, default=4, help="distinct batches")
    ap.add_argument("--train", type=int, default=3, help="pool batches trained for the models")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default="")
    return ap.parse_args(argv)


def _p50(xs):
    return round(float(np.median(xs)), 3)


def measure(submit, top, sort, batches, warmup, steps, n):
    """Alternate the two ways over the same batches; returns their p50s."""
    rec = {"top_call": [], "top_dev": [], "sort_call": [], "sort_dev": [], "sort_host": [], "back": [0, 0]}
    for i in range(warmup + steps):
        b = batches[i % len(batches)]
        submit(b)
        t = time.perf_counter()
        r = top()
        t_top = (time.perf_counter() - t) * 1e3
        submit(b)
        t = time.perf_counter()
        values, rows, dev = sort()
        t_mid = time.perf_counter()
        o = np.lexsort((rows, -values))[:n]
        best = rows[o]
        t_sort = (time.perf_counter() - t) * 1e3
        if not np.isnan(values).any():
            assert np.array_equal(best, np.asarray(r["rows"])), "the device selection differs from the host sort"
        if i >= warmup:
            rec["top_call"].append(t_top)
            rec["top_dev"].append(float(r["top_ms"]))
            rec["sort_call"].append(t_sort)
            rec["sort_dev"].append(dev)
            rec["sort_host"].append((time.perf_counter() - t_mid) * 1e3)
            rec["back"] = [8 * (4 + 3 * n), int(values.nbytes + rows.nbytes)]
    return {"top_call_ms_p50": _p50(rec["top_call"]), "top_device_ms_p50": _p50(rec["top_dev"]),
            "sort_call_ms_p50": _p50(rec["sort_call"]), "sort_device_ms_p50": _p50(rec["sort_dev"]),
            "host_lexsort_ms_p50": _p50(rec["sort_host"]),
            "selection_device_ms": round(_p50(rec["top_dev"]) - _p50(rec["sort_dev"]), 3),
            "top_bytes_back": rec["back"][0], "sort_bytes_back": rec["back"][1]}


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, HostBatchView, LRDeviceConfig
    from twitter_stream_ml_amd.sources.synthetic import SynthConfig

    device = 0
    torch.cuda.set_device(device)
    synth = SynthConfig.profile(args.profile, seed=args.seed)
    now_ms = synth.now_ms
    B, n = int(args.batch), int(args.n)
    n_pool = max(args.train, 1, args.pool)
    t_gen = time.time()
    raws, u8s, pinned = bench.utf8_pool(synth, B, n_pool, now_ms)
    for r in raws:
        r.with_scalar_range()
    t_gen = time.time() - t_gen
    max_units = max(r.total_units for r in raws) + 1024
    batches = list(range(len(raws)))
    out = {"metric": "top-N of a scored batch: device selection against predict_batch + host lexsort",
           "n": n, "steps": args.steps, "warmup": args.warmup, "pool_gen_s": round(t_gen, 1),
           "config": {"batch": B, "features": args.features, "k": args.k, "text_dims": args.text_dims,
                      "profile": args.profile, "pool_batches": n_pool, "trained_batches": args.train}}

    # ---- LR -------------------------------------------------------------------
    eng = DeviceLinearRegression(LRDeviceConfig(num_text_features=args.features, num_iterations=args.iters, max_rows=B,
                                                max_units=max_units, ingest="utf8"), device=device)
    view = HostBatchView(B, max_units, text=False)
    e = eng._eng
    for i in range(min(args.train, len(raws))):
        eng.submit(view.load_utf8(raws[i], u8s[i], copy_text=False), 0)
        eng.process(0, now_ms)
    eng.synchronize()

    def lr_submit(i):
        hb = view.load_utf8(raws[i], u8s[i], copy_text=False)
        e.submit(hb._hb, int(hb.n), int(hb.bytes), 0, int(hb.ext_text), int(now_ms), False)

    def lr_sort():
        r = e.score(0, int(now_ms), False)
        return np.asarray(r["pred"]), np.asarray(r["rows"]), float(r["score_ms"])

    out["lr"] = measure(lr_submit, lambda: e.top(0, int(now_ms), False, n, True), lr_sort, batches, args.warmup,
                        args.steps, n)
    eng.set_weights(np.zeros(eng.num_weights))
    out["lr_zero_weights"] = measure(lr_submit, lambda: e.top(0, int(now_ms), False, n, True), lr_sort, batches,
                                     args.warmup, args.steps, n)
    del eng, e
    # ---- k-means ----------------------------------------------------------------
    km = DeviceKMeans(KMDeviceConfig(k=args.k, text_dims=args.text_dims, half_life=5.0, max_rows=B,
                                     max_units=max_units, seed=args.seed), device=device)
    view._hb.scalar_cols = 2   # k-means reads retweetCount and followersCount only
    for i in range(min(args.train, len(raws))):
        km.submit(view.load_utf8(raws[i], u8s[i], copy_text=False), 0)
        km.process(0, want_pred=False)
    km.synchronize()

    def km_sort():
        r = km._eng.score(0, True, 0)
        return np.asarray(r["dist2"]), np.asarray(r["rows"]), float(r["score_ms"])

    out["kmeans"] = measure(lambda i: km.submit(view.load_utf8(raws[i], u8s[i], copy_text=False), 0),
                            lambda: km._eng.top(0, True, 0, None, n, True), km_sort, batches, args.warmup, args.steps, n)
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

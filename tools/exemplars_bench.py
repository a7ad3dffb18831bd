#!/usr/bin/env python
"""Per-cluster exemplars on the device against ``predict_batch`` + a host sort (one GPU).

The pooled batches of ``tools/km_score_bench.py`` / ``tools/top_bench.py`` --
wide profile, 1M tweets per batch, UTF-8 ingest -- under a k = 1024, d = 64
k-means model trained on a few of them.  Per batch and per m (8 and 64 by
default), two ways to the m tweets nearest each centre are timed, each from
the submit of the batch to the arrays on the host:

* ``exemplars``: ``engine.exemplars(m)`` -- the scoring kernels, the tile and
  merge passes of ``csrc/hip/exemplars.hip`` behind them, the D2H of the result
  block (``8 (4 + k + 2 k m)`` bytes);
* ``host``: ``engine.score()`` (the D2H of every row's id, label and distance
  and their copy out of the pinned buffer included: 20 B per row) and the
  ``cluster_top`` of ``twitter_stream_ml_amd/models/exemplars.py`` over them --
  what a user of ``--predictOut`` does today.

For both: the wall ms (p50) and the device ms (events); for ``exemplars`` also
``sel_ms``, the selection kernels alone (events around them).  ``top`` (n = 100,
``csrc/hip/topn.hip``) runs on the same batches for its own selection time
(its device ms less ``score()``'s: the same kernels run before it).  Every
timed batch's device selection is compared with the host's (rows, value bits,
counts).

    python tools/exemplars_bench.py [--steps 5] [--m 8,64] [--json-out FILE]
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
    ap.add_argument("--m", default="8,64", help="comma-separated exemplars per cluster")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--text-dims", type=int, default=62)
    ap.add_argument("--profile", default="wide", choices=["bench", "wide"])
    ap.add_argument("--pool", type=int, default=4, help="distinct batches")
    ap.add_argument("--train", type=int, default=3, help="pool batches trained for the model")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default="")
    return ap.parse_args(argv)


def _p50(xs):
    return round(float(np.median(xs)), 3)


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch  # noqa: F401  (binds the HIP runtime before the engine loads)
    import bench
    from twitter_stream_ml_amd.models.exemplars import cluster_top
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    from twitter_stream_ml_amd.ops.lr_engine import HostBatchView
    from twitter_stream_ml_amd.sources.synthetic import SynthConfig

    device = 0
    torch.cuda.set_device(device)
    synth = SynthConfig.profile(args.profile, seed=args.seed)
    B, k = int(args.batch), int(args.k)
    ms_list = [int(x) for x in str(args.m).split(",") if x]
    n_pool = max(args.train, 1, args.pool)
    t_gen = time.time()
    raws, u8s, pinned = bench.utf8_pool(synth, B, n_pool, synth.now_ms)
    for r in raws:
        r.with_scalar_range()
    t_gen = time.time() - t_gen
    max_units = max(r.total_units for r in raws) + 1024
    out = {"metric": "per-cluster exemplars of a scored batch: device selection against predict_batch + host "
                     "cluster_top", "steps": args.steps, "warmup": args.warmup, "pool_gen_s": round(t_gen, 1),
           "config": {"batch": B, "k": k, "text_dims": args.text_dims, "profile": args.profile,
                      "pool_batches": n_pool, "trained_batches": args.train}}

    km = DeviceKMeans(KMDeviceConfig(k=k, text_dims=args.text_dims, half_life=5.0, max_rows=B, max_units=max_units,
                                     seed=args.seed), device=device)
    view = HostBatchView(B, max_units, text=False)
    view._hb.scalar_cols = 2   # k-means reads retweetCount and followersCount only
    for i in range(min(args.train, len(raws))):
        km.submit(view.load_utf8(raws[i], u8s[i], copy_text=False), 0)
        km.process(0, want_pred=False)
    km.synchronize()
    e = km._eng

    def submit(i):
        km.submit(view.load_utf8(raws[i], u8s[i], copy_text=False), 0)

    for m in ms_list:
        rec = {key: [] for key in ("ex_wall", "ex_dev", "ex_sel", "host_wall", "host_dev", "host_sort", "top_dev")}
        scored = used = 0
        for it in range(args.warmup + args.steps):
            i = it % len(raws)
            t = time.perf_counter()
            submit(i)
            r = e.exemplars(0, True, 0, None, m, False)
            t_ex = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            submit(i)
            s = e.score(0, True, 0)
            t_mid = time.perf_counter()
            c, rows, vals, n_nan = cluster_top(s["dist2"], s["pred"], s["rows"], k=k, m=m)
            t_end = time.perf_counter()
            assert np.array_equal(np.asarray(r["counts"]), c) and np.array_equal(np.asarray(r["rows"]), rows) and \
                np.array_equal(np.asarray(r["values"]).view(np.int64), vals.view(np.int64)) and \
                int(r["n_nan"]) == n_nan, "the device selection differs from the host's"
            submit(i)
            tp = e.top(0, True, 0, None, 100, True)
            if it >= args.warmup:
                rec["ex_wall"].append(t_ex)
                rec["ex_dev"].append(float(r["ex_ms"]))
                rec["ex_sel"].append(float(r["sel_ms"]))
                rec["host_wall"].append((t_end - t) * 1e3)
                rec["host_dev"].append(float(s["score_ms"]))
                rec["host_sort"].append((t_end - t_mid) * 1e3)
                rec["top_dev"].append(float(tp["top_ms"]))
                scored, used = int(r["n_scored"]), int(np.count_nonzero(np.asarray(r["sizes"])))
        out[f"m{m}"] = {
            "exemplars_ms_p50": _p50(rec["ex_wall"]), "exemplars_device_ms_p50": _p50(rec["ex_dev"]),
            "selection_device_ms_p50": _p50(rec["ex_sel"]),
            "host_ms_p50": _p50(rec["host_wall"]), "score_device_ms_p50": _p50(rec["host_dev"]),
            "host_cluster_top_ms_p50": _p50(rec["host_sort"]),
            "top100_device_ms_p50": _p50(rec["top_dev"]),
            "top100_selection_device_ms": round(_p50(rec["top_dev"]) - _p50(rec["host_dev"]), 3),
            "n_scored": scored, "clusters_used": used,
            "exemplars_bytes_back": 8 * (4 + k + 2 * k * m) + 8 * (1 + k), "host_bytes_back": 20 * scored + 8 * (1 + k)}
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

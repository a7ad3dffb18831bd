#!/usr/bin/env python
"""Device cost of one GD iteration, squared loss vs logistic loss (one GPU).

The flagship batches of ``bench.py`` -- wide profile, 1M tweets per batch,
UTF-8 ingest -- trained by two engines that differ only in ``loss``: the same
layout, the same kernels up to the row epilogue (``csrc/hip/sgd.hip``
``row_residual<LOSS>``).  Per batch the engine reports ``train_ms`` (device
time of the GD loop) and the iterations it ran; the figure is ``train_ms /
iterations``, its median over a window of ``--steps`` batches, and the median
of ``--repeat`` windows per loss.  The windows of the two losses alternate in
one process, so both see the same box at the same time.

Prints one JSON line.

    python tools/logistic_bench.py [--steps 6] [--repeat 3] [--features 1000000]
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
    ap.add_argument("--steps", type=int, default=6, help="batches per window (= distinct pool batches)")
    ap.add_argument("--repeat", type=int, default=3, help="windows per loss (median reported)")
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=1_000_000, help="numTextFeatures")
    ap.add_argument("--hash", default="java")
    ap.add_argument("--profile", default="wide", choices=["bench", "wide"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default="")
    return ap.parse_args(argv)


def window(eng, view, raws, u8s, now_ms):
    """Train the pool once from zero weights; per batch (train_ms, iterations)."""
    eng.set_weights(np.zeros(eng.num_weights))
    out = []
    for raw, u8 in zip(raws, u8s):
        hb = view.load_utf8(raw, u8, copy_text=False)
        eng.submit(hb, 0)
        res = eng.process(0, now_ms)
        out.append((float(res["train_ms"]), int(res["iterations"]), bool(res["tiered"])))
    eng.synchronize()
    return out


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
    t_gen = time.time()
    raws, u8s, pinned = bench.utf8_pool(synth, B, max(1, args.steps), now_ms)
    for r in raws:
        r.with_scalar_range()
    t_gen = time.time() - t_gen
    max_units = max(r.total_units for r in raws) + 1024
    base = dict(num_text_features=args.features, hash=args.hash, num_iterations=args.iters, max_rows=B,
                max_units=max_units, ingest="utf8")
    # the step sizes of the two learners' defaults (the linear driver's reference.conf, MLlib's logistic)
    engines = {"squared": DeviceLinearRegression(LRDeviceConfig(loss="squared", step_size=0.005, **base), device),
               "logistic": DeviceLinearRegression(LRDeviceConfig(loss="logistic", step_size=0.1, **base), device)}
    view = HostBatchView(B, max_units, text=False)
    for eng in engines.values():   # warm-up: first launches, lazy allocations
        window(eng, view, raws[:1], u8s[:1], now_ms)
    per = {k: [] for k in engines}
    its = {k: [] for k in engines}
    tiered = set()
    for _ in range(max(1, args.repeat)):
        for name, eng in engines.items():
            w = window(eng, view, raws, u8s, now_ms)
            per[name].append(float(np.median([ms / max(1, it) for ms, it, _ in w])))
            its[name].append([it for _, it, _ in w])
            tiered.update(t for _, _, t in w)
    med = {k: float(np.median(v)) for k, v in per.items()}
    out = {
        "metric": "device ms per GD iteration (train_ms / iterations), logistic vs squared loss",
        "squared_ms_per_iteration": round(med["squared"], 4),
        "logistic_ms_per_iteration": round(med["logistic"], 4),
        "ratio_logistic_to_squared": round(med["logistic"] / med["squared"], 4),
        "windows_ms_per_iteration": {k: [round(x, 4) for x in v] for k, v in per.items()},
        "iterations_per_batch": {k: v[0] for k, v in its.items()},
        "tiered": sorted(tiered),
        "config": {"batch": B, "features": args.features, "hash": args.hash, "profile": args.profile,
                   "steps": args.steps, "repeat": args.repeat, "iters": args.iters},
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

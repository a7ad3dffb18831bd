"""K-means scoring on the GPU (``KMEngine::score``, ``k_km_cost``) against the
fp64 oracle ``CpuKMeans.predict_batch``: clusters, squared distances, cost and
cluster sizes of a raw batch under a model that scoring never changes.

Bounds.  Labels: at most 2 rows per batch may differ from ``find_closest``
among the rows whose best / second gap is resolvable (1e-9 relative) -- the
bound of ``test_gpu_kmeans.py`` for the same assign kernels.  ``dist2``: the
oracle transform is fed the device's own ``std``, then for rows with equal
labels ``|dev - ref| <= 1e-12 (|x|^2 + |c|^2)``: each term's rounding, FMA
contraction included, is below 8 * 2^-53 (x_j^2 + c_j^2), any summation order
of d <= 4002 non-negative terms adds (d - 1) 2^-53 dist2, together below
1e-12 (|x|^2 + |c|^2).  ``cost`` against ``math.fsum``: rtol 1e-9 (n <= 2^20
non-negative terms in any order: n 2^-53).
"""
import functools
import json
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.models.kmeans import CpuKMeans, StreamingKMeansModel, kmeans_features
from twitter_stream_ml_amd.oracle.mllib import KMeansState, standard_scaler_fit, standard_scaler_transform
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu
NOW = 1_700_000_000_000

# k_km_cost's geometry (csrc/hip/kmeans.hip): lanes per row = dp / 4 up to
# dp = 128 (one lane at dp = 2), a whole wave above; a workgroup of 4 waves
# takes 8 groups of rows
COST_WAVES, COST_ITERS, WAVE = 4, 8, 64
# the assign kernels cover 32 points per wave and 128 per block
ASSIGN_SIZES = (0, 1, 2, 31, 32, 33, 127, 128, 129)


def _pad_dim(d):
    return next((p for p in (2, 4, 8, 16, 32, 64, 128) if d <= p), d)


def _cost_rows(dp):
    """(rows per wave, rows per workgroup) of the cost kernel at width dp."""
    lanes = WAVE if dp > 128 else max(1, dp // 4)
    return WAVE // lanes, COST_WAVES * (WAVE // lanes) * COST_ITERS


def _cfg(k, text_dims=0, **kw):
    from twitter_stream_ml_amd.ops.kmeans_engine import KMDeviceConfig
    return KMDeviceConfig(k=k, text_dims=text_dims, max_rows=8192, max_units=8192 * 300, **kw)


def _dev(k, text_dims=0, **kw):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans
    return DeviceKMeans(_cfg(k, text_dims, seed=5, **kw), device=0)


@functools.lru_cache(maxsize=None)
def _batch(rows=4000, t=0, seed=21):
    return generate_batch(SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.2), t * rows, rows,
                          batch_time_ms=NOW + t)


@functools.lru_cache(maxsize=None)
def _features(text_dims):
    X, rows = kmeans_features(_batch(), text_dims)
    X.setflags(write=False)
    return X, rows


def _gaps(Xs, C, rel, chunk=256):
    """Per row: the fp64 closest centre (first index on ties) and whether the
    best / second gap is resolvable (direct squared differences, in chunks)."""
    n, k = Xs.shape[0], C.shape[0]
    best = np.zeros(n, np.int64)
    ok = np.ones(n, bool)
    for s in range(0, n, chunk):
        d = ((Xs[s:s + chunk, None, :] - C[None]) ** 2).sum(axis=2)
        best[s:s + chunk] = np.argmin(d, axis=1)
        if k > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            ok[s:s + chunk] = (two[:, 1] - two[:, 0]) > rel * np.maximum(two[:, 0], 1e-300)
    return best, ok


def _check(res, raw, X, rows, C, apply_filter=True, std_mode="batch", tiny=False):
    """One scored batch against the oracle's parts; returns the share of rows
    the gap mask excluded."""
    k = C.shape[0]
    n = X.shape[0]
    assert res["n_raw"] == raw.n and res["n_scored"] == n
    assert res["rows"].dtype == np.int64 and res["pred"].dtype == np.int32
    assert res["dist2"].dtype == np.float64 and res["sizes"].dtype == np.int64
    np.testing.assert_array_equal(res["rows"], rows)
    pred, dist2 = res["pred"], res["dist2"]
    assert pred.shape == dist2.shape == (n,) and res["sizes"].shape == (k,)
    np.testing.assert_array_equal(res["sizes"], np.bincount(pred, minlength=k))
    if n == 0:
        assert res["cost"] == 0.0 and not res["sizes"].any()
        return 0.0
    if std_mode == "batch":
        np.testing.assert_allclose(res["std"], standard_scaler_fit(X), rtol=1e-6)
    Xs = X if res["std"] is None else standard_scaler_transform(X, res["std"])
    want, ok = _gaps(Xs, C, 1e-9)
    mismatch = np.count_nonzero((pred != want) & ok)
    print(f"k={k} d={X.shape[1]} n={n}: label mismatches {mismatch}, gap-excluded {np.count_nonzero(~ok)}")
    assert mismatch <= 2, mismatch
    if tiny:   # a handful of points: none may differ where fp32 resolves the gap
        assert not np.any((pred != want) & _gaps(Xs, C, 1e-5)[1]), (pred, want)
    same = pred == want
    ref = ((Xs - C[want]) ** 2).sum(axis=1)
    bound = 1e-12 * ((Xs ** 2).sum(axis=1) + (C[want] ** 2).sum(axis=1))
    err = np.abs(dist2 - ref)
    print(f"  dist2 max err / bound {float((err[same] / np.maximum(bound[same], 1e-300)).max()):.3g}")
    assert np.all(err[same] <= bound[same])
    fs = math.fsum(dist2.tolist())
    print(f"  cost {res['cost']!r} fsum {fs!r}")
    assert abs(res["cost"] - fs) <= 1e-9 * fs
    return float(np.count_nonzero(~ok)) / n


# ---- 1. against the oracle ---------------------------------------------------
@pytest.mark.parametrize("k,text_dims,mfma,precision", [
    (1, 0, True, "bf16x3"), (3, 0, False, "bf16x3"), (3, 1, True, "bf16x3"), (31, 14, True, "bf16x3"),
    (33, 14, False, "bf16x3"), (64, 62, True, "fp32"), (200, 126, True, "bf16x3"), (40, 127, True, "bf16x3"),
    (1024, 62, True, "bf16x3")])
def test_score_matches_oracle(hip_module, k, text_dims, mfma, precision):
    dev = _dev(k, text_dims, mfma=mfma, precision=precision)
    C = KMeansState.random(k, 2 + text_dims, 0.0, seed=5).centers
    np.testing.assert_array_equal(dev.get_state()[0], C)
    raw = _batch()
    X, rows = _features(text_dims)
    assert X.shape[0] == 2400
    res = dev.predict_batch(raw)
    excluded = _check(res, raw, X, rows, C)
    assert excluded == 0.0   # no kept row of these nine is within 1e-9 of a tie: the mask excludes nothing
    # the CPU engine gives the same answer through its own scaler
    cpu = CpuKMeans(k, 2 + text_dims, seed=5)
    rc = cpu.predict_batch(raw, text_dims)
    assert np.count_nonzero(rc["pred"] != res["pred"]) <= 2
    np.testing.assert_allclose(res["cost"], rc["cost"], rtol=1e-5)


# ---- 2. edge shapes ------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 16, 17, 64, 128, 129, 1002])
def test_score_edge_shapes(hip_module, d):
    td = d - 2
    dp = _pad_dim(d)
    rows_per_wave, rows_per_wg = _cost_rows(dp)
    assert tuple(hip_module.KMEngine.cost_shape(dp))[1:] == (rows_per_wave, rows_per_wg)
    k = 3 if d == 1002 else 5
    dev = _dev(k, td)
    assert dev._eng.dp == dp
    C = dev.get_state()[0]
    synth = SynthConfig.profile("twitter", seed=27, unicode_fraction=0.2)
    # filtered tiny batches: the assign kernels' sizes (0 = a batch without retweets)
    sizes = (1, 33, 300) if d == 1002 else ASSIGN_SIZES
    for i, m in enumerate(sizes):
        raw = eb.kmeans_tiny_batch(synth, m, 10000 + 400 * i, short_texts=td > 0 and m >= 3)
        X, rows = kmeans_features(raw, td)
        assert X.shape[0] == m
        _check(dev.predict_batch(raw), raw, X, rows, C, tiny=m <= 33)
    # unfiltered: one below, at and one above the cost kernel's rows per wave and per workgroup
    edges = sorted({n for e in (rows_per_wave, rows_per_wg) for n in (e - 1, e, e + 1) if n >= 1})
    assert edges[-1] <= 4000
    for n in edges if d != 1002 else [e for e in edges if e <= 300]:
        raw = _batch().slice(0, n)
        X, rows = kmeans_features(raw, td, apply_filter=False)
        np.testing.assert_array_equal(rows, np.arange(n))
        _check(dev.predict_batch(raw, apply_filter=False), raw, X, rows, C, apply_filter=False, tiny=n <= 33)
    # a zero-variance column: std 0, factor 0
    raw = eb.kmeans_tiny_batch(synth, 5, 20000, equal_followers=True)
    X, rows = kmeans_features(raw, td)
    res = dev.predict_batch(raw)
    assert res["std"][1] == 0 and res["std"][0] > 0
    _check(res, raw, X, rows, C, tiny=True)
    # no rows at all: nothing touches the device
    empty = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    res = dev.predict_batch(empty)
    assert res["n_raw"] == 0 and res["n_scored"] == 0 and res["cost"] == 0.0 and res["std"] is None
    assert res["rows"].shape == res["pred"].shape == res["dist2"].shape == (0,) and not res["sizes"].any()
    np.testing.assert_array_equal(dev.get_state()[0], C)


# ---- 3. a row's bits depend on the row alone -----------------------------------------
def _by_row(res):
    return {int(r): (int(p), float(d).hex()) for r, p, d in zip(res["rows"], res["pred"], res["dist2"])}


@pytest.mark.parametrize("k,text_dims", [(33, 14), (64, 62), (5, 0), (7, 200)])
def test_score_row_determinism(hip_module, k, text_dims):
    dev = _dev(k, text_dims)
    raw = _batch()
    cut = 1777
    std = standard_scaler_fit(_features(text_dims)[0])
    for scaler in (std, "none"):
        whole = dev.predict_batch(raw, scaler=scaler)
        again = dev.predict_batch(raw, scaler=scaler)
        for key in ("rows", "pred", "dist2", "sizes"):
            np.testing.assert_array_equal(whole[key], again[key])
        assert float(whole["cost"]).hex() == float(again["cost"]).hex()
        full = _by_row(whole)
        assert len(full) == 2400
        lo = dev.predict_batch(raw.slice(0, cut), scaler=scaler)
        hi = dev.predict_batch(raw.slice(cut, raw.n), scaler=scaler)
        halves = _by_row(lo)
        halves.update({r + cut: v for r, v in _by_row(hi).items()})
        assert halves == full
        every = _by_row(dev.predict_batch(raw, apply_filter=False, scaler=scaler))
        assert len(every) == raw.n
        assert {r: every[r] for r in full} == full


# ---- 4. the model is untouched ---------------------------------------------------------
def test_score_leaves_model_and_training_alone(hip_module):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans
    k, td = 64, 30
    a = DeviceKMeans(_cfg(k, td, seed=5), device=0)
    b = DeviceKMeans(_cfg(k, td, seed=5), device=0)
    warm = [_batch(4000, t, seed=33) for t in range(3)]   # split centres and near ties are present
    for raw in warm:
        a.update_raw(raw)
        b.update_raw(raw)
    train = [_batch(4000, t, seed=8) for t in range(4)]
    other = [_batch(3000, t, seed=9) for t in range(5)]
    c0, w0 = b.get_state()
    r0 = b.predict_batch(other[0])
    c1, w1 = b.get_state()
    assert c0.tobytes() == c1.tobytes() and w0.tobytes() == w1.tobytes()
    assert r0["n_scored"] > 0
    for t, raw in enumerate(train):
        ra = a.update_raw(raw)
        b.predict_batch(other[t], scaler="none" if t % 2 else "batch")
        if t == 2:   # between the prefetch of a batch and the update that consumes it
            assert b.prefetch(raw)
            b.predict_batch(other[4], apply_filter=False)
            assert b._pipe.in_flight == 1
        rb = b.update_raw(raw)
        if t == 2:
            assert b._pipe.hits == 1
        np.testing.assert_array_equal(ra["std"], rb["std"])
        np.testing.assert_array_equal(np.asarray(ra["pred"]), np.asarray(rb["pred"]))
        (ca, wa), (cb, wb) = a.get_state(), b.get_state()
        assert ca.tobytes() == cb.tobytes() and wa.tobytes() == wb.tobytes()
    # device against device: scoring after training equals a fresh engine given the same state
    c = DeviceKMeans(_cfg(k, td, seed=5), device=0)
    c.set_state(*a.get_state())
    rb, rc = b.predict_batch(other[1]), c.predict_batch(other[1])
    for key in ("rows", "pred", "dist2", "sizes", "std"):
        np.testing.assert_array_equal(rb[key], rc[key])
    assert rb["cost"] == rc["cost"]


# ---- 5. no collective --------------------------------------------------------------------
def test_score_issues_no_collective(hip_module):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans
    k, td = 64, 14
    comm = hip_module.Comm(hip_module.rccl_unique_id(), 0, 1, 0)
    dp = DeviceKMeans(_cfg(k, td, seed=3, force_dp=True), device=0, comm=comm)
    plain = DeviceKMeans(_cfg(k, td, seed=3), device=0)
    raw = _batch()
    for e in (dp, plain):
        e.update_raw(_batch(4000, 1, seed=8))
    before = dict(comm.counters())
    assert before["allreduce_calls"] >= 3
    for kw in ({}, {"apply_filter": False}, {"scaler": "none"}):
        ra, rb = dp.predict_batch(raw, **kw), plain.predict_batch(raw, **kw)
        for key in ("rows", "pred", "dist2", "sizes"):
            np.testing.assert_array_equal(ra[key], rb[key])
        assert ra["cost"] == rb["cost"] and ra["n_scored"] > 0
        if ra["std"] is not None:
            np.testing.assert_array_equal(ra["std"], rb["std"])
    assert dict(comm.counters()) == before


# ---- 6. the driver -----------------------------------------------------------------------
def test_score_driver_gpu_matches_cpu(hip_module, tmp_path):
    from twitter_stream_ml_amd.apps import score as score_app
    from twitter_stream_ml_amd.sources import write_jsonl
    k, td = 33, 14
    st = KMeansState.random(k, 2 + td, 0.0, seed=5)
    ck = tmp_path / "km"
    StreamingKMeansModel(st.centers, np.ones(k)).save(str(ck))
    raw = _batch()
    write_jsonl(str(tmp_path / "stream.jsonl"), raw.to_statuses())
    out = {}
    for master in ("local[2]", "rocm[1]"):
        out[master] = tmp_path / master.split("[")[0]
        args = ["--master", master, "--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
                "--source", f"replay:{tmp_path / 'stream.jsonl'}", "--seconds", "0", "--batchSize", "4000",
                "--sourceRate", "0", "--numBatches", "1", "--model", str(ck), "--predictOut", str(out[master])]
        assert score_app.main(args) == 0
    rec = {m: json.loads(open(p / "predictions.jsonl").readline()) for m, p in out.items()}
    cpu, gpu = out["local[2]"], out["rocm[1]"]
    np.testing.assert_array_equal(np.load(gpu / "rows_0.npy"), np.load(cpu / "rows_0.npy"))
    pc, pg = np.load(cpu / "pred_0.npy"), np.load(gpu / "pred_0.npy")
    assert pg.dtype == np.int32 and pg.shape == (2400,) and np.load(gpu / "dist2_0.npy").dtype == np.float64
    assert np.count_nonzero(pc != pg) <= 2
    assert rec["rocm[1]"]["count"] == rec["local[2]"]["count"] == 2400
    np.testing.assert_allclose(rec["rocm[1]"]["cost"], rec["local[2]"]["cost"], rtol=1e-5)
    assert rec["rocm[1]"]["clusters_used"] == np.unique(pg).size
    assert rec["rocm[1]"]["score_ms"] > 0

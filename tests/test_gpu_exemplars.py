"""Per-cluster exemplars on the device (``csrc/hip/exemplars.hip``,
``KMEngine::exemplars``, ``DeviceKMeans.exemplars_batch``) against the host
contract ``models/exemplars.cluster_top``.

Equality here means the same value bits, the same rows in the same order, the
same counts and the same ``n_nan``: the selection is exact (unique composite
keys, full sorts, integer atomics for placement only), so nothing is compared
within a tolerance.
"""
import gc
import json
import zlib

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.models.exemplars import EXEMPLARS_MAX, EXEMPLARS_MAX_CELLS, cluster_top
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
SELECT_ROWS = 1 << 18          # capacity of the kernel-test engine: the largest input is 2^18 doubles


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _assert_ex(got, values, labels, rows, k, m, largest, what):
    c, r, v, n_nan = cluster_top(values, labels, rows, k=k, m=m, largest=largest)
    assert got["counts"].dtype == np.int64 and got["rows"].dtype == np.int64 and got["values"].dtype == np.float64
    assert got["rows"].shape == got["values"].shape == (k, m) and got["counts"].shape == (k,), what
    assert got["n_nan"] == n_nan, (what, got["n_nan"], n_nan)
    np.testing.assert_array_equal(got["counts"], c, err_msg=str(what))
    np.testing.assert_array_equal(got["rows"], r, err_msg=str(what))
    np.testing.assert_array_equal(_bits(got["values"]), _bits(v), err_msg=str(what))


# ---- the kernels alone ---------------------------------------------------------

@pytest.fixture(scope="module")
def sel(hip_module):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    eng = DeviceKMeans(KMDeviceConfig(k=3, text_dims=0, max_rows=SELECT_ROWS, max_units=SELECT_ROWS * 2), device=0)
    info = eng._eng.debug_cluster_select(np.zeros(1), np.zeros(1, np.int32), None, 1, 1, False)
    T, C = int(info["tile"]), int(info["chunk"])
    assert T * (C // EXEMPLARS_MAX + 2) <= SELECT_ROWS

    def run(values, labels, rows, k, m, largest):
        return eng._eng.debug_cluster_select(np.ascontiguousarray(values, np.float64),
                                             np.ascontiguousarray(labels, np.int32), rows, int(k), int(m),
                                             bool(largest))

    def check(values, labels, rows, k, m, largest, what):
        got = run(values, labels, rows, k, m, largest)
        _assert_ex(got, values, labels, rows, k, m, largest, what)
        assert got["n_scored"] == len(values), what
        return got

    return {"run": run, "check": check, "tile": T, "chunk": C,
            "sizes": [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5000]}


def _random_values(rng, n):
    return rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))


def test_select_row_counts_k_and_m(sel):
    """Every row count x a k of each kind x m x both directions, random values
    and labels (many clusters stay empty once k passes n)."""
    rng = np.random.default_rng(zlib.crc32(b"counts"))
    for n in sel["sizes"]:
        for k in (1, 2, 33, 1024):
            labels = rng.integers(0, k, n)
            values = _random_values(rng, n)
            for m in (1, 2, 63, 64):
                for largest in (False, True):
                    sel["check"](values, labels, None, k, m, largest, ("counts", n, k, m, largest))


def test_select_every_k(sel):
    rng = np.random.default_rng(zlib.crc32(b"k"))
    n = 5000
    values = np.round(_random_values(rng, n), 1)   # ties
    for k in (1, 2, 31, 32, 33, 65, 1024):
        labels = rng.integers(0, k, n)
        for m, largest in ((1, True), (7, False), (64, False)):
            sel["check"](values, labels, None, k, m, largest, ("k", k, m, largest))
    # k > n, every row its own cluster, in a scattered order; the most clusters m = 1 allows
    for k, n in ((5003, 5000), (EXEMPLARS_MAX_CELLS, 3000)):
        labels = rng.permutation(k)[:n]
        v = _random_values(rng, n)
        got = sel["check"](v, labels, None, k, 1, False, ("own cluster", k))
        assert int(got["counts"].sum()) == n
    got = sel["check"](v[:40], labels[:40] % 4096, None, 4096, 64, True, ("k m at the limit", 4096))


def test_select_label_layouts(sel):
    rng = np.random.default_rng(zlib.crc32(b"layouts"))
    T = sel["tile"]
    n = 2 * T + 777
    values = np.round(_random_values(rng, n), 2)
    k = 37
    asc = np.sort(rng.integers(0, k, n))
    layouts = {"ascending": asc, "descending": asc[::-1].copy(), "interleaved": np.arange(n) % k,
               "many empty": rng.choice([3, 500, 501, 1023], n), "two of k": rng.choice([0, k - 1], n)}
    # one cluster's run straddles the tile boundary: rows T - 40 .. T + 40 are cluster 5's only rows
    straddle = np.where(np.arange(n) < T, 1, 9)
    straddle[T - 40:T + 40] = 5
    layouts["straddle"] = straddle
    for name, labels in layouts.items():
        kk = 1024 if name == "many empty" else k
        for m in (1, 2, 63, 64):
            for largest in (False, True):
                sel["check"](values, labels, None, kk, m, largest, (name, m, largest))
    # m around a chosen cluster's size
    labels = np.arange(n) % k
    labels[labels == 4] = 3
    labels[:50][::2] = 4           # cluster 4 has 25 rows
    size = int(np.count_nonzero(labels == 4))
    assert size == 25
    for m in (size - 1, size, size + 1):
        for largest in (False, True):
            got = sel["check"](values, labels, None, k, m, largest, ("size_c", m, largest))
            assert got["counts"][4] == min(m, size)


def test_select_chunk_refill(sel):
    """One cluster's candidates exceed a merge chunk: every row carries one
    label, m = 64, so every tile sends 64 candidates and the merge workgroup
    refills its chunk more than once."""
    T, C = sel["tile"], sel["chunk"]
    n = T * (C // 64 + 2)
    assert (n // T) * 64 > C               # a second round of the refill loop
    rng = np.random.default_rng(zlib.crc32(b"refill"))
    values = np.round(rng.standard_normal(n) * 1000.0) / 16.0   # ties across tiles
    for k, lab in ((1, 0), (9, 6)):
        labels = np.full(n, lab)
        for largest in (False, True):
            sel["check"](values, labels, None, k, 64, largest, ("refill", k, largest))
    # the whole capacity: a third round (after the first chunk a refill brings chunk - 64)
    big = SELECT_ROWS
    assert (big // T) * 64 > 2 * C - 64
    vb = np.round(rng.standard_normal(big) * 1000.0) / 16.0
    sel["check"](vb, np.full(big, 2), None, 3, 64, False, "refill, three rounds")
    # the best rows sit in the last tiles: they arrive in a refill
    v2 = np.arange(n, 0, -1, dtype=np.float64)
    sel["check"](v2, np.zeros(n, np.int64), None, 1, 64, False, "refill, best last")
    sel["check"](v2, np.zeros(n, np.int64), None, 1, 64, True, "refill, best first")


def test_select_ties(sel):
    T = sel["tile"]
    rng = np.random.default_rng(zlib.crc32(b"ties"))
    for n in (65, T, 2 * T + 1, 5000):
        for k in (1, 3):
            labels = rng.integers(0, k, n)
            for c in (0.0, 0.75, -3.5):   # all equal: the lowest rows of each cluster
                for m, largest in ((1, False), (2, True), (64, False)):
                    got = sel["check"](np.full(n, c), labels, None, k, m, largest, ("all equal", n, k, c, m))
                    first = np.flatnonzero(labels == 0)[:m]
                    np.testing.assert_array_equal(got["rows"][0, :first.size], first)
    # a tie group straddling the m cut inside one tile, and one split over two tiles: the lower rows win
    n = 2 * T
    for lo, hi in ((100, 140), (T - 30, T + 30)):
        for largest in (False, True):
            v = rng.random(n) + 1.0          # in [1, 2)
            best = 3.0 if largest else 0.5
            v[lo:hi] = best
            for m in (1, 10, 30, 39, 40, 41, 64):
                for k, labels in ((1, np.zeros(n, np.int64)), (2, np.arange(n) % 2)):
                    got = sel["check"](v, labels, None, k, m, largest, ("tie straddle", lo, m, k, largest))
                    want = np.arange(lo, hi)[labels[lo:hi] == 0][:m]
                    np.testing.assert_array_equal(got["rows"][0, :want.size], want)


def test_select_special_values(sel):
    T = sel["tile"]
    rng = np.random.default_rng(zlib.crc32(b"special"))
    pools = {"+-0": np.array([0.0, -0.0, 1.0, -1.0]),
             "+-inf": np.array([np.inf, -np.inf, 0.0, 1e308, -1e308, np.finfo(np.float64).max]),
             "subnormals": np.array([5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0, 1e-310,
                                     -1e-310, 1e-320]),
             "one ulp": np.array([1.5, np.nextafter(1.5, 2.0), np.nextafter(1.5, 1.0), -1.5, np.nextafter(-1.5, 0.0)])}
    for name, pool in pools.items():
        for n in (2, 65, T + 1, 5000):
            for k in (1, 5):
                labels = rng.integers(0, k, n)
                v = pool[rng.integers(0, pool.size, n)]
                for m, largest in ((1, False), (3, True), (64, False), (64, True)):
                    sel["check"](v, labels, None, k, m, largest, (name, n, k, m, largest))
    # only zeros: -0.0 == +0.0, so the rows decide, and the bits are kept
    v = np.array([0.0, -0.0] * 40)
    for largest in (False, True):
        got = sel["check"](v, np.zeros(80, np.int64), None, 1, 7, largest, "zeros")
        np.testing.assert_array_equal(got["rows"][0], np.arange(7))
        np.testing.assert_array_equal(_bits(got["values"][0]), _bits(v[:7]))


def test_select_nans(sel):
    T = sel["tile"]
    nans = np.array([0x7FF8000000000000, -0x0008000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF],
                    np.int64).view(np.float64)
    assert np.isnan(nans).all()
    rng = np.random.default_rng(zlib.crc32(b"nans"))
    for n in (1, 64, 65, T + 1, 5000):
        k = 6
        labels = rng.integers(0, k, n)
        v = rng.standard_normal(n)
        hit = rng.random(n) < 0.3
        v[hit] = nans[rng.integers(0, nans.size, int(hit.sum()))]
        v[labels == 2] = nans[rng.integers(0, nans.size, int((labels == 2).sum()))]   # a cluster that is all NaN
        for m, largest in ((1, False), (5, True), (64, False)):
            got = sel["check"](v, labels, None, k, m, largest, ("NaNs", n, m, largest))
            assert got["counts"][2] == 0 and (got["rows"][2] == -1).all()
    got = sel["check"](np.full(T + 1, np.nan), np.zeros(T + 1, np.int64), None, 2, 64, False, "all NaN")
    assert got["n_nan"] == T + 1 and not got["counts"].any()


def test_select_given_rows(sel):
    rng = np.random.default_rng(zlib.crc32(b"rows"))
    T = sel["tile"]
    for n in (1, 65, 2 * T + 1):
        rows = np.cumsum(rng.integers(1, 5, n)).astype(np.int64) + 11
        v = np.round(rng.standard_normal(n) * 3.0)   # ties, so the given rows decide
        labels = rng.integers(0, 4, n)
        for m, largest in ((1, False), (9, True), (64, False)):
            sel["check"](v, labels, rows, 4, m, largest, ("rows", n, m, largest))


def test_select_is_bit_identical_across_calls(sel):
    rng = np.random.default_rng(8)
    n = 3 * sel["tile"] + 5
    v = np.round(rng.standard_normal(n) * 50.0) / 8.0
    labels = rng.integers(0, 40, n)
    other = rng.standard_normal(5000)
    for m, lg in ((5, False), (64, True)):
        a = sel["run"](v, labels, None, 40, m, lg)
        b = sel["run"](v, labels, None, 40, m, lg)
        sel["run"](other, np.zeros(5000, np.int32), None, 3, 64, not lg)
        c = sel["run"](v, labels, None, 40, m, lg)
        for r in (b, c):
            np.testing.assert_array_equal(r["rows"], a["rows"])
            np.testing.assert_array_equal(_bits(r["values"]), _bits(a["values"]))
            np.testing.assert_array_equal(r["counts"], a["counts"])
            assert r["n_nan"] == a["n_nan"]


def test_select_limits(sel):
    z, l = np.zeros(8), np.zeros(8, np.int32)
    for k, m in ((1, 0), (1, -1), (1, EXEMPLARS_MAX + 1), (EXEMPLARS_MAX_CELLS + 1, 1), (4097, 64), (0, 1)):
        with pytest.raises(ValueError):
            sel["run"](z, l, None, k, m, False)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            sel["run"](z, np.full(8, bad, np.int32), None, 3, 1, False)


# ---- the engine --------------------------------------------------------------------

def _km(k, text_dims, **kw):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, "seed": 5, **kw}
    return DeviceKMeans(KMDeviceConfig(k=k, text_dims=text_dims, **kw), device=0)


def _assert_batch(got, pb, k, m, largest, what):
    _assert_ex(got, pb["dist2"], pb["pred"], pb["rows"], k, m, largest, what)
    assert got["dist2"] is got["values"]
    assert np.float64(got["cost"]).view(np.int64) == np.float64(pb["cost"]).view(np.int64), what
    np.testing.assert_array_equal(got["sizes"], pb["sizes"])
    assert (got["n_raw"], got["n_scored"]) == (pb["n_raw"], pb["n_scored"]), what
    if pb["std"] is None:
        assert got["std"] is None
    else:
        np.testing.assert_array_equal(got["std"], pb["std"])


# the nine grid cases of tests/test_gpu_kmeans_score.py: d = 2, a padded d, d = 129 (the unpadded path above 128
# columns), the fp32 and the scalar assign paths, k > n
@pytest.mark.parametrize("k,text_dims,mfma,precision", [
    (1, 0, True, "bf16x3"), (3, 0, False, "bf16x3"), (3, 1, True, "bf16x3"), (31, 14, True, "bf16x3"),
    (33, 14, False, "bf16x3"), (64, 62, True, "fp32"), (200, 126, True, "bf16x3"), (40, 127, True, "bf16x3"),
    (1024, 62, True, "bf16x3")])
def test_exemplars_equal_own_predict_batch(hip_module, k, text_dims, mfma, precision):
    big = generate_batch(SynthConfig.profile("twitter", seed=21, unicode_fraction=0.2), 0, 4000, batch_time_ms=NOW)
    eng = _km(k, text_dims, mfma=mfma, precision=precision)
    eng.update_raw(big.slice(0, 2000), want_pred=False)   # centres off the initial ones
    c0, w0 = eng.get_state()
    frozen = np.linspace(0.5, 2.0, 2 + text_dims)
    ms = [m for m in (1, 5, 64) if k * m <= EXEMPLARS_MAX_CELLS]
    for rows in (1, 2, 31, 32, 33, 127, 128, 129, 4000):   # the assign kernels' 32 / 128 points; fewer rows than k
        raw = big.slice(0, rows)
        for scaler in ("none", frozen, "batch"):
            for filt in (True, False):
                pb = eng.predict_batch(raw, scaler=scaler, apply_filter=filt)
                assert pb["n_scored"] == rows if not filt else pb["n_scored"] <= rows
                for m in ms:
                    for lg in (False, True):
                        got = eng.exemplars_batch(raw, m, largest=lg, scaler=scaler, apply_filter=filt)
                        _assert_batch(got, pb, k, m, lg, (k, text_dims, rows, m, lg, filt))
                        assert got["n_nan"] == 0
    c1, w1 = eng.get_state()
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(w0, w1)
    got = eng.exemplars_batch(big, 3)
    assert got["ex_ms"] > 0 and got["wall_ms"] > 0 and 0 < got["sel_ms"] <= got["ex_ms"]
    # nothing kept (no retweets) and no rows
    none = eb.texts_to_raw([big.text_of(i) for i in range(50)], np.zeros(50, np.uint8), big.scalars[:, :50], NOW)
    got = eng.exemplars_batch(none, 5)
    assert got["n_raw"] == 50 and got["n_scored"] == 0 and got["cost"] == 0.0 and not got["counts"].any()
    assert (got["rows"] == -1).all() and got["rows"].shape == (k, 5) and not got["values"].any()
    h2d = eng.h2d_bytes
    got = eng.exemplars_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)), 5)
    assert got["n_raw"] == got["n_scored"] == 0 and got["sizes"].shape == (k,) and got["rows"].shape == (k, 5)
    assert eng.h2d_bytes == h2d
    with pytest.raises(ValueError, match="predict_batch"):
        eng.exemplars_batch(big, EXEMPLARS_MAX + 1)
    with pytest.raises(ValueError):
        eng.exemplars_batch(big, 0)


def test_exemplars_leave_training_alone(hip_module):
    k, td = 64, 30
    a, b = _km(k, td), _km(k, td)
    synth = lambda seed: SynthConfig.profile("twitter", seed=seed, unicode_fraction=0.2)
    train = [generate_batch(synth(8), t * 4000, 4000, batch_time_ms=NOW + t) for t in range(4)]
    other = [generate_batch(synth(9), t * 3000, 3000, batch_time_ms=NOW + t) for t in range(5)]
    for t, raw in enumerate(train):
        ra = a.update_raw(raw)
        c0, w0 = b.get_state()
        got = b.exemplars_batch(other[t], 1 + 9 * t, largest=bool(t % 2), scaler="none" if t % 2 else "batch")
        c1, w1 = b.get_state()
        assert c0.tobytes() == c1.tobytes() and w0.tobytes() == w1.tobytes() and got["n_scored"] > 0
        if t == 2:   # between the prefetch of a batch and the update that consumes it
            assert b.prefetch(raw)
            b.exemplars_batch(other[4], 64, apply_filter=False)
            assert b._pipe.in_flight == 1
        rb = b.update_raw(raw)
        if t == 2:
            assert b._pipe.hits == 1
        np.testing.assert_array_equal(ra["std"], rb["std"])
        np.testing.assert_array_equal(np.asarray(ra["pred"]), np.asarray(rb["pred"]))
        (ca, wa), (cb, wb) = a.get_state(), b.get_state()
        assert ca.tobytes() == cb.tobytes() and wa.tobytes() == wb.tobytes()


def test_exemplars_issue_no_collective(hip_module):
    k, td = 64, 14
    comm = hip_module.Comm(hip_module.rccl_unique_id(), 0, 1, 0)
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    cfg = dict(k=k, text_dims=td, max_rows=8192, max_units=8192 * 300, seed=3)
    dp = DeviceKMeans(KMDeviceConfig(force_dp=True, **cfg), device=0, comm=comm)
    plain = DeviceKMeans(KMDeviceConfig(**cfg), device=0)
    synth = SynthConfig.profile("twitter", seed=21, unicode_fraction=0.2)
    raw = generate_batch(synth, 0, 4000, batch_time_ms=NOW)
    for e in (dp, plain):
        e.update_raw(generate_batch(synth, 4000, 4000, batch_time_ms=NOW + 1))
    before = dict(comm.counters())
    assert before["allreduce_calls"] >= 3
    for kw in ({}, {"apply_filter": False}, {"scaler": "none", "largest": True}):
        ra, rb = dp.exemplars_batch(raw, 8, **kw), plain.exemplars_batch(raw, 8, **kw)
        for key in ("counts", "rows", "sizes"):
            np.testing.assert_array_equal(ra[key], rb[key])
        np.testing.assert_array_equal(_bits(ra["values"]), _bits(rb["values"]))
        assert ra["cost"] == rb["cost"] and ra["n_scored"] > 0
    assert dict(comm.counters()) == before


def test_exemplars_lifecycle(hip_module):
    gc.collect()
    hip_module.teardown_errors()
    before = hip_module.device_bytes_live()
    km = _km(8, 4)
    raw = generate_batch(SynthConfig.profile("twitter", seed=2), 0, 500, batch_time_ms=NOW)
    km.update_raw(raw)
    km.predict_batch(raw)
    base = hip_module.device_bytes_live()
    assert km.exemplars_batch(raw, 10)["n_scored"] > 0
    grown = hip_module.device_bytes_live()
    # 12 B per row of capacity for the candidates, the scan, the cursors and the result block of k x 64
    assert base < grown <= base + 8192 * 12 + (1 << 16)
    km.exemplars_batch(raw, 64, largest=True)
    km.exemplars_batch(raw, 1, apply_filter=False)
    assert hip_module.device_bytes_live() == grown    # ... by the first call only
    del km
    gc.collect()
    assert hip_module.device_bytes_live() == before
    assert list(hip_module.teardown_errors()) == []


# ---- the driver --------------------------------------------------------------------

def test_score_driver_exemplars_rocm_equals_local(hip_module, tmp_path):
    """``twtml-score --exemplars`` on ``rocm[1]`` against ``local[1]`` over the
    recorded stream of ``test_gpu_topn.py``'s driver test.  The two engines'
    labels agree on every row of it (asserted from ``--predictOut`` of the same
    runs), so both name the same clusters, sizes, rows and texts in the same
    order; the distances are each engine's own (fp64 sums in different orders),
    compared within the bound of ``test_gpu_kmeans_score.py``."""
    from twitter_stream_ml_amd.apps import score as score_app
    from twitter_stream_ml_amd.models.kmeans import StreamingKMeansModel
    from twitter_stream_ml_amd.oracle.mllib import KMeansState
    k, td = 6, 14
    st = KMeansState.random(k, 2 + td, 0.0, seed=5)
    model = tmp_path / "km"
    StreamingKMeansModel(st.centers, np.ones(k)).save(str(model))
    std = tmp_path / "std.npy"
    np.save(std, np.linspace(0.5, 2.0, 2 + td))
    out = {}
    for master in ("local[1]", "rocm[1]"):
        out[master] = tmp_path / master.replace("[", "_").replace("]", "")
        args = ["--master", master, "--model", str(model), "--exemplars", "5", "--exemplarsOut", str(out[master]),
                "--predictOut", str(out[master] / "pred"), "--scalerStd", str(std),
                "--source", "replay:synthetic:twitter:3", "--batchSize", "900", "--seconds", "0", "--sourceRate", "0",
                "--numBatches", "3", "--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]
        assert score_app.main(args) == 0
    cpu, gpu = out["local[1]"], out["rocm[1]"]
    for t in range(3):
        np.testing.assert_array_equal(np.load(gpu / "pred" / f"rows_{t}.npy"), np.load(cpu / "pred" / f"rows_{t}.npy"))
        np.testing.assert_array_equal(np.load(gpu / "pred" / f"pred_{t}.npy"), np.load(cpu / "pred" / f"pred_{t}.npy"))

    def strip(rec):
        for key in ("ms", "ex_ms", "batch_time_ms", "cost"):
            rec.pop(key, None)
        d2 = [e.pop("dist2") for c in rec["clusters"] for e in c["entries"]]
        return rec, np.array(d2)

    lc = [strip(json.loads(l)) for l in open(cpu / "exemplars.jsonl")]
    lg = [strip(json.loads(l)) for l in open(gpu / "exemplars.jsonl")]
    assert len(lg) == 3 and all(r["n_scored"] > 100 and r["clusters"] for r, _ in lg)
    for (g, dg), (c, dc) in zip(lg, lc):
        assert g == c, g["seq"]
        np.testing.assert_allclose(dg, dc, rtol=1e-9)
    sc, sg = json.load(open(cpu / "summary.json")), json.load(open(gpu / "summary.json"))
    assert sg["scaler"] == sc["scaler"] == "given"
    for cg, cc in zip(sg["clusters"], sc["clusters"]):
        assert cg["label"] == cc["label"]
        assert [(e["seq"], e["row"], e["text"]) for e in cg["entries"]] == \
            [(e["seq"], e["row"], e["text"]) for e in cc["entries"]]

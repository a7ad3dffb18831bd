"""Top-N selection on the device (``csrc/hip/topn.hip``, ``LREngine::top``,
``KMEngine::top``, ``Device*.top_batch``) against the host contract
``models/topn.top_n``.

Equality here means the same value bits and the same rows in the same order:
the selection is exact (integer histograms, unique composite keys, a full sort
of the selected entries), so nothing is compared within a tolerance.
"""
import gc
import json
import zlib

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.models.topn import TOPN_MAX, top_n
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
F = 1000
SIZES = [1, 2, 63, 64, 65, 1025, 5000]
NS = [1, 2, 63, 64, 65, TOPN_MAX]
SELECT_ROWS = 66000            # capacity of the kernel-test engine: past one full grid pass


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _assert_top(got, values, rows, n, largest, what):
    v, r, n_nan = top_n(values, rows, n, largest)
    assert got["n_top"] == v.size == min(n, len(values) - n_nan), (what, got["n_top"], v.size)
    assert got["n_nan"] == n_nan, what
    assert got["rows"].dtype == np.int64 and got["values"].dtype == np.float64
    np.testing.assert_array_equal(got["rows"], r, err_msg=str(what))
    np.testing.assert_array_equal(_bits(got["values"]), _bits(v), err_msg=str(what))


# ---- the kernels alone ---------------------------------------------------------

@pytest.fixture(scope="module")
def sel(hip_module):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    eng = DeviceLinearRegression(LRDeviceConfig(num_text_features=F, max_rows=SELECT_ROWS,
                                                max_units=SELECT_ROWS * 16), device=0)
    info = eng._eng.debug_top_select(np.zeros(1), None, 1, True)
    past_grid = int(info["max_grid"]) * int(info["block"]) + 321
    assert past_grid <= SELECT_ROWS
    shifts = np.cumsum([0] + list(info["digit_bits"])[::-1])[:-1][::-1]   # lowest bit of each value-key digit
    assert int(sum(info["digit_bits"])) == 64

    def run(values, rows, n, largest):
        return eng._eng.debug_top_select(np.ascontiguousarray(values, np.float64), rows, int(n), bool(largest))

    return {"run": run, "past_grid": past_grid, "digit_low_bits": [int(s) for s in shifts]}


def _n_values(cnt, big):
    ns = {1, 64, TOPN_MAX} if big else set(NS) | {cnt - 1, cnt, cnt + 1}
    return sorted(n for n in ns if 1 <= n <= TOPN_MAX)


def _sweep(sel, make, what, sizes=None):
    """Every size x n x direction of one kind of input; make(cnt, n, largest,
    rng) -> values or (values, rows)."""
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    for cnt in (sizes or SIZES + [sel["past_grid"]]):
        for n in _n_values(cnt, cnt > SIZES[-1]):
            for largest in (True, False):
                made = make(cnt, n, largest, rng)
                values, rows = made if isinstance(made, tuple) else (made, None)
                got = sel["run"](values, rows, n, largest)
                _assert_top(got, values, rows, n, largest, (what, cnt, n, largest))
                assert got["n_scored"] == cnt


def test_select_random(sel):
    _sweep(sel, lambda cnt, n, lg, rng: rng.standard_normal(cnt) * np.exp2(rng.integers(-30, 30, cnt)), "random")


def test_select_all_equal(sel):
    """A fresh model scores every row 0.0: the answer is rows 0 .. n-1, found
    by the index digits alone."""
    for c in (0.0, 0.75, -3.5):
        _sweep(sel, lambda cnt, n, lg, rng: np.full(cnt, c), f"all equal {c}",
               sizes=None if c == 0.0 else [65, 5000])
    got = sel["run"](np.zeros(5000), None, 100, True)
    np.testing.assert_array_equal(got["rows"], np.arange(100))
    got = sel["run"](np.zeros(sel["past_grid"]), None, TOPN_MAX, False)
    np.testing.assert_array_equal(got["rows"], np.arange(TOPN_MAX))


def test_select_tie_group_straddles_the_cut(sel):
    def make(cnt, n, largest, rng):
        best_first = np.arange(cnt, 0, -1, dtype=np.float64) if largest else np.arange(cnt, dtype=np.float64)
        lo, hi = min(max(0, n - 2), cnt - 1), min(cnt, n + 2)
        best_first[lo:hi] = best_first[lo]
        v = rng.permutation(best_first)
        if n < cnt and cnt > 1:
            s = np.sort(v)[::-1] if largest else np.sort(v)
            assert s[n - 1] == s[n]
        return v
    _sweep(sel, make, "tie straddle")


def test_select_keys_differ_in_one_digit(sel):
    """Two values whose keys differ in exactly one radix digit, one case per
    digit of the value key (its lowest bit: the last digit's is one ulp) and
    the sign bit."""
    base = np.float64(1.5).view(np.uint64)
    for bit in sel["digit_low_bits"] + [63]:
        pair = np.array([base, base ^ (np.uint64(1) << np.uint64(bit))], np.uint64).view(np.float64)
        assert not np.isnan(pair).any() and pair[0] != pair[1]
        _sweep(sel, lambda cnt, n, lg, rng: pair[rng.integers(0, 2, cnt)], f"digit bit {bit}", sizes=[2, 65, 1025, 5000])


def test_select_special_values(sel):
    zeros = np.array([0.0, -0.0, 1.0, -1.0])
    _sweep(sel, lambda cnt, n, lg, rng: zeros[rng.integers(0, 4, cnt)], "+-0 mixed")
    # only zeros: -0.0 == +0.0, so the rows decide, and the bits are kept
    v = np.array([0.0, -0.0] * 40)
    for lg in (True, False):
        got = sel["run"](v, None, 7, lg)
        np.testing.assert_array_equal(got["rows"], np.arange(7))
        np.testing.assert_array_equal(_bits(got["values"]), _bits(v[:7]))
    infs = np.array([np.inf, -np.inf, 0.0, 1e308, -1e308, np.finfo(np.float64).max])
    _sweep(sel, lambda cnt, n, lg, rng: infs[rng.integers(0, infs.size, cnt)], "+-inf")
    sub = np.array([5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0, 1e-310, -1e-310, 1e-320])
    _sweep(sel, lambda cnt, n, lg, rng: sub[rng.integers(0, sub.size, cnt)], "subnormals")


def test_select_nans(sel):
    nans = np.array([0x7FF8000000000000, -0x0008000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF],
                    np.int64).view(np.float64)
    assert np.isnan(nans).all()

    def scattered(cnt, n, lg, rng):
        v = rng.standard_normal(cnt)
        m = rng.random(cnt) < 0.3
        v[m] = nans[rng.integers(0, nans.size, int(m.sum()))]
        return v
    _sweep(sel, scattered, "NaNs scattered")
    _sweep(sel, lambda cnt, n, lg, rng: nans[rng.integers(0, nans.size, cnt)], "all NaN")
    got = sel["run"](np.full(1025, np.nan), None, 64, True)
    assert got["n_top"] == 0 and got["n_nan"] == 1025 and got["rows"].shape == (0,)


def test_select_sorted_inputs_and_rows(sel):
    _sweep(sel, lambda cnt, n, lg, rng: np.sort(rng.standard_normal(cnt)), "ascending")
    _sweep(sel, lambda cnt, n, lg, rng: np.sort(rng.standard_normal(cnt))[::-1].copy(), "descending")

    def with_rows(cnt, n, lg, rng):
        rows = np.cumsum(rng.integers(1, 5, cnt)).astype(np.int64) + 11
        return np.round(rng.standard_normal(cnt) * 3.0), rows   # ties, so the given rows decide
    _sweep(sel, with_rows, "non-contiguous rows")


def test_select_is_bit_identical_across_calls(sel):
    rng = np.random.default_rng(8)
    v = np.round(rng.standard_normal(sel["past_grid"]) * 50.0) / 8.0
    other = rng.standard_normal(5000)
    for n, lg in ((100, True), (TOPN_MAX, False)):
        a = sel["run"](v, None, n, lg)
        b = sel["run"](v, None, n, lg)
        sel["run"](other, None, 64, not lg)
        c = sel["run"](v, None, n, lg)
        for r in (b, c):
            np.testing.assert_array_equal(r["rows"], a["rows"])
            np.testing.assert_array_equal(_bits(r["values"]), _bits(a["values"]))
            assert (r["n_top"], r["n_nan"]) == (a["n_top"], a["n_nan"])


def test_n_out_of_range(sel):
    for n in (0, -1, TOPN_MAX + 1):
        with pytest.raises(ValueError):
            sel["run"](np.zeros(8), None, n, True)


# ---- LR engine -----------------------------------------------------------------

def _lr(loss="squared", **kw):
    from twitter_stream_ml_amd.ops.lr_engine import (DeviceLinearRegression, DeviceLogisticRegression,
                                                     LRDeviceConfig)
    kw = {"max_rows": 8192, "max_units": 8192 * 300, **kw}
    cls = DeviceLogisticRegression if loss == "logistic" else DeviceLinearRegression
    return cls(LRDeviceConfig(num_text_features=F, loss=loss, **kw), device=0)


def _cpu(loss="squared"):
    from twitter_stream_ml_amd.models.linear_regression import CpuLinearRegression, CpuLRConfig
    from twitter_stream_ml_amd.models.logistic_regression import CpuLogisticConfig, CpuLogisticRegression
    if loss == "logistic":
        return CpuLogisticRegression(CpuLogisticConfig(num_text_features=F))
    return CpuLinearRegression(CpuLRConfig(num_text_features=F))


def _w_dyadic(seed):
    """Text weights k / 256, |w| <= 16, numeric weights zero: every margin is
    exact in fp64 whatever the order of its sum, so the device and the CPU
    engine hold the same bits (``test_gpu_score.py``) -- and many rows tie."""
    rng = np.random.default_rng(seed)
    w = np.zeros(F + 4)
    w[:F] = rng.integers(-4096, 4097, F) / 256.0
    return w


def _assert_same(got, want, what):
    assert (got["n_top"], got["n_nan"], got["n_raw"], got["n_scored"]) == \
        (want["n_top"], want["n_nan"], want["n_raw"], want["n_scored"]), what
    np.testing.assert_array_equal(got["rows"], want["rows"], err_msg=str(what))
    np.testing.assert_array_equal(_bits(got["values"]), _bits(want["values"]), err_msg=str(what))


@pytest.fixture(scope="module")
def edge_cases():
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    cases = [("classes a", eb.length_class_batch(True)[0], False), ("classes b", eb.length_class_batch(False)[0], False)]
    cases += [(f"tiny {i}", raw, filt) for i, raw in enumerate(eb.tiny_batches(synth)) for filt in (False, True)]
    cases += [("filter boundary", eb.filter_boundary_batch(), True), ("filter boundary all", eb.filter_boundary_batch(), False)]
    return cases


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_lr_dyadic_weights_equal_cpu_engine(hip_module, edge_cases, loss):
    eng, cpu = _lr(loss), _cpu(loss)
    w = _w_dyadic(5)
    eng.set_weights(w)
    cpu.set_weights(w)
    for name, raw, filt in edge_cases:
        for n, lg in ((1, True), (7, False), (64, True), (TOPN_MAX, False)):
            got = eng.top_batch(raw, n, largest=lg, apply_filter=filt)
            want = cpu.top_batch(raw, n, largest=lg, apply_filter=filt)
            _assert_same(got, want, (name, n, lg, filt))
            assert got["top_ms"] > 0 and got["wall_ms"] > 0
    np.testing.assert_array_equal(eng.get_weights(), w)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_lr_general_weights_equal_own_margins(hip_module, loss):
    raw = generate_batch(SynthConfig.profile("twitter", seed=51, unicode_fraction=0.3), 0, 5000, batch_time_ms=NOW)
    eng = _lr(loss)
    rng = np.random.default_rng(3)
    eng.set_weights(rng.standard_normal(F + 4))
    kw = {"output": "margin"} if loss == "logistic" else {}
    for filt in (False, True):
        pm = eng.predict_batch(raw, apply_filter=filt, **kw)
        assert pm["n_scored"] > 100
        for n, lg in ((1, True), (100, True), (100, False), (TOPN_MAX, True), (TOPN_MAX, False)):
            got = eng.top_batch(raw, n, largest=lg, apply_filter=filt)
            _assert_top(got, pm["pred"], pm["rows"], n, lg, (loss, filt, n, lg))
            assert got["n_raw"] == 5000 and got["n_scored"] == pm["n_scored"]
    # n larger than the batch: everything, in order
    small = raw.slice(0, 37)
    pm = eng.predict_batch(small, **kw)
    got = eng.top_batch(small, 64)
    _assert_top(got, pm["pred"], pm["rows"], 64, True, "n > batch")
    assert got["n_top"] == 37


def test_lr_zero_weights_nothing_kept_no_rows_and_nan(hip_module):
    raw = generate_batch(SynthConfig.profile("twitter", seed=52), 0, 3000, batch_time_ms=NOW)
    eng = _lr()
    # zero weights: every margin is 0.0, the first n rows win either way
    for lg in (True, False):
        got = eng.top_batch(raw, 100, largest=lg)
        np.testing.assert_array_equal(got["rows"], np.arange(100))
        assert not got["values"].any() and got["n_nan"] == 0 and got["n_scored"] == 3000
    kept = eng.predict_batch(raw, apply_filter=True)["rows"]
    got = eng.top_batch(raw, 100, apply_filter=True)
    np.testing.assert_array_equal(got["rows"], kept[:100])
    # a filter that keeps nothing
    none = eb.texts_to_raw([raw.text_of(i) for i in range(70)], np.zeros(70, np.uint8), raw.scalars[:, :70], NOW)
    got = eng.top_batch(none, 10, apply_filter=True)
    assert got["n_raw"] == 70 and got["n_scored"] == got["n_top"] == got["n_nan"] == 0 and got["rows"].shape == (0,)
    # no rows at all: nothing is staged or launched
    h2d = eng.h2d_bytes
    got = eng.top_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)), 10)
    assert got["n_raw"] == got["n_scored"] == got["n_top"] == 0 and got["values"].dtype == np.float64
    assert eng.h2d_bytes == h2d
    # NaN margins are never selected
    # (a row whose bigrams hit both infinite text weights scores inf - inf)
    w = np.zeros(F + 4)
    w[:F] = np.random.default_rng(4).standard_normal(F)
    w[7], w[8], w[500], w[501] = np.inf, np.inf, -np.inf, -np.inf
    eng.set_weights(w)
    pm = eng.predict_batch(raw)
    assert 0 < np.isnan(pm["pred"]).sum() < 3000 and np.isinf(pm["pred"]).any()
    for lg in (True, False):
        got = eng.top_batch(raw, 200, largest=lg)
        _assert_top(got, pm["pred"], pm["rows"], 200, lg, "some NaN")
        assert got["n_nan"] == int(np.isnan(pm["pred"]).sum())
    with pytest.raises(ValueError, match="predict_batch"):
        eng.top_batch(raw, TOPN_MAX + 1)
    with pytest.raises(ValueError):
        eng.top_batch(raw, 0)


# ---- k-means ---------------------------------------------------------------------

def _km(k, text_dims, **kw):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    return DeviceKMeans(KMDeviceConfig(k=k, text_dims=text_dims, max_rows=8192, max_units=8192 * 300, seed=5, **kw),
                        device=0)


@pytest.mark.parametrize("k,text_dims", [(8, 0), (40, 6), (300, 30)])
def test_kmeans_top_equals_own_predict_batch(hip_module, k, text_dims):
    big = generate_batch(SynthConfig.profile("twitter", seed=21, unicode_fraction=0.2), 0, 4000, batch_time_ms=NOW)
    eng = _km(k, text_dims)
    eng.update_raw(big.slice(0, 2000), want_pred=False)   # centres off the initial ones
    c0, w0 = eng.get_state()
    frozen = np.linspace(0.5, 2.0, 2 + text_dims)
    for rows in (31, 32, 33, 127, 128, 129, 400, 4000):   # the assign kernels' 32 / 128 points; fewer rows than k
        raw = big.slice(0, rows)
        for scaler in ("none", frozen, "batch"):
            pb = eng.predict_batch(raw, scaler=scaler)
            ns = pb["n_scored"]
            assert 0 < ns <= rows
            for n, lg in ((1, True), (10, True), (10, False), (ns - 1, True), (ns + 1, False)):
                if not 1 <= n <= TOPN_MAX:
                    continue
                got = eng.top_batch(raw, n, largest=lg, scaler=scaler)
                what = (k, text_dims, rows, n, lg)
                _assert_top(got, pb["dist2"], pb["rows"], n, lg, what)
                np.testing.assert_array_equal(got["labels"], pb["pred"][np.searchsorted(pb["rows"], got["rows"])])
                assert got["labels"].dtype == np.int32 and got["dist2"] is got["values"]
                assert np.float64(got["cost"]).view(np.int64) == np.float64(pb["cost"]).view(np.int64), what
                np.testing.assert_array_equal(got["sizes"], pb["sizes"])
                assert (got["n_raw"], got["n_scored"], got["n_nan"]) == (rows, ns, 0)
                if pb["std"] is None:
                    assert got["std"] is None
                else:
                    np.testing.assert_array_equal(got["std"], pb["std"])
    c1, w1 = eng.get_state()
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(w0, w1)
    # nothing kept (no retweets) and no rows
    none = eb.texts_to_raw([big.text_of(i) for i in range(50)], np.zeros(50, np.uint8), big.scalars[:, :50], NOW)
    got = eng.top_batch(none, 5)
    assert got["n_raw"] == 50 and got["n_scored"] == got["n_top"] == 0 and got["cost"] == 0.0
    got = eng.top_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)), 5)
    assert got["n_raw"] == got["n_top"] == 0 and got["sizes"].shape == (k,)


# ---- non-interference ------------------------------------------------------------

def _train_snapshot(res):
    return (res["n_kept"], res["iterations"], list(res["stats"]), list(res["loss_history"]),
            np.asarray(res["pred"]).copy())


@pytest.mark.parametrize("loss", ["logistic", "squared"])
def test_non_interference(hip_module, loss):
    """Two engines train A, B, C (B prefetched before A trains and prepared
    ahead while it does, C prefetched before B trains), a snapshot begun after
    A and fetched after B.  The second engine also selects from X after A and
    from Y after B.  Every training result, the snapshot and the final weights
    must be the same bits."""
    Fw = 1 << 20
    synth = SynthConfig.profile("bench", seed=21)
    A, B, C = (generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(3))
    other = SynthConfig.profile("twitter", seed=22, unicode_fraction=0.3)
    X = generate_batch(other, 0, 2000, batch_time_ms=NOW + 7)
    Y = generate_batch(other, 2000, 1500, batch_time_ms=NOW + 8)
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, DeviceLogisticRegression, LRDeviceConfig
    cls = DeviceLogisticRegression if loss == "logistic" else DeviceLinearRegression

    def run(select):
        eng = cls(LRDeviceConfig(num_text_features=Fw, loss=loss, max_rows=8192, max_units=8192 * 300,
                                 num_iterations=10), device=0)
        snaps, tops = [], []
        assert eng.prefetch(A) and eng.prefetch(B)
        snaps.append(_train_snapshot(eng.train_batch(A, want_pred=True)))
        eng.snapshot_begin()
        if select:
            tops.append(eng.top_batch(X, 100))
        assert eng.prefetch(C)
        res = eng.train_batch(B, want_pred=True)
        assert res["prepared_ahead"]
        snaps.append(_train_snapshot(res))
        if select:
            tops.append(eng.top_batch(Y, 50, largest=False, apply_filter=True))
        snap = eng.snapshot_fetch()
        snaps.append(_train_snapshot(eng.train_batch(C, want_pred=True)))
        assert eng._pipe.hits == 3 and eng._pipe.orphaned == 0
        return snaps, eng.get_weights(), snap, tops

    s1, w1, snap1, _ = run(False)
    s2, w2, snap2, tops = run(True)
    for t, (a, b) in enumerate(zip(s1, s2)):
        assert a[0] == b[0] > 0 and a[1] == b[1] and a[2] == b[2] and a[3] == b[3], t
        np.testing.assert_array_equal(a[4], b[4])
    np.testing.assert_array_equal(w1.view(np.int64), w2.view(np.int64))
    assert snap1[0] == snap2[0] and snap1[1].shape[0] > 0
    np.testing.assert_array_equal(snap1[1], snap2[1])
    np.testing.assert_array_equal(snap1[2].view(np.int64), snap2[2].view(np.int64))
    assert tops[0]["n_scored"] == 2000 and tops[0]["n_top"] == 100
    assert 50 <= tops[1]["n_scored"] < 1500 and tops[1]["n_top"] == 50
    assert (np.diff(tops[0]["values"]) <= 0).all() and (np.diff(tops[1]["values"]) >= 0).all()


def test_forced_dp_engine_issues_no_collective(hip_module):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression, LRDeviceConfig
    comm = hip_module.Comm(hip_module.rccl_unique_id(), 0, 1, 0)
    synth = SynthConfig.profile("twitter", seed=33)
    batches = [generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(2)]
    Z = generate_batch(synth, 9000, 2400, batch_time_ms=NOW + 9)
    kw = dict(num_text_features=1 << 20, loss="logistic", label_threshold=550, num_iterations=10, max_rows=8192,
              max_units=8192 * 300)
    dp = DeviceLogisticRegression(LRDeviceConfig(force_dp=True, **kw), device=0, comm=comm)
    plain = DeviceLogisticRegression(LRDeviceConfig(**kw), device=0)
    dp.train_batch(batches[0], want_pred=False)
    plain.train_batch(batches[0], want_pred=False)
    before = dict(comm.counters())
    assert before["allreduce_calls"] > 0
    a = dp.top_batch(Z, 100)
    b = dp.top_batch(Z, 100, largest=False, apply_filter=True)
    assert dict(comm.counters()) == before
    assert a["n_scored"] == 2400 and a["n_top"] == 100 and 0 < b["n_scored"] < 2400
    _assert_same(a, plain.top_batch(Z, 100), "dp against plain")
    ra, rb = dp.train_batch(batches[1], want_pred=False), plain.train_batch(batches[1], want_pred=False)
    assert list(ra["stats"]) == list(rb["stats"]) and list(ra["loss_history"]) == list(rb["loss_history"])
    np.testing.assert_array_equal(dp.get_weights().view(np.int64), plain.get_weights().view(np.int64))
    assert dict(comm.counters())["allreduce_calls"] > before["allreduce_calls"]


def test_lifecycle(hip_module):
    gc.collect()
    hip_module.teardown_errors()
    before = hip_module.device_bytes_live()
    eng = _lr()
    raw = generate_batch(SynthConfig.profile("twitter", seed=2), 0, 500, batch_time_ms=NOW)
    eng.train_batch(raw)
    eng.predict_batch(raw)
    base = hip_module.device_bytes_live()
    assert eng.top_batch(raw, 10)["n_scored"] == 500
    grown = hip_module.device_bytes_live()
    assert base < grown <= base + (1 << 20)           # the histograms, the gathered keys and the result block
    eng.top_batch(raw, TOPN_MAX, largest=False)
    assert hip_module.device_bytes_live() == grown    # ... by the first call only
    km = _km(8, 4)
    km.predict_batch(raw)
    kbase = hip_module.device_bytes_live()
    km.top_batch(raw, 10)
    kgrown = hip_module.device_bytes_live()
    assert kbase < kgrown <= kbase + (1 << 20)
    km.top_batch(raw, 20, largest=False)
    assert hip_module.device_bytes_live() == kgrown
    del eng, km
    gc.collect()
    assert hip_module.device_bytes_live() == before
    assert list(hip_module.teardown_errors()) == []


# ---- the driver --------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["linear", "logistic"])
def test_score_driver_top_rocm_equals_local(hip_module, tmp_path, kind):
    """``twtml-score --top`` on ``rocm[1]`` against ``local[1]`` over the same
    recorded stream, dyadic weights: the same rows, value bits, texts and
    stream-wide summary."""
    from twitter_stream_ml_amd.apps import score as score_app
    from twitter_stream_ml_amd.models.linear_regression import LinearRegressionModel
    from twitter_stream_ml_amd.models.logistic_regression import LogisticRegressionModel
    model = tmp_path / "model"
    (LogisticRegressionModel if kind == "logistic" else LinearRegressionModel)(_w_dyadic(17)).save(str(model))
    out = {}
    for master in ("local[1]", "rocm[1]"):
        out[master] = tmp_path / master.replace("[", "_").replace("]", "")
        args = ["--master", master, "--model", str(model), "--top", "20", "--topOut", str(out[master]),
                "--source", "replay:synthetic:twitter:3", "--batchSize", "900", "--seconds", "0", "--sourceRate", "0",
                "--numBatches", "3", "-f", str(F), "--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9"]
        if kind == "logistic":
            args.append("--topSmallest")
        assert score_app.main(args) == 0

    def lines(d):
        recs = [json.loads(l) for l in open(d / "top.jsonl")]
        for r in recs:
            r.pop("ms"), r.pop("top_ms"), r.pop("batch_time_ms")   # the two runs' own clocks
        return recs

    cpu, gpu = lines(out["local[1]"]), lines(out["rocm[1]"])
    assert len(gpu) == 3 and all(len(r["entries"]) == 20 and r["count"] > 20 for r in gpu)
    for g, c in zip(gpu, cpu):
        assert g["entries"] == c["entries"], g["seq"]
    assert gpu == cpu
    if kind == "logistic":
        assert all("probability" in e for r in gpu for e in r["entries"])
    assert json.load(open(out["rocm[1]"] / "summary.json")) == json.load(open(out["local[1]"] / "summary.json"))

"""Held-out evaluation on the device (``csrc/hip/eval.hip``,
``LREngine::evaluate``, ``Device*Regression.evaluate_batch``).

Oracle: numpy (``models/metrics.py``) applied to the device's own
``predict_batch(output="margin")`` margins and the raw batch's
``retweetCount``.  A row's margin is bit-stable across calls, so every integer
of the accumulator -- ``hist``, ``confusion``, ``n``, ``n_nan`` -- is compared
exactly.  (That the margins agree with the fp64 CPU engine is
``test_gpu_score.py``'s subject.)

The fp64 sums: the per-row terms are fixed sequences of IEEE operations that
numpy reproduces bit for bit (``metrics.row_logloss``, ``regression_terms``),
so only the order of the sum differs: ``|sum - fsum| <= (n - 1) 2^-53 sum
|terms|``, the bound of any summation order.
"""
import math

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.models import metrics as M
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
F = 1000
U = 2.0 ** -53
SIZES = [1, 63, 64, 65, 1025, 5000]


def _cfg(loss, **kw):
    from twitter_stream_ml_amd.ops.lr_engine import LRDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, **kw}
    return LRDeviceConfig(num_text_features=F, loss=loss, **kw)


def _logistic(label_threshold, **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression
    return DeviceLogisticRegression(_cfg("logistic", label_threshold=int(label_threshold), **kw), device=0)


def _linear(**kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression
    return DeviceLinearRegression(_cfg("squared", **kw), device=0)


@pytest.fixture(scope="module")
def world(hip_module):
    """A logistic model trained for two batches, a 5000-row held-out batch and
    an engine whose label threshold is that batch's (upper) median count."""
    synth = SynthConfig.profile("twitter", seed=51, unicode_fraction=0.3)
    trainer = _logistic(550, step_size=0.1, num_iterations=20)
    for t in range(2):
        res = trainer.train_batch(generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t), want_pred=False)
        assert res["n_kept"] > 500
    w = trainer.get_weights()
    del trainer
    big = generate_batch(synth, 6000, SIZES[-1], batch_time_ms=NOW + 5)
    rc = big.scalars[0]
    lt = int(np.sort(rc)[rc.size // 2])
    eng = _logistic(lt)
    eng.set_weights(w)
    return {"w": w, "big": big, "lt": lt, "eng": eng, "synth": synth}


def _oracle_binary(eng, raw, apply_filter=False):
    pm = eng.predict_batch(raw, apply_filter=apply_filter, output="margin")
    rc = raw.scalars[0][pm["rows"]]
    acc = M.binary_accumulator(pm["pred"], rc, eng.cfg.effective_label_threshold(), eng.cfg.threshold)
    ok = ~np.isnan(pm["pred"])
    terms = M.row_logloss(pm["pred"][ok], rc[ok] >= eng.cfg.effective_label_threshold())
    return acc, terms, pm


def _assert_sum(got, terms, what):
    """The bound of any summation order of these very terms."""
    ref = math.fsum(terms.tolist())
    bound = max(terms.size - 1, 0) * U * math.fsum(np.abs(terms).tolist())
    err = abs(got - ref)
    print(f"{what}: n = {terms.size} sum = {got!r} |err| = {err:.3g} bound = {bound:.3g}")
    assert err <= bound, (what, got, ref, err, bound)


def _assert_binary(res, acc, terms, pm, raw, what):
    assert res["kind"] == "binary" and res["n_raw"] == raw.n and res["n_scored"] == pm["n_scored"]
    assert (res["n"], res["n_nan"]) == (acc["n"], acc["n_nan"]), what
    assert res["n"] + res["n_nan"] == res["n_scored"]
    assert res["confusion"] == acc["confusion"], what
    assert res["hist"].dtype == np.int64 and res["hist"].shape == (2, M.EVAL_BINS)
    np.testing.assert_array_equal(res["hist"], acc["hist"], err_msg=str(what))
    assert sum(res["confusion"]) == res["n"] == int(res["hist"].sum())
    _assert_sum(res["logloss_sum"], terms, what)


@pytest.mark.parametrize("n", SIZES)
def test_binary_equals_oracle(world, n):
    """1 row, around one wave (63 / 64 / 65), more than one workgroup with a
    ragged last wave (1025), a grid-stride batch of 20 workgroups (5000)."""
    eng, raw = world["eng"], world["big"].slice(0, n)
    acc, terms, pm = _oracle_binary(eng, raw)
    res = eng.evaluate_batch(raw)
    _assert_binary(res, acc, terms, pm, raw, n)
    assert res["label_threshold"] == world["lt"] and res["threshold"] == 0.5 and res["n_nan"] == 0
    assert res["eval_ms"] > 0 and res["wall_ms"] > 0
    np.testing.assert_array_equal(eng.get_weights(), world["w"])
    if n > 1:   # the median label threshold: both classes, and the margins are spread
        P, N = int(res["hist"][1].sum()), int(res["hist"][0].sum())
        assert P > 0 and N > 0
        bm = M.metrics_of(res)
        assert bm.areaUnderROC is not None and bm.auc_tie_bound < 0.5
    if n == SIZES[-1]:
        rc = raw.scalars[0]
        assert (rc == world["lt"]).any()                      # a count equal to the threshold is class 1
        assert int(res["hist"][1].sum()) == int((rc >= world["lt"]).sum())
        assert np.count_nonzero(res["hist"].sum(axis=0)) > 50   # two batches of training spread the margins
        bm = M.metrics_of(res)
        print(f"held-out AUC {bm.areaUnderROC:.4f} +- {bm.auc_tie_bound:.2g}, log-loss {bm.logLoss:.4f}")


def test_more_rows_than_one_grid_pass(world):
    """The grid is capped at 256 workgroups of 256 rows: 65 536 + 321 rows
    send the first workgroups through a second grid-stride pass, the last one
    with a ragged wave, and the final kernel through all 256 partials."""
    n = 256 * 256 + 321
    rng = np.random.default_rng(9)
    words = [eb.make_text("ascii", 3 + k % 23, rot=k) for k in range(64)]
    texts = [words[i] for i in rng.integers(0, 64, n)]
    sc = eb.ordinary_scalars(n, 17)
    sc[0] = rng.integers(0, 1200, n)
    raw = eb.texts_to_raw(texts, (np.arange(n) % 3 != 0).astype(np.uint8), sc)
    eng = _logistic(600, max_rows=n + 7, max_units=(n + 7) * 32)
    eng.set_weights(world["w"])
    for filt in (False, True):
        acc, terms, pm = _oracle_binary(eng, raw, apply_filter=filt)
        res = eng.evaluate_batch(raw, apply_filter=filt)
        _assert_binary(res, acc, terms, pm, raw, ("two passes", filt))
        assert res["n_scored"] == (n if not filt else pm["n_scored"]) and res["hist"][1].sum() > 0
    lin = _linear(max_rows=n + 7, max_units=(n + 7) * 32)
    lin.set_weights(world["w"] * 300.0)
    pm = lin.predict_batch(raw)
    res = lin.evaluate_batch(raw)
    for k, col in zip(M.REGRESSION_SUMS, M.regression_terms(pm["pred"], raw.scalars[0])):
        _assert_sum(res[k], col, f"{k} two passes")


def test_row_terms_are_the_hosts_bits(world):
    """One-row batches: the sum is the row's term, so the device's
    ``log1p(exp(-|m|))`` and squares must be numpy's to the bit (a fused
    multiply-add or a libm call on either side shows here)."""
    eng, big = world["eng"], world["big"]
    lin = _linear()
    for scale in (1.0, 40.0):
        eng.set_weights(world["w"] * scale)
        lin.set_weights(world["w"] * 300.0 * scale)
        for i in range(0, 24):
            raw = big.slice(i, i + 1)
            m = eng.predict_batch(raw, output="margin")["pred"]
            want = M.row_logloss(m, raw.scalars[0] >= world["lt"])[0]
            got = eng.evaluate_batch(raw)["logloss_sum"]
            assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (i, scale, m[0], got, want)
            p = lin.predict_batch(raw)["pred"]
            res = lin.evaluate_batch(raw)
            for k, col in zip(M.REGRESSION_SUMS, M.regression_terms(p, raw.scalars[0])):
                assert np.float64(res[k]).view(np.int64) == np.float64(col[0]).view(np.int64), (i, scale, k)
    eng.set_weights(world["w"])


def test_filtered(world):
    eng, raw = world["eng"], world["big"]
    acc, terms, pm = _oracle_binary(eng, raw, apply_filter=True)
    assert 0 < pm["n_scored"] < raw.n and not np.array_equal(pm["rows"], np.arange(pm["n_scored"]))
    res = eng.evaluate_batch(raw, apply_filter=True)
    _assert_binary(res, acc, terms, pm, raw, "filtered")
    # a filter that keeps nothing: no retweets
    none = eb.texts_to_raw([raw.text_of(i) for i in range(70)], np.zeros(70, np.uint8), raw.scalars[:, :70], NOW)
    res = eng.evaluate_batch(none, apply_filter=True)
    assert res["n_raw"] == 70 and res["n_scored"] == res["n"] == res["n_nan"] == 0
    assert res["hist"].sum() == 0 and res["confusion"] == [0, 0, 0, 0] and res["logloss_sum"] == 0.0
    # no rows at all: nothing is staged or launched
    h2d = eng.h2d_bytes
    res = eng.evaluate_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)))
    assert res["n_raw"] == res["n_scored"] == res["n"] == 0 and res["hist"].shape == (2, M.EVAL_BINS)
    assert res["kind"] == "binary" and eng.h2d_bytes == h2d


def test_sums_are_bit_identical_across_calls(world):
    eng, big = world["eng"], world["big"]
    a, b = big.slice(0, 3001), big.slice(3001, 5000)
    r1 = eng.evaluate_batch(a)
    r2 = eng.evaluate_batch(a)
    eng.evaluate_batch(b)
    eng.evaluate_batch(big, apply_filter=True)
    r3 = eng.evaluate_batch(a)
    for r in (r2, r3):
        assert np.float64(r["logloss_sum"]).view(np.int64) == np.float64(r1["logloss_sum"]).view(np.int64)
        np.testing.assert_array_equal(r["hist"], r1["hist"])
        assert r["confusion"] == r1["confusion"]
    lin = _linear()
    lin.set_weights(world["w"] * 300.0)
    q1 = lin.evaluate_batch(a)
    lin.evaluate_batch(b)
    q2 = lin.evaluate_batch(a)
    for k in M.REGRESSION_SUMS:
        assert np.float64(q1[k]).view(np.int64) == np.float64(q2[k]).view(np.int64), k


@pytest.mark.parametrize("n", SIZES)
def test_regression_equals_oracle(world, n):
    raw = world["big"].slice(0, n)
    lin = _linear()
    lin.set_weights(world["w"] * 300.0)
    pm = lin.predict_batch(raw)
    res = lin.evaluate_batch(raw)
    assert res["kind"] == "regression" and res["label_threshold"] == -1
    assert (res["n_raw"], res["n_scored"], res["n"], res["n_nan"]) == (n, n, n, 0)
    terms = M.regression_terms(pm["pred"], raw.scalars[0])
    for k, col in zip(M.REGRESSION_SUMS, terms):
        _assert_sum(res[k], col, f"{k} n={n}")
    assert M.metrics_of(res).meanSquaredError > 0
    if n == SIZES[-1]:   # filtered, with row ids
        pm = lin.predict_batch(raw, apply_filter=True)
        res = lin.evaluate_batch(raw, apply_filter=True)
        assert 0 < res["n_scored"] == pm["n_scored"] == res["n"] < n
        for k, col in zip(M.REGRESSION_SUMS, M.regression_terms(pm["pred"], raw.scalars[0][pm["rows"]])):
            _assert_sum(res[k], col, f"{k} filtered")


def test_zero_weights_clamps_and_nan(world):
    big, lt = world["big"], world["lt"]
    raw = big.slice(0, 1025)
    eng = _logistic(lt)
    # zero weights: every margin is 0
    res = eng.evaluate_batch(raw)
    assert int(res["hist"][:, M.ZERO_BIN].sum()) == res["n"] == 1025 == int(res["hist"].sum())
    bm = M.metrics_of(res)
    assert bm.areaUnderROC == 0.5 and bm.auc_tie_bound == 0.5
    assert res["confusion"][1] == res["confusion"][3] == 0          # 0 > logit(0.5) = 0 is false
    _assert_sum(res["logloss_sum"], M.row_logloss(np.zeros(1025), raw.scalars[0] >= lt), "zero weights")
    assert bm.logLoss == pytest.approx(math.log(2.0), rel=1e-14)
    # margins beyond +-2^12: the clamp bins (and a loss that is the hinge alone)
    eng.set_weights(world["w"] * 1e6)
    acc, terms, pm = _oracle_binary(eng, raw)
    res = eng.evaluate_batch(raw)
    _assert_binary(res, acc, terms, pm, raw, "clamped")
    assert res["hist"][:, 0].sum() > 0 and res["hist"][:, M.EVAL_BINS - 1].sum() > 0
    assert np.abs(pm["pred"]).max() > 4096.0 * 4
    # a NaN numeric weight: every margin is NaN
    w = world["w"].copy()
    w[F] = np.nan
    eng.set_weights(w)
    assert np.isnan(eng.predict_batch(raw, output="margin")["pred"]).all()
    res = eng.evaluate_batch(raw)
    assert res["n_nan"] == res["n_scored"] == 1025 and res["n"] == 0
    assert res["hist"].sum() == 0 and res["confusion"] == [0, 0, 0, 0] and res["logloss_sum"] == 0.0
    lin = _linear()
    lin.set_weights(w)
    res = lin.evaluate_batch(raw)
    assert res["n_nan"] == 1025 and res["n"] == 0 and all(res[k] == 0.0 for k in M.REGRESSION_SUMS)
    # some NaN margins only: +inf and -inf numeric weights meet in rows with both features non-zero
    w = world["w"].copy()
    w[F], w[F + 1] = np.inf, -np.inf
    eng.set_weights(w)
    acc, terms, pm = _oracle_binary(eng, raw)
    res = eng.evaluate_batch(raw)
    assert res["n_nan"] == acc["n_nan"] and res["n"] == acc["n"]
    np.testing.assert_array_equal(res["hist"], acc["hist"])
    assert res["confusion"] == acc["confusion"]


def test_one_class_only(world):
    raw = world["big"].slice(0, 1025)
    eng = _logistic(int(raw.scalars[0].max()) + 1)
    eng.set_weights(world["w"])
    acc, terms, pm = _oracle_binary(eng, raw)
    res = eng.evaluate_batch(raw)
    _assert_binary(res, acc, terms, pm, raw, "one class")
    assert res["confusion"][2:] == [0, 0] and res["confusion"][0] > 0 and res["confusion"][1] > 0
    bm = M.metrics_of(res)
    assert bm.areaUnderROC is None and bm.areaUnderPR is None and bm.auc_tie_bound is None


@pytest.mark.parametrize("span,n", [(1, 64), (1, 33), (1 << 32, 33)])
def test_label_column_widths(world, span, n):
    """retweetCount as a 1-bit stream (off and on a word boundary) and as raw
    int64: ``raw_scalar``'s two paths."""
    base = 7 if span == 1 else -12345
    raw = eb.scalar_sweep_batch([span, 10, 10, 10, 10], [base, 0, 0, 0, NOW - 100], n, seed=5, label_sweep=True)
    rc = raw.scalars[0]
    assert eb.expected_width(int(rc.max() - rc.min())) == (1 if span == 1 else 64)
    lt = base + 1 if span == 1 else 550
    for thr in sorted({lt, int(rc.max())}):
        eng = _logistic(thr)
        eng.set_weights(world["w"])
        for filt in (False, True):
            acc, terms, pm = _oracle_binary(eng, raw, apply_filter=filt)
            res = eng.evaluate_batch(raw, apply_filter=filt)
            _assert_binary(res, acc, terms, pm, raw, (span, n, thr, filt))
        full = eng.evaluate_batch(raw)
        assert int(full["hist"][1].sum()) == int((rc >= thr).sum()) > 0
        assert int(full["hist"][0].sum()) > 0
    lin = _linear()
    lin.set_weights(world["w"])
    res = lin.evaluate_batch(raw)
    assert res["sum_y"] == float(rc.sum())              # every partial sum is an exact integer
    if span == 1:
        assert res["sum_y2"] == float((rc * rc).sum())


def test_split_and_merge(world):
    eng, big = world["eng"], world["big"]
    whole = eng.evaluate_batch(big)
    parts = [eng.evaluate_batch(big.slice(0, 1999)), eng.evaluate_batch(big.slice(1999, 5000))]
    acc = M.EvalAccumulator.like(parts[0]).add(parts[0])
    acc.merge(M.EvalAccumulator.like(parts[1]).add(parts[1]))
    got = acc.result()
    assert (got["n"], got["n_nan"], got["confusion"]) == (whole["n"], whole["n_nan"], whole["confusion"])
    np.testing.assert_array_equal(got["hist"], whole["hist"])
    # two roundings more than either order of the whole
    assert got["logloss_sum"] == pytest.approx(whole["logloss_sum"], rel=5000 * U)
    m = acc.metrics()
    assert m.areaUnderROC == M.metrics_of(whole).areaUnderROC and m.auc_tie_bound == M.metrics_of(whole).auc_tie_bound


# --- non-interference ---------------------------------------------------------

def _train_snapshot(res):
    return (res["n_kept"], res["iterations"], list(res["stats"]), list(res["loss_history"]),
            np.asarray(res["pred"]).copy())


@pytest.mark.parametrize("loss", ["logistic", "squared"])
def test_non_interference(hip_module, loss):
    """Two engines train A, B, C (B prefetched before A trains and prepared
    ahead while it does, C prefetched before B trains), a snapshot begun after
    A and fetched after B.  The second engine also evaluates X after A and Y
    after B.  Every training result, the snapshot and the final weights must be
    the same bits."""
    Fw = 1 << 20
    synth = SynthConfig.profile("bench", seed=21)
    A, B, C = (generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(3))
    other = SynthConfig.profile("twitter", seed=22, unicode_fraction=0.3)
    X = generate_batch(other, 0, 2000, batch_time_ms=NOW + 7)
    Y = generate_batch(other, 2000, 1500, batch_time_ms=NOW + 8)
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, DeviceLogisticRegression, LRDeviceConfig
    cls = DeviceLogisticRegression if loss == "logistic" else DeviceLinearRegression

    def run(evaluate):
        eng = cls(LRDeviceConfig(num_text_features=Fw, loss=loss, max_rows=8192, max_units=8192 * 300,
                                 num_iterations=10), device=0)
        snaps, evals = [], []
        assert eng.prefetch(A) and eng.prefetch(B)
        snaps.append(_train_snapshot(eng.train_batch(A, want_pred=True)))
        eng.snapshot_begin()
        if evaluate:
            evals.append(eng.evaluate_batch(X))
        assert eng.prefetch(C)
        res = eng.train_batch(B, want_pred=True)
        assert res["prepared_ahead"]
        snaps.append(_train_snapshot(res))
        if evaluate:
            evals.append(eng.evaluate_batch(Y, apply_filter=True))
        snap = eng.snapshot_fetch()
        snaps.append(_train_snapshot(eng.train_batch(C, want_pred=True)))
        assert eng._pipe.hits == 3 and eng._pipe.orphaned == 0
        return snaps, eng.get_weights(), snap, evals

    s1, w1, snap1, _ = run(False)
    s2, w2, snap2, evals = run(True)
    for t, (a, b) in enumerate(zip(s1, s2)):
        assert a[0] == b[0] > 0 and a[1] == b[1] and a[2] == b[2] and a[3] == b[3], t
        np.testing.assert_array_equal(a[4], b[4])
    np.testing.assert_array_equal(w1.view(np.int64), w2.view(np.int64))
    assert snap1[0] == snap2[0] and snap1[1].shape[0] > 0
    np.testing.assert_array_equal(snap1[1], snap2[1])
    np.testing.assert_array_equal(snap1[2].view(np.int64), snap2[2].view(np.int64))
    assert evals[0]["n_scored"] == 2000 and 0 < evals[1]["n_scored"] < 1500
    assert all(e["n"] + e["n_nan"] == e["n_scored"] for e in evals)


def test_forced_dp_engine_issues_no_collective(hip_module):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLogisticRegression
    comm = hip_module.Comm(hip_module.rccl_unique_id(), 0, 1, 0)
    synth = SynthConfig.profile("twitter", seed=33)
    batches = [generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(2)]
    Z = generate_batch(synth, 9000, 2400, batch_time_ms=NOW + 9)
    from twitter_stream_ml_amd.ops.lr_engine import LRDeviceConfig
    kw = dict(num_text_features=1 << 20, loss="logistic", label_threshold=550, num_iterations=10, max_rows=8192,
              max_units=8192 * 300)
    dp = DeviceLogisticRegression(LRDeviceConfig(force_dp=True, **kw), device=0, comm=comm)
    plain = DeviceLogisticRegression(LRDeviceConfig(**kw), device=0)
    dp.train_batch(batches[0], want_pred=False)
    plain.train_batch(batches[0], want_pred=False)
    before = dict(comm.counters())
    assert before["allreduce_calls"] > 0
    a = dp.evaluate_batch(Z)
    b = dp.evaluate_batch(Z, apply_filter=True)
    assert dict(comm.counters()) == before
    assert a["n_scored"] == 2400 and 0 < b["n_scored"] < 2400
    ra, rb = dp.train_batch(batches[1], want_pred=False), plain.train_batch(batches[1], want_pred=False)
    assert list(ra["stats"]) == list(rb["stats"]) and list(ra["loss_history"]) == list(rb["loss_history"])
    np.testing.assert_array_equal(dp.get_weights().view(np.int64), plain.get_weights().view(np.int64))
    assert dict(comm.counters())["allreduce_calls"] > before["allreduce_calls"]


def test_lifecycle(hip_module):
    import gc
    gc.collect()
    hip_module.teardown_errors()
    before = hip_module.device_bytes_live()
    eng = _linear()
    raw = generate_batch(SynthConfig.profile("twitter", seed=2), 0, 500, batch_time_ms=NOW)
    eng.train_batch(raw)
    eng.predict_batch(raw)
    base = hip_module.device_bytes_live()
    assert eng.evaluate_batch(raw)["n_scored"] == 500
    grown = hip_module.device_bytes_live()
    assert base < grown <= base + (1 << 20)           # the accumulator words and partials, by the first call
    eng.evaluate_batch(raw)
    assert hip_module.device_bytes_live() == grown    # ... and only by the first
    del eng
    gc.collect()
    assert hip_module.device_bytes_live() == before
    assert list(hip_module.teardown_errors()) == []

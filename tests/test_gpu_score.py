"""Inference-only scoring on the device (``csrc/hip/score.hip``,
``LREngine::score``, ``DeviceLinearRegression.predict_batch``).

Reference: the fp64 oracle ``featurize_batch_native(...).X @ w``.

* exact case -- text weights are integer multiples of 2^-8 with |w| <= 16 and
  the numeric weights are zero: every term and every partial sum is exactly
  representable, so the device must equal the oracle bit for bit whatever its
  sum order; any wrong, missing or duplicated id shows.
* general case -- text weights ~ N(0, 1), numeric weights ~ 1e7 (the numeric
  features are ~1e-7..1e-2, so both parts matter); per row
  ``|p_dev - p_oracle| <= 2 (B + 5) 2^-53 sum |x_i w_i|`` with B the row's
  bigram count: the bound for two differently ordered recursive fp64 sums of
  the same B + 4 products.  An fp32 intermediate breaks it by ~8 orders of
  magnitude (``test_scalar_widths``).
"""
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.oracle import featurize_batch_native
from twitter_stream_ml_amd.records.batch import RawBatch
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
U = 2.0 ** -53


def _engine(F, hash="java", **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, **kw}
    return DeviceLinearRegression(LRDeviceConfig(num_text_features=F, hash=hash, **kw), device=0)


def _w_exact(F, seed):
    rng = np.random.default_rng(seed)
    w = np.zeros(F + 4)
    w[:F] = rng.integers(-4096, 4097, F) / 256.0
    return w


def _w_general(F, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(F + 4)
    w[F:] = (1.0 + rng.random(4)) * 1e7 * np.array([1.0, -1.0, 1.0, -1.0])
    return w


_ORACLE = {}


def _oracle(key, raw, F, hash, apply_filter=False):
    """The oracle's features of a batch, computed once per (batch, F, hash, filter)."""
    k = (key, F, hash, apply_filter)
    if k not in _ORACLE:
        _ORACLE[k] = featurize_batch_native(raw, F, 100, 1000, now_ms=raw.batch_time_ms, hash=hash,
                                            apply_filter=apply_filter)
    return _ORACLE[k]


def _assert_rows(res, fb, raw):
    assert res["n_raw"] == raw.n and res["n_scored"] == fb.n
    assert res["rows"].dtype == np.int64 and res["pred"].dtype == np.float64
    assert res["pred"].shape == (fb.n,)
    np.testing.assert_array_equal(res["rows"], fb.rows)


def _assert_exact(res, fb, w, what=""):
    ref = np.asarray(fb.X @ w, np.float64).reshape(-1)
    got = np.ascontiguousarray(res["pred"])
    bad = np.nonzero(got.view(np.int64) != ref.view(np.int64))[0]
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], ref[bad[:8]])


def _bound(fb, w, F):
    B = np.asarray(fb.X[:, :F].sum(axis=1)).reshape(-1)
    mass = np.asarray(abs(fb.X) @ np.abs(w)).reshape(-1)
    return 2.0 * (B + 5.0) * U * mass


def _assert_bound(res, fb, w, F, what=""):
    ref = np.asarray(fb.X @ w, np.float64).reshape(-1)
    err = np.abs(res["pred"] - ref)
    bound = _bound(fb, w, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max |err| / bound = {ratio.max() if ratio.size else 0.0:.3f} over {fb.n} rows")
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, (what, bad[:8], err[bad[:8]], bound[bad[:8]])


def _score_both(eng, key, raw, F, hash, seed, apply_filter=False):
    """Exact and general case of one batch; the model is what was set."""
    fb = _oracle(key, raw, F, hash, apply_filter)
    for kind, w in (("exact", _w_exact(F, seed)), ("general", _w_general(F, seed + 1))):
        eng.set_weights(w)
        res = eng.predict_batch(raw, apply_filter=apply_filter)
        _assert_rows(res, fb, raw)
        if kind == "exact":
            _assert_exact(res, fb, w, (key, kind))
        else:
            _assert_bound(res, fb, w, F, f"{key} {kind}")
        np.testing.assert_array_equal(eng.get_weights(), w)   # scoring leaves the model as it was
    return fb


@pytest.fixture(scope="module")
def class_batches():
    return {"a": eb.length_class_batch(True)[0], "b": eb.length_class_batch(False)[0]}


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
@pytest.mark.parametrize("F,hash", [(1000, "java"), (1 << 20, "java"), (1 << 20, "murmur3")])
def test_row_length_classes(hip_module, class_batches, ingest, F, hash):
    """Rows of 0..8192 units in ASCII, Latin-1 and Cyrillic (``edge_batches``):
    0 / 1 / 2 units, uneven quarters, the fast-chunk edge (289 / 290 units:
    k_score_narrow vs k_score), the 640-B staging limit of k_score (rows read
    from global memory beyond it), the decoder window (utf8 ingest) and rows no
    row word holds.  F = 1000 reduces every hash with term_mod; 1 << 20 with
    the Java hash takes the direct path (and the LDS weight table when on)."""
    eng = _engine(F, hash, ingest=ingest)
    for name in ("a", "b"):
        raw = class_batches[name]
        fb = _score_both(eng, name, raw, F, hash, seed=5)
        assert fb.n == raw.n
        nb = eb.wire_bytes_per_row(raw, ingest)
        assert (nb >= eb.PACKED_ROW_LIMIT).any()
        lens = np.diff(raw.offsets)
        assert {eb.LAST_FAST, eb.LAST_FAST + 1} <= set(lens.tolist())


def _short_ascii_batch(n):
    texts = [eb.make_text("ascii", 3 + (i * 7) % 40, rot=i) for i in range(n)]
    return eb.texts_to_raw(texts, (np.arange(n) % 2).astype(np.uint8), eb.ordinary_scalars(n, 104))


def test_tiny_empty_and_segment_sized_batches(hip_module):
    """1..65 rows, only empty rows, no rows; and 4095..8193 unfiltered short
    rows: kept rows == raw rows across the filter segment (kSegRows = 4096)
    and row-word tile (kRowTile = 8192) boundaries."""
    F = 1000
    eng = _engine(F, max_rows=16384, max_units=16384 * 64)
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    for i, raw in enumerate(eb.tiny_batches(synth)):
        _score_both(eng, ("tiny", i), raw, F, "java", seed=20 + i)
        _score_both(eng, ("tiny", i), raw, F, "java", seed=40 + i, apply_filter=True)
    raw = eb.empty_rows_batch()
    w = _w_general(F, 3)
    eng.set_weights(w)
    res = eng.predict_batch(raw)
    fb = _oracle("empty", raw, F, "java")
    _assert_rows(res, fb, raw)
    _assert_bound(res, fb, w, F, "empty rows")
    assert np.abs(res["pred"]).min() > 0        # the numeric part alone
    # no rows: nothing is staged or launched
    h2d = eng.h2d_bytes
    res = eng.predict_batch(eb.texts_to_raw([], [], np.zeros((5, 0), np.int64)))
    assert res["n_raw"] == 0 and res["n_scored"] == 0
    assert res["rows"].shape == (0,) and res["pred"].shape == (0,) and res["pred"].dtype == np.float64
    assert eng.h2d_bytes == h2d
    for n in (eb.SEG_ROWS - 1, eb.SEG_ROWS, eb.SEG_ROWS + 1, eb.ROW_TILE - 1, eb.ROW_TILE, eb.ROW_TILE + 1):
        raw = _short_ascii_batch(n)
        fb = _score_both(eng, ("seg", n), raw, F, "java", seed=n)
        assert fb.n == n
    # beyond the staging capacity: the ValueError of training
    with pytest.raises(ValueError):
        eng.predict_batch(_short_ascii_batch(16385))
    with pytest.raises(ValueError):
        _engine(F, max_rows=64, max_units=100).predict_batch(_short_ascii_batch(30))


@pytest.mark.parametrize("ingest", ["wire", "utf8"])
def test_filter(hip_module, ingest):
    F = 1 << 20
    eng = _engine(F, ingest=ingest)
    raw = eb.filter_boundary_batch()
    w = _w_general(F, 9)
    eng.set_weights(w)
    kept = eng.predict_batch(raw, apply_filter=True)
    fbk = _oracle("filter", raw, F, "java", True)
    assert 0 < fbk.n < raw.n
    _assert_rows(kept, fbk, raw)
    _assert_bound(kept, fbk, w, F, "filtered")
    # column 1 holds the row index: the kept rows, in order
    np.testing.assert_array_equal(raw.scalars[1, kept["rows"]], fbk.rows)
    every = eng.predict_batch(raw, apply_filter=False)
    fba = _oracle("filter", raw, F, "java", False)
    _assert_rows(every, fba, raw)
    np.testing.assert_array_equal(every["rows"], np.arange(raw.n))
    _assert_bound(every, fba, w, F, "unfiltered")
    # a row's sum order does not depend on the rows it is scored with (nor on
    # the kernel its chunk falls to: the filter moves narrow rows in and out of
    # the chunk that straddles the narrow / wide boundary) -- the same bits
    a = np.ascontiguousarray(every["pred"][kept["rows"]]).view(np.int64)
    np.testing.assert_array_equal(a, np.ascontiguousarray(kept["pred"]).view(np.int64))


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
@pytest.mark.parametrize("F,hash", [(1 << 20, "java"), (1000, "murmur3")])
def test_special_lowercasing(hip_module, ingest, F, hash):
    """U+0130, Final_Sigma, an astral cased letter and a 9000-unit row among
    ordinary rows: decode and full case mapping as for training."""
    synth = SynthConfig.profile("twitter", seed=11, unicode_fraction=0.3)
    raw = eb.with_junk_rows(eb.tiny_batches(synth)[-1])
    assert any(t in raw.text_of(i) for i in range(raw.n) for t in ("İ", "ΟΔΟΣ"))
    eng = _engine(F, hash, ingest=ingest, max_units=8192 * 300)
    _score_both(eng, "junk", raw, F, hash, seed=13)
    _score_both(eng, "junk", raw, F, hash, seed=15, apply_filter=True)


def test_scalar_widths(hip_module):
    """Packed scalar columns of 20..32 bits and raw int64 columns (negative
    values included) with non-zero numeric weights: the numeric features are
    formed in fp64.  The fp32 features of the training path would miss the
    bound by orders of magnitude -- checked here on the host, on these very
    inputs, so the bound is known to be tight enough to tell."""
    F = 1000
    spans = [0, (1 << 32) - 1, 1 << 31, (1 << 20) + 12345, 1 << 32]
    bases = [0, 10 ** 9, -12345, 7, NOW - (1 << 33)]
    sweep = eb.scalar_sweep_batch(spans, bases, 64, seed=77)
    eng = _engine(F)
    w = _w_general(F, 31)
    eng.set_weights(w)
    for name, raw in (("sweep", sweep), ("int64", eb.raw_int64_batch())):
        fb = _oracle(name, raw, F, "java")
        res = eng.predict_batch(raw)
        _assert_rows(res, fb, raw)
        _assert_bound(res, fb, w, F, name)
        # the same prediction with fp32 numeric features (featurize.hip row_scalars)
        X32 = fb.X.tolil(copy=True)
        X32[:, F:] = fb.X[:, F:].toarray().astype(np.float32).astype(np.float64)
        err32 = np.abs(np.asarray(X32.tocsr() @ w).reshape(-1) - np.asarray(fb.X @ w).reshape(-1))
        worse = err32 > _bound(fb, w, F)
        print(f"{name}: fp32 numeric features break the bound on {int(worse.sum())} of {fb.n} rows, "
              f"by up to {np.max(err32 / _bound(fb, w, F)):.3g} x")
        assert worse.mean() > 0.5, name


def test_determinism(hip_module):
    F = 1 << 20
    synth = SynthConfig.profile("twitter", seed=19, unicode_fraction=0.3)
    a = generate_batch(synth, 0, 3000, batch_time_ms=NOW)
    b = generate_batch(synth, 3000, 2500, batch_time_ms=NOW + 1)
    for hash in ("java", "murmur3"):
        eng = _engine(F, hash)
        eng.set_weights(_w_general(F, 23))
        p1 = eng.predict_batch(a)["pred"].view(np.int64)
        p2 = eng.predict_batch(a)["pred"].view(np.int64)
        eng.predict_batch(b)
        p3 = eng.predict_batch(a)["pred"].view(np.int64)
        np.testing.assert_array_equal(p1, p2)
        np.testing.assert_array_equal(p1, p3)


# --- non-interference ---------------------------------------------------------

def _train_snapshot(res):
    return (res["n_kept"], res["iterations"], list(res["stats"]), list(res["loss_history"]),
            np.asarray(res["pred"]).copy(), bool(res["tiered"]))


def non_interference_scenario(expect_tiered):
    """Two engines train A, B, C (B prefetched before A trains and prepared
    ahead while it does, C prefetched before B trains).  The second one also
    scores X after A and Y after B.  Every training result and the final
    weights must be the same bits; the scores are those of a fresh engine
    holding the weights of that moment."""
    F = 1 << 20
    synth = SynthConfig.profile("bench", seed=21)
    A, B, C = (generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(3))
    other = SynthConfig.profile("twitter", seed=22, unicode_fraction=0.3)
    X = generate_batch(other, 0, 2000, batch_time_ms=NOW + 7)
    Y = generate_batch(other, 2000, 1500, batch_time_ms=NOW + 8)
    kw = dict(num_iterations=10)

    def run(score):
        eng = _engine(F, **kw)
        snaps, scores, weights = [], {}, {}
        assert eng.prefetch(A) and eng.prefetch(B)
        snaps.append(_train_snapshot(eng.train_batch(A, want_pred=True)))
        weights["A"] = eng.get_weights()
        if score:
            scores["X"] = eng.predict_batch(X)
        assert eng.prefetch(C)
        res = eng.train_batch(B, want_pred=True)
        assert res["prepared_ahead"]
        snaps.append(_train_snapshot(res))
        weights["B"] = eng.get_weights()
        if score:
            scores["Y"] = eng.predict_batch(Y, apply_filter=True)
        snaps.append(_train_snapshot(eng.train_batch(C, want_pred=True)))
        assert eng._pipe.hits == 3 and eng._pipe.orphaned == 0
        return snaps, eng.get_weights(), weights, scores

    s1, w1, _, _ = run(False)
    s2, w2, at, scores = run(True)
    for t, (a, b) in enumerate(zip(s1, s2)):
        assert a[0] == b[0] > 0 and a[1] == b[1] and a[2] == b[2] and a[3] == b[3], t
        np.testing.assert_array_equal(a[4], b[4])
        assert a[5] == b[5] == expect_tiered, (t, a[5])
    np.testing.assert_array_equal(w1.view(np.int64), w2.view(np.int64))
    fresh = _engine(F, **kw)
    for name, raw, after, filt in (("X", X, "A", False), ("Y", Y, "B", True)):
        fresh.set_weights(at[after])
        want = fresh.predict_batch(raw, apply_filter=filt)
        np.testing.assert_array_equal(want["rows"], scores[name]["rows"])
        np.testing.assert_array_equal(want["pred"].view(np.int64), scores[name]["pred"].view(np.int64))
        fb = featurize_batch_native(raw, F, 100, 1000, now_ms=raw.batch_time_ms, apply_filter=filt)
        _assert_rows(scores[name], fb, raw)
        _assert_bound(scores[name], fb, at[after], F, name)


def test_non_interference(hip_module, monkeypatch):
    monkeypatch.delenv("TWTML_FORCE_TIERED", raising=False)
    non_interference_scenario(expect_tiered=False)


def test_non_interference_tiered(hip_module):
    """The same with the tiered layout forced, in a fresh process."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, TWTML_FORCE_TIERED="1",
               PYTHONPATH=os.pathsep.join([root, here, os.environ.get("PYTHONPATH", "")]))
    code = "import test_gpu_score as t; t.non_interference_scenario(expect_tiered=True); print('scenario ok')"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scenario ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_slot_owned_by_training_is_refused(hip_module):
    """A raw slot that holds a batch queued for training takes no score-only
    batch and is neither scored nor evaluated; the refusals leave the queued
    batch as it was: it trains to the bits of an engine that never saw them."""
    F = 1000
    synth = SynthConfig.profile("twitter", seed=3)
    A, X = (generate_batch(synth, t * 64, 64, batch_time_ms=NOW + t) for t in range(2))
    kw = dict(max_rows=1024, max_units=1024 * 300, num_iterations=5)
    direct = _engine(F, **kw)
    want = direct.train_batch(A, want_pred=False)
    assert want["n_kept"] == featurize_batch_native(A, F, 100, 1000, now_ms=A.batch_time_ms).n > 0
    eng = _engine(F, **kw)
    assert eng.prefetch(A)   # queued: submitted, not processed yet
    (_, slot), = eng._pipe._inflight.values()
    hb = eng.staging((slot + 1) % eng.raw_slots).load(X)
    owned = "queued or prepared for training"
    with pytest.raises(RuntimeError, match=owned):
        eng._eng.submit(hb._hb, int(hb.n), int(hb.bytes), int(slot), int(hb.ext_text), int(hb.batch_time_ms), False)
    with pytest.raises(RuntimeError, match=owned):
        eng._eng.score(int(slot), int(A.batch_time_ms), False, 0)
    with pytest.raises(RuntimeError, match=owned):
        eng._eng.evaluate(int(slot), int(A.batch_time_ms), False)
    got = eng.train_batch(A, want_pred=False)
    assert eng._pipe.hits == 1 and got["n_kept"] == want["n_kept"]
    assert list(got["stats"]) == list(want["stats"]) and got["iterations"] == want["iterations"]
    np.testing.assert_array_equal(eng.get_weights().view(np.int64), direct.get_weights().view(np.int64))


def test_dp_loopback_scoring_issues_no_collective(hip_module):
    """Two DP replicas (loopback communicator), each scoring a different shard
    between two trained batches: they stay bit-identical, equal the run
    without scoring, and the communicators count the same collectives."""
    from twitter_stream_ml_amd.ops._native import hip
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    F = 1 << 20
    cfg = LRDeviceConfig(num_text_features=F, max_rows=8192, max_units=8192 * 300, num_iterations=10)
    synth = SynthConfig.profile("bench", seed=33)
    batches = [generate_batch(synth, t * 3000, 3000, batch_time_ms=NOW + t) for t in range(3)]
    Z = generate_batch(SynthConfig.profile("twitter", seed=34, unicode_fraction=0.3), 0, 2400, batch_time_ms=NOW + 9)

    def run(score):
        group = hip().LoopbackGroup(2)
        comms = [group.comm(r) for r in range(2)]
        engines = [DeviceLinearRegression(cfg, device=0, comm=comms[r]) for r in range(2)]
        results, scores, errors = [[None] * 3, [None] * 3], [None, None], []

        def worker(r):
            try:
                eng = engines[r]
                shards = [full.shard(r, 2) for full in batches]
                for sh in shards:
                    assert eng.prefetch(sh)
                for t, sh in enumerate(shards):
                    results[r][t] = eng.train_batch(sh, want_pred=False)
                    if score and t == r:   # rank 0 after batch 0, rank 1 after batch 1
                        w = eng.get_weights()
                        scores[r] = (w, eng.predict_batch(Z.shard(r, 2)))
            except Exception as e:  # pragma: no cover - surfaced below
                errors.append(e)

        th = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=300)
        assert not errors, errors
        return [e.get_weights() for e in engines], results, scores, [dict(c.counters()) for c in comms]

    w_plain, res_plain, _, ctr_plain = run(False)
    w_score, res_score, scores, ctr_score = run(True)
    np.testing.assert_array_equal(w_score[0].view(np.int64), w_score[1].view(np.int64))
    np.testing.assert_array_equal(w_score[0].view(np.int64), w_plain[0].view(np.int64))
    for r in range(2):
        for t in range(3):
            assert list(res_score[r][t]["stats"]) == list(res_plain[r][t]["stats"])
            assert list(res_score[r][t]["loss_history"]) == list(res_plain[r][t]["loss_history"])
        assert ctr_score[r] == ctr_plain[r], (ctr_score[r], ctr_plain[r])
        assert ctr_score[r]["allreduce_calls"] > 0
        w, got = scores[r]
        sh = Z.shard(r, 2)
        fb = featurize_batch_native(sh, F, 100, 1000, now_ms=sh.batch_time_ms, apply_filter=False)
        _assert_rows(got, fb, sh)
        _assert_bound(got, fb, w, F, f"rank {r}")


def test_murmur3_1e8_features(hip_module):
    """F = 1e8, murmur3: ids beyond every 32-bit-float-exact integer.  (F is
    below 2^27, so the largest power of two an id can exceed is 2^26.)"""
    F = 100_000_000
    synth = SynthConfig.profile("wide", seed=41)
    raw = generate_batch(synth, 0, 64, batch_time_ms=NOW)
    fb = featurize_batch_native(raw, F, 100, 1000, now_ms=NOW, hash="murmur3", apply_filter=False)
    ids = np.unique(fb.X[:, :F].tocsr().indices)
    rng = np.random.default_rng(43)
    high = ids[ids >= 1 << 26]
    assert high.size >= 50
    pick = np.unique(np.concatenate([rng.choice(ids, 250, replace=False), rng.choice(high, 50, replace=False)]))
    w = np.zeros(F + 4)
    v = rng.integers(1, 4097, pick.size) * rng.choice([-1, 1], pick.size)
    w[pick] = v / 256.0
    eng = _engine(F, "murmur3", max_rows=1024, max_units=1024 * 300)
    eng.set_weights(w)
    res = eng.predict_batch(raw)
    _assert_rows(res, fb, raw)
    _assert_exact(res, fb, w, "1e8")
    assert np.count_nonzero(res["pred"]) > 32   # the chosen weights are the batch's own


def test_lifecycle(hip_module):
    gc.collect()
    hip_module.teardown_errors()
    before = hip_module.device_bytes_live()
    eng = _engine(1000)
    raw = generate_batch(SynthConfig.profile("twitter", seed=2), 0, 500, batch_time_ms=NOW)
    eng.train_batch(raw)
    base = hip_module.device_bytes_live()
    assert eng.predict_batch(raw)["n_scored"] == 500
    assert hip_module.device_bytes_live() > base      # the scoring scratch, allocated by the first call
    grown = hip_module.device_bytes_live()
    eng.predict_batch(raw)
    assert hip_module.device_bytes_live() == grown    # ... and only by the first
    del eng
    gc.collect()
    assert hip_module.device_bytes_live() == before
    assert list(hip_module.teardown_errors()) == []

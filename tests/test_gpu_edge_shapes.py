"""The streaming-LR engine at the hard thresholds of its hot path.

The synthetic generator's rows are 20..280 units long and its batches hold
hundreds to thousands of rows, so the rest of the GPU suite never reaches or
straddles the constants the kernels branch on.  The batches of
``edge_batches.py`` do (``test_edge_batches_cpu.py`` proves that on the CPU);
here the device is compared with the fp64 oracle on them, entry for entry,
and each test asserts from the engine's debug dumps that it reached the edge
it aims at.
"""
import numpy as np
import pytest

import edge_batches as eb
from layout_decode import (hybrid_row_counts, oracle_row_counts, oracle_row_ids, rows_from_debug,
                           scalars_by_kept)
from twitter_stream_ml_amd.models.mllib_helper import NUMBER_SCALES
from twitter_stream_ml_amd.oracle import (featurize_batch, featurize_batch_native, filter_mask,
                                          round_half_up_array, run_minibatch_sgd)
from twitter_stream_ml_amd.records.batch import RawBatch
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
NNZ_WIDE = 1 << 30   # featurize.hip kNnzWide


def _engine(F, hash="java", **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, **kw}
    return DeviceLinearRegression(LRDeviceConfig(num_text_features=F, hash=hash, **kw), device=0)


def _feed(eng, raw, want_pred=True):
    """Stage, submit and train one batch through staging slot 0; returns the
    result and the staging view (its wire encoding can then be inspected)."""
    hb = eng.staging(0).load(raw, eng.cfg.ingest)
    eng.submit(hb, 0)
    return eng.process(0, raw.batch_time_ms, want_pred), hb


def _snapshot(res):
    return (res["n_kept"], res["iterations"], list(res["stats"]), list(res["loss_history"]),
            np.asarray(res["pred"]).copy())


def _same_snapshot(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], what
    assert a[2] == b[2], what
    assert a[3] == b[3], what
    np.testing.assert_array_equal(a[4], b[4], err_msg=str(what))


def _expected_scalars(raw, rows, now=NOW):
    """Labels and numeric features of the given raw rows as the oracle forms
    them (MllibHelper.scala:58-71): fp32 of one fp64 product each."""
    sc = raw.scalars[:, rows]
    y = sc[0].astype(np.float64).astype(np.float32)
    num = np.stack([sc[1] * NUMBER_SCALES[0], sc[2] * NUMBER_SCALES[1], sc[3] * NUMBER_SCALES[2],
                    (now - sc[4]) * NUMBER_SCALES[3]], axis=1).astype(np.float64).astype(np.float32)
    return y, num


def _check_features(dbg, fb, F):
    """Device ids, active set, labels and numeric features == oracle (exact)."""
    assert int(dbg["counters"][0]) == fb.n
    rows = rows_from_debug(dbg)
    Xt = fb.X[:, :F].tocsr()
    for k in range(fb.n):
        np.testing.assert_array_equal(rows[k], oracle_row_ids(Xt, k), err_msg=f"row {k}")
    np.testing.assert_array_equal(np.sort(dbg["uniq"]), np.unique(Xt.indices))
    y, num = scalars_by_kept(dbg)
    np.testing.assert_array_equal(y, fb.y.astype(np.float32))
    # one fp64 multiply and one round-to-nearest conversion on both sides: bit-exact
    np.testing.assert_array_equal(num, fb.X[:, F:F + 4].toarray().astype(np.float32))


def _check_chunk_classes(dbg, meta_kept, want_fast_edge):
    """nnz / cfast of the prepared batch against the classes the rows belong to.

    Per kept row: bigram count len - 1 (len for len < 2), wide bit for the
    Cyrillic rows only.  Per chunk: cfast == 1 iff no row is wide and the
    longest has <= 4 * kFastMaxQ bigrams (289 units)."""
    nnz, perm, cfast, clen8 = dbg["nnz"], dbg["perm"], dbg["cfast"], dbg["clen8"]
    for k, (script, L) in enumerate(meta_kept):
        assert int(nnz[k]) & (NNZ_WIDE - 1) == eb.bigrams(L), (k, script, L)
        if L > 0:
            assert bool(int(nnz[k]) & NNZ_WIDE) == (script == "cyrillic"), (k, script, L)
    last_fast, first_slow = False, False
    for c in range(cfast.shape[0]):
        ks = [int(k) for k in perm[c * 16:(c + 1) * 16] if k >= 0]
        longest = max(int(nnz[k]) & (NNZ_WIDE - 1) for k in ks)
        wide = any(int(nnz[k]) & NNZ_WIDE for k in ks)
        per_lane = -(-longest // eb.LANES_PER_ROW)
        assert int(clen8[c]) == -(-per_lane // eb.GROUP), c
        if not wide and longest <= eb.bigrams(eb.LAST_FAST):
            assert cfast[c] == 1, (c, longest)
        else:
            assert cfast[c] == 0, (c, longest, wide)
        if want_fast_edge and longest <= eb.bigrams(eb.SHORT_CLASS_MAX):
            # the homogeneous batch: 16 rows of one class (empty rows excepted: the
            # ingest modes differ in whether they count as narrow)
            assert len({int(nnz[k]) & (NNZ_WIDE - 1) for k in ks}) == 1 or longest <= 1, (c, ks)
        last_fast |= (not wide) and longest == eb.bigrams(eb.LAST_FAST)
        first_slow |= (not wide) and longest == eb.bigrams(eb.LAST_FAST + 1)
    if want_fast_edge:
        assert last_fast and first_slow, "no narrow chunk tops out at 289 / 290 units"


_ORACLE = {}


def _oracle(name, raw, F, hash):
    """featurize_batch_native == featurize_batch on these batches (CPU suite); computed once."""
    key = (name, F, hash)
    if key not in _ORACLE:
        _ORACLE[key] = featurize_batch_native(raw, F, 100, 1000, now_ms=NOW, hash=hash)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def class_batches():
    a, meta_a = eb.length_class_batch(True)
    b, meta_b = eb.length_class_batch(False)
    return {"a": (a, meta_a), "b": (b, meta_b)}


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
@pytest.mark.parametrize("F,hash", [(1000, "java"), (1 << 20, "java"), (1 << 20, "murmur3")])
def test_row_length_classes(hip_module, class_batches, ingest, F, hash):
    """Rows of 0..8192 units in three scripts (ASCII, Latin-1, Cyrillic + ASCII).

    Thresholds covered, with the constant each length comes from:
    * bigrams of a row ``len >= 2 ? len - 1 : len`` (featurize.hip k_filter_write,
      narrow_text.h): rows of 0, 1, 2 units;
    * 4 lanes per row, contiguous quarters (kLanesPerRow): 2..9 units;
    * fast narrow chunk ``per_lane <= kFastMaxQ`` (72): 287..291 units, 289 the
      last fast length -- asserted through ``cfast``;
    * register layout ``L8 <= kMaxRegGroups`` (10; hot_split.hip hybrid vs plain
      remap, featurize.hip merge bypass with dedup=True): 320 / 321 / 322
      units, asserted through ``clen8c == -1`` beyond 321;
    * length-sort bucket clamp at kHalfBuckets - 1 bigrams: 2047 / 2048 / 2049;
    * UTF-8 decode stage window kDecStage = 6144 B: two-byte rows of 6128,
      6144, 6146, 6160 bytes (utf8 ingest);
    * row word, kRowLenBits = 13: rows of 8191 / 8192 wire bytes per ingest mode
      (8191 / 8192 narrow or ASCII units, 4095 / 4096 units as UTF-16) --
      asserted through ``rows_packed``.
    F = 1000 takes narrow_id's modulo path, 1 << 20 the direct one.

    Batch a holds 16 rows of every class up to 322 units (whole chunks of one
    class), batch b one row per class (chunks straddle classes).  With every
    hashed id kept (lazy_idx=False) ids, active set, labels and numeric
    features are compared with the oracle exactly; the layouts (lazy hybrid,
    eager hybrid, plain, merged) must then train bit-identically, and like the
    fp64 oracle within the project's SGD bounds.  The step is
    ``edge_batches.LENGTH_CLASS_STEP`` (the reference's 0.005 diverges here).
    """
    kw = dict(ingest=ingest, step_size=eb.LENGTH_CLASS_STEP, num_iterations=eb.LENGTH_CLASS_ITERS)
    eager = _engine(F, hash, lazy_idx=False, **kw)
    snaps, w_oracle = [], np.zeros(F + 4)
    for name in ("a", "b"):
        raw, meta = class_batches[name]
        fb = _oracle(name, raw, F, hash)
        res, hb = _feed(eager, raw)
        assert res["n_kept"] == fb.n == raw.n
        assert not res["diverged"]
        if ingest == "utf16":
            assert res["rows_narrowed"] > 0
        nb = eb.wire_bytes_per_row(raw, ingest)
        assert (nb >= eb.PACKED_ROW_LIMIT).any() and not hb.rows_packed
        dbg = eager._eng.debug_prepared()
        _check_features(dbg, fb, F)
        _check_chunk_classes(dbg, meta, want_fast_edge=(name == "a"))
        snaps.append(_snapshot(res))
        # training: the oracle continues from its own weights
        r = run_minibatch_sgd(fb.X, fb.y, w_oracle, eb.LENGTH_CLASS_STEP, eb.LENGTH_CLASS_ITERS)
        w_oracle = r.weights
        wg = eager.get_weights()
        assert abs(res["iterations"] - r.iterations) <= 1, (name, res["iterations"], r.iterations)
        tol = 1e-6 if res["iterations"] == r.iterations else 3e-3
        dw = np.linalg.norm(wg - w_oracle)
        print(f"{name}: iterations {res['iterations']} / {r.iterations}, |dw| / |w| = "
              f"{dw / np.linalg.norm(w_oracle):.3e}")
        assert dw <= tol * max(np.linalg.norm(w_oracle), 1e-30), (name, dw)
    w_eager = eager.get_weights()

    # the same batch without the rows no row word holds packs its rows
    raw, meta = class_batches["b"]
    nb = eb.wire_bytes_per_row(raw, ingest)
    keep = np.nonzero(nb < eb.PACKED_ROW_LIMIT)[0]
    assert nb[keep].max() >= eb.PACKED_ROW_LIMIT - 2   # 8191 B (narrow / UTF-8) or 8190 B (UTF-16) still fits
    short = raw.take(keep)
    res, hb = _feed(eager, short)
    assert hb.rows_packed and res["n_kept"] == short.n
    fb = featurize_batch_native(short, F, 100, 1000, now_ms=NOW, hash=hash)
    _check_features(eager._eng.debug_prepared(), fb, F)
    # only empty rows are kept: an empty active set
    raw0 = eb.empty_rows_batch()
    res, _ = _feed(eager, raw0)
    dbg = eager._eng.debug_prepared()
    assert res["n_kept"] == 3 and res["n_unique"] == 0 and dbg["uniq"].shape[0] == 0
    _check_features(dbg, featurize_batch_native(raw0, F, 100, 1000, now_ms=NOW, hash=hash), F)
    del eager

    # layout independence (tests/test_gpu_exact.py): bitwise the same training
    others = {"lazy hybrid": dict(hybrid=True, lazy_idx=True), "plain": dict(hybrid=False)}
    if F == 1000:
        others["merged"] = dict(dedup=True)
    for what, cfg in others.items():
        eng = _engine(F, hash, **cfg, **kw)
        for i, name in enumerate(("a", "b")):
            raw, meta = class_batches[name]
            res, _ = _feed(eng, raw)
            assert not res["diverged"]
            _same_snapshot(_snapshot(res), snaps[i], (what, name))
            if what == "lazy hybrid":   # ids re-derived from the text by the remap
                dbg = eng._eng.debug_prepared()
                hy = eng._eng.debug_hybrid()
                clen8, clen8c = dbg["clen8"], hy["clen8c"]
                assert clen8c.shape[0] == clen8.shape[0] > 0
                # chunks beyond kMaxRegGroups groups (rows > 321 units) stay in the plain layout
                np.testing.assert_array_equal(clen8c == -1, clen8 > eb.MAX_REG_GROUPS)
                if name == "a":   # whole chunks of 321 and of 322 units: both sides of the edge
                    assert (clen8 == eb.MAX_REG_GROUPS).any() and (clen8 == eb.MAX_REG_GROUPS + 1).any()
                uniq = np.sort(dbg["uniq"])
                Xt = _oracle(name, raw, F, hash).X[:, :F].tocsr()
                perm = dbg["perm"]
                for c in np.nonzero(clen8c >= 0)[0]:
                    for r in range(16):
                        k = int(perm[c * 16 + r])
                        if k >= 0:
                            assert hybrid_row_counts(hy, uniq, dbg["cbase"], c, r) == oracle_row_counts(Xt, k), \
                                (name, k, meta[k])
            if what == "merged":
                assert eng._eng.debug_merged()["clen8d"].shape[0] > 0
        np.testing.assert_array_equal(eng.get_weights(), w_eager, err_msg=what)
        del eng


# ---------------------------------------------------------------------------
# batch sizes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
def test_tiny_and_boundary_batches(hip_module, ingest):
    """Batches of 1, 2, 15, 16, 17, 63, 64, 65 kept rows (16 rows per chunk,
    kRowsPerChunk; 64 lanes, kWave; at most 5 chunks, so only chunk 0 is one
    of the kHistChunks = 16 spaced sample chunks of the hot-slot histogram and
    the lazy featurizer) after an ordinary 2500-row batch, the 17- and 65-row
    ones as every third row of 3n raw rows (kept index != raw index): kept
    count, n and sum y exactly, iterations and weights within the
    project's SGD bounds, predictions within 1 + 1e-3 |p| per row and, pooled
    over the 243 rows, fewer than 1 % rounded predictions off the oracle's."""
    F = 1000
    cfg = SynthConfig.profile("twitter", seed=41, unicode_fraction=0.1)
    eng = _engine(F, step_size=0.005, num_iterations=50, ingest=ingest)
    w = np.zeros(F + 4)
    warm = generate_batch(cfg, 0, 2500, batch_time_ms=NOW)
    fb = featurize_batch(warm, F, 100, 1000)
    res, _ = _feed(eng, warm)
    assert res["n_kept"] == fb.n
    w = run_minibatch_sgd(fb.X, fb.y, w, 0.005, 50).weights
    mism = total = 0
    for raw, n in zip(eb.tiny_batches(cfg), eb.TINY_SIZES):
        fb = featurize_batch(raw, F, 100, 1000)
        assert fb.n == n
        pred_o = round_half_up_array(fb.X @ w)
        res, _ = _feed(eng, raw)
        assert res["n_kept"] == n and not res["diverged"]
        assert res["stats"][0] == n and res["stats"][1] == fb.y.sum()
        pred_g = np.asarray(res["pred"], np.float64)
        assert pred_g.shape == (n,)
        assert np.all(np.abs(pred_g - pred_o) <= 1.0 + 1e-3 * np.abs(pred_o)), (n, pred_g, pred_o)
        mism += int((pred_g != pred_o).sum())
        total += n
        r = run_minibatch_sgd(fb.X, fb.y, w, 0.005, 50)
        w = r.weights
        wg = eng.get_weights()
        assert abs(res["iterations"] - r.iterations) <= 1, (n, res["iterations"], r.iterations)
        tol = 1e-6 if res["iterations"] == r.iterations else 3e-3
        dw = np.linalg.norm(wg - w) / max(np.linalg.norm(w), 1e-30)
        print(f"n={n}: iterations {res['iterations']} / {r.iterations}, |dw| / |w| = {dw:.3e}")
        assert dw <= tol, (n, dw)
    assert total == 243 and mism < 0.01 * total, (mism, total)


def test_empty_raw_batch_is_a_no_op(hip_module):
    """n = 0 raw rows (not a filtered-out batch): nothing kept, no iteration,
    weights bit-unchanged, and the next batch trains exactly as on a twin
    engine that never saw the empty one."""
    F = 1000
    cfg = SynthConfig.profile("twitter", seed=42)
    first = generate_batch(cfg, 0, 1500, batch_time_ms=NOW)
    nxt = generate_batch(cfg, 1500, 1500, batch_time_ms=NOW + 5000)
    for ingest in ("wire", "utf16", "utf8"):
        a, b = _engine(F, ingest=ingest, num_iterations=10), _engine(F, ingest=ingest, num_iterations=10)
        _same_snapshot(_snapshot(_feed(a, first)[0]), _snapshot(_feed(b, first)[0]), "first")
        w0 = a.get_weights()
        res, _ = _feed(a, RawBatch.empty(NOW + 2000))
        assert res["n_kept"] == 0 and res["iterations"] == 0 and res["n_raw"] == 0
        np.testing.assert_array_equal(a.get_weights(), w0)
        _same_snapshot(_snapshot(_feed(a, nxt)[0]), _snapshot(_feed(b, nxt)[0]), "next")
        np.testing.assert_array_equal(a.get_weights(), b.get_weights())


def _boundary_rows_batch(n):
    """n short rows; kept: rows 0, 4095, 4096, n - 1 and every 7th.  rc = row
    index + 1 for kept rows (distinct labels < 2^24: the kept order shows in
    y); dropped rows are non-retweets or carry an rc outside [0, 100000]."""
    i = np.arange(n)
    keep = (i % 7 == 0) | (i == 0) | (i == eb.SEG_ROWS - 1) | (i == eb.SEG_ROWS) | (i == n - 1)
    sc = eb.ordinary_scalars(n, 104)
    sc[0] = i + 1
    is_rt = np.ones(n, np.uint8)
    drop = np.nonzero(~keep)[0]
    is_rt[drop[0::3]] = 0
    sc[0, drop[1::3]] = -1 - drop[1::3]
    sc[0, drop[2::3]] = 100001 + drop[2::3]
    texts = [eb.make_text(("ascii", "latin1", "cyrillic")[j % 3], 3 + j % 23, rot=j) for j in range(n)]
    return eb.texts_to_raw(texts, is_rt, sc), keep


@pytest.mark.parametrize("ingest", ["wire", "utf8"])
def test_raw_row_count_boundaries(hip_module, ingest):
    """Raw batches of 4095 / 4096 / 4097 rows (kSegRows = 4096: one filter /
    sort segment vs two) and 8191 / 8192 / 8193 rows (kRowTile = 8192: one
    row-word scan tile vs two), kept rows on both sides of each boundary: kept
    count and order (distinct labels), ids per kept row == oracle."""
    F = 1 << 20
    eng = _engine(F, ingest=ingest, lazy_idx=False, num_iterations=1, begin=0, end=100000,
                  max_rows=8448, max_units=8448 * 32)
    for n in (eb.SEG_ROWS - 1, eb.SEG_ROWS, eb.SEG_ROWS + 1, eb.ROW_TILE - 1, eb.ROW_TILE, eb.ROW_TILE + 1):
        raw, keep = _boundary_rows_batch(n)
        eng.set_weights(np.zeros(F + 4))
        res, hb = _feed(eng, raw)
        assert hb.rows_packed
        assert res["n_raw"] == n and res["n_kept"] == int(keep.sum())
        dbg = eng._eng.debug_prepared()
        y, _ = scalars_by_kept(dbg)
        np.testing.assert_array_equal(y, (np.nonzero(keep)[0] + 1).astype(np.float32))
        fb = featurize_batch_native(raw, F, 0, 100000, now_ms=NOW)
        np.testing.assert_array_equal(fb.rows, np.nonzero(keep)[0])
        _check_features(dbg, fb, F)


# ---------------------------------------------------------------------------
# scalar wire widths
# ---------------------------------------------------------------------------

def _check_scalar_wire(hb, raw):
    """Host bytes -> numpy reader of the documented stream -> the column."""
    sw = hb._hb.scalar_wire
    assert sw["rows"] == raw.n
    spack = np.array(hb._hb.spack_bytes[:int(sw["offsets"][-1])])
    for c in range(5):
        col = raw.scalars[c]
        span = int(col.max()) - int(col.min())
        w = sw["widths"][c]
        assert w == eb.expected_width(span), (c, w, span)
        assert sw["base"][c] == (0 if w == 64 else int(col.min())), c
        buf = spack[int(sw["offsets"][c]):int(sw["offsets"][c + 1])]
        np.testing.assert_array_equal(eb.decode_scalar_stream(buf, raw.n, w, sw["base"][c]), col, err_msg=f"col {c}")
    return sw["widths"]


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
def test_scalar_width_sweep(hip_module, ingest):
    """Scalar bit stream (kernels.h raw_scalar, engine.cpp pack_scalars):
    every width 1..32 at both ends of its span class (2^(w-1) and 2^w - 1;
    span 2^32 - 1 vs 2^32 -> raw int64), bases 0 / -12345 / 1e9, 33 and 64
    rows (n * w off and on a 32-bit word boundary; at 64 rows the last value's
    second word is the slack word), one row, createdAt beyond now (negative
    age), values of +-2^40.  The label column's width is set by filtered-out
    rows carrying the extremes.  Asserted: the staged widths are the intended
    ones, the host bytes decode (pure numpy) to the columns, and the device's
    labels and numeric features equal fp32(fp64 product) exactly, for exactly
    the rows the filter keeps."""
    F = 1000
    eng = _engine(F, ingest=ingest, lazy_idx=False, num_iterations=1, max_rows=128, max_units=1024)
    zeros = np.zeros(F + 4)
    cases = [eb.scalar_sweep_batch(s, b, n, k, label_sweep=lab) for k, (s, b, n, lab) in enumerate(eb.sweep_cases())]
    cases.append(eb.raw_int64_batch())
    seen = [set() for _ in range(5)]
    kept_label_rows = 0
    for k, raw in enumerate(cases):
        eng.set_weights(zeros)
        res, hb = _feed(eng, raw, want_pred=False)
        widths = _check_scalar_wire(hb, raw)
        for c in range(5):
            seen[c].add(widths[c])
        rows = np.nonzero(filter_mask(raw, 100, 1000))[0]
        assert res["n_kept"] == rows.shape[0], k
        if rows.shape[0] < raw.n:
            kept_label_rows += rows.shape[0]
        y, num = scalars_by_kept(eng._eng.debug_prepared())
        want_y, want_num = _expected_scalars(raw, rows)
        np.testing.assert_array_equal(y, want_y, err_msg=f"case {k}")
        np.testing.assert_array_equal(num, want_num, err_msg=f"case {k}")
    for c in range(5):
        assert seen[c] >= set(range(1, 33)), (c, sorted(seen[c]))
    assert all(64 in seen[c] for c in range(5))
    assert kept_label_rows > 0


# ---------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("begin,end,require_retweet,range_filter", [
    (100, 1000, True, True), (500, 500, True, True), (1000, 100, True, True),
    (100, 1000, True, False), (100, 1000, False, True), (100, 1000, False, False)])
def test_filter_boundaries(hip_module, begin, end, require_retweet, range_filter):
    """Filter ``begin <= rc <= end``, ``require_retweet``, ``range_filter``
    (featurize.hip keep_row): rc cycles through begin - 1, begin, begin + 1,
    end - 1, end, end + 1, -1, 0, 2^31, -2^31 with both retweet flags; begin ==
    end; begin > end (keeps nothing); either switch off.  Kept count and order
    (followers = row index) equal a numpy mask; ids of the kept rows == oracle.
    Labels are fp32 on the device (featurize.hip row_scalars): every rc here is
    <= 2^24 in magnitude or a power of two, so the comparison is exact."""
    F = 1 << 20
    raw = eb.filter_boundary_batch(begin, end)
    rc = raw.scalars[0]
    mask = np.ones(raw.n, bool)
    if require_retweet:
        mask &= raw.is_retweet != 0
    if range_filter:
        mask &= (rc >= begin) & (rc <= end)
    rows = np.nonzero(mask)[0]
    for ingest in ("wire", "utf8"):
        eng = _engine(F, ingest=ingest, lazy_idx=False, num_iterations=1, begin=begin, end=end,
                      require_retweet=require_retweet, range_filter=range_filter)
        res, _ = _feed(eng, raw)
        assert res["n_kept"] == rows.shape[0]
        dbg = eng._eng.debug_prepared()
        y, num = scalars_by_kept(dbg)
        want_y, want_num = _expected_scalars(raw, rows)
        np.testing.assert_array_equal(num[:, 0], want_num[:, 0])   # followers = row index: kept set and order
        np.testing.assert_array_equal(y, want_y)
        if rows.shape[0]:
            fb = featurize_batch_native(raw.take(rows), F, 0, 0, now_ms=NOW, apply_filter=False)
            _check_features(dbg, fb, F)
        else:
            assert begin > end and res["iterations"] == 0
        del eng


# ---------------------------------------------------------------------------
# filtered-out rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
def test_filtered_rows_do_not_touch_the_model(hip_module, ingest):
    """Three ordinary batches vs the same kept rows interleaved with rows the
    filter drops -- non-retweets, out-of-range rc, empty rows, a 9000-unit
    Cyrillic row (plain-offsets fallback, wide), special-lowering rows,
    scalars of +-2^40 (raw int64 columns): bounds, hot-slot histogram and
    chunks are computed over kept rows only and every sum is an integer, so
    stats, loss history, predictions and weights are bitwise equal."""
    F = 1 << 20
    cfg = SynthConfig.profile("twitter", seed=43, unicode_fraction=0.2)
    a = _engine(F, ingest=ingest, num_iterations=10, max_rows=2048, max_units=2048 * 300)
    b = _engine(F, ingest=ingest, num_iterations=10, max_rows=2048, max_units=2048 * 300)
    for t in range(3):
        raw = generate_batch(cfg, t * 1200, 1200, batch_time_ms=NOW + t * 5000)
        junk = eb.with_junk_rows(raw)
        ra, _ = _feed(a, raw)
        rb, hb = _feed(b, junk)
        assert not hb.rows_packed and hb._hb.scalar_wire["wide_mask"] == 0b11111
        assert ra["n_kept"] == rb["n_kept"] > 0 and rb["n_raw"] == junk.n > raw.n
        _same_snapshot(_snapshot(ra), _snapshot(rb), t)
    np.testing.assert_array_equal(a.get_weights(), b.get_weights())

"""The edge-shape builders (``edge_batches.py``) are where they claim to be.

Runs without a GPU: the GPU tests of ``test_gpu_edge_shapes.py`` compare the
device with the oracle on these batches, so here the oracle side is pinned --
both featurizers agree, every class has the bigram count and wire size its
threshold needs, the scalar builder reaches every width, and the fp64 SGD is
finite and non-diverging at the step sizes those tests use.  An edited
builder that moved off an edge fails here first.
"""
import numpy as np
import pytest

import edge_batches as eb
from twitter_stream_ml_amd.oracle import (featurize_batch, featurize_batch_native, filter_mask,
                                          run_minibatch_sgd)
from twitter_stream_ml_amd.ops._native import host
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch


@pytest.fixture(scope="module")
def batches():
    return {hom: eb.length_class_batch(hom) for hom in (True, False)}


def test_length_classes_are_the_documented_edges():
    assert eb.length_classes() == [0, 1, 2, 3, 4, 5, 8, 9, 287, 288, 289, 290, 291, 320, 321, 322,
                                   2047, 2048, 2049, 4095, 4096, 8191, 8192]
    assert eb.window_classes() == [3064, 3072, 3073, 3080]
    # 289 units: 288 bigrams = 72 per lane, the last fast length; 321 units: 10 groups of 8 per lane
    q = lambda L: -(-eb.bigrams(L) // eb.LANES_PER_ROW)
    assert q(289) == eb.FAST_MAX_Q and q(290) == eb.FAST_MAX_Q + 1
    assert -(-q(321) // eb.GROUP) == eb.MAX_REG_GROUPS and -(-q(322) // eb.GROUP) == eb.MAX_REG_GROUPS + 1
    assert eb.bigrams(2048) == eb.HALF_BUCKETS - 1 and eb.bigrams(2049) == eb.HALF_BUCKETS


@pytest.mark.parametrize("hash", ["java", "murmur3"])
def test_featurizers_agree_on_the_length_classes(batches, hash):
    F = 1 << 20
    for hom, (raw, meta) in batches.items():
        a = featurize_batch(raw, F, 100, 1000, now_ms=eb.NOW, hash=hash)
        b = featurize_batch_native(raw, F, 100, 1000, now_ms=eb.NOW, hash=hash)
        assert a.n == b.n == raw.n == len(meta)
        assert (a.X != b.X).nnz == 0
        np.testing.assert_array_equal(a.y, b.y)
        # every class has len - 1 bigrams (len for len < 2)
        tot = np.asarray(a.X[:, :F].sum(axis=1)).reshape(-1)
        np.testing.assert_array_equal(tot, [eb.bigrams(L) for _, L in meta])


def test_rows_differ_within_a_class(batches):
    raw, meta = batches[True]
    seen = {}
    for i, m in enumerate(meta):
        seen.setdefault(m, set()).add(raw.text_of(i))
    for (script, L), texts in seen.items():
        if 2 <= L <= eb.SHORT_CLASS_MAX:
            assert len(texts) > 1, (script, L)
    counts = {}
    for m in meta:
        counts[m] = counts.get(m, 0) + 1
    assert all(n == (16 if L <= eb.SHORT_CLASS_MAX else 1) for (_, L), n in counts.items())


def test_wire_round_trip_and_flags(batches):
    h = host()
    for raw, meta in batches.values():
        out = np.zeros(int(h.wire_bound(raw.total_units, raw.n)), np.uint8)
        woff = np.zeros(raw.n + 1, np.int64)
        flags = np.zeros(raw.n, np.uint8)
        nb = int(h.wire_pack(raw.text, raw.offsets, raw.is_retweet, out, woff, flags))
        text, off, is_rt = h.wire_unpack(out[:nb], woff, flags)
        np.testing.assert_array_equal(np.asarray(text), raw.text)
        np.testing.assert_array_equal(np.asarray(off), raw.offsets)
        np.testing.assert_array_equal(np.asarray(is_rt), raw.is_retweet)
        kind = {}
        for (script, L), f in zip(meta, flags):
            if L > 0:
                kind.setdefault(script, set()).add("wide" if f & 2 else "cesu" if f & 4 else "narrow")
        assert kind["ascii"] == {"narrow"} and kind["latin1"] == {"narrow"}
        assert kind["cyrillic"] == {"wide", "cesu"}, kind


def test_wire_sizes_straddle_the_row_word_and_the_decode_window(batches):
    """Per ingest mode: rows on both sides of 8192 wire bytes (kRowLenBits =
    13), and, for UTF-8, non-ASCII rows on both sides of the 6144-byte decode
    window (kDecStage)."""
    raw, meta = batches[False]
    L = np.array([m[1] for m in meta])
    script = np.array([m[0] for m in meta])
    for ingest in ("wire", "utf16", "utf8"):
        nb = eb.wire_bytes_per_row(raw, ingest)
        assert (nb == eb.PACKED_ROW_LIMIT - 1).any() or (nb == eb.PACKED_ROW_LIMIT - 2).any(), ingest
        assert (nb == eb.PACKED_ROW_LIMIT).any(), ingest
        assert (nb > eb.PACKED_ROW_LIMIT).any()
    # narrow / ASCII rows: 8191 and 8192 bytes; UTF-16: 4095 and 4096 units
    nb = eb.wire_bytes_per_row(raw, "wire")
    for s in ("ascii", "latin1"):
        assert nb[(script == s) & (L == 8191)] == 8191 and nb[(script == s) & (L == 8192)] == 8192
    nb = eb.wire_bytes_per_row(raw, "utf8")
    assert nb[(script == "ascii") & (L == 8191)] == 8191 and nb[(script == "ascii") & (L == 8192)] == 8192
    for s in ("latin1", "cyrillic"):
        got = sorted(int(nb[(script == s) & (L == w)][0]) for w in eb.window_classes())
        assert got == [eb.DEC_STAGE - 16, eb.DEC_STAGE, eb.DEC_STAGE + 2, eb.DEC_STAGE + 16], (s, got)


def test_utf8_encoder_accepts_empty_rows():
    raw = eb.empty_rows_batch()
    data, off = host().utf8_encode(raw.text, raw.offsets, 0)
    assert np.asarray(off).tolist() == [0, 0, 0, 0]
    fb = featurize_batch(raw, 1000, 100, 1000, now_ms=eb.NOW)
    assert fb.n == 3 and fb.X[:, :1000].nnz == 0


# --- scalar widths -----------------------------------------------------------

def test_span_cases_cover_every_width():
    sc = eb.span_cases()
    assert sorted({w for w, _ in sc}) == list(range(1, 33)) + [64]
    for w, span in sc:
        assert eb.expected_width(span) == w
    assert eb.expected_width((1 << 32) - 1) == 32 and eb.expected_width(1 << 32) == 64


def test_bit_stream_decoder_round_trips():
    """The pure-numpy reader of the documented stream (little-endian u32
    words, value r at bit r * w) inverts a value-by-value writer, at every
    width, on and off a word boundary, for negative bases."""
    for w, span in eb.span_cases():
        for base in eb.SWEEP_BASES:
            for n in (1, 33, 64):
                col = eb.sweep_column(base, span, n, 7 * w + n)
                buf = eb.encode_scalar_stream(col, w, 0 if w == 64 else base)
                assert len(buf) == (8 * n if w == 64 else 4 * ((n * w + 31) // 32 + 1))
                np.testing.assert_array_equal(eb.decode_scalar_stream(buf, n, w, 0 if w == 64 else base), col)


def test_sweep_batches_reach_their_widths():
    seen = {c: set() for c in range(5)}
    for k, (spans, bases, n, label) in enumerate(eb.sweep_cases()):
        raw = eb.scalar_sweep_batch(spans, bases, n, k, label_sweep=label)
        assert raw.n == n
        sc = raw.scalars
        for c in (range(1) if label else range(1, 5)):
            span = int(sc[c].max()) - int(sc[c].min())
            assert span == (spans[c] if n > 1 else 0), (k, c)
            if n > 1:
                assert sc[c, 0] == sc[c].min() and sc[c, n - 1] == sc[c].max()
            seen[c].add((eb.expected_width(span), n))
        if label:   # the extremes are filtered out; kept labels lie in [100, 1000]
            m = filter_mask(raw, 100, 1000)
            assert not m[0] and not m[n - 1]
        else:
            assert filter_mask(raw, 100, 1000).all()
    assert {w for w, _ in seen[0]} == set(range(1, 33)) | {64}
    for c in range(1, 5):
        for n in eb.SWEEP_ROWS:
            assert {w for w, m in seen[c] if m == n} == set(range(1, 33)) | {64}, (c, n)
    assert any(filter_mask(eb.scalar_sweep_batch(s, b, n, k, True), 100, 1000).any()
               for k, (s, b, n, lab) in enumerate(eb.sweep_cases()) if lab)
    raw = eb.raw_int64_batch()
    for c in range(1, 5):
        assert eb.expected_width(int(raw.scalars[c].max()) - int(raw.scalars[c].min())) == 64
        assert raw.scalars[c].min() < 0 and np.abs(raw.scalars[c]).max() < 1 << 53


# --- SGD inputs --------------------------------------------------------------

@pytest.mark.parametrize("F", [1000, 1 << 20])
def test_oracle_is_stable_at_the_edge_step(batches, F):
    """LENGTH_CLASS_STEP is the largest power of ten at which the oracle's
    loss history is non-increasing on the homogeneous batch and on the
    straddling batch that follows it (ten times more is still monotone on the
    first batch alone but blows the second one up)."""
    def run(step):
        w = np.zeros(F + 4)
        hist = []
        for hom in (True, False):
            fb = featurize_batch_native(batches[hom][0], F, 100, 1000, now_ms=eb.NOW)
            r = run_minibatch_sgd(fb.X, fb.y, w, step, eb.LENGTH_CLASS_ITERS)
            w = r.weights
            hist.append(np.asarray(r.loss_history))
        return w, hist
    w, hist = run(eb.LENGTH_CLASS_STEP)
    assert np.isfinite(w).all()
    for h in hist:
        assert np.all(np.diff(h) <= 0), h
    _, hist10 = run(10 * eb.LENGTH_CLASS_STEP)
    assert any(np.any(np.diff(h) > 0) for h in hist10)


def test_oracle_is_finite_on_the_tiny_slices():
    """Warm-started fp64 SGD over the tiny batches of
    test_tiny_and_boundary_batches: finite, loss never explodes."""
    F = 1000
    cfg = SynthConfig.profile("twitter", seed=41, unicode_fraction=0.1)
    warm = generate_batch(cfg, 0, 2500, batch_time_ms=eb.NOW)
    fb = featurize_batch(warm, F, 100, 1000)
    w = run_minibatch_sgd(fb.X, fb.y, np.zeros(F + 4), 0.005, 50).weights
    for raw in eb.tiny_batches(cfg):
        fb = featurize_batch(raw, F, 100, 1000)
        r = run_minibatch_sgd(fb.X, fb.y, w, 0.005, 50)
        w = r.weights
        assert np.isfinite(w).all() and np.isfinite(r.loss_history).all()
        assert max(r.loss_history) <= 10 * r.loss_history[0] + 1.0, (fb.n, r.loss_history)


def test_junk_rows_keep_the_kept_rows():
    cfg = SynthConfig.profile("twitter", seed=43)
    raw = generate_batch(cfg, 0, 300, batch_time_ms=eb.NOW)
    junk = eb.with_junk_rows(raw)
    assert junk.n == raw.n + 60
    a = featurize_batch_native(raw, 1000, 100, 1000, now_ms=eb.NOW)
    b = featurize_batch_native(junk, 1000, 100, 1000, now_ms=eb.NOW)
    assert a.n == b.n and (a.X != b.X).nnz == 0
    np.testing.assert_array_equal(a.y, b.y)
    # the junk sets the encodings: raw int64 columns, a row no row word holds
    for c in range(5):
        assert eb.expected_width(int(junk.scalars[c].max()) - int(junk.scalars[c].min())) == 64
    assert (np.diff(junk.offsets) == 9000).any() and (np.diff(junk.offsets) == 0).any()


def test_filter_boundary_batch_meets_every_value_with_both_flags():
    raw = eb.filter_boundary_batch()
    rc, rt = raw.scalars[0], raw.is_retweet
    for v in (99, 100, 101, 999, 1000, 1001, -1, 0, 1 << 31, -(1 << 31)):
        assert set(rt[rc == v].tolist()) == {0, 1}, v
    assert np.abs(rc[(rc >= 99) & (rc <= 1001)]).max() <= 1 << 24

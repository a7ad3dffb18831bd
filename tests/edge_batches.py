"""Deterministic raw batches that sit on the engine's hard thresholds.

Every builder is a pure function of its arguments (fixed seeds only), so the
CPU suite (``test_edge_batches_cpu.py``) can check that a batch is where it
claims to be before the GPU suite relies on it.  The constants mirror
``csrc/hip``; each derived value names the constant it comes from, so a
changed constant shows up here as a wrong edge, loudly, in the
reached-the-edge assertions of ``test_gpu_edge_shapes.py``.
"""
import numpy as np

from twitter_stream_ml_amd.records.batch import RawBatch, utf16_units

NOW = 1_700_000_000_000

# --- constants of csrc/hip (keep in step) ----------------------------------
LANES_PER_ROW = 4        # common.h kLanesPerRow: a row's bigrams go to 4 lanes in contiguous quarters
ROWS_PER_CHUNK = 16      # common.h kRowsPerChunk
GROUP = 8                # common.h kGroup: entries per lane per group
FAST_MAX_Q = 72          # narrow_text.h kFastMaxQ: bigrams per lane of the narrow fast featurizer
MAX_REG_GROUPS = 10      # common.h kMaxRegGroups: groups per lane the hybrid / dedup layouts keep
HALF_BUCKETS = 2048      # featurize.hip kHalfBuckets = kLenBuckets / 2: length-sort bucket clamp
DEC_STAGE = 6144         # featurize.hip kDecStage: bytes of the UTF-8 decoder's LDS stage window
ROW_LEN_BITS = 13        # kernels.h kRowLenBits: a packed row word holds byte lengths < 2^13
SEG_ROWS = 4096          # featurize.hip kSegRows: rows per filter / sort segment
ROW_TILE = 8192          # featurize.hip kRowTile: rows per tile of the row-word scan

LAST_FAST = LANES_PER_ROW * FAST_MAX_Q + 1                  # 289 units = 288 bigrams = 72 per lane
LAST_REG = LANES_PER_ROW * GROUP * MAX_REG_GROUPS + 1       # 321 units = 320 bigrams = 10 groups
WINDOW_UNITS = DEC_STAGE // 2                               # 3072 two-byte units fill the stage window
PACKED_ROW_LIMIT = 1 << ROW_LEN_BITS                        # 8192 wire bytes no longer fit a row word


def bigrams(n_units):
    """Entries of a row: Scala's ``sliding(2)`` gives len - 1 windows, and one
    (shorter) window for a 1-unit string (featurize.hip, narrow_text.h, kmeans.hip)."""
    return n_units - 1 if n_units >= 2 else n_units


def length_classes():
    """Row lengths (UTF-16 units) on both sides of every length threshold."""
    return sorted({
        0, 1, 2,                                  # bigram count len >= 2 ? len - 1 : len
        3, 4, 5, 8, 9,                            # 4 lanes per row: lanes with 0 entries, uneven quarters
        LAST_FAST - 2, LAST_FAST - 1, LAST_FAST, LAST_FAST + 1, LAST_FAST + 2,   # 287..291: per_lane <= kFastMaxQ
        LAST_REG - 1, LAST_REG, LAST_REG + 1,     # 320..322: L8 <= kMaxRegGroups
        HALF_BUCKETS - 1, HALF_BUCKETS, HALF_BUCKETS + 1,   # 2047..2049: bucket clamp at kHalfBuckets - 1 bigrams
        PACKED_ROW_LIMIT // 2 - 1, PACKED_ROW_LIMIT // 2,   # 4095 / 4096: 8190 / 8192 bytes as UTF-16
        PACKED_ROW_LIMIT - 1, PACKED_ROW_LIMIT,   # 8191 / 8192: bytes of a narrow / ASCII row
    })


def window_classes():
    """Lengths of rows of two-byte characters around the decoder's stage
    window: 6128, 6144, 6146 and 6160 UTF-8 bytes (kDecStage = 6144)."""
    return [WINDOW_UNITS - 8, WINDOW_UNITS, WINDOW_UNITS + 1, WINDOW_UNITS + 8]


SHORT_CLASS_MAX = LAST_REG + 1   # classes up to 322 units get 16 rows each in the homogeneous batch

# alphabets: (mixed with ASCII, two-byte characters only)
SCRIPTS = {
    "ascii": ("aB cD,eF.gH!iJ kLmNoPqRsTuVwXyZ 0123456789#@", None),
    # narrow on the wire (every unit < 256), two bytes per non-ASCII unit in UTF-8
    "latin1": ("éAüb ÖñÇ dÉàÔ xÿÑ",
               "éÜöÑçÀÔÿßæÅ"),
    # mixed: cesu on the wire (smaller than UTF-16); pure: wide
    "cyrillic": ("Жжa ПрИвЕт b МиР 1",
                 "ЖжПрИвЕтМиРдЯю"),
}


def make_text(script, n_units, rot=0, pure=False):
    """n_units of the script's alphabet, rotated by rot (rows of one class differ)."""
    mixed, two = SCRIPTS[script]
    alpha = two if pure else mixed
    rot %= len(alpha)
    while script != "ascii" and ord(alpha[rot]) < 0x80:   # even a 1-unit row is of its script
        rot = (rot + 1) % len(alpha)
    alpha = alpha[rot:] + alpha[:rot]
    return (alpha * (n_units // len(alpha) + 1))[:n_units]


def texts_to_raw(texts, is_rt, scalars, now=NOW):
    """RawBatch of Python strings (UTF-16 units + cumulative offsets)."""
    units = [utf16_units(t) for t in texts]
    off = np.zeros(len(texts) + 1, np.int64)
    off[1:] = np.cumsum([u.shape[0] for u in units])
    text = np.concatenate(units) if units else np.zeros(0, np.uint16)
    return RawBatch(text, off, np.asarray(is_rt, np.uint8), np.asarray(scalars, np.int64).reshape(5, len(texts)),
                    now)


def ordinary_scalars(n, seed, now=NOW):
    """Scalars of n rows that all pass the default filter: rc in [100, 1000]."""
    rng = np.random.default_rng(seed)
    sc = np.zeros((5, n), np.int64)
    sc[0] = 100 + (np.arange(n) * 37) % 901
    sc[1] = rng.integers(0, 1_000_000, n)
    sc[2] = rng.integers(0, 50_000, n)
    sc[3] = rng.integers(0, 5_000, n)
    sc[4] = now - rng.integers(0, 10_000_000_000, n)
    return sc


# Largest power of ten at which the fp64 oracle's loss history is
# non-increasing on the homogeneous length-class batch (from zero weights) and
# on the straddling batch trained after it.  Rows of thousands of repeats of
# one bigram make the reference's 0.005 diverge; 1e-4 is still monotone on the
# first batch but takes the second one to a loss of 1e18.
# test_edge_batches_cpu.py::test_oracle_is_stable_at_the_edge_step re-derives it.
LENGTH_CLASS_STEP = 1e-5
LENGTH_CLASS_ITERS = 10


def length_class_batch(homogeneous, now=NOW):
    """The length classes in three scripts, every row a retweet with rc in
    [100, 1000].  homogeneous: classes up to 322 units have 16 rows each
    (rotated alphabets), so after the narrow-then-wide, descending-length sort
    whole chunks hold one class; longer classes one row each.  Otherwise one
    row per class (chunks straddle classes).  Returns (raw, meta) with
    meta[i] = (script, units)."""
    texts, meta = [], []
    for script in SCRIPTS:
        for L in length_classes():
            reps = ROWS_PER_CHUNK if (homogeneous and L <= SHORT_CLASS_MAX) else 1
            for r in range(reps):
                texts.append(make_text(script, L, rot=r + L))
                meta.append((script, L))
        if script != "ascii":
            for L in window_classes():
                texts.append(make_text(script, L, rot=L, pure=True))
                meta.append((script, L))
    if homogeneous:
        # The single long rows sort ahead of the 16-row classes, narrow rows
        # ahead of wide ones: fill both groups of singles up to a multiple of
        # 16 (with lengths between the classes), so every class starts a chunk.
        long_classes = [L for L in length_classes() if L > SHORT_CLASS_MAX]
        narrow = 2 * len(long_classes) + len(window_classes())   # ascii + latin1, latin1 window rows
        wide = len(long_classes) + len(window_classes())         # cyrillic
        for i in range(-narrow % ROWS_PER_CHUNK):
            texts.append(make_text("ascii", 400 + 50 * i, rot=i))
            meta.append(("ascii", 400 + 50 * i))
        for i in range(-wide % ROWS_PER_CHUNK):
            texts.append(make_text("cyrillic", 425 + 50 * i, rot=i, pure=True))
            meta.append(("cyrillic", 425 + 50 * i))
    n = len(texts)
    return texts_to_raw(texts, np.ones(n, np.uint8), ordinary_scalars(n, 101, now), now), meta


def empty_rows_batch(n=3, now=NOW):
    """Only empty rows, all kept: an empty active set with n_kept > 0."""
    return texts_to_raw([""] * n, np.ones(n, np.uint8), ordinary_scalars(n, 102, now), now)


def wire_bytes_per_row(raw, ingest):
    """Bytes of each row as the ingest mode ships it (what a row word must hold)."""
    from twitter_stream_ml_amd.ops._native import host
    if ingest == "utf16":
        return 2 * np.diff(raw.offsets)
    if ingest == "utf8":
        _, off = host().utf8_encode(raw.text, raw.offsets, 0)
        return np.diff(np.asarray(off))
    h = host()
    out = np.zeros(int(h.wire_bound(raw.total_units, raw.n)), np.uint8)
    woff = np.zeros(raw.n + 1, np.int64)
    flags = np.zeros(raw.n, np.uint8)
    h.wire_pack(raw.text, raw.offsets, raw.is_retweet, out, woff, flags)
    return np.diff(woff)


# --- scalar wire widths ------------------------------------------------------

def expected_width(span):
    """Bits per value of a column with max - min = span (engine.cpp pack_scalars)."""
    return 64 if span >= 1 << 32 else max(1, int(span).bit_length())


def span_cases():
    """(width, span): both ends of every width class 1..32, and 2^32 -> raw int64."""
    out = [(1, 0), (1, 1)]
    for w in range(2, 33):
        out += [(w, 1 << (w - 1)), (w, (1 << w) - 1)]
    out.append((64, 1 << 32))
    return out


SWEEP_BASES = (0, -12345, 10 ** 9)
SWEEP_ROWS = (33, 64)   # n * w off / on a 32-bit word boundary (64: the last value's second word is the slack word)


def sweep_column(base, span, n, seed):
    """n values in [base, base + span], the extremes at rows 0 and n - 1."""
    rng = np.random.default_rng(seed)
    v = base + rng.integers(0, span + 1, n, dtype=np.int64)
    v[0] = base
    v[n - 1] = base + span
    return v


def scalar_sweep_batch(spans, bases, n, seed, label_sweep=False, now=NOW):
    """A batch of n two-unit rows whose scalar columns have the given spans /
    bases (lists of 5; column 0's are ignored unless label_sweep).

    label_sweep=False: every row is kept (rc in [100, 1000]), columns 1..4
    carry the sweep.  label_sweep=True: column 0 carries it; rows 0 and n - 1
    (the extremes) are non-retweets and the retweet flag of the others
    alternates, so filtered-out rows set the label column's encoding; half of
    the remaining rows take labels in [100, 1000] where the range allows it.
    Column 1 then holds the row index (identifies the kept rows)."""
    sc = np.zeros((5, n), np.int64)
    is_rt = np.ones(n, np.uint8)
    for c in range(1, 5):
        sc[c] = sweep_column(bases[c], spans[c], n, seed + c) if n > 1 else bases[c]
    if label_sweep:
        col = sweep_column(bases[0], spans[0], n, seed)
        lo, hi = max(100, bases[0]), min(1000, bases[0] + spans[0])
        if lo <= hi:
            inside = lo + (np.arange(n) * 131) % (hi - lo + 1)
            col[1:n - 1:2] = inside[1:n - 1:2]
        sc[0] = col
        sc[1] = np.arange(n)
        is_rt[:] = np.arange(n) % 4 != 3
        is_rt[0] = is_rt[n - 1] = 0
    else:
        sc[0] = 100 + (np.arange(n) * 53 + seed) % 901
    return texts_to_raw(["ab"] * n, is_rt, sc, now)


def raw_int64_batch(n=33, now=NOW):
    """Values near +-2^40 in every column but the label (|v| < 2^53: exact in
    the fp64 oracle): raw int64 columns, negative values included."""
    sc = np.zeros((5, n), np.int64)
    sign = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int64)
    sc[0] = 100 + (np.arange(n) * 29) % 901
    for c in range(1, 5):
        sc[c] = sign * ((1 << 40) + 1000 * c + np.arange(n))
    return texts_to_raw(["ab"] * n, np.ones(n, np.uint8), sc, now)


def sweep_cases():
    """(spans[5], bases[5], n, label_sweep) of the scalar-width sweep.  Columns
    1..4 run through every (width, span end) x base x row count; column c is
    offset by 13 c span cases so one batch mixes widths.  The label column
    (junk-driven) takes every span once, with bases and row counts rotating."""
    sc = span_cases()
    out = []
    k = 0
    for base in SWEEP_BASES:
        for n in SWEEP_ROWS:
            for i in range(len(sc)):
                spans = [0] + [sc[(i + 13 * c) % len(sc)][1] for c in range(1, 5)]
                # column 4 = createdAt: one base beyond `now` (negative age)
                bases = [0, base, base, base, NOW + 1000 if (i + k) % 4 == 0 else base]
                out.append((spans, bases, n, False))
            k += 1
    for i, (_, span) in enumerate(sc):
        base = SWEEP_BASES[i % 3]
        n = SWEEP_ROWS[(i // 3) % 2]
        out.append(([span, 7, 3, 1, 1000], [base, 0, 0, 0, NOW - 5000], n, True))
    for base in SWEEP_BASES:   # one row: span 0, width 1, n * w = 1 bit
        out.append(([0] * 5, [0, base, base, base, base], 1, False))
    return out


def decode_scalar_stream(buf, n, bits, base):
    """Pure-numpy reader of one packed scalar column: little-endian u32 words,
    value r at bit r * bits (an offset from base), or raw int64 (bits == 64)."""
    buf = np.ascontiguousarray(buf, np.uint8)
    if bits == 64:
        return buf[:8 * n].view("<i8").astype(np.int64)
    words = buf[:(len(buf) // 4) * 4].view("<u4").astype(np.uint64)
    off = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    w0 = (off >> np.uint64(5)).astype(np.int64)
    sh = off & np.uint64(31)
    pair = words[w0] | (words[w0 + 1] << np.uint64(32))
    mask = np.uint64((1 << bits) - 1)
    return (np.int64(base) + ((pair >> sh) & mask).astype(np.int64)).astype(np.int64)


def encode_scalar_stream(col, bits, base):
    """The documented stream of one column, written value by value (the
    decoder's counterpart): ceil(n * bits / 32) words plus one slack word."""
    col = np.asarray(col, np.int64)
    n = col.shape[0]
    if bits == 64:
        return col.astype("<i8").view(np.uint8).copy()
    acc = 0
    for r, v in enumerate(col.tolist()):
        x = v - base
        assert 0 <= x < (1 << bits), (v, base, bits)
        acc |= x << (r * bits)
    nw = (n * bits + 31) // 32 + 1
    return np.frombuffer(acc.to_bytes(4 * nw, "little"), np.uint8).copy()


# --- batch sizes -------------------------------------------------------------

TINY_SIZES = (1, 2, 15, 16, 17, 63, 64, 65)   # around 16 rows per chunk and 64 lanes
TINY_EVERY_THIRD = (17, 65)                   # kept rows = every third row of a 3n-row raw batch


def tiny_batches(cfg, start=5000):
    """Batches of TINY_SIZES kept rows: consecutive slices of one generator
    batch with every row forced through the filter; for TINY_EVERY_THIRD the
    kept rows are rows 0, 3, 6, ... of 3n raw rows (kept index != raw index)."""
    from twitter_stream_ml_amd.sources.synthetic import generate_batch
    pool = generate_batch(cfg, start, 3 * sum(TINY_SIZES), batch_time_ms=NOW)
    pool.is_retweet[:] = 1
    pool.scalars[0] = 100 + (np.arange(pool.n) * 37) % 901
    out, at = [], 0
    for n in TINY_SIZES:
        m = 3 * n if n in TINY_EVERY_THIRD else n
        raw = pool.slice(at, at + m)
        raw = RawBatch(raw.text.copy(), raw.offsets.copy(), raw.is_retweet.copy(), raw.scalars.copy(), NOW)
        if m != n:
            raw.is_retweet[:] = np.arange(m) % 3 == 0
        out.append(raw)
        at += m
    return out


def kmeans_tiny_batch(cfg, m, start, short_texts=False, equal_followers=False):
    """3 m + 2 generator rows of which m (every third) are retweets; with
    short_texts the first retweets carry texts of 0, 1 and 2 units (bigram
    count len >= 2 ? len - 1 : len, kmeans.hip); equal_followers makes the
    followers column constant (zero variance: std == 0, scale factor 0)."""
    from twitter_stream_ml_amd.sources.synthetic import generate_batch
    raw = generate_batch(cfg, start, 3 * m + 2, batch_time_ms=NOW)
    texts = [raw.text_of(i) for i in range(raw.n)]
    is_rt = np.zeros(raw.n, np.uint8)
    is_rt[1:3 * m:3] = 1
    assert int(is_rt.sum()) == m
    if short_texts:
        for j, t in zip(np.nonzero(is_rt)[0], ("", "a", "ab")):
            texts[j] = t
    sc = raw.scalars.copy()
    if equal_followers:
        sc[1] = 777
    return texts_to_raw(texts, is_rt, sc, NOW)


# --- filter boundaries -------------------------------------------------------

def filter_boundary_batch(begin=100, end=1000, n=200, now=NOW):
    """Ordinary short rows whose rc cycles through the filter's boundary values
    (and the int32 extremes), retweet flag alternating.  Column 1 holds the row
    index, so the kept rows and their order can be read back exactly."""
    cyc = [begin - 1, begin, begin + 1, end - 1, end, end + 1, -1, 0, 1 << 31, -(1 << 31), 500]
    sc = ordinary_scalars(n, 103, now)
    sc[0] = [cyc[i % len(cyc)] for i in range(n)]
    sc[1] = np.arange(n)
    # the flag pattern has period 3, the rc cycle 11: every value meets both flags
    is_rt = (np.arange(n) % 3 != 1).astype(np.uint8)
    texts = [make_text(("ascii", "latin1", "cyrillic")[i % 3], 20 + i % 50, rot=i) for i in range(n)]
    return texts_to_raw(texts, is_rt, sc, now)


# --- junk rows ---------------------------------------------------------------

JUNK_TEXTS = ["", "Ж" * 9000, "İ", "ΟΔΟΣ", "\U00010400ΣΑ", "x", "no retweet"]


def with_junk_rows(raw, now=None):
    """raw's rows in order, interleaved with rows the default filter drops:
    non-retweets and out-of-range rc, with empty text, a 9000-unit Cyrillic
    row (no row word holds it; wide), special-lowering rows, and scalars of
    +-2^40 (raw int64 columns, negative bases)."""
    texts, is_rt, cols = [], [], []
    j = 0
    for i in range(raw.n):
        if i % 5 == 0:
            t = JUNK_TEXTS[j % len(JUNK_TEXTS)]
            big = (1 << 40) + j
            if j % 2 == 0:    # a retweet with rc outside [100, 1000]
                texts.append(t); is_rt.append(1)
                cols.append([(-big, 1001, 99, big)[(j // 2) % 4], big, -big, big, -big])
            else:             # not a retweet, rc inside the range
                texts.append(t); is_rt.append(0)
                cols.append([500, -big, big, -big, big])
            j += 1
        texts.append(raw.text_of(i)); is_rt.append(int(raw.is_retweet[i]))
        cols.append(raw.scalars[:, i].tolist())
    sc = np.asarray(cols, np.int64).T
    return texts_to_raw(texts, is_rt, sc, raw.batch_time_ms if now is None else now)

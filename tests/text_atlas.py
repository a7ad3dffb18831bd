"""Deterministic raw batches that walk the device text path end to end.

The synthetic generator draws a few hundred characters and rows of 20..280
units, so the UTF-8 decoder, the special-row detection and the lower-casing
tables are otherwise only exercised on a thin slice of their input space.
The builders here are pure functions (fixed seeds) in the style of
``edge_batches.py``: every UTF-16 unit value in every row kind the
featurizers distinguish, a multi-byte sequence on every split of every
boundary the decoder has, rows around its stage window, and a batch whose
rows are all special.  ``test_text_atlas_cpu.py`` proves on the CPU that each
batch is where it claims to be; ``test_gpu_text_atlas.py`` compares the
device with the host oracle on them, exactly.

The constants mirror ``csrc/hip``; each names the constant it comes from.
"""
import os
import re

import numpy as np

from edge_batches import NOW, DEC_STAGE, LAST_FAST, ordinary_scalars, texts_to_raw
from twitter_stream_ml_amd.records.batch import RawBatch, Utf8Text, units_to_str, utf16_units

# --- constants of csrc/hip (keep in step) ----------------------------------
STAGE_BYTES = 640        # text_stage.h kStageWords * 4: bytes of a row the featurizers stage in LDS
KM_STAGE_BYTES = 768     # kmeans.hip k_km_features_bal: ndw <= 3 * kWave dwords per staged row
LOWER_LDS_BLOCKS = 7     # text_stage.h kLowerLdsBlocks: delta blocks 0..6 in LDS, the others in global memory
WAVE_STEP = 256          # featurize.hip decode_step: 64 lanes x one dword per wave step
STAGE_ALIGN = 16         # featurize.hip k_cesu_decode: the stage window starts at o & ~15
GROUP_ROWS = 64          # featurize.hip k_cesu_decode: one wave per 64-row group
KM_CHUNK_DIMS = 256      # kmeans.hip kKmChunkDims: text_dims above it take the generic k_km_features
ROW_WORD_LIMIT = 1 << 13  # kernels.h kRowLenBits: byte lengths a packed row word holds

# k-means text widths of the GPU test.  The primes: an unlowered unit u - d in
# place of u moves a bigram's hash by d or 31 d, which changes its bucket
# unless the width divides that (test_text_atlas_cpu.py checks every delta of
# the tables).  256 / 257: both sides of kKmChunkDims; 300: the generic kernel.
KM_BAL_DIMS = (61, 113)
KM_EDGE_DIMS = (KM_CHUNK_DIMS, KM_CHUNK_DIMS + 1, 300)
KM_PRIME_DIMS = (61, 113, KM_CHUNK_DIMS + 1)

TABLES_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "csrc", "common", "unicode_tables.h")


def _table_source():
    with open(TABLES_H, encoding="utf-8") as f:
        return f.read()


def tables_unicode_version():
    """The Unicode version named in the header of unicode_tables.h."""
    return re.search(r"Unicode (\d+\.\d+\.\d+)", _table_source()).group(1)


def _braced_ints(src, name):
    body = src[src.index(name):]
    body = body[body.index("=") + 1:body.index(";")]
    return [int(x) for x in re.findall(r"\d+", body)]


def lower_tables():
    """(page[256], blocks[n][256], supp[(cp, lower)]) parsed from
    unicode_tables.h: uni::kLowerPage, uni::kLowerBlocks, uni::kSuppLower."""
    src = _table_source()
    page = _braced_ints(src, "kLowerPage[256]")
    flat = _braced_ints(src, "kLowerBlocks[")
    assert len(page) == 256 and len(flat) % 256 == 0
    blocks = [flat[i:i + 256] for i in range(0, len(flat), 256)]
    sl = _braced_ints(src, "kSuppLower[")
    return page, blocks, list(zip(sl[0::2], sl[1::2]))


def unit_deltas():
    """{lower(u) - u} over every unit whose per-unit lowering changes it, plus
    the deltas of the astral table (they move the low surrogate)."""
    page, blocks, supp = lower_tables()
    out = set()
    for u in range(0x10000):
        d = ((u + blocks[page[u >> 8]][u & 255]) & 0xFFFF) - u
        if d:
            out.add(d)
    out |= {lo - cp for cp, lo in supp}
    return out


# --- every code unit ---------------------------------------------------------

SHORT_UNITS = 64          # 128 B as UTF-16: staged
LONG_UNITS = 512          # 1024 B as UTF-16: beyond kStageWords (and k-means' 768 B)
INTER_UNITS = 64          # atlas units per interleaved row (each followed by an ASCII unit)
INTER_TAIL = " ok"        # keeps a row of 3-byte units smaller as cesu than as UTF-16 (wire.cpp row_kind)
LATIN_ROWS = 64           # four fast chunks of 16
LATIN_UNITS = 259         # odd: every row starts at another alignment; <= LAST_FAST (289)
LATIN_LONG_ROWS = 16      # one whole chunk of narrow rows beyond the 640-B stage
LATIN_LONG_UNITS = 781         # > 768 B: unstaged in the k-means featurizer too
ASTRAL_ROW_CPS = 60       # code points per astral row (<= 64)
UNCASED_ASTRAL = (0x10000, 0x20000)   # Linear B syllable B008 A, CJK extension B: letters without case
EMOJI = 0x1F600

assert LATIN_UNITS <= LAST_FAST and LATIN_LONG_UNITS > KM_STAGE_BYTES > STAGE_BYTES


def _cps_to_str(cps):
    return "".join(chr(c) for c in cps)


def astral_code_points():
    """Every code point of uni::kSuppLower with its neighbours on both sides
    and its lower case, two uncased astral letters and one emoji, ascending."""
    _, _, supp = lower_tables()
    s = set(UNCASED_ASTRAL) | {EMOJI}
    for cp, lo in supp:
        s |= {cp - 1, cp, cp + 1, lo}
    return sorted(s)


def codepoint_atlas(now=NOW):
    """Every UTF-16 unit value 0x0000..0xFFFF in each row kind.

    short    row r = units 64 r .. 64 r + 63 (128 B wide: staged).  The rows
             D800.. hold high surrogates only and DC00.. low ones only, so
             every surrogate stays lone.
    long     rows of 512 consecutive units (1024 B wide: read from global
             memory by the featurizers and the k-means kernels).
    inter    ``u, 'a', u + 1, 'B', ...`` and an ASCII tail: every unit between
             ASCII neighbours; cesu on the wire from U+0100 on, UTF-8 rows of
             1- to 3-byte sequences.
    latin1   64 rows of 259 units, row r = (r + j) mod 256: every byte value
             in every byte lane of the SWAR lower-casing, four fast chunks;
    latin1-long  16 narrow rows of 781.. units: beyond the 640-B stage.
    astral   surrogate pairs: every cased astral code point with both
             neighbours, two uncased astral letters, one emoji; and rows where
             an astral cased letter precedes / follows U+03A3.
    Every row is a retweet with rc in [100, 1000].  Returns (raw, meta) with
    meta[i] = (kind, first unit or code point of the row)."""
    texts, meta = [], []
    for r in range(0x10000 // SHORT_UNITS):
        u = np.arange(r * SHORT_UNITS, (r + 1) * SHORT_UNITS, dtype=np.uint16)
        texts.append(units_to_str(u))
        meta.append(("short", r * SHORT_UNITS))
    for r in range(0x10000 // LONG_UNITS):
        u = np.arange(r * LONG_UNITS, (r + 1) * LONG_UNITS, dtype=np.uint16)
        texts.append(units_to_str(u))
        meta.append(("long", r * LONG_UNITS))
    tail = utf16_units(INTER_TAIL)
    for r in range(0x10000 // INTER_UNITS):
        u = np.zeros(2 * INTER_UNITS, np.uint16)
        u[0::2] = np.arange(r * INTER_UNITS, (r + 1) * INTER_UNITS)
        u[1::4] = ord("a")
        u[3::4] = ord("B")
        texts.append(units_to_str(np.concatenate([u, tail])))
        meta.append(("inter", r * INTER_UNITS))
    for r in range(LATIN_ROWS):
        texts.append(units_to_str(((r + np.arange(LATIN_UNITS)) % 256).astype(np.uint16)))
        meta.append(("latin1", r))
    for r in range(LATIN_LONG_ROWS):
        n = LATIN_LONG_UNITS + 2 * r
        texts.append(units_to_str(((16 * r + 7 * np.arange(n)) % 256).astype(np.uint16)))
        meta.append(("latin1-long", 16 * r))
    cps = astral_code_points()
    for i in range(0, len(cps), ASTRAL_ROW_CPS):
        texts.append(_cps_to_str(cps[i:i + ASTRAL_ROW_CPS]))
        meta.append(("astral", cps[i]))
    _, _, supp = lower_tables()
    for k in range(0, len(supp), 37):          # one letter of every astral script
        cp = supp[k][0]
        for t in (chr(cp) + "Σ", "Σ" + chr(cp), "a" + chr(cp) + "Σ b" + chr(cp + 1),
                  chr(supp[k][1]) + "ΣΣ" + chr(EMOJI)):
            texts.append(t)
            meta.append(("astral-sigma", cp))
    n = len(texts)
    return texts_to_raw(texts, np.ones(n, np.uint8), ordinary_scalars(n, 201, now), now), meta


# --- UTF-8 positions -----------------------------------------------------------

# (name, hand-written bytes, code point or None).  The Latin-1 probes keep a
# row class 1 (every byte < 0xC4); the ``+c2`` variants put them into a row that
# holds a class-2 character (Cyrillic, D0 B6) elsewhere.
PROBES = [
    ("U+0080", b"\xc2\x80", 0x80),
    ("U+00FF", b"\xc3\xbf", 0xFF),
    ("U+0080+c2", b"\xc2\x80", 0x80),
    ("U+00FF+c2", b"\xc3\xbf", 0xFF),
    ("U+0100", b"\xc4\x80", 0x100),               # the first class-2 lead byte
    ("U+07FF", b"\xdf\xbf", 0x7FF),
    ("U+0800", b"\xe0\xa0\x80", 0x800),
    ("U+FFFF", b"\xef\xbf\xbf", 0xFFFF),
    ("U+10000", b"\xf0\x90\x80\x80", 0x10000),    # F0 90: flagged, not cased
    ("U+10FFFF", b"\xf4\x8f\xbf\xbf", 0x10FFFF),
    ("U+4E2D", b"\xe4\xb8\xad", 0x4E2D),
    ("U+1F600", b"\xf0\x9f\x98\x80", 0x1F600),    # F0 9F is not a special pair
    ("U+0130", b"\xc4\xb0", 0x130),
    ("U+03A3", b"\xce\xa3", 0x3A3),
    ("U+10400", b"\xf0\x90\x90\x80", 0x10400),
    ("U+1E900", b"\xf0\x9e\xa4\x80", 0x1E900),
    ("U+10400 cesu", b"\xed\xa0\x81\xed\xb0\x80", None),   # D801 DC00 as two 3-byte sequences
]
CLASS2 = b"\xd0\xb6"      # U+0436
STEP_BOUNDARIES = (WAVE_STEP, 2 * WAVE_STEP)
_FILL = b"aBcDeFgHiJkLmNoPqRsTuVwXyZ"


def _filler(n, rot):
    return bytes(_FILL[(rot + i) % len(_FILL)] for i in range(n))


def _probe_row(name, seq, p, tail, rot):
    """Cased ASCII letters up to byte p, the probe, a space and ``tail - 1``
    more letters (tail 0: the probe ends the row)."""
    head = _filler(p, rot)
    rest = (b" " + _filler(tail - 1, rot + 3)) if tail > 0 else b""
    if name.endswith("+c2"):
        if p >= 2:
            head = CLASS2 + head[2:]
        else:
            assert tail >= 3
            rest = rest[:-2] + CLASS2
    return head + seq + rest


def utf8_position_sweep(now=NOW):
    """Rows of ASCII letters with one probe sequence each, as UTF-8 bytes
    written by hand (``raw.utf8``; ``raw.text`` is their decoding), and ASCII
    pad rows of 0..15 bytes that set the next row's start alignment.

    With o the row's byte offset in the batch, p the probe's offset in the
    row and rel = (o mod 4) + p (the probe's offset from the row's first
    aligned dword, which is where the decoder's 256-byte wave steps start),
    the rows of every probe of L bytes cover: rel = 256 - L + 1 .. 256 and
    512 - L + 1 .. 512 (every split across a step boundary, and the first byte
    of a step), every rel mod 4, p = 0, and the probe as the row's last bytes.
    Row starts cycle through every o mod 16.  The first three rows are probe
    rows without pad rows between them, which makes the number of non-ASCII
    rows of the first 64-row group odd.  Returns (raw, meta); meta[i] is None
    for a pad row, else a dict: probe, L, p, o, rel, nbytes, last."""
    plan = []   # (probe index, rel or None, p or None, tail)
    for k, (name, seq, _) in enumerate(PROBES):
        L = len(seq)
        for B in STEP_BOUNDARIES:
            for rel in range(B - L + 1, B + 1):
                plan.append((k, rel, None, 5 + (rel + k) % 7))
        for j in range(4):                       # every dword split, whatever the start
            plan.append((k, 8 + j, None, 4 + j))
        plan.append((k, None, 0, 6))             # p = 0
        plan.append((k, None, 11 + k, 0))        # the probe ends the row
        plan.append((k, STEP_BOUNDARIES[1] - 1, None, 0))   # ... and is cut by a step boundary
    rows, meta = [], []
    o = 0
    for i, (k, rel, p, tail) in enumerate(plan):
        name, seq, _ = PROBES[k]
        if i >= 3:
            want = (5 * i + 3) % STAGE_ALIGN     # 5 is a unit mod 16: every alignment, every o mod 4 per probe
            pad = (want - o) % STAGE_ALIGN
            rows.append(_filler(pad, i))
            meta.append(None)
            o += pad
        if p is None:
            p = rel - o % 4
        b = _probe_row(name, seq, p, tail, i)
        rows.append(b)
        meta.append({"probe": name, "L": len(seq), "p": p, "o": o, "rel": o % 4 + p, "nbytes": len(b),
                     "last": tail == 0})
        o += len(b)
    return _utf8_rows_to_raw(rows, 202, now), meta


def _utf8_rows_to_raw(rows, seed, now):
    """RawBatch of rows given as UTF-8 bytes: ``utf8`` holds the bytes as they
    are, ``text`` what a decoder must make of them (Python's, with surrogates
    passed through: a CESU-8 pair becomes the surrogate pair)."""
    boff = np.zeros(len(rows) + 1, np.int64)
    boff[1:] = np.cumsum([len(b) for b in rows])
    data = np.frombuffer(b"".join(rows), np.uint8).copy()
    texts = [b.decode("utf-8", "surrogatepass") for b in rows]
    n = len(rows)
    raw = texts_to_raw(texts, np.ones(n, np.uint8), ordinary_scalars(n, seed, now), now)
    return RawBatch(raw.text, raw.offsets, raw.is_retweet, raw.scalars, now, utf8=Utf8Text(data, boff))


TRUNCATED = b"\xf0\x9f\x98"   # U+1F600 without its last byte


def truncated_tail_batch(first, now=NOW):
    """The one malformed case: four rows of ASCII letters that end in a
    four-byte lead with only two continuation bytes, the lead on each byte
    lane of a dword (rel mod 4 = 0..3), each followed by an ASCII row whose
    first byte is ``first``.  What such a row decodes to is not specified,
    but it must not depend on the next row's bytes.  Returns (raw, bad rows);
    ``raw.text`` holds U+FFFD for the truncated sequence (unit counts only)."""
    rows, bad, o = [], [], 0
    for j in range(4):
        p = 8 + (j - o) % 4
        rows.append(_filler(p, j) + TRUNCATED)
        bad.append(len(rows) - 1)
        o += len(rows[-1])
        rows.append(bytes([first]) + _filler(6 + j, j + 1))
        o += len(rows[-1])
    boff = np.zeros(len(rows) + 1, np.int64)
    boff[1:] = np.cumsum([len(b) for b in rows])
    n = len(rows)
    raw = texts_to_raw([b.decode("utf-8", "replace") for b in rows], np.ones(n, np.uint8),
                       ordinary_scalars(n, 205, now), now)
    u8 = Utf8Text(np.frombuffer(b"".join(rows), np.uint8).copy(), boff)
    return RawBatch(raw.text, raw.offsets, raw.is_retweet, raw.scalars, now, utf8=u8), bad


# --- the decoder's stage window ------------------------------------------------

WINDOW_ROW_UNITS = 64      # 192 B of three-byte text per row of the two window groups
WINDOW_CUT_ROWS = DEC_STAGE // (3 * WINDOW_ROW_UNITS)   # 32 rows fill the window exactly


def _cjk(n, rot=0):
    return "".join(chr(0x4E00 + (7 * (i + rot)) % 0x5000) for i in range(n))


def _emoji(n, rot=0):
    return "".join(chr(0x1F600 + (i + rot) % 80) for i in range(n))


def _mixed_to(nbytes, rot):
    """Text of exactly nbytes UTF-8 bytes: ASCII, two- and three-byte
    characters in turn, topped up with ASCII."""
    out, n, i = [], 0, rot
    while n + 6 <= nbytes:
        out.append("xY"[i % 2] + chr(0x410 + i % 32) + chr(0x4E00 + (11 * i) % 0x5000))
        n += 6
        i += 1
    return "".join(out) + "z" * (nbytes - n)


def window_rows(now=NOW):
    """Rows around the decoder's stage window (kDecStage = 6144 B, starting
    at the first row's offset rounded down to 16).

    Rows 0..63 and 64..127 are two 64-row groups of three-byte text, 64 units
    (192 B) a row.  Group A starts at byte 0, so row 31 ends with s1 - a0 ==
    6144: the window takes rows 0..31 exactly.  Group B starts at a byte
    offset = 1 mod 16 (row 63 is 11 units longer), so row 95 ends with
    s1 - a0 == 6145: the window cuts before it.  (Row ends of pure three-byte
    text differ by multiples of 3, so one window cannot see both values.)
    Then single rows: 2047 / 2048 / 2049 CJK units (6141 / 6144 / 6147 B),
    1535 / 1536 / 1537 emoji (6140 / 6144 / 6148 B), mixed rows with a three-
    and a four-byte sequence on every split of byte 6144 of the row, and a
    row of 8191 bytes that ends in a four-byte sequence.  Returns (raw, meta)
    with ``raw.utf8`` set (Python's encoder) and meta[i] the row's label."""
    texts, meta = [], []
    for r in range(2 * GROUP_ROWS):
        n = WINDOW_ROW_UNITS + (11 if r == GROUP_ROWS - 1 else 0)
        texts.append(_cjk(n, rot=r))
        meta.append("group A" if r < GROUP_ROWS else "group B")
    for n in (DEC_STAGE // 3 - 1, DEC_STAGE // 3, DEC_STAGE // 3 + 1):
        texts.append(_cjk(n, rot=n))
        meta.append(f"cjk {n}")
    for n in (DEC_STAGE // 4 - 1, DEC_STAGE // 4, DEC_STAGE // 4 + 1):
        texts.append(_emoji(n, rot=n))
        meta.append(f"emoji {n}")
    for ch in ("中", "\U00010400"):
        L = len(ch.encode("utf-8"))
        for k in range(1, L):                       # k bytes of the sequence below byte 6144
            texts.append(_mixed_to(DEC_STAGE - k, k) + ch + " " + _mixed_to(40 + k, k))
            meta.append(f"straddle U+{ord(ch):04X} at {DEC_STAGE - k}")
    texts.append(_mixed_to(ROW_WORD_LIMIT - 1 - 4, 5) + chr(EMOJI))
    meta.append("8191 B ending in a four-byte sequence")
    rows = [t.encode("utf-8") for t in texts]
    return _utf8_rows_to_raw(rows, 203, now), meta


# --- every row special ---------------------------------------------------------

def all_special_batch(n=130, now=NOW):
    """n rows that all need the full case mapping: U+0130, U+03A3 in final and
    non-final position, Deseret capitals -- rotating, with lengths 4..40, so
    the decoder's special-row list is full (stats[2] == n, every ballot has
    all its lanes) and the third 64-row group holds two rows."""
    kinds = [
        lambda i: "İstanbul"[:2 + i % 7] + " x" * (i % 9),
        lambda i: "ΟΔΟΣ" + " ab" * (i % 11),                 # final sigma, then a space
        lambda i: "ΣΟΦΙΑ"[:2 + i % 4] + "c" * (i % 13),   # not final
        lambda i: chr(0x10400 + i % 40) + "dЖ" * (1 + i % 8),
        lambda i: "q" * (i % 17) + "ΑΣ",                                # final: ends the row
    ]
    texts = [kinds[i % len(kinds)](i) for i in range(n)]
    return texts_to_raw(texts, np.ones(n, np.uint8), ordinary_scalars(n, 204, now), now)


def special_rows(raw):
    """Indices of the rows the host says need the full case mapping."""
    from twitter_stream_ml_amd.ops._native import host
    h = host()
    return [i for i in range(raw.n) if h.row_needs_special(raw.text[raw.offsets[i]:raw.offsets[i + 1]])]

"""The text-atlas builders (``text_atlas.py``) are where they claim to be.

Runs without a GPU.  ``test_gpu_text_atlas.py`` compares the device with the
host oracle on these batches; here the batches themselves are pinned: every
unit value in every row kind, every probe on every split of every decoder
boundary, the rows around the stage window, the all-special batch -- each
computed from the returned offsets and bytes, not from the builder's plan.
The builder's constants are compared with ``csrc/hip`` itself, the host
tables with Python's ``str.lower``, and both oracles with each other.
"""
import os
import re
import unicodedata

import numpy as np
import pytest

import edge_batches as eb
import text_atlas as ta
from twitter_stream_ml_amd.oracle import featurize_batch, featurize_batch_native
from twitter_stream_ml_amd.ops._native import host
from twitter_stream_ml_amd.records.batch import units_to_str, utf16_units

HIP = os.path.join(os.path.dirname(ta.TABLES_H), "..", "hip")
SAME_UNICODE = unicodedata.unidata_version == ta.tables_unicode_version()
needs_same_unicode = pytest.mark.skipif(
    not SAME_UNICODE, reason=f"Python's Unicode {unicodedata.unidata_version} is not the tables' "
                             f"{ta.tables_unicode_version()}: str.lower is no reference for them")


@pytest.fixture(scope="module")
def atlas():
    return ta.codepoint_atlas()


@pytest.fixture(scope="module")
def sweep():
    return ta.utf8_position_sweep()


@pytest.fixture(scope="module")
def window():
    return ta.window_rows()


def _row(raw, i):
    return raw.text[raw.offsets[i]:raw.offsets[i + 1]]


def _wire_flags(raw):
    h = host()
    out = np.zeros(int(h.wire_bound(raw.total_units, raw.n)), np.uint8)
    woff = np.zeros(raw.n + 1, np.int64)
    flags = np.zeros(raw.n, np.uint8)
    h.wire_pack(raw.text, raw.offsets, raw.is_retweet, out, woff, flags)
    return ["wide" if f & 2 else "cesu" if f & 4 else "narrow" for f in flags]


def _constant(path, name):
    with open(os.path.join(HIP, path), encoding="utf-8") as f:
        return int(re.search(rf"constexpr int {name} = (\d+)", f.read()).group(1))


def test_builder_constants_are_the_kernels():
    """A constant edited here or there shows as a wrong edge, not as a test
    that quietly stopped reaching it."""
    assert ta.STAGE_BYTES == 4 * _constant("text_stage.h", "kStageWords")
    assert ta.LOWER_LDS_BLOCKS == _constant("text_stage.h", "kLowerLdsBlocks")
    assert eb.DEC_STAGE == ta.DEC_STAGE == _constant("featurize.hip", "kDecStage")
    assert ta.KM_CHUNK_DIMS == _constant("kmeans.hip", "kKmChunkDims")
    assert ta.ROW_WORD_LIMIT == 1 << _constant("kernels.h", "kRowLenBits")
    assert ta.WAVE_STEP == 4 * _constant("common.h", "kWave") and ta.GROUP_ROWS == _constant("common.h", "kWave")
    assert ta.KM_STAGE_BYTES == 3 * 4 * _constant("common.h", "kWave")
    with open(os.path.join(HIP, "featurize.hip"), encoding="utf-8") as f:
        src = f.read()
    assert "& ~int64_t(15)" in src and ta.STAGE_ALIGN == 16      # k_cesu_decode: a0 = s0 & ~15
    with open(os.path.join(HIP, "kmeans.hip"), encoding="utf-8") as f:
        assert "ndw <= 3 * kWave" in f.read()
    assert ta.KM_EDGE_DIMS[0] == ta.KM_CHUNK_DIMS and ta.KM_EDGE_DIMS[1] == ta.KM_CHUNK_DIMS + 1
    assert max(ta.KM_BAL_DIMS) <= ta.KM_CHUNK_DIMS < min(ta.KM_EDGE_DIMS[1:])


# --- tables ---------------------------------------------------------------------

def test_parsed_tables_are_the_hosts():
    """text_atlas.lower_tables (the header, parsed) lowers every unit as the
    host library compiled from that header does."""
    h = host()
    page, blocks, supp = ta.lower_tables()
    assert max(page) >= ta.LOWER_LDS_BLOCKS       # some pages map to blocks the kernels keep in global memory
    for u in range(0x10000):
        if u in (0x130, 0x3A3):
            continue
        want = (u + blocks[page[u >> 8]][u & 255]) & 0xFFFF
        got = np.asarray(h.lower_row(np.array([u], np.uint16)))
        assert got.tolist() == [want], hex(u)
    assert len(supp) == 225 or not SAME_UNICODE
    for cp, lo in supp[::7]:
        assert units_to_str(np.asarray(h.lower_row(utf16_units(chr(cp))))) == chr(lo)


@needs_same_unicode
def test_host_tables_equal_python_lower():
    """host().lower_row == str.lower for every BMP scalar, every lone
    surrogate and every code point of planes 1 (0x10000..0x1FFFF)."""
    h = host()
    bad = []
    for cp in range(0x20000):
        s = chr(cp)
        got = units_to_str(np.asarray(h.lower_row(utf16_units(s))))
        if got != s.lower():
            bad.append(hex(cp))
    assert not bad, bad[:20]
    # the four units >= 256 whose lower case is < 256
    assert [ord(chr(c).lower()[0]) for c in (0x178, 0x1E9E, 0x212A, 0x212B)] == [0xFF, 0xDF, 0x6B, 0xE5]


def test_kmeans_widths_see_every_lowering_delta():
    """A unit the device failed to lower differs from the lowered one by a
    delta d of the tables; its bigrams' Java hashes 31 u0 + u1 then move by d
    or 31 d.  No prime width of the GPU test divides either, so such a bigram
    always changes its bucket."""
    deltas = ta.unit_deltas()
    assert len(deltas) > 50 and 32 in deltas and 1 in deltas
    for td in ta.KM_PRIME_DIMS:
        assert all(td % q for q in range(2, int(td ** 0.5) + 1)), td
        hit = [d for d in deltas if d % td == 0 or (31 * d) % td == 0]
        assert not hit, (td, hit)


# --- every code unit --------------------------------------------------------------

def test_every_unit_in_every_kind(atlas):
    raw, meta = atlas
    assert raw.n == len(meta) and raw.is_retweet.all()
    assert ((raw.scalars[0] >= 100) & (raw.scalars[0] <= 1000)).all()
    seen = {}
    for i, (kind, _) in enumerate(meta):
        seen.setdefault(kind, np.zeros(0x10000, bool))[_row(raw, i)] = True
    for kind in ("short", "long", "inter"):
        assert seen[kind].all(), (kind, np.nonzero(~seen[kind])[0][:8])
    for kind in ("latin1", "latin1-long"):
        assert seen[kind][:256].all() and not seen[kind][256:].any()
    # surrogates of the unit rows stay lone (no high directly before a low)
    for i, (kind, _) in enumerate(meta):
        if kind in ("short", "long", "inter"):
            u = _row(raw, i).astype(np.int64)
            hi = (u[:-1] >= 0xD800) & (u[:-1] <= 0xDBFF)
            lo = (u[1:] >= 0xDC00) & (u[1:] <= 0xDFFF)
            assert not (hi & lo).any(), (i, kind)
        if kind == "inter":   # every atlas unit between ASCII neighbours
            u = _row(raw, i)
            assert (u[1::2] < 0x80).all() and u.shape[0] == 2 * ta.INTER_UNITS + len(ta.INTER_TAIL)


def test_atlas_rows_sit_on_both_sides_of_the_stage(atlas):
    raw, meta = atlas
    kinds = np.array([k for k, _ in meta])
    wire = np.array(_wire_flags(raw))
    lens = np.diff(raw.offsets)
    assert set(wire.tolist()) == {"narrow", "cesu", "wide"}
    assert (wire[kinds == "inter"] == "cesu").sum() > 500          # from U+0100 on
    assert {"narrow", "cesu", "wide"} >= set(wire[kinds == "inter"].tolist()) >= {"narrow", "cesu"}
    # wide rows: 128 B (staged) and 1024 B (beyond kStageWords and the k-means stage)
    short_w = 2 * lens[(kinds == "short") & (wire == "wide")]
    long_w = 2 * lens[(kinds == "long") & (wire == "wide")]
    assert short_w.size > 1000 and short_w.max() + 3 <= ta.STAGE_BYTES
    assert long_w.size > 100 and long_w.min() > max(ta.STAGE_BYTES, ta.KM_STAGE_BYTES)
    # narrow rows: 259 B in fast chunks, 781.. B beyond the stage
    assert (wire[(kinds == "latin1") | (kinds == "latin1-long")] == "narrow").all()
    l1 = lens[kinds == "latin1"]
    assert l1.shape[0] == 64 and (l1 == ta.LATIN_UNITS).all() and ta.LATIN_UNITS % 2 == 1
    assert ta.LATIN_UNITS <= eb.LAST_FAST and ta.LATIN_UNITS + 3 <= ta.STAGE_BYTES
    ll = lens[kinds == "latin1-long"]
    assert ll.shape[0] >= 16 and ll.min() >= 700 and ll.min() > max(ta.STAGE_BYTES, ta.KM_STAGE_BYTES)
    # sorted narrow-first by descending length, the 64 rows of 259 units are chunks 1..4 exactly
    narrow_len = lens[wire == "narrow"]
    assert (narrow_len > ta.LATIN_UNITS).sum() % eb.ROWS_PER_CHUNK == 0
    assert (narrow_len == ta.LATIN_UNITS).sum() == 64
    # every byte value in every byte lane of a dword, every start alignment
    at = np.zeros((256, 4), bool)
    for i in np.nonzero(kinds == "latin1")[0]:
        u = _row(raw, i)
        at[u, np.arange(u.shape[0]) % 4] = True
    assert at.all()
    assert set((raw.offsets[:-1][kinds == "latin1"] % 4).tolist()) == {0, 1, 2, 3}


def test_astral_rows(atlas):
    raw, meta = atlas
    _, _, supp = ta.lower_tables()
    seen = set()
    sigma_before = sigma_after = False
    cased = {cp for cp, _ in supp}
    for i, (kind, _) in enumerate(meta):
        if not kind.startswith("astral"):
            continue
        s = units_to_str(_row(raw, i))
        assert len(s) <= 64
        seen |= {ord(c) for c in s}
        for a, b in zip(s, s[1:]):
            sigma_after |= ord(a) in cased and b == "Σ"
            sigma_before |= a == "Σ" and ord(b) in cased
    for cp, lo in supp:
        assert {cp - 1, cp, cp + 1, lo} <= seen, hex(cp)
    assert set(ta.UNCASED_ASTRAL) | {ta.EMOJI} <= seen
    assert all(chr(c).lower() == chr(c) for c in ta.UNCASED_ASTRAL) and sigma_before and sigma_after
    h = host()
    n_special = sum(bool(h.row_needs_special(_row(raw, i))) for i, (k, _) in enumerate(meta) if k.startswith("astral"))
    assert n_special >= 10


# --- UTF-8 positions --------------------------------------------------------------

def test_probe_bytes_are_the_code_points():
    for name, seq, cp in ta.PROBES:
        s = seq.decode("utf-8", "surrogatepass")
        if cp is None:
            assert utf16_units(s).tolist() == [0xD801, 0xDC00] and len(seq) == 6
        else:
            assert s == chr(cp) and f"{cp:04X}" in name, name
    special = {n for n, s, _ in ta.PROBES if host().row_needs_special(utf16_units(s.decode("utf-8", "surrogatepass")))}
    assert special == {"U+0130", "U+03A3", "U+10400", "U+1E900", "U+10400 cesu"}


def test_sweep_covers_every_split(sweep):
    raw, meta = sweep
    u8 = raw.utf8
    data, boff = u8.data, u8.offsets
    assert boff[-1] == data.shape[0] and raw.n == len(meta) and raw.is_retweet.all()
    seqs = {n: s for n, s, _ in ta.PROBES}
    cover = {n: {"rel256": set(), "rel4": set(), "p0": False, "last": False, "bounds": set()} for n in seqs}
    starts = set()
    for i, m in enumerate(meta):
        o, e = int(boff[i]), int(boff[i + 1])
        row = bytes(data[o:e])
        starts.add(o % ta.STAGE_ALIGN)
        if m is None:
            assert len(row) < ta.STAGE_ALIGN and all(b < 0x80 for b in row)
            continue
        seq = seqs[m["probe"]]
        p = row.index(seq)                       # from the bytes, not the plan
        assert (m["o"], m["p"], m["nbytes"], m["L"]) == (o, p, e - o, len(seq)), (i, m)
        rest = row[:p] + row[p + len(seq):]
        c2 = m["probe"].endswith("+c2")
        assert all(b < 0x80 for b in rest.replace(ta.CLASS2, b"")) and (ta.CLASS2 in rest) == c2
        if m["probe"] in ("U+0080", "U+00FF"):
            assert max(row) < 0xC4               # class 1: Latin-1
        else:
            assert max(row) >= 0xC4              # class 2
        rel = o % 4 + p
        assert rel == m["rel"]
        c = cover[m["probe"]]
        c["rel4"].add(rel % 4)
        for B in ta.STEP_BOUNDARIES:
            if B - len(seq) < rel <= B:
                c["rel256"].add((B, rel % ta.WAVE_STEP))
        c["p0"] |= p == 0
        c["last"] |= p + len(seq) == e - o
        if m["last"]:
            assert p + len(seq) == e - o
    assert starts == set(range(ta.STAGE_ALIGN))
    for name, seq in seqs.items():
        L, c = len(seq), cover[name]
        want = {(B, r % ta.WAVE_STEP) for B in ta.STEP_BOUNDARIES for r in range(B - L + 1, B + 1)}
        assert c["rel256"] == want, (name, sorted(want - c["rel256"]))
        assert c["rel4"] == {0, 1, 2, 3} and c["p0"] and c["last"], (name, c)
    # U+03A3 after a cased letter and before a space: Final_Sigma applies
    h = host()
    finals = sum(0x3C2 in np.asarray(h.lower_row(_row(raw, i))).tolist()
                 for i, m in enumerate(meta) if m and m["probe"] == "U+03A3")
    assert finals >= 10


def test_sweep_groups_and_the_host_encoder(sweep):
    raw, meta = sweep
    boff = raw.utf8.offsets
    nb = np.diff(boff)
    odd = big_step = False
    for g in range(0, raw.n, ta.GROUP_ROWS):
        rows = [i for i in range(g, min(g + ta.GROUP_ROWS, raw.n)) if meta[i] is not None]
        odd |= len(rows) % 2 == 1
        big_step |= any(abs(int(nb[a]) - int(nb[b])) > ta.WAVE_STEP for a, b in zip(rows, rows[1:]))
    assert odd, "no 64-row group with an odd number of non-ASCII rows"
    assert big_step, "no neighbouring non-ASCII rows whose lengths differ by more than a wave step"
    assert nb.max() < ta.ROW_WORD_LIMIT and boff[-1] < 2 << 20
    # the hand-written bytes are what the host encoder writes, except the CESU-8 rows
    data, off = host().utf8_encode(raw.text, raw.offsets, 0)
    data, off = np.asarray(data), np.asarray(off)
    n_cesu = 0
    for i, m in enumerate(meta):
        mine = bytes(raw.utf8.data[boff[i]:boff[i + 1]])
        theirs = bytes(data[off[i]:off[i + 1]])
        if m and m["probe"] == "U+10400 cesu":
            n_cesu += 1
            assert theirs == mine.replace(b"\xed\xa0\x81\xed\xb0\x80", b"\xf0\x90\x90\x80") != mine
        else:
            assert theirs == mine, i
    assert n_cesu > 10


def test_truncated_tail_batch():
    a, bad = ta.truncated_tail_batch(ord("a"))
    b, _ = ta.truncated_tail_batch(ord("b"))
    lanes = set()
    for i in range(a.n):
        ra = bytes(a.utf8.data[a.utf8.offsets[i]:a.utf8.offsets[i + 1]])
        rb = bytes(b.utf8.data[b.utf8.offsets[i]:b.utf8.offsets[i + 1]])
        if i in bad:
            assert ra == rb and ra.endswith(ta.TRUNCATED) and all(c < 0x80 for c in ra[:-3])
            lanes.add((int(a.utf8.offsets[i + 1]) - 3) % 4)      # the lead's byte lane
        else:
            assert ra[1:] == rb[1:] and ra[0] == ord("a") and rb[0] == ord("b") and all(c < 0x80 for c in ra)
            assert i - 1 in bad
    assert lanes == {0, 1, 2, 3} and (ord("a") ^ ord("b")) & 0x3F
    np.testing.assert_array_equal(a.utf8.offsets, b.utf8.offsets)


# --- the decoder's stage window -------------------------------------------------------

def test_window_rows_sit_on_the_window(window):
    raw, meta = window
    boff, data = raw.utf8.offsets, raw.utf8.data
    nb = np.diff(boff)
    henc, hoff = host().utf8_encode(raw.text, raw.offsets, 0)
    np.testing.assert_array_equal(np.asarray(hoff), boff)
    np.testing.assert_array_equal(np.asarray(henc), data)
    # group A: row 31 ends at s1 - a0 == kDecStage exactly; group B: row 95 at kDecStage + 1
    assert meta[:128] == ["group A"] * 64 + ["group B"] * 64
    for g, edge_row, want in ((0, 31, ta.DEC_STAGE), (64, 95, ta.DEC_STAGE + 1)):
        a0 = int(boff[g]) & ~(ta.STAGE_ALIGN - 1)
        ends = boff[g + 1:g + 65] - a0
        assert int(ends[edge_row - g]) == want, (g, ends[edge_row - g])
        assert int(ends[edge_row - g - 1]) < ta.DEC_STAGE < int(ends[edge_row - g + 1])
        assert all(b >= 0xE0 or 0x80 <= b < 0xC0 for b in data[boff[g]:boff[g + 64]][::97])   # three-byte text
    assert int(boff[0]) == 0 and int(boff[64]) % ta.STAGE_ALIGN == 1
    by = {m: i for i, m in enumerate(meta)}
    assert [int(nb[by[f"cjk {n}"]]) for n in (2047, 2048, 2049)] == [6141, 6144, 6147]
    assert [int(nb[by[f"emoji {n}"]]) for n in (1535, 1536, 1537)] == [6140, 6144, 6148]
    splits = set()
    for m, i in by.items():
        if m.startswith("straddle"):
            row = bytes(data[boff[i]:boff[i + 1]])
            lead = max(j for j in range(ta.DEC_STAGE) if row[j] & 0xC0 != 0x80)   # the sequence holding byte 6143
            L = 4 if row[lead] >= 0xF0 else 3 if row[lead] >= 0xE0 else 2 if row[lead] >= 0xC0 else 1
            assert lead < ta.DEC_STAGE < lead + L and len(row) > ta.DEC_STAGE
            splits.add((L, ta.DEC_STAGE - lead))
    assert splits == {(3, 1), (3, 2), (4, 1), (4, 2), (4, 3)}
    i = by["8191 B ending in a four-byte sequence"]
    assert int(nb[i]) == ta.ROW_WORD_LIMIT - 1 and bytes(data[boff[i + 1] - 4:boff[i + 1]]) == b"\xf0\x9f\x98\x80"


# --- every row special --------------------------------------------------------------

def test_all_special_batch_is_all_special():
    raw = ta.all_special_batch()
    assert raw.n == 130 and raw.n % ta.GROUP_ROWS == 2
    assert ta.special_rows(raw) == list(range(raw.n))
    assert host().count_special_rows(raw.text, raw.offsets) == raw.n
    h = host()
    low = [np.asarray(h.lower_row(_row(raw, i))).tolist() for i in range(raw.n)]
    assert sum(0x3C2 in r for r in low) >= 20 and sum(0x3C3 in r for r in low) >= 20      # final and not
    assert sum(0x307 in r for r in low) >= 20 and sum(0xD801 in r for r in low) >= 20     # U+0130, Deseret
    assert len(set(np.diff(raw.offsets).tolist())) > 10
    assert set(_wire_flags(raw)) >= {"cesu", "wide"}


# --- the two oracles agree ------------------------------------------------------------

@needs_same_unicode
@pytest.mark.parametrize("name", ["atlas", "sweep", "window", "special"])
def test_oracles_agree(name, atlas, sweep, window):
    """featurize_batch (Python's str.lower) == featurize_batch_native (the
    host tables) on every atlas batch; murmur3, hashed term by term in Python,
    on every eleventh row and every astral row."""
    raw = {"atlas": atlas[0], "sweep": sweep[0], "window": window[0], "special": ta.all_special_batch()}[name]
    F = 1 << 20
    a = featurize_batch(raw, F, 100, 1000, now_ms=eb.NOW)
    b = featurize_batch_native(raw, F, 100, 1000, now_ms=eb.NOW)
    assert a.n == b.n == raw.n
    assert (a.X != b.X).nnz == 0
    rows = [i for i in range(raw.n) if i % 11 == 0 and raw.offsets[i + 1] - raw.offsets[i] < 600]
    if name == "atlas":
        rows = sorted(set(rows) | {i for i, (k, _) in enumerate(atlas[1]) if k.startswith("astral")})
    sub = raw.take(rows)
    a = featurize_batch(sub, 1000, 100, 1000, now_ms=eb.NOW, hash="murmur3")
    b = featurize_batch_native(sub, 1000, 100, 1000, now_ms=eb.NOW, hash="murmur3")
    assert a.n == b.n == sub.n and (a.X != b.X).nnz == 0

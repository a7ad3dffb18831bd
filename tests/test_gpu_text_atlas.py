"""The device text path on the text atlas (``text_atlas.py``): UTF-8 decode
(``k_cesu_decode``), special-row detection and lower-casing (``rows.hip``),
per-unit lower-casing (``text_stage.h``, ``narrow_text.h``, ``km_lower``) and
the bigram hash, through every consumer -- the LR featurizers and the lazy
remap, the scorers, the k-means featurizers, and the normaliser's A/B
variants.

The oracle everywhere is the host featurizer (``featurize_batch_native``,
``kmeans_features``): host code on the tables of ``unicode_tables.h``,
independent of the Python build's Unicode version.  Ids are integers and the
scoring weights exactly summable, so every comparison is for equality.
``test_text_atlas_cpu.py`` proves that the batches reach the edges they are
built for.  A failure names the row, its kind and the probe with
``(o mod 16, rel mod 256)`` or the first bigram the device lost.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_batches as eb
import text_atlas as ta
from layout_decode import hybrid_row_counts, oracle_row_counts, oracle_row_ids, rows_from_debug
from test_gpu_score import _w_exact
from twitter_stream_ml_amd.models.kmeans import kmeans_features
from twitter_stream_ml_amd.ops._native import host
from twitter_stream_ml_amd.oracle import featurize_batch_native

pytestmark = pytest.mark.gpu

NOW = eb.NOW
NNZ_WIDE = 1 << 30   # featurize.hip kNnzWide
F_BIG = 1 << 20      # (31 u0 + u1) mod 2^20 changes with any single wrong unit (u < 2^16, 31 u < 2^21)


def _engine(F, hash="java", **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    kw = {"max_rows": 8192, "max_units": 8192 * 300, **kw}
    return DeviceLinearRegression(LRDeviceConfig(num_text_features=F, hash=hash, **kw), device=0)


def _feed(eng, raw):
    hb = eng.staging(0).load(raw, eng.cfg.ingest)
    eng.submit(hb, 0)
    return eng.process(0, raw.batch_time_ms, True)


@pytest.fixture(scope="module")
def batches():
    """name -> (raw, meta); built once, never modified."""
    atlas, ameta = ta.codepoint_atlas()
    latin = [i for i, (k, _) in enumerate(ameta) if k.startswith("latin1")]
    astral = [i for i, (k, _) in enumerate(ameta) if k.startswith("astral")]
    sweep, smeta = ta.utf8_position_sweep()
    window, wmeta = ta.window_rows()
    special = ta.all_special_batch()
    return {"atlas": (atlas, ameta), "sweep": (sweep, smeta), "window": (window, wmeta),
            "special": (special, ["special"] * special.n),
            "latin1": (atlas.take(latin), [ameta[i] for i in latin]),
            "astral": (atlas.take(astral), [ameta[i] for i in astral])}


_ORACLE = {}


def _oracle(name, raw, F, hash="java"):
    key = (name, F, hash)
    if key not in _ORACLE:
        _ORACLE[key] = featurize_batch_native(raw, F, 100, 1000, now_ms=NOW, hash=hash)
    return _ORACLE[key]


def _units(raw, i):
    return raw.text[raw.offsets[i]:raw.offsets[i + 1]]


def _where(name, raw, meta, i):
    """The row, its kind, and for a probe row where the probe sits."""
    m = meta[i]
    if isinstance(m, dict):
        return (f"{name} row {i}: probe {m['probe']} at p = {m['p']} of {m['nbytes']} B, "
                f"(o mod 16, rel mod 256) = ({m['o'] % 16}, {m['rel'] % 256})")
    if m is None:
        return f"{name} row {i}: ASCII pad row of {raw.offsets[i + 1] - raw.offsets[i]} B"
    if isinstance(m, tuple):
        return f"{name} row {i}: {m[0]} from U+{m[1]:04X}, {raw.offsets[i + 1] - raw.offsets[i]} units"
    return f"{name} row {i}: {m}, {raw.offsets[i + 1] - raw.offsets[i]} units"


def _lost_bigram(raw, i, mod, missing):
    """The first bigram of row i (lower-cased by the host, Java hash mod
    ``mod``) whose id is in ``missing``: which unit the device got wrong."""
    low = np.asarray(host().lower_row(_units(raw, i))).astype(np.int64)
    ids = (31 * low[:-1] + low[1:]) % mod if low.shape[0] >= 2 else low % mod
    for j, fid in enumerate(ids.tolist()):
        if fid in missing:
            pair = low[j:j + 2].tolist()
            return f"first lost bigram {j}: lowered units {[hex(u) for u in pair]} -> id {fid}"
    return "no bigram lost (the device has extra ids)"


def _check_ids(name, raw, meta, dbg, fb, F, hash):
    """Per-row id multisets, active set, unit counts and the wide bit."""
    assert int(dbg["counters"][0]) == fb.n == raw.n
    rows = rows_from_debug(dbg)
    Xt = fb.X[:, :F].tocsr()
    nnz = dbg["nnz"]
    for k in range(fb.n):
        want = oracle_row_ids(Xt, k)
        if rows[k].shape != want.shape or (rows[k] != want).any():
            missing = set(want.tolist()) - set(rows[k].tolist())
            extra = sorted(set(rows[k].tolist()) - set(want.tolist()))[:6]
            lost = _lost_bigram(raw, k, F, missing) if hash == "java" else f"missing ids {sorted(missing)[:6]}"
            pytest.fail(f"{_where(name, raw, meta, k)}: {rows[k].shape[0]} ids, oracle {want.shape[0]}; {lost}; "
                        f"extra ids {extra}")
        assert int(nnz[k]) & (NNZ_WIDE - 1) == want.shape[0], _where(name, raw, meta, k)
        u = _units(raw, k)
        if u.shape[0]:
            assert bool(int(nnz[k]) & NNZ_WIDE) == bool(u.max() >= 256), _where(name, raw, meta, k)
    np.testing.assert_array_equal(np.sort(dbg["uniq"]), np.unique(Xt.indices))


FEATURIZE_CASES = ([(b, i) for b in ("atlas", "special") for i in ("wire", "utf16", "utf8")]
                   + [("sweep", "utf8"), ("window", "utf8")])


@pytest.mark.parametrize("name,ingest", FEATURIZE_CASES)
def test_featurize_matches_the_host(hip_module, batches, name, ingest):
    """Every atlas batch through every ingest mode it exists in (the sweep
    and the window rows are UTF-8 bytes: ``load_utf8``), every hashed id kept
    (lazy_idx=False), F = 2^20 with the Java hash: per-row id multisets, the
    active set, unit counts and the wide bit equal the host's, and the device
    lower-cased exactly the rows the host calls special."""
    raw, meta = batches[name]
    eng = _engine(F_BIG, lazy_idx=False, ingest=ingest, num_iterations=1, step_size=1e-6)
    res = _feed(eng, raw)
    assert res["n_kept"] == raw.n
    _check_ids(name, raw, meta, eng._eng.debug_prepared(), _oracle(name, raw, F_BIG), F_BIG, "java")
    n_special = len(ta.special_rows(raw))
    assert res["rows_lowered"] == n_special, (name, ingest, res["rows_lowered"], n_special)
    if name == "special":
        assert res["rows_lowered"] == raw.n == 130


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
def test_featurize_murmur3_small_table(hip_module, batches, ingest):
    """The code-point atlas with murmur3 and F = 1000: the hash of the UTF-8
    bytes of every unit pair (lone surrogates as '?'), reduced by term_mod."""
    raw, meta = batches["atlas"]
    eng = _engine(1000, "murmur3", lazy_idx=False, ingest=ingest, num_iterations=1, step_size=1e-6)
    res = _feed(eng, raw)
    assert res["n_kept"] == raw.n
    _check_ids("atlas", raw, meta, eng._eng.debug_prepared(), _oracle("atlas", raw, 1000, "murmur3"), 1000,
               "murmur3")


@pytest.mark.parametrize("ingest", ["wire", "utf16", "utf8"])
@pytest.mark.parametrize("F", [1000, F_BIG])
def test_lazy_remap_of_the_latin1_rows(hip_module, batches, ingest, F):
    """The narrow rows with lazy ids: the hybrid remap re-derives the ids of
    the four fast chunks from the text (narrow_text.h: alignbyte windows,
    lower4_latin1 per byte lane); hot counts + cold entries == oracle counts.
    F = 1000 reduces the hash, 2^20 takes it directly."""
    raw, meta = batches["latin1"]
    eng = _engine(F, lazy_idx=True, hybrid=True, ingest=ingest, num_iterations=1, step_size=1e-6)
    res = _feed(eng, raw)
    assert res["n_kept"] == raw.n
    dbg, hy = eng._eng.debug_prepared(), eng._eng.debug_hybrid()
    clen8c, perm, cfast = hy["clen8c"], dbg["perm"], dbg["cfast"]
    assert int(np.count_nonzero(cfast)) == ta.LATIN_ROWS // eb.ROWS_PER_CHUNK == 4, cfast
    assert int(np.count_nonzero(clen8c >= 0)) >= 4
    uniq = np.sort(dbg["uniq"])
    Xt = _oracle("latin1", raw, F).X[:, :F].tocsr()
    np.testing.assert_array_equal(uniq, np.unique(Xt.indices))
    checked = 0
    for c in np.nonzero(clen8c >= 0)[0]:
        for r in range(16):
            k = int(perm[c * 16 + r])
            if k < 0:
                continue
            got, want = hybrid_row_counts(hy, uniq, dbg["cbase"], c, r), oracle_row_counts(Xt, k)
            if got != want:
                missing = {f for f, n in want.items() if got.get(f, 0) < n}
                pytest.fail(f"{_where('latin1', raw, meta, k)} (chunk {c}, fast {int(cfast[c])}): "
                            f"{_lost_bigram(raw, k, F, missing)}")
            checked += 1
    assert checked >= ta.LATIN_ROWS


def test_truncated_sequence_does_not_read_the_next_row(hip_module):
    """The decoder's ``rng3`` mask keeps a four-byte lead from taking
    continuation bytes beyond the row end.  Well-formed UTF-8 never puts a
    four-byte lead among a row's last three bytes, so only a truncated row
    can show it: a row that ends in F0 9F 98 must decode to the same ids
    whatever byte the next row starts with, on every byte lane of the lead;
    the well-formed rows after it equal the oracle."""
    eng = _engine(F_BIG, lazy_idx=False, ingest="utf8", num_iterations=1, step_size=1e-6)
    got = {}
    for first in (ord("a"), ord("b")):
        raw, bad = ta.truncated_tail_batch(first)
        res = _feed(eng, raw)
        assert res["n_kept"] == raw.n
        dbg = eng._eng.debug_prepared()
        rows = rows_from_debug(dbg)
        Xt = featurize_batch_native(raw, F_BIG, 100, 1000, now_ms=NOW).X[:, :F_BIG].tocsr()
        for k in range(raw.n):
            if k not in bad:
                np.testing.assert_array_equal(rows[k], oracle_row_ids(Xt, k),
                                              err_msg=f"row {k} (after a truncated row)")
        got[first] = [rows[k] for k in bad]
    for j, (x, y) in enumerate(zip(got[ord("a")], got[ord("b")])):
        assert x.shape == y.shape and (x == y).all(), \
            f"truncated row {j} (lead on byte lane rel mod 4 = {j}) decodes with the next row's first byte"


# --- scoring ----------------------------------------------------------------------

@pytest.mark.parametrize("name,ingest", [("atlas", "wire"), ("atlas", "utf16"), ("atlas", "utf8"),
                                         ("sweep", "utf8")])
def test_scoring_is_bit_exact(hip_module, batches, name, ingest):
    """``predict_batch`` with exactly summable weights (multiples of 2^-8,
    numeric weights zero): k_score_narrow on the fast chunks, k_score on the
    staged and the unstaged rows; any wrong, lost or doubled id shows."""
    raw, meta = batches[name]
    eng = _engine(F_BIG, ingest=ingest)
    fb = _oracle(name, raw, F_BIG)
    w = _w_exact(F_BIG, 31)
    eng.set_weights(w)
    res = eng.predict_batch(raw, apply_filter=False)
    assert res["n_scored"] == fb.n == raw.n
    np.testing.assert_array_equal(res["rows"], fb.rows)
    ref = np.asarray(fb.X @ w, np.float64).reshape(-1)
    got = np.ascontiguousarray(res["pred"])
    bad = np.nonzero(got.view(np.int64) != ref.view(np.int64))[0]
    assert bad.size == 0, (f"{bad.size} rows differ; first: {_where(name, raw, meta, int(bad[0]))}: "
                           f"{got[bad[0]]!r} != {ref[bad[0]]!r}")


# --- k-means features ---------------------------------------------------------------

@pytest.mark.parametrize("ingest", ["utf8", "wire"])
@pytest.mark.parametrize("text_dims", list(ta.KM_BAL_DIMS) + list(ta.KM_EDGE_DIMS))
def test_kmeans_features_match_the_host(hip_module, batches, text_dims, ingest):
    """``debug_features`` on the code-point atlas: 61 and 113 dims take
    k_km_features_bal (staged 128-B rows, unstaged 1024-B rows, lower_any
    through the LDS and the global blocks), 256 its last width, 257 and 300
    the generic k_km_features (km_lower).  The prime widths separate a
    lowered unit from an unlowered one in every case (CPU suite)."""
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans, KMDeviceConfig
    raw, meta = batches["atlas"]
    dev = DeviceKMeans(KMDeviceConfig(k=8, text_dims=text_dims, max_rows=8192, max_units=8192 * 300, seed=3,
                                      ingest=ingest), device=0)
    dev.update_raw(raw, want_pred=False)
    got = np.asarray(dev._eng.debug_features())
    key = ("km", text_dims)
    if key not in _ORACLE:
        _ORACLE[key] = kmeans_features(raw, text_dims)[0].astype(np.float32)
    want = _ORACLE[key]
    assert got.shape[0] == want.shape[0] == raw.n and got.shape[1] >= 2 + text_dims
    diff = np.nonzero((got[:, :2 + text_dims] != want).any(axis=1))[0]
    if diff.size:
        i = int(diff[0])
        short = set((np.nonzero(got[i, 2:2 + text_dims] < want[i, 2:])[0]).tolist())
        pytest.fail(f"{diff.size} rows differ; first: {_where('atlas', raw, meta, i)}: "
                    f"{_lost_bigram(raw, i, text_dims, short)}")
    assert not got[:, 2 + text_dims:].any()       # padding columns


# --- the normaliser's A/B variants ------------------------------------------------------

_VARIANT_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import text_atlas as ta
from layout_decode import rows_from_debug
from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
atlas, meta = ta.codepoint_atlas()
astral = atlas.take([i for i, (k, _) in enumerate(meta) if k.startswith("astral")])
eng = DeviceLinearRegression(LRDeviceConfig(num_text_features=1 << 20, lazy_idx=False, ingest="utf8",
                                            num_iterations=1, step_size=1e-6, max_rows=8192,
                                            max_units=8192 * 300), device=0)
h = hashlib.sha256()
for raw in (ta.utf8_position_sweep()[0], ta.all_special_batch(), astral):
    hb = eng.staging(0).load(raw, "utf8")
    eng.submit(hb, 0)
    res = eng.process(0, raw.batch_time_ms, True)
    assert res["n_kept"] == raw.n
    for ids in rows_from_debug(eng._eng.debug_prepared()):
        h.update(np.int64(ids.shape[0]).tobytes()); h.update(np.ascontiguousarray(ids, np.int64).tobytes())
    h.update(np.int64(res["rows_lowered"]).tobytes())
print("DIGEST", h.hexdigest())
"""

_DIGESTS = {}


def _variant_digest(tmp_path, env_add):
    key = tuple(sorted(env_add.items()))
    if key not in _DIGESTS:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        script = tmp_path / "normalize_variant.py"
        script.write_text(_VARIANT_SCRIPT)
        env = {k: v for k, v in os.environ.items() if k not in ("TWTML_NORMALIZE_ALL", "TWTML_NORMALIZE_LIST")}
        env.update(env_add)
        out = subprocess.run([sys.executable, str(script), repo], env=env, capture_output=True, text=True,
                             timeout=180)
        assert out.returncode == 0, out.stderr[-2000:]
        _DIGESTS[key] = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST")][-1].split()[1]
    return _DIGESTS[key]


@pytest.mark.parametrize("knob,value", [("TWTML_NORMALIZE_ALL", "1"), ("TWTML_NORMALIZE_LIST", "0")])
def test_normaliser_variants(hip_module, batches, tmp_path, knob, value):
    """``TWTML_NORMALIZE_ALL=1`` (k_row_normalize over every wide row) and
    ``TWTML_NORMALIZE_LIST=0`` (k_row_normalize over the flagged rows, by
    64-row group) in a fresh process each: the sorted ids of every row of the
    sweep, the all-special batch and the astral rows (UTF-8 ingest) and
    ``rows_lowered`` digest to what the default path (k_row_special over the
    decoder's list) gives -- and to the host oracle's digest."""
    h = hashlib.sha256()
    for name in ("sweep", "special", "astral"):
        raw, _ = batches[name]
        Xt = _oracle(name, raw, F_BIG).X[:, :F_BIG].tocsr()
        for k in range(raw.n):
            ids = oracle_row_ids(Xt, k)
            h.update(np.int64(ids.shape[0]).tobytes())
            h.update(np.ascontiguousarray(ids, np.int64).tobytes())
        h.update(np.int64(len(ta.special_rows(raw))).tobytes())
    default = _variant_digest(tmp_path, {})
    assert default == h.hexdigest(), "the default path differs from the host oracle"
    assert _variant_digest(tmp_path, {knob: value}) == default, (knob, value)

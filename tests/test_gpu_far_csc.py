"""Far CSC of the tiered layout, built from the remap's count atomics.

``k_remap_hybrid<true, ..>`` (``csrc/hip/hot_split.hip``) lists every far
entry of a chunk (``fslot``) and counts it per slot; the value the count
atomic returns is the entry's rank inside its slot (``frank``).  ``k_far_csc``
then stores the entry at ``offset[slot] + rank`` without a second atomic.  A
wrong rank or offset would be an entry in another slot's segment (or outside
the CSC), so every case below reads the whole far tier back with
``debug_far_layout()`` and recomputes it in numpy:

* per-slot counts of the listed entries, whose exclusive scan must be the CSC
  offsets, and whose sum must be the far total and the sum of ``fcount``;
* the ranks of every slot's entries are a permutation of ``0 .. count - 1``;
* the CSC range ``[off[s], off[s + 1])`` holds exactly slot s's
  ``(16 c + row, slot)`` pairs (as a multiset), each at its offset + rank.

Then the trained batch is compared with the fp64 oracle within the bounds of
``tests/test_gpu_tiered.py``.  The batches are generated from fixed seeds; the
shapes are the smallest that reach each path of the scheme (see the cases).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_batches as eb
from test_gpu_tiered import _check
from twitter_stream_ml_amd.oracle import (featurize_batch_native, round_half_up_array,
                                          run_minibatch_sgd_active)
from twitter_stream_ml_amd.sources.synthetic import SynthConfig, generate_batch

pytestmark = pytest.mark.gpu

NOW = eb.NOW
F = 1 << 20
ROWS = eb.ROWS_PER_CHUNK
ALPHA = np.array(list("abcdefghijklmnopqrstuvwxyz0123456789"))
# the reference's step (0.005, 50 iterations) diverges on rows that share
# hundreds of bigrams or hold hundreds of them (edge_batches.LENGTH_CLASS_STEP)
GENTLE = dict(step_size=eb.LENGTH_CLASS_STEP, num_iterations=eb.LENGTH_CLASS_ITERS)


def _rand_text(rng, n):
    return "".join(ALPHA[rng.integers(0, len(ALPHA), n)])


def _keep_all(raw):
    """Every row through the default filter (a retweet with rc in [100, 1000])."""
    raw.is_retweet[:] = 1
    raw.scalars[0] = 100 + (np.arange(raw.n) * 37) % 901
    return raw


def short_rows_batch(n, seed):
    """n ordinary short tweets of the synthetic source, all kept."""
    return _keep_all(generate_batch(SynthConfig.profile("twitter", seed=seed), 0, n, batch_time_ms=NOW))


def random_rows_batch(n, seed):
    """n rows of 20..140 random units over 36 characters: 1,296 bigrams, all
    about equally frequent, so a 64-slot near tier takes few of the entries."""
    rng = np.random.default_rng(seed)
    texts = [_rand_text(rng, int(k)) for k in rng.integers(20, 141, n)]
    return eb.texts_to_raw(texts, np.ones(n, np.uint8), eb.ordinary_scalars(n, seed, NOW), NOW)


def long_rows_batch(seed=23):
    """Rows on the three remap paths: 40 rows of 330..600 units (more than 320
    bigrams: the plain layout), 40 of 290..320 units (register groups, ids
    from idx) and 120 short ones (ids from the text), random over 36
    characters so that nearly every bigram is beyond a 64-slot near tier."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(330, 601, 40), rng.integers(290, 321, 40), rng.integers(5, 120, 120)])
    texts = [_rand_text(rng, int(n)) for n in lens]
    return eb.texts_to_raw(texts, np.ones(len(texts), np.uint8), eb.ordinary_scalars(len(texts), seed, NOW), NOW)


def heavy_slots_batch(n=2000, seed=29):
    """One 230-unit string (about 200 distinct bigrams, some of them more than
    once) at the start of every row, then a few units of the row's own."""
    rng = np.random.default_rng(seed)
    common = _rand_text(rng, 230)
    texts = [common + " " + _rand_text(rng, int(k)) for k in rng.integers(4, 16, n)]
    return eb.texts_to_raw(texts, np.ones(n, np.uint8), eb.ordinary_scalars(n, seed, NOW), NOW)


def near_only_batch(n=50):
    """A few dozen distinct bigrams in all: the active set fits the near tier."""
    texts = [eb.make_text("ascii", 20 + i % 10, rot=i) for i in range(n)]
    return eb.texts_to_raw(texts, np.ones(n, np.uint8), eb.ordinary_scalars(n, 31, NOW), NOW)


def _engine(raw, **kw):
    from twitter_stream_ml_amd.ops.lr_engine import DeviceLinearRegression, LRDeviceConfig
    rows = (raw.n + ROWS - 1) // ROWS * ROWS
    units = max(rows * 300, int(raw.total_units) + rows)
    return DeviceLinearRegression(LRDeviceConfig(num_text_features=F, max_rows=rows, max_units=units, **kw), device=0)


def check_far_layout(d):
    """The far tier of ``debug_far_layout()``, recomputed from its chunk lists.
    Returns (far total, per-slot counts, fcount)."""
    assert d["tiered"]
    near_end, total = int(d["near_end"]), int(d["far_total"])
    off = d["offsets"].astype(np.int64)
    n_far = off.shape[0] - 1
    fcount = d["fcount"].astype(np.int64)
    flist, frank = d["flist"].astype(np.int64), d["frank"].astype(np.int64)
    assert (fcount >= 0).all()
    assert total == int(fcount.sum()) == flist.shape[0] == frank.shape[0]
    assert d["csc_pos"].shape[0] == d["csc_slot"].shape[0] == total
    slot = flist & 0x0FFFFFFF
    pos = ROWS * np.repeat(np.arange(fcount.shape[0], dtype=np.int64), fcount) + (flist >> 28)
    if total:
        assert slot.min() >= near_end and slot.max() < near_end + n_far
    # per-slot counts -> exclusive scan = the CSC offsets
    counts = np.bincount(slot - near_end, minlength=n_far).astype(np.int64)
    want = np.zeros(n_far + 1, np.int64)
    want[1:] = np.cumsum(counts)
    np.testing.assert_array_equal(off, want)
    assert off[-1] == total
    # the ranks of a slot's entries: a permutation of 0 .. count - 1
    order = np.lexsort((frank, slot))
    np.testing.assert_array_equal(frank[order], np.arange(total) - off[slot[order] - near_end])
    # segment s of the CSC holds slot s only, and exactly its listed pairs
    cs, cp = d["csc_slot"].astype(np.int64), d["csc_pos"].astype(np.int64)
    np.testing.assert_array_equal(cs, near_end + np.repeat(np.arange(n_far, dtype=np.int64), counts))
    np.testing.assert_array_equal(np.sort((cs << 32) | cp), np.sort((slot << 32) | pos))
    # each entry at its slot's offset + its rank
    at = off[slot - near_end] + frank
    np.testing.assert_array_equal(cs[at], slot)
    np.testing.assert_array_equal(cp[at], pos)
    return total, counts, fcount


def train_and_check(raw, step=0.005, iters=50, **kw):
    """One batch from zero weights: the far layout, then oracle parity
    (the quantities and bounds of test_gpu_tiered._parity / _check)."""
    eng = _engine(raw, **kw)
    res = eng.train_batch(raw, want_pred=True)
    assert res["tiered"] and not res["diverged"]
    d = eng._eng.debug_far_layout()
    hy = eng._eng.debug_hybrid()
    total, counts, fcount = check_far_layout(d)
    fb = featurize_batch_native(raw, F, 100, 1000, now_ms=raw.batch_time_ms)
    assert res["n_kept"] == fb.n == raw.n
    w0 = np.zeros(F + 4)
    pred_o = round_half_up_array(fb.X @ w0)
    r = run_minibatch_sgd_active(fb.X, fb.y, w0, step, iters)
    w, wg = r.weights, eng.get_weights()
    pred_g = np.asarray(res["pred"], np.float64)
    n_, sy, sy2, sp_, sp2, se2 = res["stats"]
    mse_o = float(np.mean((fb.y - pred_o) ** 2))
    o = dict(it_gpu=res["iterations"], it_orc=r.iterations,
             werr=float(np.linalg.norm(wg - w) / max(np.linalg.norm(w), 1e-30)),
             wmax=float(np.abs(wg - w).max() / max(np.abs(w).max(), 1e-30)),
             pred_mis=float(np.mean(pred_g != pred_o)),
             pred_maxdiff=float(np.abs(pred_g - pred_o).max()),
             mse_rel=abs(se2 / n_ - mse_o) / mse_o,
             n_unique=res["n_unique"], n_near=res["n_near"], kept=fb.n, far_total=total,
             max_fcount=int(fcount.max()), max_slot_count=int(counts.max()) if counts.size else 0)
    print(o)
    _check([o])
    return dict(o, res=res, layout=d, counts=counts, fcount=fcount, clen8c=hy["clen8c"],
                entries=int(fb.X[:, :F].sum()))


def run_slices_case():
    """In a process with TWTML_PREP_SLICES=3 (read once per process): 2,000
    short rows in 125 chunks, a 64-slot near tier.  Common bigrams have
    entries in most chunks, so their ranks continue across the three remap
    launches and their segments are filled by the three k_far_csc launches."""
    out = train_and_check(short_rows_batch(2000, seed=11))
    fcount = out["fcount"]
    C = fcount.shape[0]
    assert out["n_near"] == 64 and C == 125
    # the launches' chunk ranges (launch_remap_slices: C k / 3 .. C (k + 1) / 3)
    launch = np.searchsorted([C * k // 3 for k in (1, 2)], np.repeat(np.arange(C), fcount), side="right")
    slot = out["layout"]["flist"].astype(np.int64) & 0x0FFFFFFF
    in_all = set(slot[launch == 0]) & set(slot[launch == 1]) & set(slot[launch == 2])
    assert len(in_all) > 100, len(in_all)   # slots whose ranks continue across all three launches
    print("slices ok")


def test_ranks_continue_across_remap_launches(hip_module):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, TWTML_FORCE_TIERED="1", TWTML_NEAR_CAP="64", TWTML_PREP_SLICES="3",
               PYTHONPATH=os.pathsep.join([root, here, os.environ.get("PYTHONPATH", "")]))
    code = "import test_gpu_far_csc as t; t.run_slices_case()"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "slices ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.fixture
def far_env(monkeypatch):
    monkeypatch.setenv("TWTML_FORCE_TIERED", "1")
    monkeypatch.setenv("TWTML_NEAR_CAP", "64")


def test_most_entries_far(hip_module, far_env):
    """300 rows of random text, a 64-slot near tier: nearly all entries are
    far and every chunk lists several times 64 of them (the lane loops of the
    remap's rank pass and of k_far_csc; the rank list under a nearly full far
    list)."""
    out = train_and_check(random_rows_batch(300, seed=13))
    assert out["far_total"] > 0.8 * out["entries"]
    assert (out["fcount"] > 64).all()


def test_plain_layout_rows(hip_module, far_env):
    """Rows of more than 320 bigrams stay in the plain layout (clen8c = -1):
    their far entries take the plain path's list, count and rank."""
    out = train_and_check(long_rows_batch(), step=GENTLE["step_size"], iters=GENTLE["num_iterations"], **GENTLE)
    plain = out["clen8c"] < 0
    assert plain.any() and not plain.all()
    assert (out["fcount"][plain] > 64).all() and (out["fcount"][~plain] > 0).any()


def test_heavy_far_slots(hip_module, far_env):
    """About 200 bigrams shared by all 2,000 rows: far slots with thousands of
    entries (a rank counter under contention from every chunk) and several
    entries of one row in one slot."""
    out = train_and_check(heavy_slots_batch(), step=GENTLE["step_size"], iters=GENTLE["num_iterations"], **GENTLE)
    assert (out["counts"] >= 2000).sum() >= 100
    d = out["layout"]
    key = (d["csc_slot"].astype(np.int64) << 32) | d["csc_pos"].astype(np.int64)
    assert np.unique(key).shape[0] < key.shape[0]   # one (row, slot) pair more than once


def test_empty_far_tier(hip_module, monkeypatch):
    """Forced tiered, the whole active set in the near tier: no far slot, no
    far entry, nothing written."""
    monkeypatch.setenv("TWTML_FORCE_TIERED", "1")
    out = train_and_check(near_only_batch())
    d = out["layout"]
    assert out["n_unique"] == out["n_near"] and out["far_total"] == 0
    assert d["offsets"].tolist() == [0] and d["csc_pos"].shape[0] == 0 and not out["fcount"].any()

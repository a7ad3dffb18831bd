"""The silhouette on the GPU (``KMEngine::silhouette``, ``csrc/hip/silhouette.hip``)
against the fp64 contract ``models/silhouette.py``, fed the device's own ``std``
and ``pred`` (labels are ``test_gpu_kmeans_score.py``'s subject).

Bounds, per row p with own cluster A, ``xn = |x_p|^2``, ``mun_G = |mu_G|^2``:

* ``gamma_p(G) = 2 (dp + 4) 2^-24 (xn + mun_G + V_G)``: the fp32 dot-product
  bound of the neighbour pass's first stage (dp products and additions, the
  fp32 roundings of x, mu and B, with a factor 2 to spare).
* ``b`` against the fp64 ``D(p, neighbor_dev)``: ``1e-12 (xn + mun)``,
  ``k_km_cost``'s bound for a sum of squared differences, plus ``2^-40 N V`` from
  the fixed-point ``W`` (``|W_dev - W| <= N 2^-40 max dev2``, so ``V = W / N`` is
  within ``2^-40 max dev2 <= 2^-40 W = 2^-40 N V``).
* ``a = (N dev2 + W) / (N - 1)``: ``(N 1e-12 (xn + mun_A) + N 2^-40 max_A dev2) /
  (N - 1)``.
* ``b_dev >= b_ref - tol`` (the reference is the minimum) and ``b_dev - b_ref <=
  gamma_p(neighbor_dev) + gamma_p(neighbor_ref)``: the device refines the two
  best fp32 scores, so it misses the true neighbour only for clusters whose
  scores are within both errors (``2 gamma_p`` when they name the same cluster).
* ``neighbor_dev == neighbor_ref`` wherever the best and second-best fp64 ``D``
  over G != A differ by more than ``4 gamma_p`` (the larger of the two
  clusters' gammas); the rows left out are at most 2 % of a case.
* ``s`` is bit-equal to the three-branch formula on the device's own a and b.
* The integer words are exact.
"""
import functools
import json

import numpy as np
import pytest

import edge_batches as eb
from test_gpu_kmeans_score import ASSIGN_SIZES, _batch, _cfg, _cost_rows, _dev, _features, _pad_dim
from twitter_stream_ml_amd.models import silhouette as S
from twitter_stream_ml_amd.models.kmeans import StreamingKMeansModel, kmeans_features
from twitter_stream_ml_amd.oracle.mllib import KMeansState, standard_scaler_fit, standard_scaler_transform
from twitter_stream_ml_amd.sources.synthetic import SynthConfig

pytestmark = pytest.mark.gpu
ROW_KEYS = ("rows", "pred", "neighbor", "a", "b", "s")


def _same_bits(r1, r2, rows=True):
    assert r1["accumulator"].to_dict() == r2["accumulator"].to_dict()
    assert r1["silhouette"] == r2["silhouette"] and float(r1["cost"]).hex() == float(r2["cost"]).hex()
    np.testing.assert_array_equal(r1["sizes"], r2["sizes"])
    if rows:
        for key in ROW_KEYS:
            assert r1[key].tobytes() == r2[key].tobytes(), key


def _check(dev, raw, X, rows, apply_filter=True, scaler="batch", max_excluded=0.02):
    """One batch through silhouette_batch against the contract; returns the
    per-row result."""
    k, n = dev.cfg.k, X.shape[0]
    kw = {"apply_filter": apply_filter, "scaler": scaler}
    pb = dev.predict_batch(raw, **kw)
    r = dev.silhouette_batch(raw, per_row=True, **kw)
    # pred, sizes, cost: predict_batch's bits
    assert r["n_raw"] == raw.n and r["n_scored"] == n == pb["n_scored"]
    np.testing.assert_array_equal(r["rows"], rows)
    np.testing.assert_array_equal(r["pred"], pb["pred"])
    np.testing.assert_array_equal(r["sizes"], pb["sizes"])
    assert float(r["cost"]).hex() == float(pb["cost"]).hex()
    if pb["std"] is None:
        assert r["std"] is None
    else:
        np.testing.assert_array_equal(r["std"], pb["std"])
    assert r["neighbor"].dtype == np.int32 and r["pred"].dtype == np.int32 and r["a"].dtype == np.float64
    acc = r["accumulator"]
    # per_row off and a second call: the same bits (the W path is reproducible)
    _same_bits(r, dev.silhouette_batch(raw, per_row=True, **kw))
    _same_bits(r, dev.silhouette_batch(raw, **kw), rows=False)
    if n == 0:
        assert r["silhouette"] is None and acc.to_dict() == S.SilhouetteAccumulator(k).to_dict()
        return r
    pred = r["pred"].astype(np.int64)
    N = np.bincount(pred, minlength=k)
    if np.count_nonzero(N) < 2:   # undefined
        assert r["silhouette"] is None and acc.n_undefined == n and acc.n_total == 0 and acc.n_single == 0
        assert not any(acc.s_fix) and acc.batches == 1
        assert np.all(r["neighbor"] == -1) and not r["a"].any() and not r["b"].any() and not r["s"].any()
        return r
    # the integer words
    assert acc.n == [int(v) for v in N] and acc.n_undefined == 0 and acc.batches == 1
    assert acc.n_single == int(np.count_nonzero(N == 1))
    fix = S.s_fixed(r["s"])
    assert acc.s_fix == [int(fix[pred == g].sum()) for g in range(k)]
    assert r["silhouette"] == acc.silhouette
    # per-row values
    Xs = X if r["std"] is None else standard_scaler_transform(X, r["std"])
    st = S.cluster_stats(Xs, pred, k)
    D = S.mean_dist2(Xs, st["mu"], st["V"], N)
    idx = np.arange(n)
    D[idx, pred] = np.inf
    order = np.argsort(D, axis=1, kind="stable")[:, :2]
    nb_ref = order[:, 0]
    b_ref = D[idx, nb_ref]
    second = D[idx, order[:, 1]] if k > 2 else np.full(n, np.inf)
    xn, mun = (Xs ** 2).sum(axis=1), (st["mu"] ** 2).sum(axis=1)
    dp = dev._eng.dp
    nb = r["neighbor"].astype(np.int64)
    assert np.all((nb >= 0) & (nb < k) & (nb != pred)) and np.all(N[nb] > 0)

    def gamma(g):
        return 2 * (dp + 4) * 2.0 ** -24 * (xn + mun[g] + st["V"][g])

    tol_b = 1e-12 * (xn + mun[nb]) + 2.0 ** -40 * st["W"][nb]
    err_b = np.abs(r["b"] - D[idx, nb])
    assert np.all(err_b <= tol_b), float((err_b / np.maximum(tol_b, 1e-300)).max())
    assert np.all(r["b"] >= b_ref - tol_b)
    over = r["b"] - b_ref
    assert np.all(over <= gamma(nb) + gamma(nb_ref)), float(over.max())
    g2 = np.maximum(gamma(nb_ref), gamma(order[:, 1])) if k > 2 else gamma(nb_ref)
    clear = second - b_ref > 4 * g2
    excluded = 1.0 - np.count_nonzero(clear) / n
    np.testing.assert_array_equal(nb[clear], nb_ref[clear])
    maxdev = np.zeros(k)
    np.maximum.at(maxdev, pred, st["dev2"])
    Na = N[pred]
    multi = Na > 1
    a_ref = np.zeros(n)
    a_ref[multi] = (Na[multi] * st["dev2"][multi] + st["W"][pred[multi]]) / (Na[multi] - 1)
    tol_a = np.zeros(n)
    tol_a[multi] = (Na[multi] * 1e-12 * (xn[multi] + mun[pred[multi]]) + Na[multi] * 2.0 ** -40 * maxdev[pred[multi]]) \
        / (Na[multi] - 1)
    err_a = np.abs(r["a"] - a_ref)
    assert np.all(err_a <= tol_a), float((err_a[multi] / np.maximum(tol_a[multi], 1e-300)).max())
    assert not r["a"][~multi].any() and not r["s"][~multi].any()
    want_s = S.point_silhouette(r["a"], r["b"])
    want_s[~multi] = 0.0
    assert r["s"].tobytes() == want_s.tobytes()
    print(f"k={k} d={X.shape[1]} n={n}: b err/tol {float((err_b / np.maximum(tol_b, 1e-300)).max()):.3g} "
          f"a err/tol {float((err_a[multi] / np.maximum(tol_a[multi], 1e-300)).max()) if multi.any() else 0:.3g} "
          f"excluded {excluded:.4f} neighbour differs {np.count_nonzero(nb != nb_ref)} "
          f"negative s {np.count_nonzero(r['s'] < 0) / n:.3f} silhouette {r['silhouette']:.6f}")
    assert excluded <= max_excluded, excluded
    return r


# ---- 1. + 2. per-row values and the integer words ---------------------------------------------
@pytest.mark.parametrize("k,text_dims,mfma,precision", [
    (1, 0, True, "bf16x3"), (3, 0, False, "bf16x3"), (3, 1, True, "bf16x3"), (31, 14, True, "bf16x3"),
    (33, 14, False, "bf16x3"), (64, 62, True, "fp32"), (200, 126, True, "bf16x3"), (40, 127, True, "bf16x3"),
    (1024, 62, True, "bf16x3")])
def test_silhouette_matches_contract(hip_module, k, text_dims, mfma, precision):
    dev = _dev(k, text_dims, mfma=mfma, precision=precision)
    C = KMeansState.random(k, 2 + text_dims, 0.0, seed=5).centers
    np.testing.assert_array_equal(dev.get_state()[0], C)
    X, rows = _features(text_dims)
    assert X.shape[0] == 2400
    r = _check(dev, _batch(), X, rows)
    if k == 1:
        assert r["silhouette"] is None and r["accumulator"].n_undefined == 2400
    np.testing.assert_array_equal(dev.get_state()[0], C)


def test_silhouette_with_centres_at_the_cluster_means(hip_module):
    k, td = 33, 14
    dev = _dev(k, td)
    X, rows = _features(td)
    raw = _batch()
    pb = dev.predict_batch(raw)
    Xs = standard_scaler_transform(X, pb["std"])
    for _ in range(3):   # a few Lloyd steps on the host: centres at their clusters' means
        C = dev.get_state()[0].copy()
        pred = dev.predict_batch(raw)["pred"]
        for g in np.unique(pred):
            C[g] = Xs[pred == g].mean(axis=0)
        dev.set_state(C, np.ones(k))
    r = _check(dev, raw, X, rows)
    assert np.count_nonzero(r["s"] > 0) > 0.5 * X.shape[0] and r["silhouette"] > 0


# ---- 3. edge shapes -------------------------------------------------------------------------
def _spread(dev, X, scaler="batch"):
    """Centres on the batch's own first scaled rows (the rest far away), so tiny
    batches use several clusters."""
    k, d = dev.cfg.k, X.shape[1]
    std = standard_scaler_fit(X) if isinstance(scaler, str) and scaler == "batch" else None
    Xs = X if std is None else standard_scaler_transform(X, std)
    C = np.full((k, d), 1e3) + np.arange(k)[:, None]
    m = min(k, Xs.shape[0])
    C[:m] = Xs[np.linspace(0, Xs.shape[0] - 1, m).astype(int)]
    dev.set_state(C, np.ones(k))


@pytest.mark.parametrize("d", [2, 3, 16, 17, 64, 128, 129, 1002])
def test_silhouette_edge_shapes(hip_module, d):
    td = d - 2
    dp = _pad_dim(d)
    rows_per_wave, rows_per_wg = _cost_rows(dp)
    k = 3 if d == 1002 else 5
    dev = _dev(k, td)
    assert dev._eng.dp == dp
    synth = SynthConfig.profile("twitter", seed=27, unicode_fraction=0.2)
    defined = 0
    sizes = (1, 2, 33, 300) if d == 1002 else ASSIGN_SIZES[1:]   # k > n at 1 and 2 rows
    for i, m in enumerate(sizes):
        raw = eb.kmeans_tiny_batch(synth, m, 10000 + 400 * i, short_texts=td > 0 and m >= 3)
        X, rows = kmeans_features(raw, td)
        assert X.shape[0] == m
        _spread(dev, X)
        r = _check(dev, raw, X, rows, max_excluded=1.0 if m <= 33 else 0.02)
        defined += r["silhouette"] is not None
    # (the neighbour kernel's workgroup takes 128 rows, a wave 32: ASSIGN_SIZES above)
    edges = sorted({n for e in (rows_per_wave, rows_per_wg) for n in (e - 1, e, e + 1) if n >= 1})
    for n in edges if d != 1002 else [e for e in edges if e <= 300]:
        raw = _batch().slice(0, n)
        X, rows = kmeans_features(raw, td, apply_filter=False)
        _spread(dev, X)
        r = _check(dev, raw, X, rows, apply_filter=False, max_excluded=1.0 if n <= 33 else 0.02)
        defined += r["silhouette"] is not None
    assert defined >= 4
    # a zero-variance column: std 0, factor 0
    raw = eb.kmeans_tiny_batch(synth, 5, 20000, equal_followers=True)
    X, rows = kmeans_features(raw, td)
    _spread(dev, X)
    r = _check(dev, raw, X, rows, max_excluded=1.0)
    assert r["std"][1] == 0 and r["std"][0] > 0
    # no rows, and nothing kept: nothing beyond predict_batch's launches, an empty accumulator
    empty = eb.texts_to_raw([], [], np.zeros((5, 0), np.int64))
    r = dev.silhouette_batch(empty, per_row=True)
    assert r["n_raw"] == 0 and r["n_scored"] == 0 and r["silhouette"] is None and r["s"].shape == (0,)
    assert r["accumulator"].to_dict() == S.SilhouetteAccumulator(k).to_dict()
    none = eb.texts_to_raw(["ab", "cd"], [0, 0], eb.ordinary_scalars(2, 3))
    r = _check(dev, none, np.zeros((0, d)), np.zeros(0, np.int64))
    assert r["n_raw"] == 2 and r["accumulator"].batches == 0


@pytest.mark.parametrize("k", [2, 31, 32, 33, 65])
def test_silhouette_cluster_counts(hip_module, k):
    td = 14
    dev = _dev(k, td)
    raw = _batch().slice(0, 300)
    X, rows = kmeans_features(raw, td, apply_filter=False)
    _spread(dev, X)
    r = _check(dev, raw, X, rows, apply_filter=False, max_excluded=1.0 if k == 2 else 0.02)
    assert r["silhouette"] is not None and np.count_nonzero(r["sizes"]) >= 2


def test_silhouette_degenerate_batches(hip_module):
    k, td = 5, 14
    dev = _dev(k, td)
    raw = _batch().slice(0, 300)
    X, rows = kmeans_features(raw, td, apply_filter=False)
    Xs = standard_scaler_transform(X, standard_scaler_fit(X))
    far = np.full((k, 2 + td), 1e6) * (1 + np.arange(k))[:, None]
    # every row in one cluster: undefined
    C = far.copy()
    C[2] = Xs.mean(axis=0)
    dev.set_state(C, np.ones(k))
    r = _check(dev, raw, X, rows, apply_filter=False)
    assert r["silhouette"] is None and r["accumulator"].n_undefined == 300 and r["sizes"][2] == 300
    # exactly two non-empty clusters, one of them a singleton: an outlier in followers (below 2^30)
    lone = 7
    sc = raw.scalars.copy()
    sc[1, lone] = 500_000_000
    raw = eb.texts_to_raw([raw.text_of(i) for i in range(raw.n)], raw.is_retweet, sc)
    X, rows = kmeans_features(raw, td, apply_filter=False)
    Xs = standard_scaler_transform(X, standard_scaler_fit(X))
    C = far.copy()
    C[1], C[3] = Xs[lone], np.delete(Xs, lone, axis=0).mean(axis=0)
    dev.set_state(C, np.ones(k))
    r = _check(dev, raw, X, rows, apply_filter=False, max_excluded=1.0)
    assert r["sizes"][1] == 1 and r["sizes"][3] == 299 and r["accumulator"].n_single == 1
    assert r["s"][lone] == 0.0 and r["a"][lone] == 0.0 and r["neighbor"][lone] == 3 and r["b"][lone] > 0
    assert np.all(np.delete(r["neighbor"], lone) == 1)
    # all rows identical: one cluster whatever the centres (every column has zero variance)
    same = eb.texts_to_raw(["same text"] * 40, np.ones(40, np.uint8), np.tile(eb.ordinary_scalars(1, 4), (1, 40)))
    Xi, ri = kmeans_features(same, td)
    assert Xi.shape[0] == 40 and not np.ptp(Xi, axis=0).any()
    for scaler in ("batch", "none"):
        r = _check(dev, same, Xi, ri, scaler=scaler)
        assert r["silhouette"] is None and r["accumulator"].n_undefined == 40


# ---- 4. a row depends on its batch only through the cluster statistics -------------------------
def test_silhouette_filtered_equals_unfiltered_on_retweets(hip_module):
    k, td = 33, 14
    dev = _dev(k, td)
    X, rows = _features(td)
    raw = _batch()
    only = raw.take(rows)   # all retweets
    Xo, ro = kmeans_features(only, td)
    np.testing.assert_array_equal(Xo, X)
    std = standard_scaler_fit(X)
    _spread(dev, standard_scaler_transform(X, std), scaler="none")
    a = dev.silhouette_batch(only, per_row=True, scaler=std, apply_filter=True)
    b = dev.silhouette_batch(only, per_row=True, scaler=std, apply_filter=False)
    _same_bits(a, b)
    assert a["n_scored"] == 2400 and a["silhouette"] is not None


# ---- 5. nothing else moves -----------------------------------------------------------------
def test_silhouette_leaves_model_training_and_memory_alone(hip_module):
    import torch
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans
    k, td = 64, 30
    a = DeviceKMeans(_cfg(k, td, seed=5), device=0)
    b = DeviceKMeans(_cfg(k, td, seed=5), device=0)
    for raw in [_batch(4000, t, seed=33) for t in range(3)]:
        a.update_raw(raw)
        b.update_raw(raw)
    train = [_batch(4000, t, seed=8) for t in range(4)]
    other = [_batch(3000, t, seed=9) for t in range(5)]
    c0, w0 = b.get_state()
    p0 = b.predict_batch(other[0])
    s0 = b.silhouette_batch(other[0])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    assert s0["n_scored"] > 0 and s0["silhouette"] is not None
    c1, w1 = b.get_state()
    assert c0.tobytes() == c1.tobytes() and w0.tobytes() == w1.tobytes()
    # a predict_batch right after it returns what it returned before it (the cached centres are untouched)
    p1 = b.predict_batch(other[0])
    for key in ("rows", "pred", "dist2", "sizes", "std"):
        assert p0[key].tobytes() == p1[key].tobytes()
    assert p0["cost"] == p1["cost"]
    for t, raw in enumerate(train):
        ra = a.update_raw(raw)
        b.silhouette_batch(other[t], scaler="none" if t % 2 else "batch", per_row=bool(t & 2))
        if t == 2:   # between the prefetch of a batch and the update that consumes it
            assert b.prefetch(raw)
            b.silhouette_batch(other[4], apply_filter=False)
            assert b._pipe.in_flight == 1
        rb = b.update_raw(raw)
        if t == 2:
            assert b._pipe.hits == 1
        np.testing.assert_array_equal(ra["std"], rb["std"])
        np.testing.assert_array_equal(np.asarray(ra["pred"]), np.asarray(rb["pred"]))
        (ca, wa), (cb, wb) = a.get_state(), b.get_state()
        assert ca.tobytes() == cb.tobytes() and wa.tobytes() == wb.tobytes()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free0   # the scratch was allocated by the first call


def test_silhouette_issues_no_collective(hip_module):
    from twitter_stream_ml_amd.ops.kmeans_engine import DeviceKMeans
    k, td = 64, 14
    comm = hip_module.Comm(hip_module.rccl_unique_id(), 0, 1, 0)
    dp = DeviceKMeans(_cfg(k, td, seed=3, force_dp=True), device=0, comm=comm)
    plain = DeviceKMeans(_cfg(k, td, seed=3), device=0)
    raw = _batch()
    for e in (dp, plain):
        e.update_raw(_batch(4000, 1, seed=8))
    before = dict(comm.counters())
    assert before["allreduce_calls"] >= 3
    for kw in ({}, {"apply_filter": False}, {"scaler": "none"}):
        ra, rb = dp.silhouette_batch(raw, per_row=True, **kw), plain.silhouette_batch(raw, per_row=True, **kw)
        _same_bits(ra, rb)
        assert ra["n_scored"] > 0
    assert dict(comm.counters()) == before


# ---- 6. the driver -------------------------------------------------------------------------
def test_silhouette_driver_gpu_matches_cpu(hip_module, tmp_path):
    """``silhouette``: both drivers average per-row s over the same rows; a
    row's s moves by at most ``(|da| + |db|) / max(a, b)`` with a and b inside
    case 1's per-row tolerances, orders of magnitude below the 1e-6 asserted,
    unless a label or a neighbour differs (at most 2 labels, as in
    ``test_score_driver_gpu_matches_cpu``, each moving the mean by <= 2 / n and
    its clusters' statistics slightly): 1e-3 covers those on 2400 rows."""
    from twitter_stream_ml_amd.apps import score as score_app
    from twitter_stream_ml_amd.sources import write_jsonl
    k, td = 33, 14
    st = KMeansState.random(k, 2 + td, 0.0, seed=5)
    ck = tmp_path / "km"
    StreamingKMeansModel(st.centers, np.ones(k)).save(str(ck))
    raw = _batch()
    write_jsonl(str(tmp_path / "stream.jsonl"), raw.to_statuses())
    out = {}
    for master in ("local[1]", "rocm[1]"):
        out[master] = tmp_path / master.split("[")[0]
        args = ["--master", master, "--lightning", "http://127.0.0.1:9", "--twtweb", "http://127.0.0.1:9",
                "--source", f"replay:{tmp_path / 'stream.jsonl'}", "--seconds", "0", "--batchSize", "4000",
                "--sourceRate", "0", "--numBatches", "1", "--model", str(ck), "--silhouetteOut", str(out[master])]
        assert score_app.main(args) == 0
    rec = {m: json.loads(open(p / "silhouette.jsonl").readline()) for m, p in out.items()}
    summ = {m: json.load(open(p / "summary.json")) for m, p in out.items()}
    cpu, gpu = rec["local[1]"], rec["rocm[1]"]
    assert gpu["n_raw"] == cpu["n_raw"] == 4000 and gpu["n_scored"] == cpu["n_scored"] == 2400
    assert gpu["n_undefined"] == cpu["n_undefined"] == 0
    ng, nc = np.array(gpu["accumulator"]["n"]), np.array(cpu["accumulator"]["n"])
    assert ng.sum() == nc.sum() == 2400 and np.abs(ng - nc).sum() <= 4   # at most 2 labels differ
    moved = int(np.abs(ng - nc).sum())
    print(f"silhouette gpu {gpu['silhouette']!r} cpu {cpu['silhouette']!r} labels moved {moved}")
    assert abs(gpu["silhouette"] - cpu["silhouette"]) <= (1e-6 if moved == 0 else 1e-3)
    if moved == 0:
        assert gpu["n_single"] == cpu["n_single"] and gpu["clusters_used"] == cpu["clusters_used"]
    np.testing.assert_allclose(gpu["cost"], cpu["cost"], rtol=1e-5)
    assert gpu["sil_ms"] > 0
    for m in out:
        acc = S.SilhouetteAccumulator.from_dict(rec[m]["accumulator"])
        assert summ[m]["accumulator"] == acc.to_dict() and summ[m]["silhouette"] == acc.silhouette

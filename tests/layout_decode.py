"""Host-side decoders of the engine's debug dumps, shared by the GPU tests.

``debug_prepared`` / ``debug_hybrid`` return the prepared batch in the layout
the iteration kernels read (SELL-16x4: chunk c = 16 rows, row r owns lanes
4r..4r+3, groups of 8 entries per lane); these helpers turn it back into per
kept row feature ids, so a test can compare them with the oracle.
"""
import numpy as np


def rows_from_debug(dbg):
    """Per kept row (kept order) -> sorted multiset of hashed feature ids.

    SELL-16x4 layout: chunk c = 16 rows, row r owns lanes 4r..4r+3.
    """
    nk = int(dbg["counters"][0])
    idx, clen8, cbase, perm = dbg["idx"], dbg["clen8"], dbg["cbase"], dbg["perm"]
    rows = [None] * nk
    for c in range(clen8.shape[0]):
        g0, L8 = int(cbase[c]), int(clen8[c])
        block = idx[g0 * 512:(g0 + L8) * 512].reshape(L8, 64, 8)
        for r in range(16):
            k = int(perm[c * 16 + r])
            if k < 0:
                continue
            v = block[:, 4 * r:4 * r + 4, :].reshape(-1)
            rows[k] = np.sort(v[v >= 0])
    return rows


def hybrid_row_counts(hy, uniq, cbase, c, r):
    """``{feature id: count}`` of row r of chunk c in the hybrid layout: the
    4-bit counts of the 128 hot slots (lane 4r+t holds hot ids 32t..32t+31)
    plus one per cold-stream entry (count overflow lands there too).
    ``uniq`` is the sorted active set, ``cbase`` from ``debug_prepared``."""
    nU = uniq.shape[0]
    hot_slot = hy["hot_slot"]
    dense = hy["hot_dense"].reshape(-1, 64, 4)
    L4c = int(hy["clen8c"][c])            # cold 4-entry groups per lane
    g0 = int(cbase[c])
    blk = hy["cslot"][g0 * 512:g0 * 512 + L4c * 256].reshape(L4c, 64, 4)
    got = {}
    for t in range(4):
        words = dense[c, 4 * r + t]
        for i in range(32):
            n = (int(words[i // 8]) >> (4 * (i % 8))) & 15
            if n:
                fid = int(uniq[hot_slot[32 * t + i] - 4])
                got[fid] = got.get(fid, 0) + n
    sl = blk[:, 4 * r:4 * r + 4, :].reshape(-1)
    sl = sl[(sl >= 4) & (sl < 4 + nU)]
    for fid in uniq[sl - 4].tolist():
        got[fid] = got.get(fid, 0) + 1
    return got


def oracle_row_ids(Xt, k):
    """Sorted multiset of text-feature ids of oracle row k (CSR ``Xt``)."""
    s, e = Xt.indptr[k], Xt.indptr[k + 1]
    return np.sort(np.repeat(Xt.indices[s:e], Xt.data[s:e].astype(np.int64)))


def oracle_row_counts(Xt, k):
    """``{feature id: count}`` of oracle row k (CSR ``Xt``)."""
    a, b = Xt.indptr[k], Xt.indptr[k + 1]
    return dict(zip(Xt.indices[a:b].tolist(), Xt.data[a:b].astype(int).tolist()))


def scalars_by_kept(dbg):
    """Device labels [nk] and numeric features [nk, 4] in kept order (they are
    stored by sorted position; ``perm`` maps position -> kept index)."""
    nk = int(dbg["counters"][0])
    y = np.zeros(nk, np.float32)
    num = np.zeros((nk, 4), np.float32)
    perm = dbg["perm"]
    R = perm.shape[0]
    for pos in range(R):
        k = int(perm[pos])
        if k >= 0:
            y[k] = dbg["y"][pos]
            num[k] = dbg["num"][np.arange(4) * R + pos]
    return y, num

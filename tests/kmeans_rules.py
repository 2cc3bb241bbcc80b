"""Numpy restatement of the GPU k-means rules, independent of the project's code.

Not a test module (no test_ prefix): tests/test_kmeans_host.py checks it against the fixture and tests/test_gpu_kmeans.py
uses its exact key as the arbiter of near ties.  tools/gen_golden_kmeans.py uses it to measure each fixture case's margins,
and tools/gen_golden_kmeans_edges.py also reads each case's stated property from `lloyd`'s trace and stores its centres.

  key(x, c)    fp64 fma chain of (x_k - c_k)^2 over k ascending (fma emulated exactly where it matters: `fma_key_rows`)
  seeding      sklearn's _kmeans_plusplus with closest = f32(key), fp64 cumulative sums, pots = f32(fp64 sum)
  Lloyd        sklearn's _kmeans_single_lloyd with exact labels, fp64 cluster sums, f32(sum / count), relocation by
               (key descending, row ascending), a cluster left empty placed as sklearn's _average_centers places it,
               strict / tol (fp64 sum of fp64 shift^2) / max_iter stopping
"""
from fractions import Fraction

import numpy as np


def fma_key_rows(x: np.ndarray, C: np.ndarray) -> np.ndarray:
    """Keys of one row x against the rows of C, every fma rounded once (exact rational arithmetic; slow: few rows only)."""
    out = np.empty(len(C), dtype=np.float64)
    for j in range(len(C)):
        acc = 0.0
        for k in range(x.shape[0]):
            t = float(x[k]) - float(C[j, k])                  # one fp64 rounding, as the kernel's subtraction
            acc = float(Fraction(t) * Fraction(t) + Fraction(acc))   # fma: exact t*t + acc, rounded once (int / int)
        out[j] = acc
    return out


def keys_fast(X: np.ndarray, C: np.ndarray) -> np.ndarray:
    """fp64 keys without fma (each product and sum rounded): within a few fp64 ulps of the fma chain."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    acc = np.zeros((len(X), len(C)), dtype=np.float64)
    for k in range(X.shape[1]):
        t = X64[:, k:k + 1] - C64[None, :, k]
        acc += t * t
    return acc


def exact_argmin(X: np.ndarray, C: np.ndarray, rel: float = 1e-12):
    """argmin of the exact key per row, ties to the lowest index, and those keys.  Screens with keys_fast and re-keys rows
    whose two best keys lie within `rel` of each other with fma_key_rows (all centres within the band)."""
    K = keys_fast(X, C)
    lab = K.argmin(1)
    best = K[np.arange(len(X)), lab]
    keys = best.copy()
    band = K <= best[:, None] * (1 + rel) + 1e-300
    near = np.nonzero(band.sum(1) > 1)[0]
    for i in near:
        js = np.nonzero(band[i])[0]
        kk = fma_key_rows(X[i], C[js])
        m = kk.min()
        lab[i] = js[np.nonzero(kk == m)[0][0]]
        keys[i] = m
    # rows decided without re-keying: their key with exact fma
    return lab, keys, near


def kmeans_plusplus(X: np.ndarray, n_clusters: int, first: int, u: np.ndarray):
    """Seeding of one start from its draws (first index, u [K-1][L]); returns indices and per-step margins:
    the smallest |u*pot - cumsum boundary| / pot over all draws and the smallest relative gap between the best candidate pot
    and the pot of any candidate whose min array differs from the winner's."""
    n = len(X)
    idx = np.full(n_clusters, -1, dtype=np.int64)
    idx[0] = first
    closest = keys_fast(X, X[[first]])[:, 0].astype(np.float32)
    pot = np.float32(closest.astype(np.float64).sum())
    draw_gap, pot_gap = np.inf, np.inf
    for c in range(1, n_clusters):
        cs = np.cumsum(closest.astype(np.float64))
        v = u[c - 1] * np.float64(pot)
        cand = np.searchsorted(cs, v)
        cand = np.minimum(cand, n - 1)
        if pot > 0:
            pos = np.searchsorted(cs, v)
            hi = np.abs(cs[np.minimum(pos, n - 1)] - v)
            lo = np.where(pos > 0, np.abs(cs[np.maximum(pos - 1, 0)] - v), np.inf)
            draw_gap = min(draw_gap, float(np.minimum(hi, lo).min()) / float(pot))
        d = keys_fast(X[cand], X).astype(np.float32)
        m = np.minimum(closest[None, :], d)
        pots = m.astype(np.float64).sum(1).astype(np.float32)
        b = int(np.argmin(pots))
        # candidates whose min arrays equal the winner's tie exactly in every implementation: only the others compete
        others = [float(pots[t]) for t in range(len(cand)) if not np.array_equal(m[t], m[b])]
        if others and pots[b] > 0:
            pot_gap = min(pot_gap, (min(others) - float(pots[b])) / float(pots[b]))
        pot = pots[b]
        closest = m[b]
        idx[c] = cand[b]
    return idx, draw_gap, pot_gap


def lloyd(X: np.ndarray, init: np.ndarray, max_iter: int, tol: float, trace: list = None):
    """One Lloyd run (X already centred, init f32 [K][d]).  Returns centres, labels, inertia, n_iter, strict, relocations.
    A list given as `trace` receives one dict per iteration: "moved" [(row, donor, new cluster)] in the order of the moves,
    "left_empty" (clusters with no row after the moves, ascending) and "big" (the biggest cluster then, first maximum)."""
    n, d = X.shape
    K = len(init)
    centers = init.astype(np.float32).copy()
    labels_old = np.full(n, -1, dtype=np.int64)
    strict = False
    relocations = 0
    X64 = X.astype(np.float64)
    for i in range(max_iter):
        lab, keys, _ = exact_argmin(X, centers)
        counts = np.bincount(lab, minlength=K).astype(np.int64)
        sums = np.zeros((K, d), dtype=np.float64)
        np.add.at(sums, lab, X64)
        empty = np.nonzero(counts == 0)[0]
        moved = []
        if len(empty) and keys.max() > 0:
            order = np.lexsort((np.arange(n), -keys))[:len(empty)]
            for e, r in zip(empty, order):
                old = lab[r]
                sums[old] -= X64[r]
                sums[e] = X64[r]
                counts[e] = 1
                counts[old] -= 1
                relocations += 1
                moved.append((int(r), int(old), int(e)))
        new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0).astype(np.float32)
        big = int(np.argmax(counts))                  # sklearn _average_centers: empty -> the biggest cluster's row as it
        for e in np.nonzero(counts <= 0)[0]:          # stands in the ascending loop (still the sum when it comes later)
            new[e] = (sums[big] if e < big else sums[big] / counts[big]).astype(np.float32)
        if trace is not None:
            trace.append({"moved": moved, "left_empty": [int(e) for e in np.nonzero(counts <= 0)[0]], "big": big})
        shift2 = ((new.astype(np.float64) - centers.astype(np.float64)) ** 2).sum(1)
        centers = new
        if np.array_equal(lab, labels_old):
            strict = True
            break
        if shift2.sum() <= tol:
            break
        labels_old = lab
    if not strict:
        lab, _, _ = exact_argmin(X, centers)
    keys = keys_fast(X, centers)[np.arange(n), lab]
    return centers, lab.astype(np.int32), float(keys.sum()), i + 1, strict, relocations


def is_same_clustering(l1, l2, K):
    mapping = np.full(K, -1, dtype=np.int64)
    mapping[l1] = l2
    return bool(np.array_equal(mapping[l1], l2))


def seeding_draws(rs, n, K, n_starts, L):
    w = np.ones(n, dtype=np.float32)
    first = np.empty(n_starts, dtype=np.int64)
    u = np.empty((n_starts, max(K - 1, 1), L))
    for s in range(n_starts):
        first[s] = rs.choice(n, p=w / w.sum())
        for c in range(1, K):
            u[s, c - 1] = rs.uniform(size=L)
    return first, u


def fit(X: np.ndarray, K: int, seed: int, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4):
    """KMeans(K, random_state=seed, n_init=n_init).fit(X) by the stated rules; returns a dict (best start included)."""
    n = len(X)
    tol_abs = np.mean(np.var(X, axis=0)) * tol if tol else 0
    mean = X.mean(axis=0)
    Xc = X - mean
    L = 2 + int(np.log(K))
    first, u = seeding_draws(np.random.RandomState(seed), n, K, n_init, L)
    best = None
    runs = []
    for s in range(n_init):
        idx, _, _ = kmeans_plusplus(Xc, K, int(first[s]), u[s])
        res = lloyd(Xc, Xc[idx], max_iter, float(tol_abs))
        runs.append(res)
        if best is None or (res[2] < runs[best][2] and not is_same_clustering(res[1], runs[best][1], K)):
            best = s
    c, lab, inertia, n_iter, strict, _ = runs[best]
    return {"centers": c + mean, "labels": lab, "inertia": inertia, "n_iter": n_iter, "best_start": best}

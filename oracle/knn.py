"""CPU restatement of src/geo/knn_graph_optimized.py (reference).  TEST INFRASTRUCTURE ONLY.

The neighbour search (sklearn in the reference, knn_graph_optimized.py:40-42) is restated as an exact
fp64-ranked brute force in geo_oracle.c; the CSR assembly / symmetrisation (:54-66) with plain numpy
key arithmetic; connected components (:173-181) with a scan-order flood fill.
"""
import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
from scipy import sparse

from ._clib import lib


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def knn_search(z: np.ndarray, n_neighbors: int) -> Tuple[np.ndarray, np.ndarray]:
    """(distances fp64 (N,kq), indices int64 (N,kq)) including self, sorted by (distance, index).

    sklearn's algorithm="auto" picks the kd-tree for d <= 15 and brute force above
    (sklearn/neighbors/_base.py:627): the squared distance is formed directly for the former and by
    the |x|^2 - 2xy + |y|^2 expansion for the latter.
    """
    z = np.ascontiguousarray(z, dtype=np.float32)
    N, d = z.shape
    idx = np.empty((N, n_neighbors), np.int64)
    d2 = np.empty((N, n_neighbors), np.float64)
    form = 1 if d > 15 else 0
    rc = lib().oracle_knn(_ptr(z), N, d, n_neighbors, form, 0, N, _ptr(idx), _ptr(d2))
    if rc != 0:
        raise RuntimeError(f"oracle_knn failed: {rc}")
    return np.sqrt(d2), idx


def knn_pair_keys(z: np.ndarray, qi: np.ndarray, qj: np.ndarray, form: int) -> np.ndarray:
    """The fp64 key oracle_knn ranks the pair (qi[p], qj[p]) by (same C function), for arbitrary pairs."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    qi = np.ascontiguousarray(qi, dtype=np.int64)
    qj = np.ascontiguousarray(qj, dtype=np.int64)
    out = np.empty(qi.shape[0], np.float64)
    rc = lib().oracle_knn_pair_keys(_ptr(z), z.shape[0], z.shape[1], int(form), _ptr(qi), _ptr(qj), qi.shape[0], _ptr(out))
    if rc != 0:
        raise RuntimeError(f"oracle_knn_pair_keys failed: {rc}")
    return out


def _host(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def check_knn_lists(z, idx, d2, n_neighbors: int, form: int, row0: int = 0, device=None,
                    block_bytes: int = 1 << 30) -> Dict[str, float]:
    """Exact check of kNN lists on EVERY row: idx / d2 [rows, n_neighbors] for the query rows [row0, row0 + rows) of the
    corpus z [N, d] (float32), form as for oracle_knn.  Raises AssertionError naming the first failing row when
      - an index is outside [0, N) or repeated in its row, or a row is not ordered by (distance, index);
      - a key differs in any bit from oracle_knn's key of that pair (oracle_knn_pair_keys);
      - some corpus row j outside row i's list has (key_ij, j) < (d2[i, -1], idx[i, -1]): a missed neighbour.
    The last test screens all N pairs of every row with torch's fp64 arithmetic on `device` (blocks of rows,
    block_bytes of fp64 per block) and re-evaluates the flagged pairs exactly.  Nothing here runs the project's code.
    Returns counts and the wall time."""
    import time
    import torch
    t0 = time.perf_counter()
    zh = _host(z, np.float32)
    ih = _host(idx, np.int64)
    dh = _host(d2, np.float64)
    N, d = zh.shape
    assert ih.ndim == 2 and ih.shape[1] == n_neighbors, f"kNN lists: shape {ih.shape}, expected (rows, {n_neighbors})"
    assert dh.shape == ih.shape, f"kNN keys: shape {dh.shape} against lists {ih.shape}"
    rows, kq = ih.shape
    assert 0 <= row0 and row0 + rows <= N and kq <= N, f"kNN lists: rows [{row0}, {row0 + rows}) of a corpus of {N}"

    def fail(bad, why):
        r = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"kNN row {row0 + r} ({int(bad.sum())} bad row(s)): {why(r)}; "
                             f"list {ih[r].tolist()}, keys {dh[r].tolist()}")

    # structure
    bad = ((ih < 0) | (ih >= N)).any(axis=1)
    if bad.any():
        fail(bad, lambda r: "index outside [0, N)")
    bad = (np.diff(np.sort(ih, axis=1), axis=1) == 0).any(axis=1)
    if bad.any():
        fail(bad, lambda r: "repeated index")
    bad = ~np.isfinite(dh).all(axis=1)
    if bad.any():
        fail(bad, lambda r: "non-finite key")
    a_d, b_d, a_i, b_i = dh[:, :-1], dh[:, 1:], ih[:, :-1], ih[:, 1:]
    bad = ~((a_d < b_d) | ((a_d == b_d) & (a_i < b_i))).all(axis=1)
    if bad.any():
        fail(bad, lambda r: "not ordered by (distance, index)")
    # keys, bit for bit
    qi = np.repeat(np.arange(row0, row0 + rows, dtype=np.int64), kq)
    ref = knn_pair_keys(zh, qi, ih.ravel(), form).reshape(rows, kq)
    bad = (ref.view(np.int64) != dh.view(np.int64)).any(axis=1)
    if bad.any():
        def why(r):
            c = int(np.flatnonzero(ref[r].view(np.int64) != dh[r].view(np.int64))[0])
            return f"key of neighbour {int(ih[r, c])} (position {c}) is {dh[r, c]!r}, the oracle's {ref[r, c]!r}"
        fail(bad, why)
    # completeness.  Screen: A_ij = -2 x_i.x_j + (1 - c) |x_i|^2 + (1 - c) |x_j|^2 <= T_i (the row's last key), one fp64 GEMM
    # of [-2 x, (1 - c) |x|^2, 1] by [y, 1, (1 - c) |y|^2]^T, i.e. the approximate squared distance <= T_i + c (|x_i|^2 + |x_j|^2).
    # First-order error bounds, u = 2^-53, any summation order: the GEMM's d + 2 terms have sum |.| <= 2 (|x|^2 + |y|^2) and err
    # by <= (d + 1) u of that; torch's norms err by <= d u |x|^2, the (1 - c) scaling by u; so A is within (3 d + 5) u (|x|^2 +
    # |y|^2) of the exact value.  oracle_knn's key is within (2 d + 4) u (|x|^2 + |y|^2) of it (expansion: d-term chains for the
    # norms and the dot product, two additions of magnitude <= 2 (|x|^2 + |y|^2); direct: d-term chain of squared differences,
    # each difference rounded once, sum <= 2 (|x|^2 + |y|^2); the clamp at 0 only raises it).  Together < 5 (d + 2) u (|x|^2 +
    # |y|^2): with c = 16 (d + 2) u every pair whose oracle key is <= T_i is flagged, with ample room for the second-order terms
    # (float32 inputs neither underflow nor overflow in fp64).  Flagged pairs outside the list are re-evaluated with the
    # oracle's own key and compared lexicographically with (T_i, idx[i, -1]).
    dev = torch.device(device) if device is not None else torch.device("cpu")
    c = 16.0 * (d + 2) * 2.0 ** -53
    Z = torch.from_numpy(zh).to(dev).to(torch.float64)
    nrm = (Z * Z).sum(dim=1)
    left = torch.cat([-2.0 * Z, ((1.0 - c) * nrm)[:, None], torch.ones_like(nrm)[:, None]], dim=1)
    right = torch.cat([Z, torch.ones_like(nrm)[:, None], ((1.0 - c) * nrm)[:, None]], dim=1)
    T = torch.from_numpy(dh[:, -1].copy()).to(dev)
    I = torch.from_numpy(ih).to(dev)
    B = int(max(1, min(rows, block_bytes // (8 * N))))
    flagged = 0
    for b0 in range(0, rows, B):
        b1 = min(rows, b0 + B)
        A = left[row0 + b0:row0 + b1] @ right.T
        ii, jj = torch.nonzero(A <= T[b0:b1, None], as_tuple=True)
        del A
        flagged += int(ii.numel())
        out = ~(I[b0 + ii] == jj[:, None]).any(dim=1)
        ii, jj = (ii[out] + b0).cpu().numpy(), jj[out].cpu().numpy()
        if ii.size == 0:
            continue
        key = knn_pair_keys(zh, ii + row0, jj, form)
        miss = (key < dh[ii, -1]) | ((key == dh[ii, -1]) & (jj < ih[ii, -1]))
        if miss.any():
            p = int(np.flatnonzero(miss)[0])
            r, j = int(ii[p]), int(jj[p])
            bad = np.zeros(rows, bool)
            bad[r] = True
            fail(bad, lambda r: f"misses neighbour {j} (key {key[p]!r}) ahead of its last entry "
                                f"({int(ih[r, -1])}, {dh[r, -1]!r}); {int(miss.sum())} missed pair(s) in rows "
                                f"[{row0 + b0}, {row0 + b1})")
    return {"rows": rows, "flagged_pairs": flagged, "block_rows": B, "seconds": time.perf_counter() - t0}


def drop_self(distances: np.ndarray, indices: np.ndarray):
    """knn_graph_optimized.py:45-52: drop column 0 when it is self everywhere, else each row's first minimum."""
    N = indices.shape[0]
    if (indices[:, 0] == np.arange(N)).all():
        return distances[:, 1:], indices[:, 1:]
    pos = np.argmin(distances, axis=1)
    keep = np.ones(distances.shape, dtype=bool)
    keep[np.arange(N), pos] = False
    return distances[keep].reshape(N, -1), indices[keep].reshape(N, -1)


def symmetrise(N: int, indices: np.ndarray, weights: np.ndarray, sym: str) -> sparse.csr_matrix:
    """Directed kNN lists -> canonical symmetric CSR (f32), zero diagonal, no stored zeros (:54-66)."""
    if sym not in ("mutual", "union"):
        raise ValueError(f"Invalid symmetry mode: {sym}")
    rows = np.repeat(np.arange(N, dtype=np.int64), indices.shape[1])
    cols = indices.ravel().astype(np.int64)
    w = weights.ravel().astype(np.float32)
    fwd = rows * N + cols
    bwd = cols * N + rows
    keys = np.union1d(fwd, bwd)
    a = np.zeros(keys.shape[0], np.float32)          # W[r, c], absent = 0
    b = np.zeros(keys.shape[0], np.float32)          # W[c, r]
    a[np.searchsorted(keys, fwd)] = w
    b[np.searchsorted(keys, bwd)] = w
    val = np.maximum(a, b) if sym == "union" else np.minimum(a, b)
    r, c = keys // N, keys % N
    keep = (r != c) & (val != 0)
    return sparse.csr_matrix((val[keep], (r[keep], c[keep])), shape=(N, N), dtype=np.float32)


def build_knn_graph_sklearn(z: np.ndarray, k: int = 10, metric: str = "euclidean", mode: str = "distance",
                            sym: str = "mutual") -> Tuple[sparse.csr_matrix, Dict[str, np.ndarray]]:
    assert z.ndim == 2, "z must be (N,D)"
    if metric not in ("euclidean", "cosine"):
        raise NotImplementedError("oracle restates the euclidean and cosine metrics only")
    N = z.shape[0]
    if N == 0:
        return (sparse.csr_matrix((0, 0), dtype=np.float32),
                {"distances": np.empty((0, 0), np.float32), "indices": np.empty((0, 0), dtype=int)})
    k_eff = max(0, min(k, N - 1))
    if k_eff == 0:
        return (sparse.csr_matrix((N, N), dtype=np.float32),
                {"distances": np.empty((N, 0), np.float32), "indices": np.empty((N, 0), dtype=int)})
    if metric == "cosine":
        # sklearn: cosine_distances = 1 - <x/|x|, y/|y|>, clipped to [0, 2] (sklearn/metrics/pairwise.py); for unit rows
        # that is |x^ - y^|^2 / 2, ranked here in fp64 on the float32-rounded unit rows (zero rows stay zero, as in
        # sklearn's normalize)
        z64 = z.astype(np.float64)
        nrm = np.sqrt((z64 * z64).sum(axis=1, keepdims=True))
        zn = (z64 / np.where(nrm == 0.0, 1.0, nrm)).astype(np.float32)
        dist, idx = knn_search(zn, min(k_eff + 1, N))
        dist = np.clip(dist * dist * 0.5, 0.0, 2.0)
    else:
        dist, idx = knn_search(z, min(k_eff + 1, N))
    dist, idx = drop_self(dist, idx)
    weights = dist if mode == "distance" else np.ones_like(dist)
    W = symmetrise(N, idx, weights, sym)
    return W, {"distances": dist.astype(np.float32), "indices": idx}


def build_knn_graph_auto(z, k=10, metric="euclidean", mode="distance", sym="mutual",
                         force_method: Optional[str] = None, size_threshold: int = 50000):
    if force_method == "faiss":
        raise RuntimeError("force_method='faiss' but FAISS not available")
    return build_knn_graph_sklearn(z, k=k, metric=metric, mode=mode, sym=sym)


def build_knn_graph(z, k=10, metric="euclidean", mode="distance", sym="mutual"):
    return build_knn_graph_auto(z, k=k, metric=metric, mode=mode, sym=sym)


def build_knn_graph_faiss_semantics(z, k=10, metric="euclidean", mode="distance", sym="mutual"):
    """knn_graph_optimized.py:70-126 with faiss.IndexFlatL2 / IndexFlatIP restated from their published definition
    (faiss 1.x, not installed here: PARITY UNPINNED): exhaustive search, `search` returns SQUARED L2 distances resp. inner
    products as float32, nearest / largest first.  Small inputs only (dense N x N matrix)."""
    z = np.asarray(z)
    N = z.shape[0]
    if metric == "euclidean":
        x = np.ascontiguousarray(z.astype(np.float32)).astype(np.float64)
        score = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
        order = np.argsort(score, axis=1, kind="stable")[:, :min(k + 1, N)]
        dist = np.take_along_axis(score, order, axis=1).astype(np.float32)
    elif metric == "cosine":
        x = np.ascontiguousarray((z / (np.linalg.norm(z, axis=1, keepdims=True) + 1e-8)).astype(np.float32)).astype(np.float64)
        sim = x @ x.T
        order = np.argsort(-sim, axis=1, kind="stable")[:, :min(k + 1, N)]
        dist = (np.float32(1.0) - np.take_along_axis(sim, order, axis=1).astype(np.float32)).astype(np.float32)
    else:
        raise ValueError(f"FAISS metric '{metric}' not supported. Use 'euclidean' or 'cosine'.")
    idx = order.astype(np.int64)
    if idx.shape[1] > 1 and (idx[:, 0] == np.arange(N)).all():
        dist, idx = dist[:, 1:], idx[:, 1:]
    kk = idx.shape[1]
    data = dist.ravel() if mode == "distance" else np.ones(N * kk, dtype=np.float32)
    W = sparse.csr_matrix((data, (np.repeat(np.arange(N), kk), idx.ravel())), shape=(N, N))
    if sym == "mutual":
        W = W.minimum(W.T)
    elif sym == "union":
        W = W.maximum(W.T)
    else:
        raise ValueError(f"Invalid symmetry mode: {sym}")
    W.setdiag(0.0)
    W.eliminate_zeros()
    return W.tocsr(), {"distances": dist, "indices": idx}


def connected_components(W: sparse.spmatrix) -> Tuple[int, np.ndarray]:
    W = sparse.csr_matrix(W)
    WT = W.T.tocsr()
    n = W.shape[0]
    labels = np.empty(n, np.int32)
    ip, ix = W.indptr.astype(np.int32), W.indices.astype(np.int32)
    ipT, ixT = WT.indptr.astype(np.int32), WT.indices.astype(np.int32)
    ncomp = lib().oracle_cc(n, _ptr(ip), _ptr(ix), _ptr(ipT), _ptr(ixT), _ptr(labels))
    return int(ncomp), labels


def largest_connected_component(W: sparse.spmatrix) -> np.ndarray:
    """knn_graph_optimized.py:173-181."""
    ncomp, labels = connected_components(W)
    if ncomp <= 1:
        return np.ones(W.shape[0], dtype=bool)
    return labels == np.argmax(np.bincount(labels))


def analyze_graph_connectivity(W: sparse.spmatrix) -> Dict:
    """knn_graph_optimized.py:184-219 (stats only, no prints)."""
    N = W.shape[0]
    ncomp, labels = connected_components(W)
    if ncomp > 1:
        largest = int(np.bincount(labels).max())
        ratio = largest / N
    else:
        largest, ratio = N, 1.0
    deg = np.asarray(W.sum(axis=1)).ravel()
    return {"n_nodes": N, "n_edges": W.nnz, "n_components": ncomp, "largest_component_size": largest,
            "connectivity_ratio": ratio, "avg_degree": deg.mean(), "min_degree": deg.min(),
            "max_degree": deg.max()}

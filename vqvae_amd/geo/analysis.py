"""Scores and the PCA view of the geodesic k-medoids analysis (the reference's demos/kmedoids_geodesic_analysis.py) on the
MI355X: csrc/analysis.hip reduces the n-sized inputs on the device, the host only sees K-, C- and K x K-sized results.

    clustering_scores(assign, labels, K)      purity / NMI / ARI / perplexity / code usage counts
    distance_feature_pca(D, n_components)     PCA of X = D^T with the demo's replacement of non-finite distances

Definitions: compute_purity and compute_perplexity of the demo; scikit-learn's normalized_mutual_info_score (arithmetic mean
of the two entropies, 1.0 when both labellings have a single value, 0.0 when the mutual information is 0) and
adjusted_rand_score (pair-confusion counts as Python integers, 1.0 when fp = fn = 0); PCA(n_components) with scikit-learn's
sign rule (svd_flip, u_based_decision=False: the entry of largest magnitude of every component is positive).
"""
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._device import ptr, stream_ptr, workspace

MAX_K, MAX_C = 4096, 1024


# ---- host formulas over the K- and C-sized sums ------------------------------------------------------------------------------
def _xlogx_sum(v: np.ndarray) -> float:
    v = np.asarray(v, dtype=np.float64)
    v = v[v > 1]
    return float(np.sum(v * np.log(v)))


def _pairs(v) -> int:
    return sum(int(x) * (int(x) - 1) // 2 for x in np.asarray(v).ravel())


def perplexity_from_counts(counts: np.ndarray) -> float:
    """compute_perplexity of the demo on the code usage counts (0.0 without any assigned row)."""
    counts = np.asarray(counts).astype(np.float64)
    if counts.sum() == 0:
        return 0.0
    probs = counts / counts.sum()
    nz = probs[probs > 0]
    return float(np.exp(-np.sum(nz * np.log(nz + 1e-12))))


def scores_from_sums(n: int, n_total: int, purity_num: int, row_counts: np.ndarray, col_counts: np.ndarray,
                     pairs_kc: int, pairs_k: int, pairs_c: int, s_kc: float, s_k: float, s_c: float) -> Dict[str, float]:
    """purity, nmi, ari, perplexity from what geo_cluster_label_scores returns.  n = rows counted, n_total = len(assign)
    (the demo's purity divides by it); s_* = sum x log x over the table, the row sums, the column sums."""
    n, purity_num, pairs_kc, pairs_k, pairs_c = int(n), int(purity_num), int(pairs_kc), int(pairs_k), int(pairs_c)
    n_clusters = int(np.count_nonzero(row_counts))
    n_classes = int(np.count_nonzero(col_counts))
    purity = float(purity_num / n_total) if n_total > 0 else float("nan")
    # normalized_mutual_info_score
    if n_classes == n_clusters == 1 or n_classes == n_clusters == 0:
        nmi = 1.0
    elif n_classes == 1 or n_clusters == 1:
        nmi = 0.0                                         # mutual_info_score returns 0.0 for a single class or cluster
    else:
        log_n = math.log(n)
        mi = max((s_kc - s_k - s_c) / n + log_n, 0.0)
        nmi = 0.0 if mi == 0 else float(mi / np.mean([log_n - s_c / n, log_n - s_k / n]))
    # adjusted_rand_score: ordered pairs, exact integers
    tp = 2 * pairs_kc
    fp, fn = 2 * (pairs_k - pairs_kc), 2 * (pairs_c - pairs_kc)
    tn = n * (n - 1) - tp - fp - fn
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return {"purity": purity, "nmi": float(nmi), "ari": float(ari), "perplexity": perplexity_from_counts(row_counts)}


def scores_from_contingency(table: np.ndarray, n_total: Optional[int] = None) -> Dict[str, float]:
    """The same scores from a K x C contingency table (integer counts) alone."""
    table = np.asarray(table, dtype=np.int64)
    rows, cols = table.sum(axis=1), table.sum(axis=0)
    n = int(table.sum())
    return scores_from_sums(n, n if n_total is None else n_total, int(table.max(axis=1).sum()) if table.size else 0, rows, cols,
                            _pairs(table), _pairs(rows), _pairs(cols), _xlogx_sum(table), _xlogx_sum(rows), _xlogx_sum(cols))


def svd_flip_rows(components: np.ndarray) -> np.ndarray:
    """scikit-learn's svd_flip(u_based_decision=False) on components [n_components][K]: every row's entry of largest magnitude
    (the first one on ties, np.argmax) becomes positive."""
    components = np.array(components, dtype=np.float64, copy=True)
    idx = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), idx])
    signs[signs == 0] = 1.0
    return components * signs[:, None]


# ---- device entry points ------------------------------------------------------------------------------------------------------
def _i32(t, dev=None) -> torch.Tensor:
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if dev is not None:
        t = t.to(dev)
    return t.to(torch.int32).contiguous()


def label_scores_device(assign, labels, K: int, C: Optional[int] = None, grid_blocks: int = 0) -> Dict[str, torch.Tensor]:
    """geo_cluster_label_scores on the current stream.  assign / labels: integer tensors on the GPU (host arrays are uploaded),
    C defaults to labels.max() + 1.  Returns the device outputs: table i64 [K][C], row_counts i64 [K], col_counts i64 [C],
    isums i64 [6], fsums f64 [3] (include/geo_hip.h)."""
    from .._device import device
    dev = assign.device if torch.is_tensor(assign) and assign.is_cuda else device()
    a, l = _i32(assign, dev), _i32(labels, dev)
    if a.numel() != l.numel():
        raise ValueError("assign and labels must have the same length")
    if C is None:
        C = int(l.max()) + 1 if l.numel() else 1
    out = {"table": torch.empty((K, C), dtype=torch.int64, device=dev), "row_counts": torch.empty(K, dtype=torch.int64, device=dev),
           "col_counts": torch.empty(C, dtype=torch.int64, device=dev), "isums": torch.empty(6, dtype=torch.int64, device=dev),
           "fsums": torch.empty(3, dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(_lib.load().geo_cluster_label_scores(ptr(a), ptr(l), a.numel(), int(K), int(C), int(grid_blocks),
                                                        ptr(out["table"]), ptr(out["row_counts"]), ptr(out["col_counts"]),
                                                        ptr(out["isums"]), ptr(out["fsums"]), stream_ptr()),
                   "geo_cluster_label_scores")
    return out


def clustering_scores(assign, labels, K: int, C: Optional[int] = None) -> dict:
    """purity, nmi, ari, perplexity (floats) and counts (code usage, int64 [K]) of the codes `assign` (values in [0, K),
    negative = not assigned) against the class labels.  Device tensors in; only K- and C-sized results reach the host."""
    out = label_scores_device(assign, labels, K, C)
    isums = out["isums"].cpu().numpy()
    if isums[5]:
        raise ValueError(f"{int(isums[5])} rows have a code >= K={K} or a label outside [0, {out['col_counts'].numel()})")
    fs = out["fsums"].cpu().numpy()
    counts = out["row_counts"].cpu().numpy()
    n_total = int(assign.numel() if torch.is_tensor(assign) else len(assign))
    res = scores_from_sums(int(isums[0]), n_total, int(isums[1]), counts, out["col_counts"].cpu().numpy(), int(isums[2]),
                           int(isums[3]), int(isums[4]), float(fs[0]), float(fs[1]), float(fs[2]))
    res["counts"] = counts
    return res


def feature_moments_device(D: torch.Tensor):
    """(colmax f32 [K], fill f32 [K], mean f64 [K], gram f64 [K][K]) of a device matrix D f32 [K][n]: geo_feature_colstats and
    geo_feature_gram."""
    if not (torch.is_tensor(D) and D.is_cuda and D.dtype == torch.float32 and D.dim() == 2 and D.stride(1) == 1):
        raise ValueError("D must be a float32 [K][n] tensor on the GPU with contiguous rows")
    lib = _lib.load()
    dev = D.device
    K, n = int(D.shape[0]), int(D.shape[1])
    if not (1 <= K <= MAX_K and n >= 1):
        raise ValueError(f"K={K} outside [1, {MAX_K}] or no columns")
    colmax = torch.empty(K, dtype=torch.float32, device=dev)
    fill = torch.empty(K, dtype=torch.float32, device=dev)
    mean = torch.empty(K, dtype=torch.float64, device=dev)
    gram = torch.empty((K, K), dtype=torch.float64, device=dev)
    ws = workspace(lib.geo_feature_workspace_bytes(n, K), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_feature_colstats(ptr(D), D.stride(0), K, n, ptr(colmax), ptr(fill), ptr(mean), ptr(ws), ws.numel(),
                                            stream_ptr()), "geo_feature_colstats")
        _lib.check(lib.geo_feature_gram(ptr(D), D.stride(0), K, n, ptr(fill), ptr(mean), ptr(gram), ptr(ws), ws.numel(),
                                        stream_ptr()), "geo_feature_gram")
    return colmax, fill, mean, gram


def distance_feature_pca(D: torch.Tensor, n_components: int = 2) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """PCA(n_components).fit_transform of the demo's features: X = D^T, non-finite entries of a medoid's column replaced by 1.1 x
    its largest finite value (1.0 where that is 0).  D f32 [K][n] on the GPU (what sssp_multi_device returns).  The K x K
    centred Gram matrix and the projection are computed on the device in fp64, the eigen-decomposition (numpy.linalg.eigh of
    the K x K matrix) on the host.  Returns (coords f32 [n][n_components], explained_variance f64 [n_components], components
    f64 [n_components][K])."""
    colmax, fill, mean, gram = feature_moments_device(D)
    K, n = int(D.shape[0]), int(D.shape[1])
    if not 1 <= n_components <= min(K, 8):
        raise ValueError(f"n_components={n_components} outside [1, min(K, 8)]")
    w, v = np.linalg.eigh(gram.cpu().numpy())
    order = np.argsort(w)[::-1][:n_components]
    components = svd_flip_rows(v[:, order].T)
    explained = np.maximum(w[order], 0.0) / max(n - 1, 1)
    V = torch.from_numpy(np.ascontiguousarray(components.T)).to(D.device)
    Z = torch.empty((n, n_components), dtype=torch.float32, device=D.device)
    with torch.cuda.device(D.device):
        _lib.check(_lib.load().geo_feature_project(ptr(D), D.stride(0), K, n, ptr(fill), ptr(mean), ptr(V), int(n_components),
                                                   ptr(Z), stream_ptr()), "geo_feature_project")
    return Z.cpu().numpy(), explained, components

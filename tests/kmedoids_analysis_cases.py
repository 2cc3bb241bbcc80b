"""Inputs and restated rules shared by tools/gen_golden_kmedoids_analysis.py and the k-medoids analysis tests: the fixture
stores seeds, graphs and results; latents and labels are regenerated here."""
import numpy as np
from scipy import sparse

K_VALUES = (32, 64, 128)
INITS = ("kpp", "random")
SEED = 42

# seeded Gaussian mixtures, the mixture component is the label.  "disc": far centres, the mutual kNN graph falls apart
# (most of the K x N matrix is inf); "conn": close centres and a union graph, one component.
CASES = {
    "disc": dict(n=1500, d=16, centres=10, spread=2.0, noise=0.7, k=10, sym="mutual"),
    "conn": dict(n=1500, d=16, centres=10, spread=0.6, noise=1.0, k=10, sym="union"),
}


def make_latents(case: str, seed: int):
    """(z float32 [n][d], y int64 [n])."""
    c = CASES[case]
    r = np.random.RandomState(seed)
    cen = c["spread"] * r.randn(c["centres"], c["d"])
    y = r.randint(0, c["centres"], c["n"])
    z = (cen[y] + c["noise"] * r.randn(c["n"], c["d"])).astype(np.float32)
    return z, y.astype(np.int64)


def pack_graph(W):
    """Upper triangle of a symmetric CSR graph as (rows u16, cols u16, weights f32)."""
    U = sparse.triu(W.tocsr(), k=1).tocoo()
    order = np.lexsort((U.col, U.row))
    return U.row[order].astype(np.uint16), U.col[order].astype(np.uint16), U.data[order].astype(np.float32)


def unpack_graph(rows, cols, w, n: int):
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    W = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([rows, cols]), np.concatenate([cols, rows]))),
                          shape=(n, n), dtype=np.float32).tocsr()
    W.sort_indices()
    return W


def replaced_features(D: np.ndarray) -> np.ndarray:
    """X = D^T (float32) with the non-finite entries of a column set to 1.1 x the column's largest finite value (1.0 where that
    is 0), in float32 arithmetic."""
    X = np.asarray(D, dtype=np.float32).T
    fin = np.isfinite(X)
    col_max = np.where(fin, X, -np.inf).max(axis=0).astype(np.float32)
    col_max[col_max == 0] = 1.0
    fill = (col_max * np.float32(1.1)).astype(np.float32)
    return np.where(fin, X, fill[None, :]).astype(np.float32)


def flip_rows(components: np.ndarray) -> np.ndarray:
    idx = np.argmax(np.abs(components), axis=1)
    s = np.sign(components[np.arange(len(components)), idx])
    s[s == 0] = 1.0
    return components * s[:, None]


def pca_fp64(X: np.ndarray, n_components: int = 2):
    """PCA in fp64 throughout: eigh of the centred covariance.  Returns coords, eigenvalues (all, descending), components,
    gap = min(l1 - l2, l2 - l3) / l1."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    w, v = np.linalg.eigh(Xc.T @ Xc / (len(X) - 1))
    w, v = w[::-1], v[:, ::-1]
    comps = flip_rows(v[:, :n_components].T)
    gap = min(w[0] - w[1], w[1] - w[2]) / w[0]
    return Xc @ comps.T, w, comps, float(gap)


def contingency(assign: np.ndarray, labels: np.ndarray, K: int, C: int) -> np.ndarray:
    t = np.zeros((K, C), dtype=np.int64)
    ok = assign >= 0
    np.add.at(t, (assign[ok], labels[ok]), 1)
    return t

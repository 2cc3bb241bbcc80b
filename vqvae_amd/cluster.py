"""Euclidean k-means on the MI355X: a drop-in for `sklearn.cluster.KMeans` (algorithm "lloyd", k-means++ seeding) and
`sklearn.cluster.kmeans_plusplus` -- the Euclidean side of the reference's codebook comparison
(demos/codebook_comparison.py:73-77).

Covered envelope (the HIP path, libgeo_hip.so geo_kmeans_*): dense float32 X of shape (N, d) with 1 <= d <= 128,
1 <= n_clusters <= min(N, 4096), finite values, sample_weight None, init "k-means++" or an array, a GPU present.  Any other
input goes to scikit-learn unchanged (`path_` records which ran).

What the HIP path computes:
  - labels: argmin over centres of the exact key, the fp64 fma chain of (x_c - c_jc)^2 over c ascending; ties to the lowest
    index.  Every row is decided by that key (a float32 matrix-core screen in front, with a proven margin);
  - seeding: sklearn's stream -- for each start rs.choice(n, p=w / w.sum()) with float32 unit weights, then
    rs.uniform(size=(K - 1, L)), L = 2 + int(log K); the draws, sums and minima of _kmeans_plusplus on the device with fp64
    sums in a fixed order;
  - Lloyd: sklearn's _kmeans_single_lloyd on X - X.mean(0) with fp64 per-cluster sums, empty-cluster relocation, strict / tol /
    max_iter stopping, a final relabel without strict convergence; inertia = fp64 sum of the keys;
  - the best start as KMeans.fit picks it: lower inertia wins unless the labelling is the same clustering.
On data whose outcome does not hinge on rounding this equals scikit-learn (tests/golden/kmeans.npz); at scale it follows the
stated rules, not sklearn's float32 BLAS trajectory (README "Parity").
"""
import ctypes
import numbers
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._device import ptr, stream_ptr

MAX_D = 128
MAX_K = 4096

_last_path = None


def last_path() -> Optional[str]:
    """"hip" or "sklearn": which implementation the last fit / predict / kmeans_plusplus call of this module ran."""
    return _last_path


def _set_path(p: str) -> None:
    global _last_path
    _last_path = p


def check_random_state(seed):
    """sklearn.utils.check_random_state."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def n_local_trials_for(n_clusters: int) -> int:
    return 2 + int(np.log(n_clusters))


def seeding_draws(rs: np.random.RandomState, n: int, n_clusters: int, n_starts: int, n_local_trials: int):
    """The random draws of `n_starts` consecutive k-means++ seedings, in sklearn's order: per start the first centre
    (rs.choice with float32 unit weights) and then (K - 1) x L uniforms.  Lloyd draws nothing, so the draws of all starts
    can be taken before any of them runs."""
    w = np.ones(n, dtype=np.float32)
    first = np.empty(n_starts, dtype=np.int32)
    u = np.empty((n_starts, max(n_clusters - 1, 1), n_local_trials), dtype=np.float64)
    for s in range(n_starts):
        first[s] = rs.choice(n, p=w / w.sum())
        for c in range(1, n_clusters):
            u[s, c - 1] = rs.uniform(size=n_local_trials)
    return first, u


def _tolerance(X: np.ndarray, tol: float):
    """sklearn.cluster._kmeans._tolerance for dense X (numpy arithmetic kept as is)."""
    if tol == 0:
        return 0
    return np.mean(np.var(X, axis=0)) * tol


def _is_same_clustering(labels1: np.ndarray, labels2: np.ndarray, n_clusters: int) -> bool:
    """sklearn's _is_same_clustering: equal up to a permutation of the labels (labels1 -> labels2 is a function)."""
    mapping = np.full(n_clusters, -1, dtype=np.int64)
    mapping[labels1] = labels2
    return bool(np.array_equal(mapping[labels1], labels2))


def _sklearn():
    try:
        import sklearn.cluster
    except ImportError as e:   # pragma: no cover - depends on the environment
        raise ImportError("this input is outside the GPU k-means envelope and needs scikit-learn") from e
    return sklearn.cluster


def in_envelope(X, n_clusters, sample_weight=None) -> bool:
    """True when the HIP path covers this input (module docstring)."""
    if sample_weight is not None or not isinstance(X, np.ndarray) or X.dtype != np.float32 or X.ndim != 2:
        return False
    n, d = X.shape
    if not (1 <= d <= MAX_D) or not isinstance(n_clusters, numbers.Integral) or not (1 <= n_clusters <= min(n, MAX_K)):
        return False
    if not torch.cuda.is_available():
        return False
    return bool(np.isfinite(X).all())


def _as_input(X):
    """numpy view of X for the envelope test: torch tensors and ndarrays pass through, anything else is left alone."""
    if isinstance(X, torch.Tensor):
        return X.detach().cpu().numpy()
    return X


def _dev():
    from ._device import device
    return device()


def _workspace(dev, n, d, K, S=1, L=1):
    nbytes = _lib.load().geo_kmeans_workspace_bytes(n, d, K, S, L)
    if nbytes == 0:
        raise _lib.GeoHipError(f"geo_kmeans_workspace_bytes rejected n={n} d={d} K={K} starts={S} trials={L}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def assign(X: torch.Tensor, C: torch.Tensor):
    """Exact labels of the rows of X (device f32 [n][d]) against centres C (device f32 [K][d]).
    Returns (labels i32 [n], keys f64 [n], number of rows the screen left to the exact fallback)."""
    n, d = X.shape
    K = C.shape[0]
    X, C = X.contiguous(), C.contiguous()
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    keys = torch.empty(n, dtype=torch.float64, device=X.device)
    ws = _workspace(X.device, n, d, K)
    nfb = ctypes.c_int64(0)
    L = _lib.load()
    _lib.check(L.geo_kmeans_assign(ptr(X), n, d, ptr(C), K, ptr(labels), ptr(keys), ctypes.byref(nfb), ptr(ws), ws.numel(),
                                   stream_ptr()), "geo_kmeans_assign")
    return labels, keys, int(nfb.value)


def plusplus_device(Xd: torch.Tensor, n_clusters: int, first: np.ndarray, u: np.ndarray):
    """k-means++ of len(first) starts on the device: (centres f32 [S][K][d], indices i32 [S][K]), both on the device."""
    n, d = Xd.shape
    S, L = len(first), u.shape[2]
    idx = torch.empty((S, n_clusters), dtype=torch.int32, device=Xd.device)
    centers = torch.empty((S, n_clusters, d), dtype=torch.float32, device=Xd.device)
    ws = _workspace(Xd.device, n, d, n_clusters, S, L)
    first = np.ascontiguousarray(first, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64)
    lib = _lib.load()
    _lib.check(lib.geo_kmeans_pp(ptr(Xd), n, d, n_clusters, S, L, first.ctypes.data_as(ctypes.c_void_p),
                                 u.ctypes.data_as(ctypes.c_void_p), ptr(idx), ptr(centers), ptr(ws), ws.numel(), stream_ptr()),
               "geo_kmeans_pp")
    return centers, idx


def lloyd_device(Xd: torch.Tensor, init: torch.Tensor, max_iter: int, tol: float):
    """Lloyd from each of init's starts (device f32 [S][K][d]).  Returns a dict of device centres [S][K][d], labels [S][n],
    and host inertia f64 [S], n_iter i32 [S], strict i32 [S], n_fallback."""
    n, d = Xd.shape
    S, K = init.shape[0], init.shape[1]
    init = init.contiguous()
    centers = torch.empty((S, K, d), dtype=torch.float32, device=Xd.device)
    labels = torch.empty((S, n), dtype=torch.int32, device=Xd.device)
    inertia = np.zeros(S, dtype=np.float64)
    n_iter = np.zeros(S, dtype=np.int32)
    strict = np.zeros(S, dtype=np.int32)
    nfb = ctypes.c_int64(0)
    ws = _workspace(Xd.device, n, d, K)
    lib = _lib.load()
    _lib.check(lib.geo_kmeans_lloyd(ptr(Xd), n, d, K, S, ptr(init), int(max_iter), float(tol), ptr(centers), ptr(labels),
                                    inertia.ctypes.data_as(ctypes.c_void_p), n_iter.ctypes.data_as(ctypes.c_void_p),
                                    strict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nfb), ptr(ws), ws.numel(),
                                    stream_ptr()), "geo_kmeans_lloyd")
    return {"centers": centers, "labels": labels, "inertia": inertia, "n_iter": n_iter, "strict": strict,
            "n_fallback": int(nfb.value)}


def kmeans_plusplus(X, n_clusters, *, sample_weight=None, x_squared_norms=None, random_state=None, n_local_trials=None):
    """sklearn.cluster.kmeans_plusplus: (centers, indices); no centring, like sklearn's public function."""
    Xn = _as_input(X)
    L = n_local_trials_for(n_clusters) if n_local_trials is None and isinstance(n_clusters, numbers.Integral) and n_clusters > 0 \
        else n_local_trials
    if not in_envelope(Xn, n_clusters, sample_weight) or not isinstance(L, numbers.Integral) or not 1 <= L <= 64:
        _set_path("sklearn")
        return _sklearn().kmeans_plusplus(X, n_clusters, sample_weight=sample_weight, x_squared_norms=x_squared_norms,
                                          random_state=random_state, n_local_trials=n_local_trials)
    rs = check_random_state(random_state)
    n = Xn.shape[0]
    first, u = seeding_draws(rs, n, n_clusters, 1, L)
    Xd = torch.from_numpy(np.ascontiguousarray(Xn)).to(_dev())
    centers, idx = plusplus_device(Xd, n_clusters, first, u)
    _set_path("hip")
    return centers[0].cpu().numpy(), idx[0].cpu().numpy().astype(np.int64)


class KMeans:
    """sklearn.cluster.KMeans (subset: n_clusters, init, n_init, max_iter, tol, random_state), lloyd on the MI355X.

    Attributes after fit: cluster_centers_ (f32 [K][d]), labels_ (int32 [N]), inertia_ (float), n_iter_ (int),
    n_features_in_, path_ ("hip" or "sklearn"); on the HIP path also n_fallback_rows_ (rows the screen left to the exact
    key, over every assignment of every start), best_start_ (index of the start kept) and centered_centers_ (the centres in
    the frame the fit ran in, X - X.mean(0): labels_ is the exact argmin against them)."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state

    # -- sklearn's parameter handling (KMeans._check_params_vs_input) -------------------------------------------------
    def _resolve_n_init(self, init_is_array: bool) -> int:
        if self.n_init == "auto":
            n_init = 1 if (self.init == "k-means++" or init_is_array) else 10
        else:
            n_init = int(self.n_init)
        if init_is_array and n_init != 1:
            warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of "
                          f"n_init={n_init}.", RuntimeWarning, stacklevel=3)
            n_init = 1
        return n_init

    def _covered(self, Xn, sample_weight) -> bool:
        init_is_array = not isinstance(self.init, str) and not callable(self.init)
        if not init_is_array and self.init != "k-means++":
            return False
        if not (isinstance(self.max_iter, numbers.Integral) and self.max_iter >= 1):
            return False
        if not (isinstance(self.tol, numbers.Real) and self.tol >= 0):
            return False
        if not (self.n_init == "auto" or (isinstance(self.n_init, numbers.Integral) and self.n_init >= 1)):
            return False
        if not in_envelope(Xn, self.n_clusters, sample_weight):
            return False
        if init_is_array:
            a = np.asarray(self.init)
            if a.shape != (self.n_clusters, Xn.shape[1]) or not np.isfinite(a).all():
                return False
        return True

    def _fit_sklearn(self, X, sample_weight):
        km = _sklearn().KMeans(n_clusters=self.n_clusters, init=self.init, n_init=self.n_init, max_iter=self.max_iter,
                               tol=self.tol, random_state=self.random_state)
        km.fit(X, sample_weight=sample_weight)
        self._sk = km
        self.cluster_centers_ = km.cluster_centers_
        self.labels_ = km.labels_
        self.inertia_ = km.inertia_
        self.n_iter_ = km.n_iter_
        self.n_features_in_ = km.n_features_in_
        self.path_ = "sklearn"
        _set_path("sklearn")
        return self

    def fit(self, X, y=None, sample_weight=None):
        Xn = _as_input(X)
        if not self._covered(Xn, sample_weight):
            return self._fit_sklearn(X, sample_weight)
        self._sk = None
        n, d = Xn.shape
        K = int(self.n_clusters)
        init_is_array = not isinstance(self.init, str)
        n_init = self._resolve_n_init(init_is_array)
        rs = check_random_state(self.random_state)
        tol = _tolerance(Xn, self.tol)
        X_mean = Xn.mean(axis=0)
        dev = _dev()
        Xd = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
        Xc = (Xd - torch.from_numpy(X_mean).to(dev)).contiguous()     # float32 X - X_mean, as sklearn centres in place
        if init_is_array:
            init = np.array(self.init, dtype=np.float32, copy=True) - X_mean
            init_d = torch.from_numpy(np.ascontiguousarray(init)).to(dev)[None]
        else:
            L = n_local_trials_for(K)
            first, u = seeding_draws(rs, n, K, n_init, L)
            init_d, _ = plusplus_device(Xc, K, first, u)
        res = lloyd_device(Xc, init_d, self.max_iter, float(tol))
        labels = res["labels"].cpu().numpy()
        best = None
        for s in range(n_init):
            inertia = float(res["inertia"][s])
            if best is None or (inertia < float(res["inertia"][best]) and
                                not _is_same_clustering(labels[s], labels[best], K)):
                best = s
        self.centered_centers_ = res["centers"][best].cpu().numpy()
        centers = self.centered_centers_ + X_mean
        self.cluster_centers_ = centers.astype(np.float32, copy=False)
        self.labels_ = labels[best].astype(np.int32, copy=True)
        self.inertia_ = float(res["inertia"][best])
        self.n_iter_ = int(res["n_iter"][best])
        self.n_features_in_ = d
        self.best_start_ = best
        self.n_fallback_rows_ = res["n_fallback"]
        self.path_ = "hip"
        _set_path("hip")
        distinct = len(np.unique(self.labels_))
        if distinct < K:
            warnings.warn(f"Number of distinct clusters ({distinct}) found smaller than n_clusters ({K}). Possibly due to "
                          "duplicate points in X.", RuntimeWarning, stacklevel=2)
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_

    def predict(self, X):
        """Exact-key labels of X against cluster_centers_ (no centring, as sklearn's predict)."""
        if not hasattr(self, "cluster_centers_"):
            raise ValueError("This KMeans instance is not fitted yet. Call 'fit' first.")
        Xn = _as_input(X)
        covered = (isinstance(Xn, np.ndarray) and Xn.dtype == np.float32 and Xn.ndim == 2
                   and Xn.shape[0] >= 1 and Xn.shape[1] == self.n_features_in_ and bool(np.isfinite(Xn).all()))
        if getattr(self, "_sk", None) is not None or not covered:
            if getattr(self, "_sk", None) is None:
                raise ValueError("predict: X is outside the GPU envelope of a model fitted on the GPU "
                                 f"(need float32 [N][{self.n_features_in_}], finite, N >= 1)")
            _set_path("sklearn")
            return self._sk.predict(X)
        dev = _dev()
        Xd = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
        C = torch.from_numpy(np.ascontiguousarray(self.cluster_centers_, dtype=np.float32)).to(dev)
        labels, keys, nfb = assign(Xd, C)
        self.last_predict_fallback_rows_ = nfb
        _set_path("hip")
        return labels.cpu().numpy()

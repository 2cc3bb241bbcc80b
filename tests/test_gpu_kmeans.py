"""GPU k-means (vqvae_amd.cluster, csrc/kmeans.hip) against scikit-learn's fixture, near ties, and an every-row checker.

The checker uses no project code: labels are screened with torch fp64 distances and rows whose two best keys lie within
1e-12 (relative) of each other are re-keyed with the exact fma chain in kmeans_rules.fma_key_rows.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kmeans_rules as R  # noqa: E402
from gen_golden_kmeans import far_init, make_input  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans")


def _cluster():
    from vqvae_amd import cluster
    return cluster


def _pp_tags(fx):
    return sorted({k[:-5] for k in fx.files if k.startswith("pp_") and k.endswith("_meta")})


def test_fixture_seeding_indices(fx):
    cl = _cluster()
    tags = _pp_tags(fx)
    assert len(tags) == 9
    for tag in tags:
        n, d, K, seed = (int(v) for v in fx[tag + "_meta"])
        X = make_input("blobs", n, d, seed)
        centers, idx = cl.kmeans_plusplus(X, K, random_state=seed)
        assert cl.last_path() == "hip", tag
        np.testing.assert_array_equal(idx, fx[tag + "_indices"], err_msg=tag)
        np.testing.assert_array_equal(centers, X[idx], err_msg=tag)


@pytest.mark.parametrize("name", ["strict", "tol", "maxiter", "relocate"])
def test_fixture_lloyd_from_init(fx, name):
    cl = _cluster()
    tag = f"lloyd_{name}"
    n, d, K, seed, max_iter = (int(v) for v in fx[tag + "_meta"])
    kind = str(fx[tag + "_kind"])
    X = make_input(kind, n, d, seed)
    init = far_init(X, K, seed) if name == "relocate" else X[np.random.RandomState(seed).choice(n, K, replace=False)].copy()
    km = cl.KMeans(K, init=init, n_init=1, max_iter=max_iter, tol=float(fx[tag + "_tol"])).fit(X)
    assert km.path_ == "hip"
    np.testing.assert_array_equal(km.labels_, fx[tag + "_labels"])
    assert km.labels_.dtype == np.int32
    assert km.n_iter_ == int(fx[tag + "_n_iter"])
    np.testing.assert_allclose(km.cluster_centers_, fx[tag + "_centers"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(km.inertia_, float(fx[tag + "_inertia"]), rtol=1e-5)


@pytest.mark.parametrize("name", ["full", "dups"])
def test_fixture_full_fit(fx, name):
    cl = _cluster()
    tag = f"fit_{name}"
    n, d, K, seed, n_init = (int(v) for v in fx[tag + "_meta"])
    X = make_input(str(fx[tag + "_kind"]), n, d, seed)
    with pytest.warns(RuntimeWarning) if name == "dups" else _nullcontext():
        km = cl.KMeans(K, random_state=seed, n_init=n_init).fit(X)
    assert km.path_ == "hip"
    np.testing.assert_array_equal(km.labels_, fx[tag + "_labels"])
    assert km.n_iter_ == int(fx[tag + "_n_iter"])
    assert km.best_start_ == int(fx[tag + "_best_start"])
    np.testing.assert_allclose(km.cluster_centers_, fx[tag + "_centers"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(km.inertia_, float(fx[tag + "_inertia"]), rtol=1e-5)
    np.testing.assert_array_equal(km.fit_predict(X), km.labels_)
    np.testing.assert_array_equal(km.predict(X), km.labels_)


class _nullcontext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _exact_labels_small(X, C):
    """Exact-key argmin with every key from the exact fma chain (small inputs only)."""
    keys = np.stack([R.fma_key_rows(x, C) for x in X])
    return keys.argmin(1), keys


def test_near_ties_fit_labels_are_exact_argmin():
    """Integer data (mean exactly 0, so the centred frame is the input's): integer distances tie all over, and duplicate
    initial centres.  Every label of fit must be the exact argmin with ties to the lowest index."""
    cl = _cluster()
    r = np.random.RandomState(5)
    half = r.randint(-3, 4, size=(96, 6)).astype(np.float32)
    X = np.concatenate([half, -half])
    assert (X.mean(axis=0) == 0).all()
    init = X[[0, 1, 2, 3, 3, 4, 5, 6]].copy()                    # a duplicate centre
    km = cl.KMeans(8, init=init, n_init=1, max_iter=1).fit(X)     # one step: the relabel runs with final centres
    assert km.path_ == "hip"
    lab, _ = _exact_labels_small(X, km.cluster_centers_)
    np.testing.assert_array_equal(km.labels_, lab)
    assert km.n_fallback_rows_ > 0
    np.testing.assert_array_equal(km.predict(X), lab)


def test_near_ties_predict_midpoints_duplicates_offset():
    """Rows exactly between two centres, duplicate centres, and a 1e3 offset that wrecks |c|^2 - 2 x.c in float32."""
    cl = _cluster()
    d, K = 16, 8
    r = np.random.RandomState(11)
    C = (r.randint(-8, 9, size=(K, d)) * 0.25).astype(np.float32)
    C[5] = C[2]                                                   # duplicate centres: ties must go to 2
    mids = ((C[0].astype(np.float64) + C[1]) / 2).astype(np.float32)[None]   # exact: quarter-integers
    mid2 = ((C[2].astype(np.float64) + C[3]) / 2).astype(np.float32)[None]
    X = np.concatenate([mids, mid2, C, C + np.float32(0.25), (r.randint(-8, 9, size=(200, d)) * 0.25).astype(np.float32)])
    fit_on = (r.randn(64, d)).astype(np.float32)
    for offset in (0.0, 1e3):
        km = cl.KMeans(K, random_state=0, n_init=1).fit(fit_on)
        km.cluster_centers_ = (C + np.float32(offset)).astype(np.float32)
        Xo = (X + np.float32(offset)).astype(np.float32)
        got = km.predict(Xo)
        assert cl.last_path() == "hip"
        lab, keys = _exact_labels_small(Xo, km.cluster_centers_)
        np.testing.assert_array_equal(got, lab, err_msg=f"offset {offset}")
        assert km.last_predict_fallback_rows_ > 0
        assert not (got == 5).any()                               # the duplicate of centre 2 never wins
    # at 1e3 the float32 expansion cannot separate anything: the screen hands most rows to the exact key
    assert km.last_predict_fallback_rows_ > len(X) // 2


# ---------------------------------------------------------------------------------------------------------------------
# every-row checker
# ---------------------------------------------------------------------------------------------------------------------
def check_labels_exact(Xc: np.ndarray, C: np.ndarray, labels: np.ndarray, rel=1e-12):
    """Every label is the exact-key argmin (ties lowest).  Returns (exact keys of the labels, rows re-keyed exactly)."""
    dev = torch.device("cuda", 0)
    Ct = torch.from_numpy(C).to(dev, torch.float64)
    cn = (Ct * Ct).sum(1)
    keys = np.empty(len(Xc))
    rekeyed = 0
    for a in range(0, len(Xc), 65536):
        xb = torch.from_numpy(Xc[a:a + 65536]).to(dev, torch.float64)
        D = ((xb * xb).sum(1, keepdim=True) + cn[None] - 2.0 * xb @ Ct.T).clamp_min(0)
        lab = torch.from_numpy(labels[a:a + 65536].astype(np.int64)).to(dev)
        dl = D.gather(1, lab[:, None])[:, 0]
        dmin = D.min(1).values
        scale = (xb * xb).sum(1) + cn.max()
        # the fp64 expansion is within ~(d + 2) 2^-53 scale of the key: anything beyond 1e-12 scale is a real difference
        tol = 1e-12 * scale
        bad = (dl > dmin + tol).nonzero()[:, 0].cpu().numpy()
        assert len(bad) == 0, f"rows {a + bad[:5]} are not labelled with their nearest centre"
        near = ((D <= (dmin + tol)[:, None]).sum(1) > 1).nonzero()[:, 0].cpu().numpy()
        keys[a:a + len(xb)] = _keys_of_labels(Xc[a:a + 65536], C, labels[a:a + 65536])
        for i in near:
            x = Xc[a + i]
            band = (D[i] <= dmin[i] + tol[i]).nonzero()[:, 0].cpu().numpy()
            kk = R.fma_key_rows(x, C[band])
            want = band[np.nonzero(kk == kk.min())[0][0]]
            assert labels[a + i] == want, f"row {a + i}: label {labels[a + i]}, exact argmin {want}"
            rekeyed += 1
    return keys, rekeyed


def _keys_of_labels(X, C, labels):
    X64, Cl = X.astype(np.float64), C[labels].astype(np.float64)
    acc = np.zeros(len(X))
    for k in range(X.shape[1]):
        t = X64[:, k] - Cl[:, k]
        acc += t * t
    return acc


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _blobs(n, d, k, seed):
    r = np.random.RandomState(seed)
    cen = r.randn(k, d) * 4
    return (cen[r.randint(0, k, n)] + r.randn(n, d)).astype(np.float32)


@pytest.mark.parametrize("n,d,K,n_init", [(60_000, 16, 512, 10), (200_000, 128, 256, 1), (960_000, 16, 512, 1)])
def test_every_row_checker(n, d, K, n_init):
    cl = _cluster()
    X = _blobs(n, d, 40, n + d)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        km = cl.KMeans(K, random_state=0, n_init=n_init).fit(X)
    assert km.path_ == "hip"
    Xc = X - X.mean(axis=0)
    Cc = km.centered_centers_
    # labels: exact argmin against the final centres of the centred frame
    keys, rekeyed = check_labels_exact(Xc, Cc, km.labels_)
    # inertia: fp64 sum of the keys
    np.testing.assert_allclose(km.inertia_, keys.sum(), rtol=1e-12)
    # centres: one more Lloyd step from the final centres gives, for every cluster not touched by a relocation, the float32
    # rounding of the fp64 mean of its rows (within 1 ulp)
    dev = torch.device("cuda", 0)
    res = cl.lloyd_device(torch.from_numpy(Xc).to(dev), torch.from_numpy(Cc).to(dev)[None], 1, 0.0)
    C1 = res["centers"][0].cpu().numpy()
    counts = np.bincount(km.labels_, minlength=K)
    sums = np.zeros((K, d))
    np.add.at(sums, km.labels_, Xc.astype(np.float64))
    ok = counts > 0
    if (counts == 0).any():                     # relocation moved rows: leave out the clusters it touched
        ok &= ~np.isin(np.arange(K), km.labels_[np.argsort(-keys, kind="stable")[:(counts == 0).sum()]])
    mean = (sums[ok] / counts[ok][:, None]).astype(np.float32)
    assert ulp_diff(C1[ok], mean).max() <= 1
    # determinism: another stream, same bits
    with torch.cuda.stream(s2):
        km2 = cl.KMeans(K, random_state=0, n_init=n_init).fit(X)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(km.labels_, km2.labels_)
    assert km.cluster_centers_.tobytes() == km2.cluster_centers_.tobytes()
    assert km.inertia_ == km2.inertia_ and km.n_iter_ == km2.n_iter_
    print(f"n={n} d={d} K={K}: n_iter {km.n_iter_}, fallback rows {km.n_fallback_rows_}, checker re-keyed {rekeyed}")


def test_assign_bit_identical_across_workspace_sizes():
    cl = _cluster()
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    dev = torch.device("cuda", 0)
    X = torch.from_numpy(_blobs(20_000, 24, 30, 3)).to(dev)
    C = X[:300].clone()
    lab1, key1, _ = cl.assign(X, C)
    L = _lib.load()
    nb = L.geo_kmeans_workspace_bytes(X.shape[0], 24, 300, 1, 1)
    ws = torch.zeros(nb + (1 << 20), dtype=torch.uint8, device=dev)
    lab2 = torch.empty_like(lab1)
    key2 = torch.empty_like(key1)
    _lib.check(L.geo_kmeans_assign(ptr(X), X.shape[0], 24, ptr(C), 300, ptr(lab2), ptr(key2), None, ptr(ws), ws.numel(),
                                   stream_ptr()), "assign")
    torch.cuda.synchronize()
    assert torch.equal(lab1, lab2) and torch.equal(key1, key2)
    np.testing.assert_array_equal(lab1[:300].cpu().numpy(), np.arange(300))   # each centre row is its own nearest
    assert L.geo_kmeans_workspace_bytes(X.shape[0], 129, 300, 1, 1) == 0


def test_path_record():
    sklearn = pytest.importorskip("sklearn")  # noqa: F841
    cl = _cluster()
    X = _blobs(2000, 8, 10, 1)
    assert cl.KMeans(10, random_state=0, n_init=1).fit(X).path_ == "hip"
    assert cl.last_path() == "hip"
    assert cl.KMeans(10, random_state=0, n_init=1).fit(X.astype(np.float64)).path_ == "sklearn"
    assert cl.KMeans(10, random_state=0, n_init=1).fit(X, sample_weight=np.ones(len(X))).path_ == "sklearn"
    assert cl.KMeans(10, init="random", random_state=0, n_init=1).fit(X).path_ == "sklearn"
    assert cl.KMeans(4, random_state=0, n_init=1).fit(_blobs(100, 130, 4, 2)).path_ == "sklearn"
    cl.kmeans_plusplus(X, 10, random_state=0)
    assert cl.last_path() == "hip"
    cl.kmeans_plusplus(X.astype(np.float64), 10, random_state=0)
    assert cl.last_path() == "sklearn"

"""The update half of the GPU k-means and its seeding on the routes tests/golden/kmeans.npz never takes, against
tests/golden/kmeans_edges.npz (scikit-learn's results and those of the numpy rules, tools/gen_golden_kmeans_edges.py):
several relocations in one iteration (two rows from one donor, equal keys, keys of 0), a donor left empty below and above the
biggest cluster, d = 1, 2, 3, 17, 100, 127, K = 1025 and 4096, and the assignment at the wave, block and chunk edges of n;
seeding with n above 2^20, 20 and 64 local trials, n around one segment, K = n, and three starts in one call.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_kmeans_edges as G  # noqa: E402
from test_gpu_kmeans import check_labels_exact, ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans_edges")


def _cluster():
    from vqvae_amd import cluster
    return cluster


# ---------------------------------------------------------------------------------------------------------------------
# Lloyd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.LLOYD_CASES))
def test_lloyd_case(fx, name):
    cl = _cluster()
    tag = f"lloyd_{name}"
    n, d, K, seed, max_iter = (int(v) for v in fx[tag + "_meta"])
    X, init, max_iter, tol = G.lloyd_case(name, seed)
    assert X.shape == (n, d) and init.shape == (K, d)
    km = cl.KMeans(K, init=init, n_init=1, max_iter=max_iter, tol=tol).fit(X)
    assert km.path_ == "hip"
    np.testing.assert_array_equal(km.labels_, fx[tag + "_labels"].astype(np.int32))
    assert km.n_iter_ == int(fx[tag + "_n_iter"])
    # scikit-learn (float32)
    np.testing.assert_allclose(km.cluster_centers_, fx[tag + "_centers"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(km.inertia_, float(fx[tag + "_inertia"]), rtol=1e-5)
    # the rules, in the centred frame: every centre, those a relocation touched included
    Xc = X - X.mean(axis=0)
    Cc = km.centered_centers_
    worst = int(ulp_diff(Cc, fx[tag + "_rules_centers"]).max())
    keys, rekeyed = check_labels_exact(Xc, Cc, km.labels_)
    print(f"{name}: n_iter {km.n_iter_}, centres within {worst} ulp of the rules, inertia {km.inertia_!r} against "
          f"{keys.sum()!r}, checker re-keyed {rekeyed}")
    assert worst <= 1
    np.testing.assert_allclose(km.inertia_, keys.sum(), rtol=1e-12)


@pytest.mark.parametrize("name", G.TIE_CASES)
def test_relocation_ties_follow_the_rules(fx, name):
    """(key descending, row ascending) where scikit-learn's pick is arbitrary: one step on integer data, used as it is."""
    cl = _cluster()
    tag = f"lloyd_{name}"
    assert int(fx[tag + "_rules_only"]) == 1
    X, init = G.tie_case(name)
    dev = torch.device("cuda", 0)
    res = cl.lloyd_device(torch.from_numpy(X).to(dev), torch.from_numpy(init).to(dev)[None], 1, 0.0)
    C = res["centers"][0].cpu().numpy()
    want = fx[tag + "_rules_centers"]
    diff = ulp_diff(C, want)
    print(f"{name}: moved {fx[tag + '_moved'].tolist()}, clusters off by more than 1 ulp: {np.nonzero((diff > 1).any(1))[0]}")
    assert int(res["n_iter"][0]) == int(fx[tag + "_n_iter"]) == 1
    assert diff.max() <= 1
    np.testing.assert_array_equal(res["labels"][0].cpu().numpy(), fx[tag + "_labels"].astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# assignment at the edges of n, for d and K off the tile sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(1, 1), (2, 31), (3, 33), (17, 32), (100, 5), (127, 64)])
def test_assign_edges(d, K):
    cl = _cluster()
    dev = torch.device("cuda", 0)
    r = np.random.RandomState(1000 * d + K)
    C = (r.randn(K, d) * 3).astype(np.float32)
    if K > 1:
        C[K - 1] = C[0]                                  # duplicate centres: the lowest index wins
    if K > 3:
        C[K // 2] = C[1]
    first = np.array([np.nonzero((C == C[j]).all(1))[0][0] for j in range(K)])
    Cd = torch.from_numpy(C).to(dev)
    for n in (1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025):
        X = (r.randn(n, d) * 3).astype(np.float32)
        labels, keys, _ = cl.assign(torch.from_numpy(X).to(dev), Cd)
        want_keys, _ = check_labels_exact(X, C, labels.cpu().numpy())
        np.testing.assert_allclose(keys.cpu().numpy(), want_keys, rtol=1e-12, atol=0, err_msg=f"n={n}")
        # each centre row appended to X is labelled with the lowest index of its duplicates
        X2 = np.concatenate([X, C])
        lab2 = cl.assign(torch.from_numpy(X2).to(dev), Cd)[0].cpu().numpy()
        check_labels_exact(X2, C, lab2)
        np.testing.assert_array_equal(lab2[:n], labels.cpu().numpy(), err_msg=f"n={n}")
        np.testing.assert_array_equal(lab2[n:], first, err_msg=f"n={n}")


# ---------------------------------------------------------------------------------------------------------------------
# seeding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, v in G.PP_CASES.items() if v[4] == 1])
def test_seeding_case(fx, name):
    cl = _cluster()
    n, d, K, seed, L, S = (int(v) for v in fx[name + "_meta"])
    X, K, L, S = G.pp_input(name, seed)
    want = fx[name + "_indices"][0]
    centers, idx = cl.kmeans_plusplus(X, K, random_state=seed, n_local_trials=G.PP_CASES[name][3])
    assert cl.last_path() == "hip"
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(centers, X[idx])
    first, u = cl.seeding_draws(np.random.RandomState(seed), n, K, 1, L)
    Xd = torch.from_numpy(X).to(torch.device("cuda", 0))
    cd, id_ = cl.plusplus_device(Xd, K, first, u)
    np.testing.assert_array_equal(id_[0].cpu().numpy(), want)
    np.testing.assert_array_equal(cd[0].cpu().numpy(), X[want])


def test_seeding_several_starts_equal_each_start_alone(fx):
    cl = _cluster()
    name = "pp_multistart"
    n, d, K, seed, L, S = (int(v) for v in fx[name + "_meta"])
    X, K, L, S = G.pp_input(name, seed)
    assert S == 3
    want = fx[name + "_indices"]
    first, u = cl.seeding_draws(np.random.RandomState(seed), n, K, S, L)
    Xd = torch.from_numpy(X).to(torch.device("cuda", 0))
    cd, id_ = cl.plusplus_device(Xd, K, first, u)
    together = id_.cpu().numpy()
    np.testing.assert_array_equal(together, want)
    np.testing.assert_array_equal(cd.cpu().numpy(), X[want])
    for s in range(S):
        c1, i1 = cl.plusplus_device(Xd, K, first[s:s + 1], u[s:s + 1])
        np.testing.assert_array_equal(i1[0].cpu().numpy(), together[s], err_msg=f"start {s}")
        np.testing.assert_array_equal(c1[0].cpu().numpy(), X[want[s]], err_msg=f"start {s}")

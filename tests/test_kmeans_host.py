"""CPU side of the GPU k-means: the numpy restatement of the stated rules (tests/kmeans_rules.py) reproduces scikit-learn's
fixture, the host draw stream reproduces sklearn's kmeans_plusplus, and inputs outside the envelope / the CLI's --help behave
as documented."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kmeans_rules as R  # noqa: E402
from gen_golden_kmeans import far_init, make_input  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans")


def test_fixture_has_every_case(fx):
    pp = sorted(k for k in fx.files if k.startswith("pp_") and k.endswith("_meta"))
    assert len(pp) == 9
    for name in ("strict", "tol", "maxiter", "relocate"):
        assert f"lloyd_{name}_labels" in fx.files
    for name in ("full", "dups"):
        assert f"fit_{name}_best_start" in fx.files
    for k in pp:
        dg, pg = fx[k.replace("_meta", "_margins")]
        assert dg >= 2.0 ** -20 and pg >= 2.0 ** -20


def test_restatement_reproduces_seeding_fixture(fx):
    from vqvae_amd.cluster import seeding_draws
    for k in sorted(k for k in fx.files if k.startswith("pp_") and k.endswith("_meta")):
        n, d, K, seed = (int(v) for v in fx[k])
        X = make_input("blobs", n, d, seed)
        first, u = seeding_draws(np.random.RandomState(seed), n, K, 1, 2 + int(np.log(K)))
        idx, dg, pg = R.kmeans_plusplus(X, K, int(first[0]), u[0])
        np.testing.assert_array_equal(idx, fx[k.replace("_meta", "_indices")], err_msg=k)


@pytest.mark.parametrize("name", ["strict", "tol", "maxiter", "relocate"])
def test_restatement_reproduces_lloyd_fixture(fx, name):
    tag = f"lloyd_{name}"
    n, d, K, seed, max_iter = (int(v) for v in fx[tag + "_meta"])
    X = make_input(str(fx[tag + "_kind"]), n, d, seed)
    init = far_init(X, K, seed) if name == "relocate" else X[np.random.RandomState(seed).choice(n, K, replace=False)].copy()
    tol = float(fx[tag + "_tol"])
    mean = X.mean(axis=0)
    tol_abs = np.mean(np.var(X, axis=0)) * tol if tol else 0
    c, lab, inertia, n_iter, strict, reloc = R.lloyd(X - mean, init - mean, max_iter, float(tol_abs))
    np.testing.assert_array_equal(lab, fx[tag + "_labels"])
    assert n_iter == int(fx[tag + "_n_iter"])
    np.testing.assert_allclose(c + mean, fx[tag + "_centers"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(inertia, float(fx[tag + "_inertia"]), rtol=1e-5)
    assert {"strict": strict, "tol": not strict, "maxiter": not strict, "relocate": reloc == 1}[name]


@pytest.mark.parametrize("name", ["full", "dups"])
def test_restatement_reproduces_full_fit_fixture(fx, name):
    tag = f"fit_{name}"
    n, d, K, seed, n_init = (int(v) for v in fx[tag + "_meta"])
    X = make_input(str(fx[tag + "_kind"]), n, d, seed)
    got = R.fit(X, K, seed, n_init=n_init)
    np.testing.assert_array_equal(got["labels"], fx[tag + "_labels"])
    assert got["n_iter"] == int(fx[tag + "_n_iter"])
    assert got["best_start"] == int(fx[tag + "_best_start"])
    np.testing.assert_allclose(got["centers"], fx[tag + "_centers"], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/kmeans_edges.npz (tools/gen_golden_kmeans_edges.py): the rules reproduce every case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fxe(golden):
    return golden("kmeans_edges")


def test_edges_fixture_has_every_case(fxe):
    import gen_golden_kmeans_edges as G
    for name in G.LLOYD_CASES:
        for part in ("meta", "labels", "centers", "inertia", "n_iter", "rules_centers", "rules_inertia"):
            assert f"lloyd_{name}_{part}" in fxe.files
        assert int(fxe[f"lloyd_{name}_rules_only"]) == 0
    for name in G.TIE_CASES:                       # the rules' result only: scikit-learn's pick among equal keys is arbitrary
        assert int(fxe[f"lloyd_{name}_rules_only"]) == 1 and f"lloyd_{name}_centers" not in fxe.files
    for name in G.PP_CASES:
        dg, pg = fxe[name + "_margins"]
        n = int(fxe[name + "_meta"][0])
        assert float(fxe[name + "_draw_bound"]) == (2.0 ** -28 if n > 1 << 20 else 2.0 ** -20)
        assert dg >= float(fxe[name + "_draw_bound"]) and pg >= 2.0 ** -20
    lloyd = {k for k in fxe.files if k.startswith("lloyd_") and k.endswith("_meta")}
    assert len(lloyd) == len(G.LLOYD_CASES) + len(G.TIE_CASES)
    assert len([k for k in fxe.files if k.startswith("pp_") and k.endswith("_meta")]) == len(G.PP_CASES)


def _edges_lloyd_names():
    import gen_golden_kmeans_edges as G
    return list(G.LLOYD_CASES)


@pytest.mark.parametrize("name", _edges_lloyd_names())
def test_restatement_reproduces_edges_lloyd_fixture(fxe, name):
    import gen_golden_kmeans_edges as G
    tag = f"lloyd_{name}"
    n, d, K, seed, max_iter = (int(v) for v in fxe[tag + "_meta"])
    X, init, max_iter, tol = G.lloyd_case(name, seed)
    assert X.shape == (n, d) and init.shape == (K, d)
    mean = X.mean(axis=0)
    trace = []
    c, lab, inertia, n_iter, strict, reloc = R.lloyd(X - mean, init - mean, max_iter, tol, trace)
    np.testing.assert_array_equal(lab, fxe[tag + "_labels"].astype(np.int32))
    assert n_iter == int(fxe[tag + "_n_iter"]) and len(trace) == n_iter
    np.testing.assert_allclose(c + mean, fxe[tag + "_centers"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(inertia, float(fxe[tag + "_inertia"]), rtol=1e-5)
    np.testing.assert_array_equal(c, fxe[tag + "_rules_centers"])
    assert inertia == float(fxe[tag + "_rules_inertia"]) and reloc == int(fxe[tag + "_relocations"])
    assert G.lloyd_property(name, trace, K), name       # the route the case exists for is the one it takes


@pytest.mark.parametrize("name", ["tie_rows", "tie_rounds", "zero_keys"])
def test_restatement_reproduces_relocation_tie_fixture(fxe, name):
    import gen_golden_kmeans_edges as G
    tag = f"lloyd_{name}"
    X, init = G.tie_case(name)
    trace = []
    c, lab, inertia, n_iter, strict, reloc = R.lloyd(X, init, 1, 0.0, trace)
    np.testing.assert_array_equal(lab, fxe[tag + "_labels"].astype(np.int32))
    np.testing.assert_array_equal(c, fxe[tag + "_rules_centers"])
    assert n_iter == int(fxe[tag + "_n_iter"]) == 1
    np.testing.assert_array_equal(np.array(trace[0]["moved"]), fxe[tag + "_moved"])
    G.check_tie_case(name, X, init, trace[0]["moved"])
    for row, donor, new in trace[0]["moved"]:            # a moved row is its new cluster's only member: the centre is the row
        np.testing.assert_array_equal(c[new], X[row])


def test_restatement_reproduces_edges_seeding_fixture(fxe):
    import gen_golden_kmeans_edges as G
    from vqvae_amd.cluster import seeding_draws
    for name in G.PP_CASES:
        n, d, K, seed, L, S = (int(v) for v in fxe[name + "_meta"])
        X, K2, L2, S2 = G.pp_input(name, seed)
        assert (X.shape, K2, L2, S2) == ((n, d), K, L, S)
        first, u = seeding_draws(np.random.RandomState(seed), n, K, S, L)
        runs = [R.kmeans_plusplus(X, K, int(first[s]), u[s]) for s in range(S)]
        np.testing.assert_array_equal(np.stack([r[0] for r in runs]), fxe[name + "_indices"], err_msg=name)
        np.testing.assert_allclose([min(r[1] for r in runs), min(r[2] for r in runs)], fxe[name + "_margins"], rtol=1e-6,
                                   err_msg=name)
        if K == n:
            assert sorted(runs[0][0]) == list(range(n))   # every row is a centre, once


def test_host_stream_model_matches_sklearn_kmeans_plusplus():
    skc = pytest.importorskip("sklearn.cluster")
    from vqvae_amd.cluster import n_local_trials_for, seeding_draws
    for n, d, K, seed in [(500, 8, 16, 0), (800, 16, 40, 3)]:
        X = make_input("blobs", n, d, seed)
        _, want = skc.kmeans_plusplus(X, K, random_state=seed)
        first, u = seeding_draws(np.random.RandomState(seed), n, K, 1, n_local_trials_for(K))
        assert first[0] == want[0]
        idx, _, _ = R.kmeans_plusplus(X, K, int(first[0]), u[0])
        np.testing.assert_array_equal(idx, want)
    # the draws of consecutive starts are consecutive in the stream: start 2 of one RandomState = a seeding after start 1
    rs = np.random.RandomState(9)
    f2, u2 = seeding_draws(rs, 300, 8, 2, 4)
    rs = np.random.RandomState(9)
    seeding_draws(rs, 300, 8, 1, 4)
    f1, u1 = seeding_draws(rs, 300, 8, 1, 4)
    assert f1[0] == f2[1] and np.array_equal(u1[0], u2[1])


def test_same_clustering_rule():
    from vqvae_amd.cluster import _is_same_clustering
    a = np.array([0, 0, 1, 2, 2], dtype=np.int32)
    assert _is_same_clustering(a, np.array([2, 2, 0, 1, 1], dtype=np.int32), 3)
    assert not _is_same_clustering(a, np.array([2, 2, 0, 1, 0], dtype=np.int32), 3)
    assert not _is_same_clustering(a, np.array([2, 1, 0, 1, 1], dtype=np.int32), 3)


def test_envelope():
    import torch
    from vqvae_amd.cluster import in_envelope
    X = np.zeros((100, 16), np.float32)
    gpu = torch.cuda.is_available()
    assert in_envelope(X, 8) == gpu
    assert not in_envelope(X.astype(np.float64), 8)
    assert not in_envelope(X, 8, sample_weight=np.ones(100))
    assert not in_envelope(np.zeros((100, 129), np.float32), 8)
    assert not in_envelope(X, 101)
    assert not in_envelope(np.zeros((5000, 4), np.float32), 4097)
    assert not in_envelope(X, 0)
    bad = X.copy()
    bad[3, 3] = np.nan
    assert not in_envelope(bad, 8)
    assert not in_envelope(X[0], 1)


def test_outside_envelope_goes_to_sklearn():
    skc = pytest.importorskip("sklearn.cluster")
    from vqvae_amd import cluster
    X = make_input("blobs", 400, 6, 2).astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = cluster.KMeans(5, random_state=1, n_init=2).fit(X)
        sk = skc.KMeans(5, random_state=1, n_init=2).fit(X)
    assert km.path_ == "sklearn" and cluster.last_path() == "sklearn"
    np.testing.assert_array_equal(km.labels_, sk.labels_)
    np.testing.assert_array_equal(km.cluster_centers_, sk.cluster_centers_)
    assert km.inertia_ == pytest.approx(sk.inertia_, rel=1e-12) and km.n_iter_ == sk.n_iter_ and km.n_features_in_ == 6
    np.testing.assert_array_equal(km.predict(X[:7]), sk.predict(X[:7]))
    c, i = cluster.kmeans_plusplus(X, 5, random_state=4)
    c2, i2 = skc.kmeans_plusplus(X, 5, random_state=4)
    np.testing.assert_array_equal(i, i2)
    assert cluster.last_path() == "sklearn"


def test_cli_help():
    r = subprocess.run([sys.executable, "-m", "vqvae_amd.scripts.codebook_comparison", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("experiment_dir", "--K", "--k_graph", "--seed"):
        assert flag in r.stdout

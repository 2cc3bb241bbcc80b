"""CPU-side checks of the k-medoids analysis: the CLI's flags and defaults are the reference demo's, the score formulas on
hand-built contingency tables (degenerate ones included), the PCA sign rule, and the new symbols in header, binding and
library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from kmedoids_analysis_cases import flip_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("geo_cluster_label_scores", "geo_feature_workspace_bytes", "geo_feature_colstats", "geo_feature_gram",
               "geo_feature_project")


def test_cli_flags_and_defaults_are_the_reference_demo_s():
    from vqvae_amd.scripts.kmedoids_geodesic_analysis import KEYS, parse_args
    a = parse_args(["some/exp"])
    # demos/kmedoids_geodesic_analysis.py parse_args: positional experiment_dir and these six options with these defaults
    assert vars(a) == {"experiment_dir": "some/exp", "k_graph": 10, "graph_sym": "mutual", "K_values": "32,64,128",
                       "inits": "kpp,random", "seed": 42, "out_dir": None}
    b = parse_args(["e", "--k_graph", "7", "--graph_sym", "union", "--K_values", "8, 4", "--inits", "random", "--seed", "3",
                    "--out_dir", "o"])
    assert (b.k_graph, b.graph_sym, b.K_values, b.inits, b.seed, b.out_dir) == (7, "union", "8, 4", "random", 3, "o")
    with pytest.raises(SystemExit):
        parse_args(["e", "--graph_sym", "none"])
    assert KEYS == ("graph", "K", "init", "seed", "qe_geo_finite", "finite_fraction", "purity", "nmi", "ari", "perplexity")


def _brute(table):
    """Scores straight from the definitions, on the expanded label vectors."""
    table = np.asarray(table)
    a = np.repeat(np.arange(table.shape[0]), table.sum(axis=1))
    l = np.concatenate([np.repeat(np.arange(table.shape[1]), row) for row in table])
    n = len(a)
    same_a, same_l = a[:, None] == a[None, :], l[:, None] == l[None, :]
    off = ~np.eye(n, dtype=bool)
    tp, fp = int((same_a & same_l & off).sum()), int((same_a & ~same_l & off).sum())
    fn, tn = int((~same_a & same_l & off).sum()), int((~same_a & ~same_l & off).sum())
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))

    def H(v):
        p = np.bincount(v) / n
        p = p[p > 0]
        return -np.sum(p * np.log(p))
    p = table / n
    pa, pl = p.sum(axis=1, keepdims=True), p.sum(axis=0, keepdims=True)
    nz = p > 0
    mi = float(np.sum(p[nz] * np.log(p[nz] / (pa @ pl)[nz])))
    return {"purity": table.max(axis=1).sum() / n, "mi": mi, "h": 0.5 * (H(a) + H(l)), "ari": ari}


def test_scores_on_hand_built_tables():
    from vqvae_amd.geo.analysis import scores_from_contingency
    for table in ([[5, 1, 0], [0, 4, 2], [3, 0, 6]], [[2, 2], [2, 2]], [[7, 0, 1], [0, 0, 0], [1, 9, 0]]):
        s, b = scores_from_contingency(table), _brute(table)
        assert s["purity"] == pytest.approx(b["purity"], rel=1e-15)
        assert s["ari"] == pytest.approx(b["ari"], rel=1e-14, abs=1e-15)
        if b["mi"] < 1e-14:
            assert s["nmi"] == pytest.approx(0.0, abs=1e-14)
        else:
            assert s["nmi"] == pytest.approx(b["mi"] / b["h"], rel=1e-13)
    # perfect agreement under a permutation of the code numbers
    s = scores_from_contingency([[0, 4, 0], [3, 0, 0], [0, 0, 5]])
    assert s["purity"] == 1.0 and s["ari"] == 1.0 and s["nmi"] == pytest.approx(1.0, rel=1e-14)
    counts = np.array([4, 3, 5]) / 12
    assert s["perplexity"] == pytest.approx(math.exp(-np.sum(counts * np.log(counts + 1e-12))), rel=1e-15)


def test_degenerate_tables_follow_scikit_learn():
    from vqvae_amd.geo.analysis import scores_from_contingency
    one_one = scores_from_contingency([[9]])                       # one cluster, one class: both 1.0
    assert one_one["nmi"] == 1.0 and one_one["ari"] == 1.0 and one_one["purity"] == 1.0 and one_one["perplexity"] == pytest.approx(1.0)
    one_cluster = scores_from_contingency([[3, 4, 2], [0, 0, 0]])  # one cluster, several classes: MI = 0 -> 0.0
    assert one_cluster["nmi"] == 0.0 and one_cluster["ari"] == 0.0 and one_cluster["purity"] == pytest.approx(4 / 9)
    one_class = scores_from_contingency([[3], [4], [2]])
    assert one_class["nmi"] == 0.0 and one_class["ari"] == 0.0 and one_class["purity"] == 1.0
    # all singletons against all singletons: fp = fn = 0 -> ARI 1.0, NMI 1.0
    single = scores_from_contingency(np.eye(6, dtype=np.int64))
    assert single["ari"] == 1.0 and single["nmi"] == pytest.approx(1.0, rel=1e-14) and single["perplexity"] == pytest.approx(6.0)
    # all singletons against one class: one class -> 0.0; pair counts tp = fp = 0, fn = n(n-1), tn = 0
    single_one = scores_from_contingency(np.ones((6, 1), dtype=np.int64))
    assert single_one["nmi"] == 0.0 and single_one["ari"] == 0.0
    empty = scores_from_contingency(np.zeros((3, 2), dtype=np.int64))
    assert empty["nmi"] == 1.0 and empty["ari"] == 1.0 and math.isnan(empty["purity"]) and empty["perplexity"] == 0.0


def test_purity_divides_by_all_rows_like_the_demo():
    from vqvae_amd.geo.analysis import scores_from_contingency
    assert scores_from_contingency([[3, 1], [0, 4]], n_total=10)["purity"] == 0.7


def test_sign_rule_makes_the_largest_entry_positive():
    from vqvae_amd.geo.analysis import svd_flip_rows
    c = np.array([[0.1, -0.9, 0.3], [0.5, 0.2, -0.4], [-0.7, 0.7, 0.1]])
    f = svd_flip_rows(c)
    assert np.array_equal(f, np.array([[-0.1, 0.9, -0.3], [0.5, 0.2, -0.4], [0.7, -0.7, -0.1]]))   # tie: the first one decides
    assert np.array_equal(f, flip_rows(c))
    assert np.array_equal(svd_flip_rows(f), f)


def test_new_symbols_are_declared_bound_and_exported():
    from vqvae_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geo_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS, name
        assert re.search(r" T %s\b" % name, out), name
    lib = _lib.load()
    assert lib.geo_feature_workspace_bytes(0, 4) == 0 and lib.geo_feature_workspace_bytes(100, 4097) == 0
    assert lib.geo_feature_workspace_bytes(1500, 32) >= 32 * 32 * 8


def test_fit_kmedoids_path_is_exported_and_validates():
    from vqvae_amd.geo import fit_kmedoids_path
    from scipy import sparse
    W = sparse.csr_matrix((np.ones(2, np.float32), ([0, 1], [1, 0])), shape=(2, 2))
    with pytest.raises(ValueError):
        fit_kmedoids_path(W, [2], init="pam")
    with pytest.raises(ValueError):
        fit_kmedoids_path(W, [])

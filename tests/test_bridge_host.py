"""Component bridging without a GPU: the algorithmic claim behind geo_bridge_components (Boruvka rounds that leave the
largest component out of the queries give Kruskal's edges under the order (key, lo, hi)) on the oracle of
tests/bridge_cases.py, and the host-side surface of the feature (CLI flag, wrapper validation, exports)."""
import math

import numpy as np
import pytest
from scipy import sparse

import bridge_cases as bc


@pytest.mark.parametrize("name", bc.GRAPH_CASES)
def test_graph_cases_have_the_recorded_components(name):
    case = bc.graph_case(name)
    sizes = np.bincount(case["labels"])
    assert (case["C"], int(sizes.max())) == bc.GRAPH_COMPONENTS[name]
    assert case["edges"].shape == (case["C"] - 1, 2)


def _check_rounds(case):
    edges, keys, rounds, queries = bc.boruvka_skip_largest(case["z"], case["labels"], case["form"])
    np.testing.assert_array_equal(edges, case["edges"])
    assert keys.view(np.int64).tolist() == case["keys"].view(np.int64).tolist()
    assert rounds <= math.ceil(math.log2(case["C"]))
    assert queries[0] == len(case["z"]) - np.bincount(case["labels"]).max()
    return rounds, queries


@pytest.mark.parametrize("name", bc.GRAPH_CASES)
def test_rounds_without_the_largest_component_give_kruskals_edges(name):
    rounds, queries = _check_rounds(bc.graph_case(name))
    if name == "giant_plus_outliers":
        assert queries[0] == 357


@pytest.mark.parametrize("name", bc.LABEL_CASES)
def test_rounds_give_kruskals_edges_for_given_labels(name):
    _check_rounds(bc.label_case(name))


def test_oracle_edges_are_sorted_and_span():
    for case in [bc.graph_case("grid_ties"), bc.label_case("singletons_d7")]:
        e, k = case["edges"], case["keys"]
        order = np.lexsort((e[:, 1], e[:, 0], k))
        assert order.tolist() == list(range(len(k))) and (e[:, 0] < e[:, 1]).all()
        n = len(case["z"])
        lab = case["labels"]
        A = sparse.csr_matrix((np.ones(len(e)), (lab[e[:, 0]], lab[e[:, 1]])), shape=(case["C"], case["C"]))
        assert sparse.csgraph.connected_components(A, directed=False)[0] == 1 and n >= case["C"]
    assert len(np.unique(bc.graph_case("grid_ties")["keys"])) < 10          # equal keys everywhere: the tie rule decides


def test_nearest_foreign_oracle_matches_the_definition():
    case = bc.label_case("halves_d16")
    nbr, key = bc.nearest_foreign(case["z"], case["labels"], np.array([0, 399, 0]), case["form"])
    assert nbr[0] == nbr[2] and nbr[0] >= 200 and nbr[1] < 200 and key[0] == key[2]
    nbr, key = bc.nearest_foreign(case["z"], np.zeros(400, np.int32), np.array([5]), case["form"])
    assert nbr[0] == -1 and np.isinf(key[0])


def test_cli_flag_defaults_to_off():
    from vqvae_amd.scripts.build_codebook import make_parser
    base = ["--latents_path", "z.pt", "--out_dir", "o", "--vae_ckpt_path", "c.pt", "--in_channels", "1", "--output_image_size", "28",
            "--latent_dim", "8", "--enc_channels", "64", "--dec_channels", "64", "--recon_loss", "mse", "--norm_type", "batch"]
    assert make_parser().parse_args(base).connect_components is False
    assert make_parser().parse_args(base + ["--connect_components"]).connect_components is True


def test_connect_components_is_euclidean_only():
    from vqvae_amd.geo import connect_components
    W = sparse.csr_matrix((np.ones(2, np.float32), ([0, 1], [1, 0])), shape=(3, 3))
    z = np.zeros((3, 4), np.float32)
    for metric in ("cosine", "manhattan"):
        with pytest.raises(ValueError):
            connect_components(W, z, metric=metric)
    with pytest.raises(ValueError):
        connect_components(W, z, mode="nonsense")
    with pytest.raises(ValueError):
        connect_components(W, np.zeros((4, 4), np.float32))


def test_new_names_are_exported():
    from vqvae_amd import _lib, geo
    for name in ("nearest_foreign_device", "bridge_components_device", "connect_components"):
        assert name in geo.__all__ and callable(getattr(geo, name))
    for name in ("geo_nearest_foreign", "geo_nearest_foreign_workspace_bytes", "geo_bridge_components",
                 "geo_bridge_components_workspace_bytes", "geo_csr_insert_workspace_bytes", "geo_csr_insert_count",
                 "geo_csr_insert_fill"):
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES, name
    assert _lib.load().geo_version() >= 114
    import inspect
    from vqvae_amd.scripts.build_codebook import build_codebook_device
    assert inspect.signature(build_codebook_device).parameters["connect_components"].default is False

"""Cell-restricted medoid update, the parts that need no GPU: the ABI, the CLI defaults, the argument checks of the Python
wrappers (before the library is loaded) and the host restatement of tests/cell_cases.py on a hand-computed example."""
import os
import re

import numpy as np
import pytest
import torch

import cell_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("geo_cell_costs", "geo_cell_costs_workspace_bytes", "geo_cell_costs_min_workspace_bytes", "geo_cell_costs_tile",
       "geo_cell_costs_resident_max_nodes")


def test_new_symbols_are_declared_bound_and_exported():
    from vqvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "geo_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES, name
    assert len(_lib._SIGNATURES["geo_cell_costs"][1]) == 16
    import vqvae_amd.geo as geo
    for name in ("cell_medoid_update_device", "fit_kmedoids_voronoi_graph"):
        assert name in geo.__all__ and callable(getattr(geo, name))


def test_library_answers_the_size_queries():
    """Host arithmetic only: the tile, the resident bound that follows from 160 KiB of LDS, and workspace sizes that grow with
    the largest cell and never fall below the minimum."""
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.geo_version() >= 112
    S, R = lib.geo_cell_costs_tile(), lib.geo_cell_costs_resident_max_nodes()
    assert S >= 1 and R >= 64 and S * R * 8 <= 160 * 1024
    lo = lib.geo_cell_costs_min_workspace_bytes(10000, 200000, 40, 300)
    hi = lib.geo_cell_costs_workspace_bytes(10000, 200000, 40, 300)
    assert 0 < lo <= hi
    assert lib.geo_cell_costs_min_workspace_bytes(10000, 200000, 40, 3000) - lo == (3000 - 300) * S * 8
    assert lib.geo_cell_costs_min_workspace_bytes(10000, 400000, 40, 300) - lo == 200000 * 8


def test_cli_defaults_leave_the_build_as_it_is():
    from vqvae_amd.scripts.build_codebook import make_parser
    base = ["--latents_path", "z.pt", "--out_dir", "o", "--vae_ckpt_path", "c.pt", "--in_channels", "1", "--output_image_size", "28",
            "--latent_dim", "16", "--enc_channels", "64", "--dec_channels", "64", "--recon_loss", "mse", "--norm_type", "batch"]
    args = make_parser().parse_args(base)
    assert args.refine_iters == 0 and args.refine_power == 2
    args = make_parser().parse_args(base + ["--refine_iters", "3", "--refine_power", "1"])
    assert args.refine_iters == 3 and args.refine_power == 1
    with pytest.raises(SystemExit):
        make_parser().parse_args(base + ["--refine_power", "3"])


def _cpu_graph():
    from vqvae_amd._device import DeviceCSR
    W, assign, medoids, _, _ = cc.seven_node_example()
    return DeviceCSR.from_scipy(W, torch.device("cpu")), assign, medoids


def test_wrappers_refuse_bad_arguments_before_the_library_is_loaded(monkeypatch):
    from vqvae_amd import _lib
    from vqvae_amd.geo.kmeans_optimized import cell_medoid_update_device, fit_kmedoids_voronoi_graph

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_load)
    G, assign, medoids = _cpu_graph()
    for power in (0, 3, 2.5, None):
        with pytest.raises(ValueError, match="power"):
            cell_medoid_update_device(G, assign, medoids, power)
        with pytest.raises(ValueError, match="power"):
            fit_kmedoids_voronoi_graph(G, K=3, power=power)
    with pytest.raises(ValueError, match="assign"):
        cell_medoid_update_device(G, assign[:-1], medoids)
    with pytest.raises(ValueError, match="assign"):
        cell_medoid_update_device(G, np.where(assign == 1, 3, assign), medoids)         # a value == K
    with pytest.raises(ValueError, match="assign"):
        cell_medoid_update_device(G, np.where(assign == 1, -2, assign), medoids)
    for bad in (np.array([0, 5, 7]), np.array([-1, 5, 6])):
        with pytest.raises(ValueError, match="medoids"):
            cell_medoid_update_device(G, assign, bad)
    with pytest.raises(ValueError, match="resident_nodes_max"):
        cell_medoid_update_device(G, assign, medoids, resident_nodes_max=0)
    with pytest.raises(AssertionError, match="library was loaded"):                     # good arguments do reach the library
        cell_medoid_update_device(G, assign, medoids)


@pytest.mark.parametrize("power", [1, 2])
def test_restatement_reproduces_the_seven_node_example(power):
    W, assign, medoids, costs, new_expected = cc.seven_node_example()
    cut = cc.cut_graph(W, assign)
    assert cut.nnz == W.nnz - 4 and cut[2, 3] == 0 and cut[5, 6] == 0 and cut[0, 2] == 4.0
    new, cost, kept = cc.restated_update(W, assign, medoids, power)
    np.testing.assert_array_equal(cost, costs[power])
    np.testing.assert_array_equal(new, new_expected)
    assert kept == 0


def test_selection_keeps_the_medoid_of_an_all_inf_cell():
    """Path 0-1-2-3-4 with cells (0, 1, 0, 1, 1): neither induced subgraph is connected, every cost is +inf, both medoids stay
    (np.argmin would move each to its first member); with one finite cost the lowest index among the smallest wins."""
    from scipy import sparse
    r = [0, 1, 2, 3]
    W = sparse.csr_matrix((np.ones(8, dtype=np.float32), (r + [1, 2, 3, 4], [1, 2, 3, 4] + r)), shape=(5, 5))
    assign = np.array([0, 1, 0, 1, 1])
    new, cost, kept = cc.restated_update(W, assign, np.array([2, 4]), 2)
    assert np.isinf(cost).all() and kept == 2
    np.testing.assert_array_equal(new, [2, 4])
    new, kept = cc.select_medoids(np.array([3.0, np.inf, 3.0, 1.0, 1.0]), assign, np.array([2, 1]))
    np.testing.assert_array_equal(new, [0, 3])
    assert kept == 0

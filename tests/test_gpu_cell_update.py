"""Cell-restricted medoid update (csrc/cell.hip, extension without a reference implementation) on the GPU against the host
restatement of tests/cell_cases.py: oracle/kmedoids.py's medoid_update over the all-pairs matrix of the CUT graph.  Costs are
compared bit for bit (same fp64 shortest-path rule, same summation tree)."""
import json
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import cell_cases as cc

pytestmark = pytest.mark.gpu


def _run(W, assign, medoids, power, **kw):
    from vqvae_amd.geo.kmeans_optimized import _to_device_graph, cell_medoid_update_device
    info = {}
    new, cost = cell_medoid_update_device(_to_device_graph(W), assign.astype(np.int32), medoids.astype(np.int32), power, info=info, **kw)
    return new.cpu().numpy(), cost.cpu().numpy(), info


_voronoi_cache = {}


def _voronoi_case(n, d, k, seed, K):
    """(W, assign, medoids) with K random medoids and the float32 nearest-medoid assignment, once per process."""
    key = (n, d, k, seed, K)
    if key not in _voronoi_cache:
        W = cc.knn_graph(n, d, k, seed)
        med = np.random.RandomState(1).choice(W.shape[0], K, replace=False)
        _, assign = cc.host_assign(W, med)
        _voronoi_cache[key] = (W, assign, med, {})
    return _voronoi_cache[key]


def _restated(case, power):
    W, assign, med, memo = case
    if power not in memo:
        memo[power] = cc.restated_update(W, assign, med, power)
    return memo[power]


@pytest.mark.parametrize("power", [2, 1])
def test_costs_and_medoids_equal_the_restatement_on_every_route(power):
    """~60-node cells: LDS by default; resident_nodes_max = 1 sends every cell of two or more nodes through the workspace;
    the smallest legal workspace leaves one slice.  One result, bit for bit; a workspace below the minimum is refused."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.kmeans_optimized import _to_device_graph
    case = _voronoi_case(2500, 16, 10, 5, 40)
    W, assign, med, _ = case
    new_o, cost_o, kept_o = _restated(case, power)
    sizes = np.bincount(assign, minlength=40)
    lib = _lib.load()
    assert 1 < sizes.max() <= lib.geo_cell_costs_resident_max_nodes()
    new_r, cost_r, info_r = _run(W, assign, med, power)
    np.testing.assert_array_equal(cost_r, cost_o)
    np.testing.assert_array_equal(new_r, new_o)
    assert info_r["resident_cells"] == int((sizes > 0).sum()) and info_r["workspace_cells"] == 0
    assert info_r["kept_cells"] == kept_o and info_r["max_sweeps"] >= 2
    new_w, cost_w, info_w = _run(W, assign, med, power, resident_nodes_max=1)
    np.testing.assert_array_equal(cost_w, cost_o)
    np.testing.assert_array_equal(new_w, new_o)
    assert info_w["workspace_cells"] == int((sizes > 1).sum()) and info_w["resident_cells"] == int((sizes == 1).sum())
    G = _to_device_graph(W)
    least = lib.geo_cell_costs_min_workspace_bytes(G.n, G.nnz, 40, int(sizes.max()))
    assert least < lib.geo_cell_costs_workspace_bytes(G.n, G.nnz, 40, int(sizes.max()))
    new_m, cost_m, info_m = _run(W, assign, med, power, resident_nodes_max=1, max_workspace_bytes=least)
    np.testing.assert_array_equal(cost_m, cost_o)
    np.testing.assert_array_equal(new_m, new_o)
    assert info_m["workspace_cells"] == info_w["workspace_cells"] and info_m["max_sweeps"] >= 2
    with pytest.raises(_lib.GeoHipError, match="status -2"):
        _run(W, assign, med, power, max_workspace_bytes=least - 256)


def test_large_cells_equal_the_restatement():
    """Three planar cells, two of them beyond a thousand nodes: past the default resident bound, so they take the workspace
    route unasked, the third stays in LDS in the same call; a bound of 256 is given as well."""
    from vqvae_amd import _lib
    case = _voronoi_case(3000, 2, 8, 9, 3)
    W, assign, med, _ = case
    new_o, cost_o, _ = _restated(case, 2)
    sizes = np.bincount(assign, minlength=3)
    default = _lib.load().geo_cell_costs_resident_max_nodes()
    assert sizes.max() > default > 256 and 0 < sizes.min() <= 256
    for kw, bound in (({}, default), ({"resident_nodes_max": 256}, 256)):
        new_g, cost_g, info = _run(W, assign, med, 2, **kw)
        np.testing.assert_array_equal(cost_g, cost_o)
        np.testing.assert_array_equal(new_g, new_o)
        assert info["workspace_cells"] == int((sizes > bound).sum()) and info["resident_cells"] == int((sizes <= bound).sum())


@pytest.mark.parametrize("power", [2, 1])
def test_tile_and_size_edges_in_one_assignment(power):
    """Cells of 1, 2, S-1, S, S+1 and 2S+1 connected nodes (S = the library's tile), an empty cell, nodes of no cell, a duplicate
    medoid, and the path 0-1-2-3-4 split (a, b, a, b, b): both of its cells are disconnected inside, keep their medoids and are
    the two kept cells."""
    from vqvae_amd import _lib
    S = _lib.load().geo_cell_costs_tile()
    base = cc.knn_graph(600, 4, 6, 3)
    nb = base.shape[0]
    r = [0, 1, 2, 3]
    path = sparse.csr_matrix((np.full(8, 0.5, dtype=np.float32), (r + [1, 2, 3, 4], [1, 2, 3, 4] + r)), shape=(5, 5))
    W = sparse.block_diag([base, path], format="csr").astype(np.float32)
    n = W.shape[0]
    assign = np.full(n, -1, dtype=np.int64)
    taken, seeds = set(), np.random.RandomState(7).permutation(nb)
    sizes = [1, 2, S - 1, S, S + 1, 2 * S + 1]
    for c, size in enumerate(sizes):
        seed = next(int(s) for s in seeds if int(s) not in taken)
        cell = cc.grow_cell(base, seed, size, taken)
        taken.update(cell)
        assign[cell] = c
    K = len(sizes) + 3                                           # cell 6 stays empty, cells 7 and 8 share the path
    assign[nb:] = [7, 8, 7, 8, 8]
    medoids = np.array([int(np.flatnonzero(assign == c)[-1]) for c in range(len(sizes))] + [0, nb + 2, nb + 4])
    medoids[6] = medoids[3]                                      # the empty cell's medoid duplicates another
    assert (assign < 0).sum() > 100
    new_o, cost_o, kept_o = cc.restated_update(W, assign, medoids, power)
    assert kept_o == 2 and np.isfinite(cost_o[assign == 5]).all()
    for kw in ({}, {"resident_nodes_max": 1}, {"resident_nodes_max": S}):
        new_g, cost_g, info = _run(W, assign, medoids, power, **kw)
        np.testing.assert_array_equal(cost_g, cost_o)
        np.testing.assert_array_equal(new_g, new_o)
        assert info["kept_cells"] == 2 and info["tile"] == S
    assert np.isinf(cost_g[assign < 0]).all() and np.isinf(cost_g[nb:]).all()
    assert new_g[6] == medoids[6] and new_g[7] == nb + 2 and new_g[8] == nb + 4


@pytest.mark.parametrize("d,k,init,min_updates", [(2, 8, "kpp", 5), (16, 10, "kpp", 1), (2, 8, "random", 5)])
def test_fit_end_to_end_equals_the_host_loop(d, k, init, min_updates):
    from oracle import kmedoids as okm
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_voronoi_graph
    W = cc.knn_graph(3000, d, k, 9)
    med0, _, _ = okm.fit_kmedoids_optimized(W, K=64, init=init, seed=42)
    med_o, assign_o, hist_o, rejected_o, _ = cc.host_voronoi_graph(W, med0, max_iter=10)
    info = {}
    med_g, assign_g, qe_g, hist_g = fit_kmedoids_voronoi_graph(W, K=64, init=init, seed=42, max_iter=10, info=info)
    print(f"d={d} init={init}: {len(hist_g) - 1} updates, objective {hist_g[0]:.3f} -> {hist_g[-1]:.3f}, rejected {info['rejected']}")
    np.testing.assert_array_equal(med_g, med_o)
    np.testing.assert_array_equal(assign_g, assign_o)
    assert hist_g == hist_o and info["rejected"] == rejected_o and info["iterations"] == len(hist_g) - 1
    assert all(b < a for a, b in zip(hist_g, hist_g[1:]))
    assert len(hist_g) - 1 >= min_updates
    dmin, _ = cc.host_assign(W, med_o)
    assert qe_g == okm.quantization_error_from(dmin)


def _write_inputs(tmp, d, seed, n_img):
    from oracle import metric as om
    sd = om.make_decoder_state(seed, d, 1, norm_type="batch")
    z4 = np.random.RandomState(seed).randn(n_img * 16, d).astype(np.float32).reshape(n_img, 4, 4, d)
    z4 = np.ascontiguousarray(np.transpose(z4, (0, 3, 1, 2)))
    state = {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    torch.save({"model_state_dict": state, "epoch": 0}, os.path.join(tmp, "best.pt"))
    torch.save(torch.from_numpy(z4), os.path.join(tmp, "z.pt"))
    return z4


def test_cli_refine_flags(tmp_path):
    """--refine_iters 0 writes what a run without the flag writes, byte for byte; --refine_iters 3 writes the same three
    artefacts in the same format with the refined medoids and codes, plus refine.json."""
    from vqvae_amd.scripts.build_codebook import main, make_parser
    from vqvae_amd.training.assign_codes_val_geodesic import load_build
    tmp = str(tmp_path)
    n_img, d = 48, 8
    _write_inputs(tmp, d, 11, n_img)

    def build(name, extra):
        out = os.path.join(tmp, name)
        main(make_parser().parse_args([
            "--latents_path", os.path.join(tmp, "z.pt"), "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
            "--in_channels", "1", "--output_image_size", "28", "--latent_dim", str(d), "--enc_channels", "64", "128", "256",
            "--dec_channels", "256", "128", "64", "--recon_loss", "mse", "--norm_type", "batch", "--mse_use_sigmoid",
            "--k", "8", "--sym", "union", "--K", "12", "--init", "kpp", "--seed", "42", "--batch_size", "256"] + extra))
        return out

    plain, zero, refined = build("plain", []), build("zero", ["--refine_iters", "0"]), build("refined", ["--refine_iters", "3"])
    names = ["codebook.pt", "codes.npy", "knn_graph_geodesic.npz"]
    assert sorted(os.listdir(plain)) == sorted(os.listdir(zero)) == names
    cb_p = torch.load(os.path.join(plain, "codebook.pt"), weights_only=False)
    cb_z = torch.load(os.path.join(zero, "codebook.pt"), weights_only=False)
    assert open(os.path.join(plain, "codes.npy"), "rb").read() == open(os.path.join(zero, "codes.npy"), "rb").read()
    # the two containers carry what is not the build's (zip member times, the out_dir string in config): their contents, byte for byte
    W_p, W_z = (sparse.load_npz(os.path.join(o, "knn_graph_geodesic.npz")) for o in (plain, zero))
    for part in ("indptr", "indices", "data"):
        assert getattr(W_p, part).dtype == getattr(W_z, part).dtype and getattr(W_p, part).tobytes() == getattr(W_z, part).tobytes()
    assert cb_p["medoid_indices"].dtype == cb_z["medoid_indices"].dtype
    assert cb_p["medoid_indices"].tobytes() == cb_z["medoid_indices"].tobytes()
    assert cb_p["z_medoid"].dtype == cb_z["z_medoid"].dtype and torch.equal(cb_p["z_medoid"], cb_z["z_medoid"])
    assert {k: v for k, v in cb_p["config"].items() if k != "out_dir"} == {k: v for k, v in cb_z["config"].items() if k != "out_dir"}
    assert sorted(os.listdir(refined)) == sorted(names + ["refine.json"])
    cb_r = torch.load(os.path.join(refined, "codebook.pt"), weights_only=False)
    assert list(cb_r["config"].keys()) == list(cb_p["config"].keys()) and list(cb_r.keys()) == list(cb_p.keys())
    codes_p, codes_r = np.load(os.path.join(plain, "codes.npy")), np.load(os.path.join(refined, "codes.npy"))
    assert codes_r.dtype == codes_p.dtype == np.int32 and codes_r.shape == codes_p.shape == (n_img, 4, 4)
    assert cb_r["medoid_indices"].dtype == np.int32 and cb_r["medoid_indices"].shape == cb_p["medoid_indices"].shape
    rj = json.load(open(os.path.join(refined, "refine.json")))
    assert rj["refine_iters"] == 3 and rj["refine_power"] == 2 and rj["iterations"] == len(rj["history"]) - 1 <= 3
    assert all(b < a for a, b in zip(rj["history"], rj["history"][1:]))
    assert (rj["iterations"] > 0) == (not np.array_equal(cb_r["medoid_indices"], cb_p["medoid_indices"]))
    for key in ("resident_cells", "workspace_cells", "max_sweeps", "kept_cells"):
        assert key in rj["info"]["updates"][0]
    codebook, W, z_lcc = load_build(refined)                      # raises unless z_lcc[medoid_indices] == z_medoid bit for bit
    assert torch.equal(z_lcc[torch.from_numpy(cb_r["medoid_indices"].astype(np.int64))], cb_r["z_medoid"])
    # the refined codes are the nearest refined medoids
    _, assign = cc.host_assign(W, cb_r["medoid_indices"])
    np.testing.assert_array_equal(codes_r.reshape(-1)[codes_r.reshape(-1) >= 0], assign)


def test_two_streams_give_the_same_bits():
    case = _voronoi_case(2500, 16, 10, 5, 40)
    W, assign, med, _ = case
    from vqvae_amd._device import device
    _, cost_a, _ = _run(W, assign, med, 2)
    with torch.cuda.stream(torch.cuda.Stream(device=device())):
        _, cost_b, _ = _run(W, assign, med, 2)
        _, cost_c, _ = _run(W, assign, med, 2, resident_nodes_max=32)
    assert cost_a.tobytes() == cost_b.tobytes() == cost_c.tobytes()


def test_library_refuses_bad_arguments_and_writes_nothing():
    """GEO_E_ARG (-1) for power, K, a null pointer (before any launch) and for offsets[K] > n or an order that names a node
    twice (found by the plan, before any solve); cost_out keeps what it held."""
    from vqvae_amd import _lib
    from vqvae_amd._device import device, ptr, stream_ptr
    from vqvae_amd.geo.kmeans_optimized import _to_device_graph
    lib, dev = _lib.load(), device()
    W, assign, _, _, _ = cc.seven_node_example()
    G = _to_device_graph(W)
    n, K = 7, 3
    a = torch.from_numpy(assign.astype(np.int32)).to(dev)
    order = torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 3, 6, 6], dtype=torch.int32, device=dev)
    ws = torch.empty(lib.geo_cell_costs_workspace_bytes(n, G.nnz, K, 3), dtype=torch.uint8, device=dev)
    cost = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    status = np.zeros(4, dtype=np.int32)

    def call(power=2, K_=K, order_=order, offsets_=offsets, cost_=cost):
        with torch.cuda.device(dev):
            return lib.geo_cell_costs(ptr(G.indptr), ptr(G.indices), ptr(G.data), n, G.nnz, ptr(a), ptr(order_), ptr(offsets_), K_, power, 0,
                                      ptr(cost_), ptr(ws), ws.numel(), status.ctypes.data, stream_ptr())

    assert call(power=3) == -1 and call(K_=0) == -1 and call(cost_=None) == -1
    assert call(offsets_=torch.tensor([0, 3, 6, 8], dtype=torch.int32, device=dev)) == -1
    assert call(order_=torch.tensor([0, 1, 1, 3, 4, 5, 6], dtype=torch.int32, device=dev)) == -1
    assert b"inconsistent" in lib.geo_last_error()
    assert (cost == -7.0).all()
    assert call() == 0
    W7, assign7, med7, costs7, new7 = cc.seven_node_example()
    np.testing.assert_array_equal(cost.cpu().numpy(), costs7[2])
    assert list(status) == [2, 0, int(status[2]), 0] and status[2] >= 2

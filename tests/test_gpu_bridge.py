"""Bridging the components of a kNN graph on the GPU (csrc/knn.hip: geo_nearest_foreign, geo_bridge_components; csrc/graph.hip:
geo_csr_insert_*) against the CPU oracle of tests/bridge_cases.py: Kruskal over all cross-label pairs ordered by
(oracle.knn.knn_pair_keys(z, lo, hi, form), lo, hi).  Every comparison is exact: indices equal, keys equal in every bit."""
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import bridge_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _canonical(W):
    W = sparse.csr_matrix(W)
    for a, b in zip(W.indptr[:-1], W.indptr[1:]):
        assert np.all(np.diff(W.indices[a:b]) > 0)               # ascending, no repeated column
    assert (W.diagonal() == 0).all() and (W.data != 0).all()
    assert (abs(W - W.T)).nnz == 0


# ------------------------------------------------------------------------------------------------ nearest foreign node
@pytest.mark.parametrize("name,kind", [("random7_d16", "strided"), ("random7_d16", "wrap4"), ("random7_d16", "wrap8"),
                                       ("random7_d12", "strided"), ("random7_d12", "wrap4"), ("random7_d12", "wrap8"),
                                       ("chunks_d40", "strided"), ("chunks_d40", "wrap4"), ("singletons_d7", "strided"),
                                       ("halves_d16", "wrap4")])
def test_nearest_foreign_matches_brute_force(name, kind):
    from vqvae_amd.geo import nearest_foreign_device
    case = bc.label_case(name)
    z, labels = case["z"], case["labels"]
    rows = bc.query_rows(len(z), kind)
    if name == "halves_d16":                    # every query of one component: the waves' labels are uniform at four per wave
        rows = (200 + rows % 200).astype(np.int32)
    ref_nbr, ref_key = bc.nearest_foreign(z, labels, rows, case["form"])
    nbr, key = nearest_foreign_device(_dev(z), _dev(labels), _dev(rows), form=case["form"])
    np.testing.assert_array_equal(nbr.cpu().numpy(), ref_nbr)
    np.testing.assert_array_equal(_bits(key.cpu().numpy()), _bits(ref_key))


def test_nearest_foreign_of_a_graph_case_with_ties():
    from vqvae_amd.geo import nearest_foreign_device
    case = bc.graph_case("grid_ties")
    rows = np.arange(len(case["z"]), dtype=np.int32)
    ref_nbr, ref_key = bc.nearest_foreign(case["z"], case["labels"], rows, case["form"])
    nbr, key = nearest_foreign_device(_dev(case["z"]), _dev(case["labels"]), _dev(rows))
    np.testing.assert_array_equal(nbr.cpu().numpy(), ref_nbr)
    np.testing.assert_array_equal(_bits(key.cpu().numpy()), _bits(ref_key))


def test_nearest_foreign_without_a_foreign_node_and_without_queries():
    from vqvae_amd.geo import nearest_foreign_device
    z = _dev(bc.label_case("halves_d16")["z"])
    labels = torch.zeros(400, dtype=torch.int32, device=DEV)
    nbr, key = nearest_foreign_device(z, labels, _dev(np.array([0, 7, 399], np.int32)))
    assert nbr.cpu().tolist() == [-1, -1, -1] and torch.isinf(key).all() and (key > 0).all()
    nbr, key = nearest_foreign_device(z, labels, torch.empty(0, dtype=torch.int32, device=DEV))
    assert nbr.numel() == 0 and key.numel() == 0
    with pytest.raises(ValueError):
        nearest_foreign_device(z, labels, _dev(np.array([400], np.int32)))


# ------------------------------------------------------------------------------------------------ bridges of given labels
@pytest.mark.parametrize("name", bc.LABEL_CASES)
def test_bridges_of_given_labels(name):
    from vqvae_amd.geo.knn_graph_optimized import bridge_edges_device
    case = bc.label_case(name)
    edges, keys, info = bridge_edges_device(_dev(case["z"]), _dev(case["labels"]), case["C"], form=case["form"])
    np.testing.assert_array_equal(edges.cpu().numpy(), case["edges"])
    np.testing.assert_array_equal(_bits(keys.cpu().numpy()), _bits(case["keys"]))
    assert 1 <= info["rounds"] <= math.ceil(math.log2(case["C"]))
    sizes = np.bincount(case["labels"])
    assert info["queries_first_round"] == len(case["z"]) - sizes.max() and info["queries"] >= info["queries_first_round"]
    if name == "halves_d16":                    # the largest component is tied: label 0 stays out, label 1 asks
        assert info == {"components": 2, "rounds": 1, "queries_first_round": 200, "queries": 200}


def test_bridge_errors_write_nothing():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    case = bc.label_case("halves_d16")
    z, n, d = _dev(case["z"]), 400, 16
    edges = torch.full((1, 2), -7, dtype=torch.int32, device=DEV)
    keys = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    status = np.full(4, -7, np.int32)
    need = lib.geo_bridge_components_workspace_bytes(n, d, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(labels, C, nbytes):
        return lib.geo_bridge_components(ptr(z), n, d, 1, ptr(labels), C, ptr(edges), ptr(keys), status.ctypes.data, ptr(ws), nbytes,
                                         stream_ptr())

    good = _dev(case["labels"])
    bad = good.clone()
    bad[17] = 2                                 # outside [0, C): found by the plan
    neg = good.clone()
    neg[399] = -1
    assert call(bad, 2, need) != 0 and call(neg, 2, need) != 0 and call(good, 0, need) != 0
    assert call(good, 2, need - 1) != 0         # below the size query
    assert lib.geo_bridge_components(None, n, d, 1, ptr(good), 2, ptr(edges), ptr(keys), status.ctypes.data, ptr(ws), need,
                                     stream_ptr()) != 0
    torch.cuda.synchronize()
    assert edges.cpu().tolist() == [[-7, -7]] and keys.cpu().tolist() == [-7.0] and status.tolist() == [-7] * 4
    assert call(good, 2, need) == 0
    assert edges.cpu().numpy().tolist() == case["edges"].tolist() and status.tolist() == [1, 200, 200, 0]


# ------------------------------------------------------------------------------------------------ bridges of a graph
_graph_runs = {}


def _graph_run(name):
    """The product's graph of a case and its bridged version (connectivity mode), once per process."""
    if name not in _graph_runs:
        from vqvae_amd.geo.knn_graph_optimized import bridge_components_device, connected_components_device, knn_graph_device
        case = bc.graph_case(name)
        z = _dev(case["z"])
        G, _, _ = knn_graph_device(z, case["k"], mode="connectivity", sym=case["sym"])
        C, labels = connected_components_device(G)
        assert C == case["C"]
        np.testing.assert_array_equal(labels.cpu().numpy(), case["labels"])
        G2, edges, keys, info = bridge_components_device(G, z, mode="connectivity")
        _graph_runs[name] = (z, G, G2, edges, keys, info)
    return _graph_runs[name]


@pytest.mark.parametrize("name", bc.GRAPH_CASES)
def test_bridges_of_a_graph(name):
    from vqvae_amd.geo import dijkstra_multi_source
    case = bc.graph_case(name)
    z, G, G2, edges, keys, info = _graph_run(name)
    C = case["C"]
    e, k = edges.cpu().numpy(), keys.cpu().numpy()
    np.testing.assert_array_equal(e, case["edges"])
    np.testing.assert_array_equal(_bits(k), _bits(case["keys"]))
    assert np.lexsort((e[:, 1], e[:, 0], k)).tolist() == list(range(C - 1))
    assert info["components"] == C and 1 <= info["rounds"] <= math.ceil(math.log2(C))
    assert info["queries_first_round"] == len(case["z"]) - bc.GRAPH_COMPONENTS[name][1]
    # exactly the old entries plus the 2 (C - 1) new ones
    W, W2 = G.to_scipy(), G2.to_scipy()
    _canonical(W2)
    assert W2.nnz == W.nnz + 2 * (C - 1) and W2.dtype == np.float32
    B = sparse.csr_matrix((np.ones(2 * (C - 1), np.float32), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=W.shape)
    assert W.multiply(B).nnz == 0                                   # no bridge was a stored pair
    assert (abs(W2 - (W + B))).nnz == 0
    assert sparse.csgraph.connected_components(W2, directed=False)[0] == 1
    D = dijkstra_multi_source(W2, [0, len(case["z"]) - 1])
    assert np.isfinite(D).all()


@pytest.mark.parametrize("name", ["blobs_d5", "giant_plus_outliers"])
def test_bridges_do_not_depend_on_workspace_stream_or_run(name):
    from vqvae_amd.geo.knn_graph_optimized import bridge_edges_device
    case = bc.graph_case(name)
    z, G, G2, edges, keys, info = _graph_run(name)
    labels = _dev(case["labels"])
    runs = [bridge_edges_device(z, labels, case["C"]),                                    # the minimum workspace, again
            bridge_edges_device(z, labels, case["C"], extra_workspace_bytes=3 << 20)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(bridge_edges_device(z, labels, case["C"]))
    side.synchronize()
    for e, k, i in runs:
        assert torch.equal(e, edges) and torch.equal(k.view(torch.int64), keys.view(torch.int64)) and i == info


def test_distance_mode_weights_and_duplicates():
    """Distance mode stores float32(sqrt(key)); duplicate rows in different components get FLT_MIN, a stored entry."""
    from vqvae_amd.geo.knn_graph_optimized import bridge_components_device
    from vqvae_amd._device import DeviceCSR
    r = np.random.RandomState(9)
    z = r.randn(70, 5).astype(np.float32)
    z[40] = z[3]                                                      # a duplicate across the two components
    rows = np.r_[np.arange(0, 34), np.arange(35, 69)]                 # two paths: 0..34 and 35..69
    w = np.linalg.norm(z[rows] - z[rows + 1], axis=1).astype(np.float32)
    W = sparse.csr_matrix((np.r_[w, w], (np.r_[rows, rows + 1], np.r_[rows + 1, rows])), shape=(70, 70))
    W.sort_indices()
    G2, edges, keys, info = bridge_components_device(DeviceCSR.from_scipy(W, torch.device(DEV)), _dev(z), mode="distance")
    assert edges.cpu().tolist() == [[3, 40]] and keys.cpu().tolist() == [0.0] and info["components"] == 2
    W2 = G2.to_scipy()
    _canonical(W2)
    assert W2.nnz == W.nnz + 2 and W2[3, 40] == W2[40, 3] == np.finfo(np.float32).tiny
    z[40] += 0.25                                                      # no duplicate: the plain distance
    labels = np.repeat([0, 1], 35).astype(np.int32)
    ref_e, ref_k = bc.kruskal(z, labels, 0)
    G2, edges, keys, _ = bridge_components_device(DeviceCSR.from_scipy(W, torch.device(DEV)), _dev(z), mode="distance")
    assert edges.cpu().numpy().tolist() == ref_e.tolist() and _bits(keys.cpu().numpy()).tolist() == _bits(ref_k).tolist()
    a, b = ref_e[0]
    assert G2.to_scipy()[a, b] == np.float32(np.sqrt(ref_k[0]))


def test_connected_graph_is_returned_unchanged():
    from vqvae_amd.geo import connect_components
    from vqvae_amd.geo.knn_graph_optimized import bridge_components_device, knn_graph_device
    z = _dev(np.random.RandomState(2).randn(300, 8).astype(np.float32))
    G, _, _ = knn_graph_device(z, 12, mode="connectivity", sym="union")
    G2, edges, keys, info = bridge_components_device(G, z)
    assert G2 is G and edges.shape == (0, 2) and keys.numel() == 0
    assert info == {"components": 1, "rounds": 0, "queries_first_round": 0, "queries": 0}
    # the scipy wrapper on a disconnected distance graph
    case = bc.graph_case("blobs_d16")
    from oracle import knn as ok
    W, _ = ok.build_knn_graph(case["z"], k=case["k"], mode="distance", sym=case["sym"])
    W2, winfo = connect_components(W, case["z"], mode="distance")
    np.testing.assert_array_equal(winfo["edges"], case["edges"])
    assert winfo["components"] == case["C"] and W2.nnz == W.nnz + 2 * (case["C"] - 1)
    e = case["edges"]
    got = np.asarray(W2[e[:, 0], e[:, 1]]).ravel()
    want = np.sqrt(case["keys"]).astype(np.float32)
    np.testing.assert_array_equal(got, np.where(want == 0, np.finfo(np.float32).tiny, want))
    assert sparse.csgraph.connected_components(W2, directed=False)[0] == 1


# ------------------------------------------------------------------------------------------------ CSR insertion on its own
def _insert_case():
    # rows 0 and 9 are empty; row 4 holds columns 2, 5, 7
    r = np.array([1, 2, 2, 4, 4, 4, 5, 7, 3, 6])
    c = np.array([2, 1, 4, 2, 5, 7, 4, 4, 6, 3])
    v = (np.arange(10) + 2).astype(np.float32)
    W = sparse.csr_matrix((v, (r, c)), shape=(10, 10))
    W.sort_indices()
    return W


def test_csr_insert_merges_edges():
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.knn_graph_optimized import csr_insert_device
    W = _insert_case()
    # into two empty rows; before the first column of row 4; behind its last; between; a stored pair (both directions known);
    # the same edge twice (its first weight counts)
    src = np.array([0, 4, 4, 4, 2, 8, 8], np.int32)
    dst = np.array([9, 0, 8, 6, 4, 1, 1], np.int32)
    w = np.array([0.5, 1.5, 2.5, 3.5, 99.0, 4.5, 77.0], np.float32)
    G2 = csr_insert_device(DeviceCSR.from_scipy(W, torch.device(DEV)), _dev(src), _dev(dst), _dev(w))
    want = W.tolil()
    for a, b, x in [(0, 9, 0.5), (4, 0, 1.5), (4, 8, 2.5), (4, 6, 3.5), (8, 1, 4.5)]:
        want[a, b] = x
        want[b, a] = x
    want = want.tocsr()
    want.sort_indices()
    got = G2.to_scipy()
    assert got.indptr.tolist() == want.indptr.tolist() and got.indices.tolist() == want.indices.tolist()
    assert got.data.tolist() == want.data.astype(np.float32).tolist()
    assert got[2, 4] == W[2, 4] and got[4, 2] == W[4, 2]
    # no edge: a copy; a graph without data: ones
    G0 = csr_insert_device(DeviceCSR.from_scipy(W, torch.device(DEV)), _dev(src[:0]), _dev(dst[:0]), _dev(w[:0]))
    assert (abs(G0.to_scipy() - W)).nnz == 0 and G0.nnz == W.nnz
    G1 = csr_insert_device(DeviceCSR.from_scipy(W, torch.device(DEV), with_data=False), _dev(src[:1]), _dev(dst[:1]), _dev(w[:1]))
    assert sorted(G1.to_scipy().data.tolist()) == sorted([1.0] * W.nnz + [0.5, 0.5])


@pytest.mark.parametrize("src,dst", [([0, 3], [9, 3]), ([0, 10], [9, 1]), ([0, -1], [9, 1]), ([0, 1], [9, 10])])
def test_csr_insert_refuses_bad_edges_before_writing(src, dst):
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, ptr, stream_ptr
    lib = _lib.load()
    G = DeviceCSR.from_scipy(_insert_case(), torch.device(DEV))
    indptr_new = torch.full((11,), -7, dtype=torch.int32, device=DEV)
    nnz = np.full(1, -7, np.int64)
    ws = torch.empty(lib.geo_csr_insert_workspace_bytes(10, 2), dtype=torch.uint8, device=DEV)
    rc = lib.geo_csr_insert_count(ptr(G.indptr), ptr(G.indices), 10, ptr(_dev(np.array(src, np.int32))), ptr(_dev(np.array(dst, np.int32))),
                                  ptr(_dev(np.ones(2, np.float32))), 2, ptr(indptr_new), nnz.ctypes.data, ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and nnz[0] == -7 and indptr_new.cpu().tolist() == [-7] * 11


# ------------------------------------------------------------------------------------------------ the build and its CLI
def _write_inputs(tmp, d, seed, n_img):
    """A tiny decoder checkpoint and clustered spatial latents (4 x 4 cells per image)."""
    from oracle import metric as om
    sd = om.make_decoder_state(seed, d, 1, norm_type="batch")
    r = np.random.RandomState(seed)
    ctr = r.randn(10, d).astype(np.float32) * 4
    zf = (ctr[r.randint(0, 10, n_img * 16)] + 0.5 * r.randn(n_img * 16, d)).astype(np.float32)
    z4 = np.ascontiguousarray(np.transpose(zf.reshape(n_img, 4, 4, d), (0, 3, 1, 2)))
    state = {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    torch.save({"model_state_dict": state, "epoch": 0}, os.path.join(tmp, "best.pt"))
    torch.save(torch.from_numpy(z4), os.path.join(tmp, "z.pt"))
    return zf


def test_cli_connect_components(tmp_path):
    """--connect_components: every latent gets a code, the saved graph is the whole graph, bridges.json holds the oracle's
    edges.  Without the flag: the three artefacts of a build that never heard of the flag, and no bridges.json."""
    from oracle import knn as ok
    from vqvae_amd.scripts.build_codebook import build_codebook_device, main, make_parser
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    tmp = str(tmp_path)
    n_img, d = 40, 8
    zf = _write_inputs(tmp, d, 13, n_img)
    n = n_img * 16

    def build(name, extra):
        out = os.path.join(tmp, name)
        main(make_parser().parse_args([
            "--latents_path", os.path.join(tmp, "z.pt"), "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
            "--in_channels", "1", "--output_image_size", "28", "--latent_dim", str(d), "--enc_channels", "64", "128", "256",
            "--dec_channels", "256", "128", "64", "--recon_loss", "mse", "--norm_type", "batch", "--mse_use_sigmoid",
            "--k", "3", "--sym", "mutual", "--K", "8", "--init", "kpp", "--seed", "42", "--batch_size", "256"] + extra))
        return out

    plain, bridged = build("plain", []), build("bridged", ["--connect_components"])
    names = ["codebook.pt", "codes.npy", "knn_graph_geodesic.npz"]
    assert sorted(os.listdir(plain)) == names and sorted(os.listdir(bridged)) == sorted(names + ["bridges.json"])
    # the oracle's bridges of the oracle's graph
    W, _ = ok.build_knn_graph(zf, k=3, mode="connectivity", sym="mutual")
    C, labels = ok.connected_components(W)
    assert C > 1
    ref_e, ref_k = bc.kruskal(zf, labels, bc.key_form(d))
    bj = json.load(open(os.path.join(bridged, "bridges.json")))
    assert bj["connect_components"] is True and bj["components"] == C and 1 <= bj["rounds"] <= math.ceil(math.log2(C))
    assert bj["edges"] == ref_e.tolist() and _bits(np.array(bj["keys"])).tolist() == _bits(ref_k).tolist()
    assert len(bj["lengths"]) == C - 1 and all(x > 0 for x in bj["lengths"])
    codes_b, codes_p = np.load(os.path.join(bridged, "codes.npy")), np.load(os.path.join(plain, "codes.npy"))
    assert codes_b.shape == (n_img, 4, 4) and codes_b.dtype == np.int32 and (codes_b >= 0).all() and (codes_p == -1).any()
    W_b = sparse.load_npz(os.path.join(bridged, "knn_graph_geodesic.npz"))
    assert W_b.shape == (n, n) and W_b.nnz == W.nnz + 2 * (C - 1)
    assert sparse.csgraph.connected_components(W_b, directed=False)[0] == 1
    got = np.asarray(W_b[ref_e[:, 0], ref_e[:, 1]]).ravel()
    assert got.tolist() == np.array(bj["lengths"], np.float32).tolist()
    cb_b = torch.load(os.path.join(bridged, "codebook.pt"), weights_only=False)
    cb_p = torch.load(os.path.join(plain, "codebook.pt"), weights_only=False)
    assert list(cb_b["config"].keys()) == list(cb_p["config"].keys()) and list(cb_b.keys()) == list(cb_p.keys())
    # without the flag: what build_codebook_device gives when the argument is never named
    dec = load_decoder_from_checkpoint(os.path.join(tmp, "best.pt"), in_channels=1, dec_channels=[256, 128, 64], latent_dim=d,
                                       output_image_size=28, norm_type="batch", device=torch.device(DEV))
    res = build_codebook_device(_dev(zf), dec, k=3, sym="mutual", K=8, init="kpp", seed=42, batch_size=256)
    assert "bridges" not in res
    assert codes_p.tobytes() == res["assign_flat"].reshape(n_img, 4, 4).tobytes()
    W_p, W_r = sparse.load_npz(os.path.join(plain, "knn_graph_geodesic.npz")), res["W_lcc"].to_scipy()
    for part in ("indptr", "indices", "data"):
        assert getattr(W_p, part).tobytes() == getattr(W_r, part).tobytes()
    assert cb_p["medoid_indices"].tobytes() == res["medoids"].astype(np.int32).tobytes()
    assert torch.equal(cb_p["z_medoid"], res["z_medoid"].float())
    assert W_p.shape[0] < n                                           # the plain build kept the largest component only

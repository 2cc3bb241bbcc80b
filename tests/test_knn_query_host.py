"""Host side of the held-out search: the assign_codes_val_geodesic parser, the LCC-row reconstruction from codes.npy, the
flattening of held-out latents and the ValueErrors of kneighbors / knn_query_device, all without a GPU."""
import numpy as np
import pytest
import torch


def test_parser_defaults_and_required_flags():
    from vqvae_amd.training.assign_codes_val_geodesic import make_parser
    p = make_parser()
    a = p.parse_args(["--codebook_dir", "cb", "--latents_path", "z.pt", "--out_dir", "out"])
    assert (a.codebook_dir, a.latents_path, a.out_dir) == ("cb", "z.pt", "out")
    assert a.k == 20 and a.metric == "riemannian" and a.batch_size == 512 and a.train_latents_path is None
    a = p.parse_args(["--codebook_dir", "cb", "--latents_path", "z.pt", "--out_dir", "out", "--k", "5", "--metric", "euclidean",
                      "--batch_size", "64", "--train_latents_path", "t.pt"])
    assert a.k == 5 and a.metric == "euclidean" and a.batch_size == 64 and a.train_latents_path == "t.pt"
    for argv in (["--latents_path", "z.pt", "--out_dir", "out"], ["--codebook_dir", "cb", "--out_dir", "out"],
                 ["--codebook_dir", "cb", "--latents_path", "z.pt"],
                 ["--codebook_dir", "cb", "--latents_path", "z.pt", "--out_dir", "out", "--metric", "cosine"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_lcc_rows_from_codes():
    from vqvae_amd.training.assign_codes_val_geodesic import lcc_rows
    codes = np.array([[[3, -1], [0, 2]], [[-1, -1], [1, 0]]], dtype=np.int32)          # (N, h, w) = (2, 2, 2)
    np.testing.assert_array_equal(lcc_rows(codes), [0, 2, 3, 6, 7])
    np.testing.assert_array_equal(lcc_rows(np.array([-1, -1])), [])
    np.testing.assert_array_equal(lcc_rows(np.zeros((2, 1, 3), np.int32)), np.arange(6))


def test_flatten_latents_takes_n_h_w_order():
    from vqvae_amd.training.assign_codes_val_geodesic import flatten_latents
    z = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2)
    f = flatten_latents(z)
    assert f.shape == (8, 3) and f.is_contiguous()
    for n in range(2):
        for h in range(2):
            for w in range(2):
                assert torch.equal(f[(n * 2 + h) * 2 + w], z[n, :, h, w])
    z2 = torch.randn(5, 3)
    assert torch.equal(flatten_latents(z2), z2)
    with pytest.raises(ValueError):
        flatten_latents(torch.zeros(2, 3, 4))


def test_load_build_refuses_pieces_that_do_not_belong_together(tmp_path):
    from scipy import sparse
    from vqvae_amd.training.assign_codes_val_geodesic import load_build
    z = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2)
    torch.save(z, tmp_path / "z.pt")
    codes = np.array([[[1, -1], [0, 1]], [[-1, 0], [1, 0]]], dtype=np.int32)
    np.save(tmp_path / "codes.npy", codes)
    sparse.save_npz(tmp_path / "knn_graph_geodesic.npz", sparse.csr_matrix(np.ones((6, 6), np.float32) - np.eye(6, dtype=np.float32)))
    flat = z.permute(0, 2, 3, 1).reshape(-1, 3)
    rows = [0, 2, 3, 5, 6, 7]
    med = np.array([4, 1], dtype=np.int32)
    good = {"medoid_indices": med, "z_medoid": flat[rows][[4, 1]].clone(), "config": {"latents_path": str(tmp_path / "z.pt")}}
    torch.save(good, tmp_path / "codebook.pt")
    cb, W, z_lcc = load_build(tmp_path)
    assert W.shape == (6, 6) and torch.equal(z_lcc, flat[rows]) and list(cb["medoid_indices"]) == [4, 1]
    bad = dict(good, z_medoid=good["z_medoid"] + 1.0)
    torch.save(bad, tmp_path / "codebook.pt")
    with pytest.raises(ValueError, match="do not belong together"):
        load_build(tmp_path)
    torch.save(dict(good, medoid_indices=np.array([6, 1], dtype=np.int32)), tmp_path / "codebook.pt")
    with pytest.raises(ValueError, match="do not belong together"):
        load_build(tmp_path)
    torch.save(good, tmp_path / "codebook.pt")
    torch.save(z[:1], tmp_path / "short.pt")
    with pytest.raises(ValueError, match="do not belong together"):
        load_build(tmp_path, train_latents_path=str(tmp_path / "short.pt"))


def test_kneighbors_value_errors_need_no_gpu(monkeypatch):
    from vqvae_amd import _lib
    from vqvae_amd.geo import kneighbors, knn_query_device

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    z, q = np.zeros((10, 4), np.float32), np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="not supported"):
        kneighbors(z, q, 2, metric="cosine")
    with pytest.raises(ValueError, match="columns"):
        kneighbors(z, np.zeros((3, 5), np.float32), 2)
    with pytest.raises(ValueError, match="2-D"):
        kneighbors(z, np.zeros(4, np.float32), 2)
    for k in (0, 11, 257):
        with pytest.raises(ValueError, match="n_neighbors"):
            kneighbors(z, q, k)
    with pytest.raises(ValueError, match="n_neighbors"):
        kneighbors(np.zeros((300, 4), np.float32), q, 257)
    with pytest.raises(ValueError, match="dimension"):
        kneighbors(np.zeros((10, 129), np.float32), np.zeros((3, 129), np.float32), 2)
    zt, qt = torch.zeros(10, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="n_neighbors"):
        knn_query_device(zt, qt, 11)
    with pytest.raises(ValueError, match="float32"):
        knn_query_device(zt.double(), qt.double(), 2)
    with pytest.raises(ValueError, match="columns"):
        knn_query_device(zt, torch.zeros(3, 5), 2)

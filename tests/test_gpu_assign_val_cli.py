"""python -m vqvae_amd.training.assign_codes_val_geodesic end to end: a codebook built by the build_codebook CLI on 128 seeded
16 x 4 x 4 latents (2 048 nodes, the C1 shape) with a seeded 28-px decoder, then 8 held-out images through the new CLI."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu

D, COUT, SIZE, N_IMG, N_VAL = 16, 1, 28, 128, 8
JSON_KEYS = ["k", "knn_path", "metric", "n_latents", "quantization_error", "unreachable"]


def _build(tmp, name, seed):
    """One build_codebook run in tmp/name on latents of the given seed (the decoder checkpoint is shared)."""
    from vqvae_amd.scripts.build_codebook import main, make_parser
    os.makedirs(os.path.join(tmp, name))
    z4 = np.random.RandomState(seed).randn(N_IMG * 16, D).astype(np.float32).reshape(N_IMG, 4, 4, D)
    z_path = os.path.join(tmp, name, "z.pt")
    torch.save(torch.from_numpy(np.ascontiguousarray(np.transpose(z4, (0, 3, 1, 2)))), z_path)
    out = os.path.join(tmp, name, "codebook")
    main(make_parser().parse_args([
        "--latents_path", z_path, "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
        "--in_channels", str(COUT), "--output_image_size", str(SIZE), "--latent_dim", str(D),
        "--enc_channels", "64", "128", "256", "--dec_channels", "256", "128", "64", "--recon_loss", "mse",
        "--norm_type", "batch", "--mse_use_sigmoid", "--k", "20", "--sym", "union", "--K", "64", "--init", "kpp",
        "--seed", "42", "--batch_size", "512"]))
    return out


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    from oracle import metric as om
    tmp = str(tmp_path_factory.mktemp("assign_val"))
    sd = om.make_decoder_state(7, D, COUT, norm_type="batch")
    state = {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    torch.save({"model_state_dict": state, "epoch": 0}, os.path.join(tmp, "best.pt"))
    out = _build(tmp, "a", 7)
    other = _build(tmp, "b", 8)
    z_val = torch.from_numpy(np.random.RandomState(70).randn(N_VAL, D, 4, 4).astype(np.float32))
    torch.save(z_val, os.path.join(tmp, "z_val.pt"))
    return {"tmp": tmp, "codebook": out, "other": other, "z_val": os.path.join(tmp, "z_val.pt")}


def _cli(build, out_name, *extra, latents=None, codebook_dir=None):
    from vqvae_amd.training.assign_codes_val_geodesic import main, make_parser
    out = os.path.join(build["tmp"], out_name)
    main(make_parser().parse_args(["--codebook_dir", codebook_dir or build["codebook"], "--latents_path", latents or build["z_val"],
                                   "--out_dir", out, *extra]))
    return (np.load(os.path.join(out, "codes_val.npy")), np.load(os.path.join(out, "dist_val.npy")),
            json.load(open(os.path.join(out, "assign_val.json"))))


def _resident(build):
    """(z_new, z_lcc, G, medoids, codebook) on the GPU, put together as the CLI documents it."""
    from vqvae_amd._device import DeviceCSR, device
    dev = device()
    cb = torch.load(os.path.join(build["codebook"], "codebook.pt"), weights_only=False)
    codes = np.load(os.path.join(build["codebook"], "codes.npy"))
    W = sparse.load_npz(os.path.join(build["codebook"], "knn_graph_geodesic.npz"))
    z_train = torch.load(cb["config"]["latents_path"]).float().permute(0, 2, 3, 1).reshape(-1, D)
    z_lcc = z_train[torch.from_numpy(np.flatnonzero(codes.reshape(-1) >= 0))].contiguous().to(dev)
    z_new = torch.load(build["z_val"]).float().permute(0, 2, 3, 1).reshape(-1, D).contiguous().to(dev)
    return z_new, z_lcc, DeviceCSR.from_scipy(W, dev), cb["medoid_indices"], cb


def test_riemannian_cli_equals_the_direct_call(build):
    from vqvae_amd.geo import knn_query_device
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    from vqvae_amd.training.assign_codes_val_geodesic import assign_codes_geodesic
    codes, dist, summary = _cli(build, "val_riem")
    assert codes.dtype == np.int32 and codes.shape == (N_VAL, 4, 4) and dist.dtype == np.float32 and dist.shape == (N_VAL, 4, 4)
    z_new, z_lcc, G, med, cb = _resident(build)
    cfg = cb["config"]
    dec = load_decoder_from_checkpoint(cfg["vae_ckpt_path"], in_channels=COUT, dec_channels=cfg["dec_channels"], latent_dim=D,
                                       output_image_size=SIZE, norm_type="batch", device=z_lcc.device).eval()
    before = {k: v.clone() for k, v in dec.state_dict().items()}
    want = assign_codes_geodesic(z_new, z_lcc, G, med, decoder=dec, batch_size=512,
                                 neighbors=knn_query_device(z_lcc, z_new, 20, form=0))
    for k, v in dec.state_dict().items():                          # eval(): attachment batches move no BatchNorm statistic
        assert torch.equal(v, before[k]), k
    np.testing.assert_array_equal(codes.reshape(-1), want["codes"].cpu().numpy().astype(np.int32))
    np.testing.assert_array_equal(dist.reshape(-1).view(np.int32), want["dist"].cpu().numpy().view(np.int32))
    assert sorted(summary) == JSON_KEYS
    finite = np.isfinite(dist)
    assert summary["n_latents"] == N_VAL * 16 and summary["k"] == 20 and summary["metric"] == "riemannian"
    assert summary["knn_path"] == 1                                # 2 048 nodes: the exact scan
    assert summary["unreachable"] == int((~finite).sum())
    assert summary["quantization_error"] == float(np.sum(dist[finite] ** 2))
    assert (codes >= 0).all() and (codes < 64).all()


def test_euclidean_cli_equals_the_torch_search_path(build):
    from vqvae_amd.geo import knn_query_device
    from vqvae_amd.training.assign_codes_val_geodesic import assign_codes_geodesic, attach_neighbors_device
    codes, dist, summary = _cli(build, "val_euc", "--metric", "euclidean")
    z_new, z_lcc, G, med, _ = _resident(build)
    idx_t, _ = attach_neighbors_device(z_new, z_lcc, 20)
    idx_k, _ = knn_query_device(z_lcc, z_new, 20, form=0)
    assert torch.equal(idx_t, idx_k), "the torch search and knn_query_device(form=0) rank some attachment differently"
    want = assign_codes_geodesic(z_new, z_lcc, G, med, k=20)       # the default path: torch search, Euclidean lengths
    np.testing.assert_array_equal(codes.reshape(-1), want["codes"].cpu().numpy().astype(np.int32))
    np.testing.assert_array_equal(dist.reshape(-1).view(np.int32), want["dist"].cpu().numpy().view(np.int32))
    assert sorted(summary) == JSON_KEYS and summary["metric"] == "euclidean"


def test_copies_of_graph_nodes_get_the_nodes_code(build):
    """2-D held-out latents that are copies of graph nodes, attached with k = 1: the one attachment is the node itself at
    length 0 (no two nodes of these Gaussian latents coincide), so the code is the node's training code.  (A longer list adds
    Euclidean attachment edges to a graph whose own edges carry pull-back lengths: the node's code is then likely, not
    certain, so nothing is asserted for it.)"""
    _, z_lcc, _, _, _ = _resident(build)
    codes_train = np.load(os.path.join(build["codebook"], "codes.npy")).reshape(-1)
    codes_lcc = codes_train[codes_train >= 0]
    rows = np.random.RandomState(3).choice(z_lcc.shape[0], size=50, replace=False)
    path = os.path.join(build["tmp"], "z_copies.pt")
    torch.save(z_lcc[torch.from_numpy(rows).to(z_lcc.device)].cpu(), path)
    codes, dist, summary = _cli(build, "val_copies", "--metric", "euclidean", "--k", "1", latents=path)
    assert codes.shape == (50,) and dist.shape == (50,) and summary["n_latents"] == 50 and summary["k"] == 1
    np.testing.assert_array_equal(codes, codes_lcc[rows])


def test_a_codebook_of_another_build_is_refused(build):
    """codebook.pt of build b next to the graph and codes of build a, searched over a's training latents."""
    mixed = os.path.join(build["tmp"], "mixed")
    shutil.copytree(build["codebook"], mixed)
    shutil.copy(os.path.join(build["other"], "codebook.pt"), os.path.join(mixed, "codebook.pt"))
    with pytest.raises(ValueError, match="do not belong together"):
        _cli(build, "val_mixed", "--train_latents_path", os.path.join(build["tmp"], "a", "z.pt"), codebook_dir=mixed)
    assert not os.path.exists(os.path.join(build["tmp"], "val_mixed"))

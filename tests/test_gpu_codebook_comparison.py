"""The codebook-comparison CLI (vqvae_amd.scripts.codebook_comparison) end to end on a seeded vanilla-VAE checkpoint."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"reconstruction_mse", "perplexity", "quantization_error", "valid_samples"}


def _experiment(tmp_path, n=2000, d=128):
    from vqvae_amd.vae import Decoder
    torch.manual_seed(0)
    dec = Decoder(1, (256, 128, 64), d, 28, "batch")
    for m in dec.modules():                           # non-trivial running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    state = {"decoder." + k: v for k, v in dec.state_dict().items()}
    state["encoder.dummy"] = torch.zeros(1)
    exp = tmp_path / "exp_seeded"
    (exp / "vae" / "run0" / "checkpoints").mkdir(parents=True)
    (exp / "vae" / "run0" / "latents_val").mkdir(parents=True)
    cfg = {"in_channels": 1, "latent_dim": d, "dec_channels": [256, 128, 64], "output_image_size": 28, "norm_type": "batch"}
    torch.save({"model_state_dict": state, "config": cfg}, exp / "vae" / "run0" / "checkpoints" / "best.pt")
    r = np.random.RandomState(1)
    cen = r.randn(12, d) * 2
    z = (cen[r.randint(0, 12, n)] + 0.7 * r.randn(n, d)).astype(np.float32)
    torch.save({"z": torch.from_numpy(z)}, exp / "vae" / "run0" / "latents_val" / "z.pt")
    return exp, dec, z


def test_codebook_comparison_cli(tmp_path):
    exp, dec, z = _experiment(tmp_path)
    K, k_graph, seed = 32, 10, 7
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "vqvae_amd.scripts.codebook_comparison", str(exp),
                        "--K", str(K), "--k_graph", str(k_graph), "--seed", str(seed)],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    outs = list((tmp_path / "demo_outputs").glob("codebook_comparison_exp_seeded_*"))
    assert len(outs) == 1
    out = outs[0]
    metrics = json.loads((out / "metrics.json").read_text())
    assert set(metrics) == {"euclidean", "geodesic"}
    assert set(metrics["euclidean"]) == KEYS and set(metrics["geodesic"]) == KEYS
    assert (out / "config.yaml").exists()
    try:
        import matplotlib  # noqa: F401
        assert (out / "codebook_comparison.png").stat().st_size > 0
    except ImportError:
        pass

    dev = torch.device("cuda", 0)
    dec = dec.to(dev).eval()

    def mse(a, b):
        with torch.no_grad():
            return torch.nn.functional.mse_loss(torch.sigmoid(dec(torch.from_numpy(b).to(dev))),
                                                torch.sigmoid(dec(torch.from_numpy(a).to(dev)))).item()

    def ppl(assign):
        p = np.bincount(assign, minlength=K) / len(assign)
        p = p[p > 0]
        return float(np.exp(-np.sum(p * np.log(p + 1e-12))))

    # Euclidean side: recomputed from the fitted codebook
    from vqvae_amd.cluster import KMeans
    km = KMeans(K, random_state=seed, n_init=10)
    a = km.fit_predict(z)
    assert km.path_ == "hip"
    zq = km.cluster_centers_[a]
    e = metrics["euclidean"]
    assert e["valid_samples"] == len(z)
    np.testing.assert_allclose(e["reconstruction_mse"], mse(z, zq), rtol=1e-6)
    assert e["perplexity"] == pytest.approx(ppl(a), rel=1e-12)
    qe = float(((torch.from_numpy(z).double() - torch.from_numpy(zq).double()) ** 2).sum(1).mean())
    np.testing.assert_allclose(e["quantization_error"], qe, rtol=1e-5)

    # geodesic side: direct calls to the vqvae_amd.geo API
    from vqvae_amd.geo import build_knn_graph, dijkstra_multi_source
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_optimized
    from vqvae_amd.geo.knn_graph_optimized import largest_connected_component
    W, _ = build_knn_graph(z, k=k_graph, metric="euclidean", mode="distance", sym="mutual")
    mask = largest_connected_component(W)
    W_lcc = W[mask][:, mask] if mask.sum() < W.shape[0] else W
    med, a_lcc, _ = fit_kmedoids_optimized(W_lcc, K=K, init="kpp", seed=seed)
    g = metrics["geodesic"]
    assert g["valid_samples"] == int(mask.sum())
    z_lcc = z[mask]
    np.testing.assert_allclose(g["reconstruction_mse"], mse(z_lcc, z_lcc[med][a_lcc]), rtol=1e-6)
    assert g["perplexity"] == pytest.approx(ppl(a_lcc), rel=1e-12)
    D = dijkstra_multi_source(W_lcc, med)
    dmin = D[a_lcc, np.arange(len(a_lcc))]
    np.testing.assert_allclose(g["quantization_error"], float(np.mean(dmin[np.isfinite(dmin)] ** 2)), rtol=1e-6)

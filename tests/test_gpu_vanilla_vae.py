"""The vanilla VAE on the MI355X: one optimisation step with the HIP ELBO against the torch ELBO, checkpoint loading and
resident encoding against the reference's outputs, the Euclidean legacy builder against the reference's artefacts
(tests/golden/legacy_euclidean.npz) and a two-epoch run of the trainer."""
import os

import numpy as np
import pytest
import torch
from scipy import sparse

from test_vanilla_vae_host import CONFIGS, golden_model

pytestmark = pytest.mark.gpu


def fixed_eps(monkeypatch, eps):
    from vqvae_amd.vae import VAE
    monkeypatch.setattr(VAE, "reparameterize", staticmethod(lambda mu, logvar: mu + eps.to(mu.device) * torch.exp(0.5 * logvar)))


def one_step(g, name, device, native):
    """Gradients and AdamW-updated parameters of one training step of the golden model on the golden batch."""
    model = golden_model(g, name).to(device).train()
    model.native_loss = native
    model.free_bits_default, model.capacity_max_default = 0.25, 25.0
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    x = torch.from_numpy(g[f"{name}/x"]).to(device)
    x_logits, mu, logvar, _ = model(x)
    loss, _, _ = model.loss(x, x_logits, mu, logvar, beta=1.0, step=10)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}
    opt.step()
    return grads, {k: p.detach().double().cpu() for k, p in model.named_parameters()}


def gap(a, b):
    """Largest difference over all tensors, relative to the largest magnitude over all tensors of b (a per-tensor scale
    would compare rounding noise with rounding noise where a gradient is zero in exact arithmetic: a bias under batch norm)."""
    return max((a[k] - b[k]).abs().max().item() for k in b) / max(b[k].abs().max().item() for k in b)


@pytest.mark.parametrize("name", ["28px_batch", "32px_none"])
def test_one_step_with_hip_loss_matches_torch_loss(golden, monkeypatch, name):
    """The HIP-loss step may differ from the torch-loss step on the GPU by at most 4 x what the torch-loss step on the GPU
    differs from the same step on the CPU (two float32 implementations of the reference).  Measured figures: DESIGN.md
    section 13."""
    g = golden("vanilla_vae")
    fixed_eps(monkeypatch, torch.from_numpy(g[f"{name}/eps"]))
    hip_g, hip_p = one_step(g, name, "cuda", True)
    gpu_g, gpu_p = one_step(g, name, "cuda", False)
    cpu_g, cpu_p = one_step(g, name, "cpu", False)
    figures = {"grad hip-vs-torch": gap(hip_g, gpu_g), "grad gpu-vs-cpu": gap(gpu_g, cpu_g),
               "param hip-vs-torch": gap(hip_p, gpu_p), "param gpu-vs-cpu": gap(gpu_p, cpu_p)}
    print(name, figures)
    assert figures["grad gpu-vs-cpu"] > 0
    assert figures["grad hip-vs-torch"] <= 4 * figures["grad gpu-vs-cpu"], figures
    assert figures["param hip-vs-torch"] <= 4 * figures["param gpu-vs-cpu"], figures


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_load_vae_and_resident_encode_reproduce_the_golden_latents(golden, monkeypatch, tmp_path, name):
    from vqvae_amd.utils.latents import encode_latents_device
    from vqvae_amd.vae import load_vae
    g = golden("vanilla_vae")
    path = str(tmp_path / "best.pt")
    torch.save({"model_state_dict": golden_model(g, name).state_dict(), "epoch": 1}, path)
    model, cfg = load_vae(path, device="cuda")
    assert cfg["in_channels"] == CONFIGS[name]["in_channels"] and cfg["latent_dim"] == 4 and cfg["norm_type"] == CONFIGS[name]["norm_type"]
    eps = torch.from_numpy(g[f"{name}/eps"])
    fixed_eps(monkeypatch, eps)
    x = torch.from_numpy(g[f"{name}/x"])
    z, mu, logvar, y = encode_latents_device(model, [(x, torch.arange(5))], torch.device("cuda"))
    assert z.is_cuda and mu.is_cuda and logvar.is_cuda and not y.is_cuda and z.shape == (5, 4)
    for got, key in ((mu, "mu"), (logvar, "logvar")):
        want = g[f"{name}/{key}"]
        assert np.all(np.abs(got.cpu().numpy() - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), key
    want_z = mu.cpu() + eps * torch.exp(0.5 * logvar.cpu())
    assert torch.allclose(z.cpu(), want_z, rtol=1e-6, atol=1e-6)
    assert np.all(np.abs(z.cpu().numpy() - g[f"{name}/z"]) <= 2e-5 * np.maximum(1.0, np.abs(g[f"{name}/z"])))


@pytest.mark.parametrize("case", ["split", "connected"])
def test_euclidean_legacy_builder_artefacts_equal_reference(golden, tmp_path, case):
    from vqvae_amd.training.build_codebook_legacy import build_and_save
    g = golden("legacy_euclidean")
    tmp = str(tmp_path)
    torch.save(torch.from_numpy(g[f"{case}/z"]), os.path.join(tmp, "z.pt"))
    cfg = {"data": {"latents_path": os.path.join(tmp, "z.pt")},
           "graph": {"k": 10, "metric": "euclidean", "sym": "union", "mode": "connectivity"},
           "quantize": {"K": 16, "init": "kpp", "seed": 42}, "out": {"dir": os.path.join(tmp, "out")}}
    out = build_and_save(cfg)
    assert sorted(os.listdir(out)) == ["codebook.pt", "codes.npy", "knn_graph.npz"]
    W = sparse.load_npz(out / "knn_graph.npz").tocsr()
    W.sort_indices()
    np.testing.assert_array_equal(W.indptr, g[f"{case}/indptr"])
    np.testing.assert_array_equal(W.indices, g[f"{case}/indices"])
    np.testing.assert_array_equal(W.data, g[f"{case}/data"])
    cb = torch.load(out / "codebook.pt", weights_only=False)
    assert set(cb) == {"medoid_indices", "z_medoid", "config"} and cb["config"] == cfg
    assert cb["medoid_indices"].dtype == np.int32 and cb["z_medoid"].dtype == torch.float32
    np.testing.assert_array_equal(cb["medoid_indices"], g[f"{case}/medoid_indices"])
    np.testing.assert_array_equal(cb["z_medoid"].numpy(), g[f"{case}/z_medoid"])
    codes = np.load(out / "codes.npy")
    np.testing.assert_array_equal(codes, g[f"{case}/codes"])
    assert str(codes.dtype) == str(g[f"{case}/codes_dtype"])          # int32 with -1 when split, k-medoids' own array otherwise
    assert (codes < 0).any() == (case == "split")


def test_two_epoch_training_run_writes_the_reference_files(tmp_path):
    from vqvae_amd.eval.experiment import detect_layout, load_decoder
    from vqvae_amd.scripts.train_vanilla_vae import run
    from vqvae_amd.training.data import ResidentLoader, resident_images
    r = np.random.RandomState(0)
    images = r.randint(0, 256, (512, 28, 28)).astype(np.uint8)
    data = resident_images(images, r.randint(0, 10, 512), "cuda")
    val = resident_images(images[:100], np.arange(100) % 10, "cuda")
    out = tmp_path / "exp" / "vae"
    cfg = {"seed": 42, "device": "cuda", "max_epochs": 2, "lr": 3e-4, "weight_decay": 1e-4, "early_stop": 20, "optimizer": "adamw",
           "scheduler": {"name": "cosine"}, "grad_clip_max_norm": 1.0, "beta": 1.0, "out_dir": str(out), "save_latents": True,
           "mlflow_tracking_uri": str(tmp_path / "mlruns"), "experiment_name": "t", "run_name": "t",
           "model": dict(in_channels=1, output_image_size=28, latent_dim=8, enc_channels=[8, 16, 32], dec_channels=[32, 16, 8],
                         recon_loss="mse", norm_type="batch", mse_use_sigmoid=True, free_bits_default=0.25,
                         capacity_max_default=25.0, capacity_anneal_steps_default=100000, capacity_mode_default="abs")}
    run(cfg, loaders=(ResidentLoader(data, 128, True), ResidentLoader(val, 128, False)))
    for f in ("checkpoints/best.pt", "checkpoints/latest.pt", "recon_grid.png"):
        assert (out / f).exists(), f
    for split, n in (("latents_train", 512), ("latents_val", 100)):
        for f in ("z", "mu", "logvar"):
            t = torch.load(out / split / f"{f}.pt")
            assert t.shape == (n, 8) and t.dtype == torch.float32 and not t.is_cuda and torch.isfinite(t).all()
        assert torch.load(out / split / "y.pt").shape == (n,)
    try:
        import mlflow  # noqa: F401
    except ImportError:
        rows = (out / "metrics.csv").read_text().strip().splitlines()
        assert rows[0].startswith("step,train_loss,train_recon,train_kl,val_loss") and len(rows) == 3
        assert all(np.isfinite(float(v)) for v in rows[2].split(","))
    latest = torch.load(out / "checkpoints" / "latest.pt", weights_only=False)
    assert set(latest) == {"model_state_dict", "epoch"} and latest["epoch"] == 2
    paths = detect_layout(str(tmp_path / "exp"))
    assert paths.layout == "vanilla"
    decoder, dcfg = load_decoder(paths, None, torch.device("cuda"))
    assert dcfg["latent_dim"] == 8 and decoder(torch.zeros(2, 8, device="cuda")).shape == (2, 1, 28, 28)

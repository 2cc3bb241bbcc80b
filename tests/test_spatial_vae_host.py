"""Spatial VAE training on the host: the torch-path `SpatialVAE.loss` against tests/golden/spatial_vae.npz (the reference's own
values and gradients, tools/gen_golden_spatial_vae.py), the SpatialTrainingEngine on the CPU and the train_vae command line.
Loss and golden are the same float32 torch CPU operations in the same order, so the comparisons are exact."""
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

CASES = ("bce_28", "mse_log_32", "mse_sig_32", "one_28")
TINY = dict(enc_channels=[4, 8, 8], dec_channels=[8, 8, 8], latent_dim=2, norm_type="batch")


def tiny_model(in_channels=1, size=28, recon_loss="bce", mse_use_sigmoid=True):
    from vqvae_amd.spatial_vae import SpatialVAE
    return SpatialVAE(in_channels=in_channels, output_image_size=size, recon_loss=recon_loss, mse_use_sigmoid=mse_use_sigmoid, **TINY)


def case_model(g, name):
    mode = int(g[f"{name}/recon_mode"])
    x = g[f"{name}/x"]
    return tiny_model(x.shape[1], x.shape[2], "bce" if mode == 0 else "mse", mode != 2)


def loss_and_grads(model, g, name, beta, device="cpu", dtype=torch.float32, **kw):
    """((total, recon, kl) tensors, [d_x_logits, d_mu, d_logvar]) of one loss call on a golden case."""
    x, logits, mu, logvar = (torch.from_numpy(g[f"{name}/{k}"]).to(device=device, dtype=dtype) for k in ("x", "x_logits", "mu", "logvar"))
    leaves = [t.requires_grad_(True) for t in (logits, mu, logvar)]
    triple = model.loss(x, leaves[0], leaves[1], leaves[2], beta=beta, **kw)
    triple[0].backward()
    return [t.detach() for t in triple], [t.grad for t in leaves]


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", CASES)
def test_cpu_loss_reproduces_the_golden_values_and_gradients(golden, one_thread, name):
    g = golden("spatial_vae")
    model = case_model(g, name)
    assert g[f"{name}/mu"].shape == (1 if name == "one_28" else 3, 2, 4, 4) and list(g["betas"]) == [0.0, 0.25, 1.0]
    assert np.abs(g[f"{name}/logvar"]).max() >= 8.0
    for i, beta in enumerate(g["betas"]):
        triple, grads = loss_and_grads(model, g, name, float(beta), step=3)
        assert [float(v) for v in triple] == [float(v) for v in g[f"{name}/triples"][i]], (name, beta)
        np.testing.assert_array_equal(grads[0].numpy(), g[f"{name}/d_x_logits"])
        np.testing.assert_array_equal(grads[1].numpy(), g[f"{name}/d_mu"][i])
        np.testing.assert_array_equal(grads[2].numpy(), g[f"{name}/d_logvar"][i])
        triple64, _ = loss_and_grads(model, g, name, float(beta), dtype=torch.float64)
        assert [float(v) for v in triple64] == list(g[f"{name}/triples_f64"][i])
        assert float(triple64[0]) == pytest.approx(float(triple64[1]) + beta * float(triple64[2]), rel=1e-15)


def test_loss_ignores_extra_keywords_and_keeps_the_reference_attributes(golden):
    g = golden("spatial_vae")
    model = case_model(g, "bce_28")
    assert model._step == 0
    plain, _ = loss_and_grads(model, g, "bce_28", 0.25)
    extra, _ = loss_and_grads(model, g, "bce_28", 0.25, step=7, free_bits=0.5, anything="else")
    assert [float(v) for v in plain] == [float(v) for v in extra] and model._step == 0
    with pytest.raises(TypeError):
        model.loss(*(torch.zeros(1) for _ in range(4)))                  # beta has no default, as in the reference


class _Recorder:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step=None):
        self.rows.append((step, dict(metrics)))

    def log_artifact(self, path):
        self.artifact = path


def _loaders(n=24, batch=8):
    r = torch.Generator().manual_seed(3)
    x = torch.rand(n, 1, 28, 28, generator=r)
    y = torch.arange(n) % 10
    return [(x[s:s + batch], y[s:s + batch]) for s in range(0, n, batch)]


def test_spatial_engine_runs_on_the_cpu(tmp_path):
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    from vqvae_amd.training.engine import TrainingEngine
    from vqvae_amd.training.spatial_engine import SpatialTrainingEngine
    torch.manual_seed(1)
    model = tiny_model()
    engine = SpatialTrainingEngine(model=model, optimizer=torch.optim.AdamW(model.parameters(), lr=1e-3), device=torch.device("cpu"))
    assert isinstance(engine, TrainingEngine)                           # one loop: only the latent writer differs
    loader = _loaders()
    got = engine.run_epoch(loader, train=True, epoch=1, num_epochs=1, beta=1.0, grad_clip_max_norm=1.0, global_step_start=4)
    assert len(got) == 6 and got[3] == 7 and got[4:] == (0, 0) and all(np.isfinite(got[:3]))
    got = engine.run_epoch(loader, train=False, epoch=1, num_epochs=1, beta=1.0, global_step_start=7)
    assert len(got) == 6 and got[3] == 7 and 0 < got[4] < 40 and 0 <= got[5] <= 1

    log = _Recorder()
    out = Path(tmp_path) / "run"
    assert engine.train(loader, loader, num_epochs=2, early_stop=0, checkpoint_dir=out / "checkpoints", logger=log, output_dir=out,
                        save_latents_flag=True, beta=0.5, grad_clip_max_norm=1.0) is None
    assert [s for s, _ in log.rows] == [1, 2] and log.rows[0][1]["beta"] == 0.5
    best = torch.load(out / "checkpoints" / "best.pt", weights_only=False)
    latest = torch.load(out / "checkpoints" / "latest.pt", weights_only=False)
    assert set(best) == {"model_state_dict", "epoch"} == set(latest) and latest["epoch"] == 2 and best["epoch"] in (1, 2)
    assert set(best["model_state_dict"]) == set(model.state_dict())
    tiny_model().load_state_dict(best["model_state_dict"], strict=True)
    dec = load_decoder_from_checkpoint(str(out / "checkpoints" / "best.pt"), in_channels=1, dec_channels=TINY["dec_channels"],
                                       latent_dim=2, output_image_size=28, norm_type="batch", device="cpu")
    assert dec(torch.zeros(2, 2, 4, 4)).shape == (2, 1, 28, 28)
    for split in ("latents_train", "latents_val"):
        for name in ("z", "mu", "logvar"):
            t = torch.load(out / split / f"{name}.pt")
            assert t.shape == (24, 2, 4, 4) and t.dtype == torch.float32
        assert torch.load(out / split / "y.pt").shape == (24,)
    assert (out / "recon_grid.png").exists() and log.artifact == out / "recon_grid.png"


def test_early_stop_when_validation_cannot_improve(tmp_path, capsys, monkeypatch):
    """lr = 0, no batch statistics and the sampling noise pinned to zero: every epoch's validation loss is the same number, a
    tie is no improvement, so early_stop=1 stops in epoch 2; latest.pt still carries num_epochs."""
    from vqvae_amd.spatial_vae import SpatialVAE
    from vqvae_amd.training.spatial_engine import SpatialTrainingEngine
    monkeypatch.setattr(SpatialVAE, "reparameterize", staticmethod(lambda mu, logvar: mu))
    torch.manual_seed(2)
    model = SpatialVAE(in_channels=1, output_image_size=28, recon_loss="mse", **dict(TINY, norm_type="none"))
    engine = SpatialTrainingEngine(model, torch.optim.SGD(model.parameters(), lr=0.0), torch.device("cpu"))
    loader = _loaders()
    out = Path(tmp_path)
    engine.train(loader, loader, num_epochs=5, early_stop=1, checkpoint_dir=out / "ck", logger=None, output_dir=None,
                 save_latents_flag=False)
    assert "Early stopping at epoch 2" in capsys.readouterr().out
    assert torch.load(out / "ck" / "best.pt", weights_only=False)["epoch"] == 1
    assert torch.load(out / "ck" / "latest.pt", weights_only=False)["epoch"] == 5


def _write_idx(path, array):
    with open(path, "wb") as f:
        f.write(bytes([0, 0, 0x08, array.ndim]) + b"".join(struct.pack(">I", n) for n in array.shape) + array.tobytes())


def test_train_vae_command_line_on_idx_files(tmp_path, capsys):
    import yaml
    from vqvae_amd.scripts import train_vae
    r = np.random.RandomState(0)
    images = r.randint(0, 256, (11, 28, 28)).astype(np.uint8)
    labels = r.randint(0, 10, 11).astype(np.uint8)
    raw = tmp_path / "data" / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    _write_idx(raw / "train-images-idx3-ubyte", images)
    _write_idx(raw / "train-labels-idx1-ubyte", labels)
    _write_idx(raw / "t10k-images-idx3-ubyte", images[:4])
    _write_idx(raw / "t10k-labels-idx1-ubyte", labels[:4])
    cfg = {"seed": 42, "device": "cpu", "max_epochs": 1, "lr": 1e-3, "weight_decay": 1e-5, "early_stop": 20, "optimizer": "adamw",
           "scheduler": {"name": "cosine", "t_max": 1}, "grad_clip_max_norm": 1.0, "out_dir": str(tmp_path / "exp" / "vae"),
           "save_latents": True, "mlflow_tracking_uri": str(tmp_path / "mlruns"), "experiment_name": "t", "run_name": "t",
           "kl_anneal_epochs": 10,
           "data": {"name": "FashionMNIST", "root": str(tmp_path / "data"), "batch_size": 4, "num_workers": 4, "pin_memory": True,
                    "persistent_workers": True, "augment": False},
           "model": dict(in_channels=1, output_image_size=28, recon_loss="mse", beta=0.5, mse_use_sigmoid=True, **TINY)}
    path = tmp_path / "vae.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out = train_vae.main(str(path))
    assert out == tmp_path / "exp" / "vae" / "spatial_vae_fashionmnist"
    text = capsys.readouterr().out
    assert text.rstrip().endswith(f"Done. Artifacts in: {out}") and "Epoch 1/1 (beta=0.5000)" in text   # model.beta, constant
    for f in ("checkpoints/best.pt", "checkpoints/latest.pt", "recon_grid.png", "latents_train/z.pt", "latents_val/z.pt"):
        assert (out / f).exists(), f
    assert torch.load(out / "latents_train" / "z.pt").shape == (11, 2, 4, 4)
    assert torch.load(out / "latents_val" / "mu.pt").shape == (4, 2, 4, 4)


def test_resident_loader_fused_argument_on_the_cpu():
    from vqvae_amd.training.data import ResidentLoader, assemble_batch, resident_images
    r = np.random.RandomState(0)
    data = resident_images(r.randint(0, 256, (5, 28, 28)).astype(np.uint8), np.arange(5), "cpu")
    assert ResidentLoader(data, 4, False).fused is False and ResidentLoader(data, 4, False, fused=False).fused is False
    with pytest.raises(ValueError):
        ResidentLoader(data, 4, False, fused=True)
    with pytest.raises(ValueError):
        assemble_batch(data, torch.arange(2))

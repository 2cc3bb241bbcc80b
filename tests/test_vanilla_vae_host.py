"""Vanilla VAE on the host: model, torch-path ELBO, training engine, latent files, configuration parsing and the idx
train-split reader, against tests/golden/vanilla_vae.npz (the reference's own outputs, tools/gen_golden_vanilla_vae.py).
Both sides run the same torch CPU operations, so the comparisons are exact."""
import os
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

CONFIGS = {f"{size}px_{norm}": dict(in_channels=ch, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8), latent_dim=4,
                                   output_image_size=size, norm_type=norm)
           for size, ch in ((28, 1), (32, 3)) for norm in ("batch", "none")}


@pytest.fixture
def one_thread():
    """The fixture was computed with one torch thread: the CPU transposed convolution's summation order depends on the count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def golden_model(g, name):
    from vqvae_amd.vae import VAE
    model = VAE(**CONFIGS[name])
    prefix = f"{name}/sd/"
    state = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    model.load_state_dict(state, strict=True)
    return model.eval()


def apply_setting(model, row):
    """A row of the fixture's settings table -> the model's loss attributes and the keyword arguments of loss()."""
    recon_mode, free_bits, beta, cmax, anneal, step, mode = row
    model.recon_loss = "bce" if recon_mode == 0 else "mse"
    model.mse_use_sigmoid = recon_mode != 2
    model.free_bits_default = None if np.isnan(free_bits) else float(free_bits)
    return dict(beta=float(beta), capacity_max=float(cmax), capacity_anneal_steps=int(anneal), step=int(step),
                capacity_mode="abs" if mode == 0 else "clipped")


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_model_loads_reference_state_and_reproduces_its_forward(golden, one_thread, name):
    g = golden("vanilla_vae")
    model = golden_model(g, name)
    torch.manual_seed(int(g["eps_seed"]))
    with torch.no_grad():
        x_logits, mu, logvar, z = model(torch.from_numpy(g[f"{name}/x"]))
    for got, key in ((mu, "mu"), (logvar, "logvar"), (z, "z"), (x_logits, "x_logits")):
        np.testing.assert_array_equal(got.numpy(), g[f"{name}/{key}"], err_msg=key)
    np.testing.assert_array_equal(z.numpy(), (mu + torch.from_numpy(g[f"{name}/eps"]) * torch.exp(0.5 * logvar)).numpy())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_torch_loss_reproduces_every_golden_triple(golden, one_thread, name):
    g = golden("vanilla_vae")
    model = golden_model(g, name)
    x, x_logits, mu, logvar = (torch.from_numpy(g[f"{name}/{k}"]) for k in ("x", "x_logits", "mu", "logvar"))
    assert len(g["settings"]) == 30
    for row, want, want64 in zip(g["settings"], g[f"{name}/triples"], g[f"{name}/triples_f64"]):
        kw = apply_setting(model, row)
        got = [float(v) for v in model.loss(x, x_logits, mu, logvar, **kw)]
        assert got == [float(v) for v in want], (row, got, want)
        got64 = [float(v) for v in model.loss(x.double(), x_logits.double(), mu.double(), logvar.double(), **kw)]
        assert got64 == list(want64), (row, got64, want64)


def test_loss_defaults_and_step_counter():
    from vqvae_amd.vae import VAE
    torch.manual_seed(0)
    model = VAE(latent_dim=4, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8))
    assert (model.free_bits_default, model.capacity_max_default, model.capacity_anneal_steps_default,
            model.capacity_mode_default, model.recon_loss, model.mse_use_sigmoid) == (0.5, 15.0, 50_000, "abs", "bce", True)
    x = torch.rand(3, 1, 28, 28)
    out = model(x)
    assert [tuple(t.shape) for t in out] == [(3, 1, 28, 28), (3, 4), (3, 4), (3, 4)]
    x_logits, mu, logvar, _ = out
    assert model._step == 0
    first = model.loss(x, x_logits, mu, logvar)
    second = model.loss(x, x_logits, mu, logvar)
    assert model._step == 2
    model.loss(x, x_logits, mu, logvar, step=40_000)                   # an explicit step leaves the counter alone
    assert model._step == 2
    # the counter is the capacity step: calls 0 and 1 equal explicit steps 0 and 1 with the defaults spelled out
    for step, got in ((0, first), (1, second)):
        want = model.loss(x, x_logits, mu, logvar, beta=1.0, free_bits=0.5, capacity_max=15.0, capacity_anneal_steps=50_000,
                          step=step, capacity_mode="abs")
        assert [float(a.detach()) for a in got] == [float(b.detach()) for b in want]
    kl = float(first[2])
    assert kl >= 4 * 0.5                                                # free bits: every dimension counts at least 0.5
    assert float(first[0]) == pytest.approx(float(first[1]) + abs(kl - 0.0), rel=1e-6)
    # eval mode samples too
    model.eval()
    assert not torch.equal(model(x)[3], model(x)[3])
    with pytest.raises(AssertionError):
        VAE(recon_loss="l1")


def test_load_vae_is_the_full_model_sibling_of_load_vae_decoder(golden, tmp_path):
    from vqvae_amd.vae import load_vae, load_vae_decoder
    g = golden("vanilla_vae")
    model = golden_model(g, "32px_batch")
    path = str(tmp_path / "best.pt")
    torch.save({"model_state_dict": model.state_dict(), "epoch": 3}, path)
    full, cfg = load_vae(path)
    dec, cfg_dec = load_vae_decoder(path)
    assert cfg == cfg_dec and cfg["in_channels"] == 3 and cfg["enc_channels"] == (8, 16, 32) and cfg["norm_type"] == "batch"
    assert not full.training
    for k, v in model.state_dict().items():
        assert torch.equal(full.state_dict()[k], v), k
    for k, v in dec.state_dict().items():
        assert torch.equal(full.decoder.state_dict()[k], v), k
    torch.save(model.state_dict(), path)                               # a bare state dict is accepted too
    assert load_vae(path)[1] == cfg
    with pytest.raises(FileNotFoundError):
        load_vae(str(tmp_path / "missing.pt"))


class _Recorder:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step=None):
        self.rows.append((step, dict(metrics)))

    def log_artifact(self, path):
        self.artifact = path


def _cpu_loaders(n=64, batch=24):
    r = torch.Generator().manual_seed(3)
    x = torch.rand(n, 1, 28, 28, generator=r)
    y = torch.arange(n) % 10
    batches = [(x[s:s + batch], y[s:s + batch]) for s in range(0, n, batch)]
    return batches, batches[:2]


def test_training_engine_follows_the_reference_rules(tmp_path, monkeypatch):
    from vqvae_amd.training.engine import TrainingEngine
    from vqvae_amd.vae import VAE
    torch.manual_seed(1)
    model = VAE(latent_dim=4, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8), recon_loss="mse", norm_type="batch")
    calls = []
    inner = model.loss

    def spy(x, x_logits, mu, logvar, **kw):
        calls.append((model.training, kw["step"], kw["beta"], x.size(0)))
        return inner(x, x_logits, mu, logvar, **kw)

    monkeypatch.setattr(model, "loss", spy)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)

    class Sched:
        steps = 0

        def step(self):
            Sched.steps += 1

    train_loader, val_loader = _cpu_loaders()
    log = _Recorder()
    out = Path(tmp_path) / "run"
    TrainingEngine(model, opt, torch.device("cpu")).train(
        train_loader, val_loader, num_epochs=2, early_stop=0, checkpoint_dir=out / "checkpoints", logger=log, output_dir=out,
        save_latents_flag=True, kl_anneal_epochs=4, beta=2.0, grad_clip_max_norm=1.0, scheduler=Sched())
    # global step carries across epochs; validation uses the post-training step; beta = 2 * epoch / 4
    assert [c[:3] for c in calls] == [(True, 0, 0.5), (True, 1, 0.5), (True, 2, 0.5), (False, 3, 0.5), (False, 3, 0.5),
                                     (True, 3, 1.0), (True, 4, 1.0), (True, 5, 1.0), (False, 6, 1.0), (False, 6, 1.0)]
    assert [c[3] for c in calls[:3]] == [24, 24, 16]
    assert Sched.steps == 2 and [s for s, _ in log.rows] == [1, 2]
    keys = {"train_loss", "train_recon", "train_kl", "val_loss", "val_recon", "val_kl", "beta", "val_psnr", "val_ssim",
            "train_recon_per_pixel", "val_recon_per_pixel"}
    assert set(log.rows[0][1]) == keys and log.rows[1][1]["beta"] == 1.0
    row = log.rows[0][1]
    assert row["train_recon_per_pixel"] == row["train_recon"] / 784 and 0 < row["val_psnr"] < 40 and 0 <= row["val_ssim"] <= 1
    best = torch.load(out / "checkpoints" / "best.pt", weights_only=False)
    latest = torch.load(out / "checkpoints" / "latest.pt", weights_only=False)
    assert set(best) == {"model_state_dict", "epoch"} == set(latest) and latest["epoch"] == 2 and best["epoch"] in (1, 2)
    assert set(best["model_state_dict"]) == set(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(latest["model_state_dict"][k], v), k
    assert (out / "recon_grid.png").exists() and log.artifact == out / "recon_grid.png"
    from PIL import Image
    assert Image.open(out / "recon_grid.png").size == (8 * 30 + 2, 2 * 30 + 2)
    for split, n in (("latents_train", 64), ("latents_val", 48)):
        for name in ("z", "mu", "logvar"):
            t = torch.load(out / split / f"{name}.pt")
            assert t.shape == (n, 4) and t.dtype == torch.float32 and t.device.type == "cpu"
        y = torch.load(out / split / "y.pt")
        assert y.shape == (n,) and y.dtype == torch.int64


def test_training_engine_averages_and_early_stop(tmp_path):
    """Averages divide the per-batch sums by len(loader); best.pt only on strict improvement; early stop after `early_stop`
    epochs without one, before that epoch's scheduler step; latest.pt still carries num_epochs."""
    from vqvae_amd.training.engine import TrainingEngine

    class Fixed(torch.nn.Module):                 # loss = the batch's mean pixel, whatever the weights do
        recon_loss, mse_use_sigmoid = "mse", True

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            z = torch.zeros(x.size(0), 2) + self.w
            return x + self.w, z, z, z

        def loss(self, x, x_logits, mu, logvar, *, beta, step):
            v = x.mean() + 0 * self.w.sum()
            return v, v.detach(), 0 * v.detach()

    model = Fixed()
    eng = TrainingEngine(model, torch.optim.SGD(model.parameters(), lr=0.0), torch.device("cpu"))
    loader = [(torch.full((4, 1, 4, 4), 1.0), torch.zeros(4)), (torch.full((1, 1, 4, 4), 4.0), torch.zeros(1))]
    avg = eng.run_epoch(loader, train=False, epoch=1, num_epochs=1, beta=1.0, global_step_start=5)
    assert avg[0] == 2.5 and avg[1] == 2.5 and avg[2] == 0.0 and avg[3] == 5          # (1 + 4) / 2 batches, not per image
    assert eng.run_epoch(loader, train=True, epoch=1, num_epochs=1, beta=1.0, global_step_start=5)[3:] == (7, 0, 0)

    class Sched:
        steps = 0

        def step(self):
            Sched.steps += 1

    out = Path(tmp_path)
    eng.train(loader, loader, num_epochs=9, early_stop=2, checkpoint_dir=out / "ck", logger=None, output_dir=None,
              save_latents_flag=False, scheduler=Sched())
    # epoch 1 improves on inf, epochs 2 and 3 tie (no strict improvement): stop in epoch 3 after two scheduler steps
    assert torch.load(out / "ck" / "best.pt", weights_only=False)["epoch"] == 1
    assert torch.load(out / "ck" / "latest.pt", weights_only=False)["epoch"] == 9 and Sched.steps == 2


def test_save_latents_and_resident_encode(tmp_path):
    from vqvae_amd.utils.latents import encode_latents_device, save_latents
    from vqvae_amd.vae import VAE
    torch.manual_seed(2)
    model = VAE(in_channels=3, latent_dim=6, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8), output_image_size=32)
    loader = [(torch.rand(7, 3, 32, 32), torch.arange(7)), (torch.rand(3, 3, 32, 32), torch.arange(3))]
    model.train()
    save_latents(model, loader, torch.device("cpu"), tmp_path / "lat")
    assert not model.training
    assert sorted(os.listdir(tmp_path / "lat")) == ["logvar.pt", "mu.pt", "y.pt", "z.pt"]
    mu = torch.load(tmp_path / "lat" / "mu.pt")
    assert mu.shape == (10, 6) and mu.dtype == torch.float32
    assert torch.equal(torch.load(tmp_path / "lat" / "y.pt"), torch.cat([torch.arange(7), torch.arange(3)]))
    z, mu2, logvar, y = encode_latents_device(model, loader, torch.device("cpu"))
    assert torch.equal(mu2, mu) and torch.equal(logvar, torch.load(tmp_path / "lat" / "logvar.pt")) and z.shape == (10, 6)
    assert not torch.equal(z, torch.load(tmp_path / "lat" / "z.pt"))                   # a fresh draw per call


def test_job_parsing_of_both_legacy_builders():
    from vqvae_amd.training.build_riemannian_codebook_legacy import GraphJob, LegacyJob
    cfg = {"data": {"latents_path": "a/z.pt"}, "graph": {"k": "10", "metric": "euclidean", "sym": "union", "mode": "connectivity"},
           "quantize": {"K": 16, "init": "kpp", "seed": "42"}, "out": {"dir": "o"}}
    job = GraphJob.from_config(cfg)
    assert (job.latents, job.out_dir, job.k, job.metric, job.sym, job.graph_mode, job.K, job.init, job.seed) == (
        Path("a/z.pt"), Path("o"), 10, "euclidean", "union", "connectivity", 16, "kpp", 42)
    for data, want in (({"dataset": " Fashion "}, "experiments/vae_fashion"), ({"dataset": "cifar10"}, "experiments/vae_cifar10"),
                       ({"dataset": "other"}, "experiments/vae_mnist"), ({}, "experiments/vae_mnist"), ("not a dict", "experiments/vae_mnist")):
        assert GraphJob.from_config(dict(cfg, data=data)).latents == Path(want) / "latents_train" / "z.pt"
    with pytest.raises(ValueError):
        LegacyJob.from_config(cfg)                                      # the Riemannian builder needs a VAE configuration
    full = LegacyJob.from_config(dict(cfg, data={"dataset": "cifar10"}, model={"latent_dim": 4, "checkpoint_path": "m.pt"},
                                      riemannian={"mode": "full", "max_edges": 7}))
    assert (full.checkpoint, full.vae_config["latent_dim"], full.reweight_mode, full.max_edges, full.batch_size, full.k,
            full.latents) == (Path("m.pt"), 4, "full", 7, 512, 10, Path("experiments/vae_cifar10/latents_train/z.pt"))
    assert LegacyJob.from_config(dict(cfg, data={}, vae={"x": 1})).checkpoint == Path("experiments/vae_fashion/checkpoints/best.pt")
    with pytest.raises(KeyError):
        GraphJob.from_config({"graph": cfg["graph"], "quantize": cfg["quantize"]})


def _write_idx(path, array):
    with open(path, "wb") as f:
        f.write(bytes([0, 0, 0x08, array.ndim]) + b"".join(struct.pack(">I", n) for n in array.shape) + array.tobytes())


def test_train_split_reader_and_resident_loader(tmp_path):
    from vqvae_amd.eval.data import fashionmnist_train, idx_split, mnist_train
    from vqvae_amd.training.data import ROTATION_MESSAGE, ResidentLoader, get_data_loaders, resident_images
    r = np.random.RandomState(0)
    images = r.randint(0, 256, (11, 28, 28)).astype(np.uint8)
    labels = r.randint(0, 10, 11).astype(np.uint8)
    raw = tmp_path / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    _write_idx(raw / "train-images-idx3-ubyte", images)
    _write_idx(raw / "train-labels-idx1-ubyte", labels)
    _write_idx(raw / "t10k-images-idx3-ubyte", images[:4])
    _write_idx(raw / "t10k-labels-idx1-ubyte", labels[:4])
    got_images, got_labels = fashionmnist_train(str(tmp_path))
    np.testing.assert_array_equal(got_images, images)
    assert got_labels.dtype == np.int64 and got_labels.tolist() == labels.tolist()
    assert idx_split(str(tmp_path), "FashionMNIST", train=False)[0].shape == (4, 28, 28)
    with pytest.raises(FileNotFoundError):
        mnist_train(str(tmp_path))

    train, val = get_data_loaders("Fashion-MNIST", str(tmp_path), batch_size=4, device="cpu", num_workers=4, pin_memory=True)
    assert (len(train), len(val)) == (3, 1) and val.normalize is None
    want = torch.from_numpy(images).float().div(255).unsqueeze(1)
    # a seeded epoch is the DataLoader(shuffle=True) epoch: same draws from the CPU generator, tail batch kept
    torch.manual_seed(5)
    got = list(train)
    torch.manual_seed(5)
    order = [b for b in torch.utils.data.DataLoader(range(11), batch_size=4, shuffle=True)]
    assert [x.shape[0] for x, _ in got] == [4, 4, 3]
    for (x, y), rows in zip(got, order):
        assert torch.equal(x, want[rows]) and torch.equal(y, torch.from_numpy(got_labels)[rows])
    (xv, yv), = list(val)
    assert torch.equal(xv, want[:4]) and xv.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="RandomRotation"):
        get_data_loaders("FashionMNIST", str(tmp_path), 4, "cpu", augment=True)
    assert "RandomRotation" in ROTATION_MESSAGE

    # CIFAR-style crop + flip: reproducible under a seed, every output a shifted (zero-padded) or mirrored copy
    rgb = r.randint(1, 256, (6, 32, 32, 3)).astype(np.uint8)
    norm = ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    data = resident_images(rgb, np.arange(6), "cpu", norm)
    torch.manual_seed(9)
    a = [x for x, _ in ResidentLoader(data, 6, False, norm, crop_flip=True)]
    torch.manual_seed(9)
    b = [x for x, _ in ResidentLoader(data, 6, False, norm, crop_flip=True)]
    assert torch.equal(a[0], b[0]) and a[0].shape == (6, 3, 32, 32)
    plain = next(iter(ResidentLoader(data, 6, False, norm)))[0]
    assert not torch.equal(a[0], plain)
    pad = torch.nn.functional.pad(plain, (4, 4, 4, 4), value=float("nan"))
    zero = (0 - 0.5) / 0.25
    for i in range(6):
        hits = 0
        for oy in range(9):
            for ox in range(9):
                win = torch.nan_to_num(pad[i, :, oy:oy + 32, ox:ox + 32], nan=zero)
                hits += int(torch.equal(a[0][i], win)) + int(torch.equal(a[0][i], win.flip(2)))
        assert hits >= 1, i

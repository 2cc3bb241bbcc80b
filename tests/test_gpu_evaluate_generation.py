"""python -m vqvae_amd.scripts.evaluate_generation end to end on tiny experiments (a spatial VAE as tiny_setup writes it, a
vanilla VAE with encoder and decoder): both files are written, every figure equals prdc_device recomputed from features
the test encodes itself, the ceiling is there, and two runs with one seed write byte-identical JSON.  The fakes and the reals
that are scored are rebuilt here without the CLI's helpers: the label cycle, the token-to-grid layout and the eval-mode
decode from the reference's formulas on the torch modules, the reals from the idx file."""
import json

import numpy as np
import pytest
import torch

from test_prior_sample_host import tiny_setup

pytestmark = pytest.mark.gpu

FIGURES = ("precision", "recall", "density", "coverage")
ARRAYS = ("real_radius2", "fake_radius2", "fake_count", "real_count", "real_near_key", "real_near_idx")


def _write_idx(path, array):
    with open(path, "wb") as f:
        f.write(bytes([0, 0, 0x08, array.ndim]) + b"".join(int(s).to_bytes(4, "big") for s in array.shape) + array.tobytes())


def _tiny_fashionmnist(root):
    r = np.random.RandomState(9)
    raw = root / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    for prefix in ("train", "t10k"):
        _write_idx(raw / f"{prefix}-images-idx3-ubyte", r.randint(0, 256, (64, 28, 28)).astype(np.uint8))
        _write_idx(raw / f"{prefix}-labels-idx1-ubyte", r.randint(0, 10, 64).astype(np.uint8))


def _setup(tmp, vanilla):
    """tiny_setup's experiment; the vanilla one gets a whole VAE (tiny_setup's holds the decoder alone)."""
    path, cfg = tiny_setup(str(tmp), vanilla=vanilla)
    if vanilla:
        from vqvae_amd.vae import VAE
        torch.manual_seed(12)
        torch.save({"model_state_dict": VAE(**cfg["vae"]).state_dict(), "epoch": 3}, cfg["vae_ckpt_path"])
    return path, cfg


@pytest.mark.parametrize("vanilla", [False, True], ids=["spatial", "vanilla"])
def test_cli_scores_equal_a_recomputation(tmp_path, vanilla):
    from vqvae_amd._device import device
    from vqvae_amd.eval.prdc import prdc_device
    from vqvae_amd.scripts import evaluate_generation as cli
    _tiny_fashionmnist(tmp_path / "data")
    config, cfg = _setup(tmp_path, vanilla)
    outs = [tmp_path / "run_a", tmp_path / "run_b"]
    for out in outs:
        cli.main(["--config", config, "--dataset", "FashionMNIST", "--data_root", str(tmp_path / "data"), "--split", "test",
                  "--num_samples", "48", "--k", "3", "--out_dir", str(out), "--seed", "7"])
        assert (out / "generation_metrics.json").exists() and (out / "generation_prdc.npz").exists()
    a, b = [(out / "generation_metrics.json").read_bytes() for out in outs]
    assert a == b, "two runs with one seed differ"
    got = json.loads(a)
    width = cfg["vae"]["latent_dim"] * (1 if vanilla else 16)
    assert (got["k"], got["n"], got["m"], got["feature_width"], got["seed"]) == (3, 64, 48, width, 7)
    assert got["prdc_route"] == "hip" and got["encode_path"] in ("hip", "torch") and got["decode_path"] in ("hip", "torch")
    assert sorted(got["ceiling"]) == sorted(FIGURES) and all(0.0 <= got["ceiling"][f] for f in FIGURES)

    dev = device()
    model = cli.load_model(cfg, dev)
    fake_images = cli.generate_images(cfg, model, dev, 48, "FashionMNIST", 7)
    assert fake_images.shape == (48, 1, 28, 28) and float(fake_images.min()) >= 0 and float(fake_images.max()) <= 1
    loader, norm = cli.real_images("FashionMNIST", str(tmp_path / "data"), "test", None, dev)
    assert norm is None

    # what the CLI scores, rebuilt without its helpers.  Fakes: the yaml's classes cycled over the samples, one sampling call
    # after the seed, generate_samples' lookup (token t of a spatial sequence at grid position (t // 4, t % 4)), the torch
    # decoder in eval mode, sigmoid.  Reals: the idx file's bytes / 255 in file order.
    from vqvae_amd.prior import Transformer, sample
    prior = Transformer(**cfg["transformer"]).to(dev)
    prior.load_state_dict(torch.load(cfg["transformer_ckpt_path"], map_location=dev))
    table = torch.load(cfg["codebook_path"], map_location=dev, weights_only=False)["z_medoid"].float()
    classes = cfg["class_labels"]
    y = torch.tensor([classes[i % len(classes)] for i in range(48)], dtype=torch.int64, device=dev)
    V, T = cfg["transformer"]["num_tokens"], cfg["transformer"]["max_seq_len"]
    torch.manual_seed(7)
    if vanilla:
        start = torch.full((48, 1), V - 1, dtype=torch.int64, device=dev)
        codes = sample(prior, start, steps=T - 1, temperature=cfg["temperature"], top_k=cfg["top_k"], y=y)[:, 1:]
        zq = table[codes[:, 0]]
    else:
        start = torch.randint(0, V, (48, 1), device=dev)
        codes = sample(prior, start, steps=T - 1, temperature=cfg["temperature"], top_k=cfg["top_k"], y=y)
        zq = table[codes].permute(0, 2, 1).reshape(48, cfg["vae"]["latent_dim"], 4, 4)
    with torch.no_grad():
        own_images = model.decoder(zq).sigmoid()
    assert not model.decoder.training
    worst = float((own_images - fake_images).abs().max())
    print(f"fake images, CLI helper against the torch decode of independently drawn codes: max abs difference {worst:.3e}")
    assert worst <= 1e-5, worst                     # float32 decodes of values in [0, 1]: a wrong label or grid cell is O(0.1)
    raw = (tmp_path / "data" / "FashionMNIST" / "raw" / "t10k-images-idx3-ubyte").read_bytes()
    pixels = torch.from_numpy(np.frombuffer(raw, np.uint8, offset=16).reshape(64, 1, 28, 28).copy()).to(dev)
    assert torch.equal(torch.cat([x for x, _ in loader]), pixels.float() / 255)

    from vqvae_amd.encode import encode_latents                             # the experiment's encoder, by the CLI's route
    real = torch.cat([encode_latents(model.encoder, x)[0].reshape(x.shape[0], -1) for x, _ in loader]).contiguous()
    fake = encode_latents(model.encoder, fake_images)[0].reshape(48, -1).contiguous()
    assert real.shape == (64, width) and fake.shape == (48, width)
    arrays = np.load(outs[0] / "generation_prdc.npz")
    assert sorted(arrays.files) == sorted(ARRAYS)
    ref = prdc_device(real, fake, 3)
    for f in FIGURES:
        assert got[f] == ref[f], (f, got[f], ref[f])
    for name in ARRAYS:
        np.testing.assert_array_equal(arrays[name], ref[name].cpu().numpy(), err_msg=name)
    order = torch.from_numpy(np.random.RandomState(7).permutation(64)).to(dev)
    ceiling = prdc_device(real[order[:32]].contiguous(), real[order[32:]].contiguous(), 3)
    assert all(got["ceiling"][f] == ceiling[f] for f in FIGURES)


def test_cli_refuses_a_decoder_only_checkpoint(tmp_path):
    from vqvae_amd.scripts import evaluate_generation as cli
    _tiny_fashionmnist(tmp_path / "data")
    config, _ = tiny_setup(str(tmp_path), vanilla=True)
    with pytest.raises(ValueError, match="encoder.fc_mu.weight"):
        cli.main(["--config", config, "--dataset", "FashionMNIST", "--data_root", str(tmp_path / "data"), "--num_samples", "48",
                  "--k", "3", "--out_dir", str(tmp_path / "out")])

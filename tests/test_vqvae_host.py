"""Baseline VQ-VAE on the host: initial weights and layout against the reference's fixture, the CPU quantizer (fp64 rules)
against the reference's outputs, batch order and CPU RNG use against torch's DataLoader, the CIFAR-10 train reader, config
overrides, the log / checkpoint layout and the evaluation JSON keys."""
import argparse
import hashlib
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_rules as R  # noqa: E402

CIFAR = dict(in_channels=3, z_channels=128, hidden=256, n_res_blocks=2, n_codes=512, beta=0.25, ema_decay=0.99, ema_eps=1e-5)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("vqvae_baseline")


def test_initial_weights_match_reference(fx):
    from vqvae_amd.baseline import VQVAE
    torch.manual_seed(42)
    sd = VQVAE(**CIFAR).state_dict()
    assert list(sd.keys()) == [str(n) for n in fx["sd_names"]]
    for i, (k, t) in enumerate(sd.items()):
        shape = [int(v) for v in fx["sd_shapes"][i] if v >= 0]
        assert list(t.shape) == shape, k
        assert hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() == str(fx["sd_sha256"][i]), k


def test_cpu_quantizer_matches_reference(fx):
    from vqvae_amd.baseline import VectorQuantizerEMA
    K, C, B, H, W, steps = (int(v) for v in fx["dims"])
    torch.manual_seed(int(fx["seed"]))
    q = VectorQuantizerEMA(n_codes=K, code_dim=C)
    assert np.array_equal(q.embed.numpy(), fx["embed0"])
    for s in range(steps + 1):
        q.train(s < steps)
        z = torch.from_numpy(fx["z_e"][s])
        before = q.embed.numpy().copy()
        z_q_st, loss, idx, z_q, z_e = q(z)
        assert z_e is z
        assert np.array_equal(idx.numpy(), fx[f"idx_{s}"])
        # bit-identical given the same codebook (step 0); later codebooks carry the EMA's rounding (rtol 1e-6)
        want = R.forward(fx["z_e"][s], before, None, None, training=False, idx=idx.numpy())
        assert np.array_equal(z_q.numpy(), want["z_q"]) and np.array_equal(z_q_st.numpy(), want["z_q_st"])
        if s == 0:
            assert np.array_equal(z_q.numpy(), fx["z_q_0"]) and np.array_equal(z_q_st.numpy(), fx["z_q_st_0"])
        np.testing.assert_allclose(z_q_st.numpy(), fx[f"z_q_st_{s}"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(loss.item(), fx[f"loss_{s}"], rtol=1e-6)
        for b in ("cluster_size", "embed_avg", "embed"):
            np.testing.assert_allclose(getattr(q, b).numpy(), fx[f"{b}_{s}"], rtol=1e-6, atol=1e-6, err_msg=f"{b} step {s}")


def test_rules_restatement_matches_reference(fx):
    K, C, B, H, W, steps = (int(v) for v in fx["dims"])
    emb, cs, ea = fx["embed0"], np.zeros(K, np.float32), fx["embed0"].copy()
    for s in range(steps + 1):
        o = R.forward(fx["z_e"][s], emb, cs, ea, training=s < steps)
        assert np.array_equal(o["idx"], fx[f"idx_{s}"])
        np.testing.assert_allclose(o["z_q_st"], fx[f"z_q_st_{s}"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(o["loss"], fx[f"loss_{s}"], rtol=1e-6)
        emb, cs, ea = o["embed"], o["cluster_size"], o["embed_avg"]
        np.testing.assert_allclose(emb, fx[f"embed_{s}"], rtol=1e-6, atol=1e-6)


def test_cpu_quantizer_gradient():
    from vqvae_amd.baseline import VectorQuantizerEMA
    torch.manual_seed(3)
    q = VectorQuantizerEMA(n_codes=16, code_dim=8).eval()
    z = (torch.randn(2, 8, 4, 4) * 1.5).requires_grad_()
    z_q_st, loss, *_ = q(z)
    g = torch.randn_like(z_q_st)
    (z_q_st * g).sum().add(loss * 3.0).backward()
    want = R.backward(g.numpy(), 3.0, z.detach().numpy(), z_q_st.detach().numpy())
    np.testing.assert_allclose(z.grad.numpy(), want, rtol=1e-5, atol=1e-7)


def test_batch_order_and_rng_match_dataloader():
    from torch.utils.data import DataLoader
    from vqvae_amd.baseline.data import DeviceImages, shuffled_order
    n, bs = 203, 16
    imgs = np.arange(n, dtype=np.uint8)[:, None, None, None].repeat(32, 1).repeat(32, 2).repeat(3, 3)
    torch.manual_seed(5)
    ref = [b.tolist() for b in DataLoader(torch.arange(n), batch_size=bs, shuffle=True, drop_last=True)]
    ref_state = torch.get_rng_state()
    torch.manual_seed(5)
    assert shuffled_order(n, bs) == ref
    assert torch.equal(torch.get_rng_state(), ref_state)
    data = DeviceImages(imgs, np.zeros(n, np.int64), "cpu", [0.5] * 3, [0.5] * 3)
    torch.manual_seed(5)
    got = [((x[:, 0, 0, 0] * 0.5 + 0.5) * 255).round().long().tolist() for x in data.shuffled_batches(bs)]
    assert got == ref
    assert torch.equal(torch.get_rng_state(), ref_state)
    # shuffle=False iteration draws the iterator's seed too
    torch.manual_seed(5)
    list(DataLoader(torch.arange(n), batch_size=bs))
    s = torch.get_rng_state()
    torch.manual_seed(5)
    list(data.ordered_batches(bs))
    assert torch.equal(torch.get_rng_state(), s)


def test_device_images_transform():
    from vqvae_amd.baseline.data import DeviceImages
    r = np.random.RandomState(0)
    imgs = r.randint(0, 256, (5, 32, 32, 3)).astype(np.uint8)
    data = DeviceImages(imgs, np.zeros(5, np.int64), "cpu", [0.4914, 0.4822, 0.4465], [0.247, 0.243, 0.261])
    x = data.batch([3, 1])
    mean = torch.tensor([0.4914, 0.4822, 0.4465]).view(3, 1, 1)
    std = torch.tensor([0.247, 0.243, 0.261]).view(3, 1, 1)
    for i, k in enumerate([3, 1]):
        want = torch.from_numpy(imgs[k]).permute(2, 0, 1).contiguous().float().div(255).sub(mean).div(std)
        assert torch.equal(x[i], want)


def _write_cifar(root, n_per=7, seed=0):
    r = np.random.RandomState(seed)
    d = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(d, exist_ok=True)
    out = {}
    for name in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]:
        data = r.randint(0, 256, (n_per, 3072)).astype(np.uint8)
        labels = r.randint(0, 10, n_per).tolist()
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"data": data, "labels": labels}, f)
        out[name] = (data, labels)
    return out


def test_cifar10_train_reader(tmp_path):
    from vqvae_amd.eval.data import cifar10_train
    raw = _write_cifar(str(tmp_path))
    images, labels = cifar10_train(str(tmp_path))
    want = np.concatenate([raw[f"data_batch_{i}"][0] for i in range(1, 6)]).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    assert images.shape == (35, 32, 32, 3) and images.dtype == np.uint8
    assert np.array_equal(images, want)
    assert labels.tolist() == sum((raw[f"data_batch_{i}"][1] for i in range(1, 6)), [])
    os.remove(os.path.join(str(tmp_path), "cifar-10-batches-py", "data_batch_3"))
    with pytest.raises(FileNotFoundError):
        cifar10_train(str(tmp_path))


def test_config_overrides(tmp_path):
    from vqvae_amd.baseline.train import load_config
    cfg = {"seed": 1, "train": {"epochs": 5, "batch_size": 8, "lr": 1e-3}, "model": {"beta": 0.25, "n_codes": 16,
                                                                                     "ema_decay": 0.99}}
    p = tmp_path / "config.yaml"
    p.write_text(yaml.safe_dump(cfg))
    args = argparse.Namespace(epochs=2, batch_size=None, lr=5e-4, beta=0.5, n_codes=None, ema_decay=0.9)
    got = load_config(str(p), args)
    assert got["train"] == {"epochs": 2, "batch_size": 8, "lr": 5e-4}
    assert got["model"] == {"beta": 0.5, "n_codes": 16, "ema_decay": 0.9}
    assert load_config(str(p)) == cfg


def test_log_header_and_checkpoint_layout(tmp_path):
    from vqvae_amd.baseline import VQVAE
    from vqvae_amd.baseline.train import LOG_HEADER, CSVLogger, checkpoint_state
    assert LOG_HEADER == ["epoch", "split", "loss", "rec", "vq", "q_mse", "perplex", "usage", "dead", "embed_norm_mean",
                          "embed_norm_min", "embed_norm_max"]
    path = str(tmp_path / "out" / "log.csv")
    for _ in range(2):
        lg = CSVLogger(path, LOG_HEADER)
        lg.log([1, "train"] + [0.5] * 10)
        lg.close()
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(LOG_HEADER) and len(lines) == 3
    m = VQVAE(z_channels=16, hidden=32, n_codes=8)
    opt = torch.optim.Adam(m.parameters())
    st = checkpoint_state(m, opt, {"seed": 1}, 3)
    assert sorted(st) == ["cfg", "epoch", "model", "opt"] and st["epoch"] == 3
    m2 = VQVAE(z_channels=16, hidden=32, n_codes=8)
    m2.load_state_dict(st["model"], strict=True)


def test_evaluation_json_keys():
    from vqvae_amd.scripts.evaluate_baseline import results_dict
    res = results_dict(20.1234567, 0.81234567, 100, 9.5, 0.1, 100, 10, {"entropy": 5.5, "used": 400, "dead_codes": 112}, 512)
    # what compare_all_approaches.extract_metrics reads, in its order of preference
    assert res["model_type"] == "baseline_vqvae"
    assert res["generation_quality"]["psnr"] == 9.5 and res["generation_quality"]["ssim"] == 0.1
    assert res["reconstruction_quality"] == {"psnr": 20.123457, "ssim": 0.812346, "samples_evaluated": 100}
    cb = res["codebook_health"]
    assert cb == {"entropy": 5.5, "used_codes": 400, "dead_codes": 112, "usage_percent": 78.12, "codebook_size": 512}
    assert "lpips" not in res["generation_quality"]

"""CPU checks of the evaluation stage (vqvae_amd.eval, the evaluate_* CLIs): the fp64 host metrics against the reference's
values (tests/golden/eval.npz, tools/gen_golden_eval.py), the dataset readers, layout detection and the CLIs' --help."""
import gzip
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from vqvae_amd.eval import data as D
from vqvae_amd.eval.experiment import detect_layout
from vqvae_amd.eval.metrics import codebook_stats, image_pair_moments_numpy, psnr, ssim_simple
from vqvae_amd.vae import auto_detect_vae_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ("rand4_c1_28", "rand4_c3_32", "close4_c1_28", "const4_c1_28", "ident4_c3_32", "rand3_c3_32", "const3_c1_28",
         "struct4_c1_28")
CODES = ("codes_dead", "codes_kbig", "codes_neg", "codes_allneg", "codes_uniform")
CLIS = ("evaluate_vae_quality", "evaluate_quantization_loss", "evaluate_codebook_health", "evaluate_model")


@pytest.mark.parametrize("name", PAIRS)
def test_cpu_psnr_ssim_match_reference(golden, name):
    g = golden("eval")
    x, y = torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"])
    assert abs(psnr(x, y) - float(g[f"{name}/psnr"])) <= 1e-4
    assert abs(ssim_simple(x, y) - float(g[f"{name}/ssim"])) <= 1e-5


def test_identical_pairs_clamp_mse(golden):
    g = golden("eval")
    x = torch.from_numpy(g["ident4_c3_32/x"])
    assert psnr(x, x.clone()) == pytest.approx(120.0, abs=1e-9)        # 10 log10(1 / 1e-12)
    assert float(g["ident4_c3_32/psnr"]) == pytest.approx(120.0, abs=1e-4)


def test_sum_form_denominator_of_the_batched_branch():
    """4-D input: the reference adds the two factors of the denominator; other ranks multiply them."""
    r = np.random.RandomState(0)
    x, y = r.rand(1, 1, 8, 8).astype(np.float32), r.rand(1, 1, 8, 8).astype(np.float32)
    mx, my, vx, vy, cxy, _ = image_pair_moments_numpy(x.reshape(1, -1), y.reshape(1, -1))[0]
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    num = (2 * mx * my + C1) * (2 * cxy + C2)
    assert ssim_simple(torch.from_numpy(x), torch.from_numpy(y)) == pytest.approx(
        min(max(num / ((mx ** 2 + my ** 2 + C1) + (vx + vy + C2)), 0), 1), abs=1e-15)
    assert ssim_simple(torch.from_numpy(x[0]), torch.from_numpy(y[0])) == pytest.approx(
        min(max(num / ((mx ** 2 + my ** 2 + C1) * (vx + vy + C2)), 0), 1), abs=1e-15)


@pytest.mark.parametrize("name", CODES)
def test_codebook_stats_match_reference(golden, name):
    g = golden("eval")
    s = codebook_stats(torch.from_numpy(g[f"{name}/codes"]), int(g[f"{name}/K"]))
    assert abs(s["entropy"] - float(g[f"{name}/entropy"])) <= 1e-5
    assert s["dead_codes"] == int(g[f"{name}/dead"])
    assert s["used"] == int(g[f"{name}/used"])


def test_auto_detect_matches_the_fixture_architecture(golden):
    g = golden("eval")
    state = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("vae/")}
    cfg = auto_detect_vae_config(state)
    assert cfg == {"in_channels": 1, "enc_channels": (8, 16, 32), "dec_channels": (32, 16, 8), "norm_type": "batch",
                   "output_image_size": 28, "latent_dim": 4}


def _write_idx(path, arr, code, gz):
    head = bytes([0, 0, code, arr.ndim]) + b"".join(int(s).to_bytes(4, "big") for s in arr.shape)
    with (gzip.open(path + ".gz", "wb") if gz else open(path, "wb")) as f:
        f.write(head + arr.tobytes())


@pytest.mark.parametrize("gz", [False, True])
def test_fashionmnist_reader(tmp_path, gz):
    r = np.random.RandomState(1)
    imgs = r.randint(0, 256, size=(9, 28, 28)).astype(np.uint8)
    labels = r.randint(0, 10, size=9).astype(np.uint8)
    raw = tmp_path / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    _write_idx(str(raw / "t10k-images-idx3-ubyte"), imgs, 0x08, gz)
    _write_idx(str(raw / "t10k-labels-idx1-ubyte"), labels, 0x08, gz)
    got, lab = D.load_test_split("FashionMNIST", str(tmp_path))
    assert np.array_equal(got, imgs) and np.array_equal(lab, labels.astype(np.int64))
    t = D.to_tensor(got[3])
    assert t.shape == (3, 28, 28) and torch.equal(t[0], torch.from_numpy(imgs[3]).float().div(255))
    assert torch.equal(D.to_tensor(got[3], 28), t)                      # Resize at the native size changes nothing


def test_cifar_reader(tmp_path):
    r = np.random.RandomState(2)
    flat = r.randint(0, 256, size=(5, 3072)).astype(np.uint8)
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    with open(d / "test_batch", "wb") as f:
        pickle.dump({"data": flat, "labels": [3, 1, 4, 1, 5]}, f)
    imgs, labels = D.load_test_split("cifar10", str(tmp_path))
    assert imgs.shape == (5, 32, 32, 3) and list(labels) == [3, 1, 4, 1, 5]
    t = D.to_tensor(imgs[2])
    assert torch.equal(t, torch.from_numpy(flat[2].reshape(3, 32, 32)).float().div(255))


def test_missing_dataset_file_names_the_path(tmp_path):
    with pytest.raises(FileNotFoundError, match="t10k-images-idx3-ubyte"):
        D.load_test_split("fashionmnist", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="test_batch"):
        D.load_test_split("cifar10", str(tmp_path))
    with pytest.raises(ValueError, match="Unknown dataset"):
        D.load_test_split("svhn", str(tmp_path))


def _ckpt(path, key):
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"model_state_dict": {key: torch.zeros(1)}, "epoch": 1}, path)


def test_layout_detection(tmp_path):
    van = tmp_path / "van"
    _ckpt(van / "vae" / "checkpoints" / "best.pt", "decoder.fc.weight")
    p = detect_layout(str(van))
    assert p.layout == "vanilla" and p.latents == van / "vae" / "latents_val" / "z.pt"
    assert p.codebook == van / "codebook" / "codebook.pt" and p.codes == van / "codebook" / "codes.npy"

    sp = tmp_path / "sp"
    _ckpt(sp / "vae" / "spatial_vae_fashionmnist" / "checkpoints" / "best.pt", "decoder.conv_in.weight")
    p = detect_layout(str(sp))
    assert p.layout == "spatial" and p.latents == sp / "vae" / "spatial_vae_fashionmnist" / "latents_val" / "z.pt"

    other = tmp_path / "elsewhere" / "best.pt"
    _ckpt(other, "decoder.conv_in.weight")
    p = detect_layout(str(tmp_path / "none"), vae_ckpt_path=str(other), latents_path=str(tmp_path / "z.pt"),
                      codebook_path=str(tmp_path / "cb.pt"))
    assert p.layout == "spatial" and p.latents == tmp_path / "z.pt" and p.codebook == tmp_path / "cb.pt"
    with pytest.raises(FileNotFoundError, match="vae_ckpt_path"):
        detect_layout(str(tmp_path / "none"))


@pytest.mark.parametrize("cli", CLIS)
def test_cli_help(cli):
    r = subprocess.run([sys.executable, "-m", f"vqvae_amd.scripts.{cli}", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--" in r.stdout

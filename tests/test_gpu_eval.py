"""GPU checks of the evaluation stage: geo_image_pair_moments against an fp64 numpy restatement, its determinism, the GPU
metrics against the CPU ones, the three evaluate_* CLIs against the reference's JSON (tests/golden/eval_*.json), the spatial
extension and the recorded assignment path."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

from vqvae_amd import _lib
from vqvae_amd.eval import reconstruction as R
from vqvae_amd.eval.metrics import MAX_PIX, codebook_stats, image_pair_moments, psnr, ssim_simple
from vqvae_amd.spatial_decoder import SpatialDecoder

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda", 0)


def moments_ref(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """fp64 restatement: means, biased centred variances and covariance, sum of squared differences."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    mx, my = x.mean(1), y.mean(1)
    dx, dy = x - mx[:, None], y - my[:, None]
    return np.stack([mx, my, (dx * dx).mean(1), (dy * dy).mean(1), (dx * dy).mean(1), ((x - y) ** 2).sum(1)], 1)


def assert_moments_close(got: np.ndarray, ref: np.ndarray, x: np.ndarray, y: np.ndarray):
    """1e-12 relative; quantities that cancel to ~0 (a covariance, a constant image's variance) against the image's scale."""
    scale = np.maximum(np.abs(x).max(1), np.abs(y).max(1)).astype(np.float64) ** 2 + 1e-300
    for k in range(6):
        s = scale * (x.shape[1] if k == 5 else 1)
        err = np.abs(got[:, k] - ref[:, k])
        assert (err <= 1e-12 * np.maximum(np.abs(ref[:, k]), s if k >= 2 else np.sqrt(s))).all(), (k, err.max())


SHAPES = [(b, p) for b in (1, 7) for p in (1, 3, 784, 785, 3072, 16384)] + [(60000, 784), (60000, 3), (60000, 1)]


@pytest.mark.parametrize("B,P", SHAPES)
def test_moments_match_fp64_restatement(B, P):
    r = np.random.RandomState(B * 7 + P)
    x = r.rand(B, P).astype(np.float32)
    y = (x + 0.1 * r.randn(B, P)).astype(np.float32)
    got = image_pair_moments(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)).cpu().numpy()
    assert_moments_close(got, moments_ref(x, y), x, y)


@pytest.mark.parametrize("P", [784, 785, 3072])
def test_moments_constant_images(P):
    x = np.full((5, P), 0.3, np.float32)
    y = np.full((5, P), 0.7, np.float32)
    y[2] = 0.3
    got = image_pair_moments(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)).cpu().numpy()
    assert (got[:, 2:5] == 0).all()
    assert np.array_equal(got[:, 0], np.full(5, np.float64(np.float32(0.3))))
    assert got[2, 5] == 0 and abs(got[0, 5] - P * (np.float64(np.float32(0.7)) - np.float64(np.float32(0.3))) ** 2) < 1e-12 * P


def test_n_pix_above_the_cap_is_rejected_without_launch():
    x = torch.rand(2, MAX_PIX + 1, device=DEV)
    out = torch.full((2, 6), -7.0, dtype=torch.float64, device=DEV)
    L = _lib.load()
    st = L.geo_image_pair_moments(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), 2, MAX_PIX + 1,
                                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == -1                                                       # GEO_E_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.geo_image_pair_moments(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), 2, 0,
                                    ctypes.c_void_p(out.data_ptr()), None) == -1


@pytest.mark.parametrize("P", [784, 785, 3072, 16384])
def test_moments_bit_identical_across_calls_streams_and_batches(P):
    g = torch.Generator(device=DEV).manual_seed(P)
    x = torch.rand(33, P, device=DEV, generator=g)
    y = torch.rand(33, P, device=DEV, generator=g)
    a = image_pair_moments(x, y)
    b = image_pair_moments(x, y)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = image_pair_moments(x, y)
    with torch.cuda.stream(s2):
        d = image_pair_moments(x, y)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    for i in (0, 5, 32):                                                   # an image alone gives the same bits as in the batch
        assert torch.equal(image_pair_moments(x[i:i + 1], y[i:i + 1])[0], a[i])
    assert torch.equal(image_pair_moments(x[3:10], y[3:10]), a[3:10])


PAIRS = ("rand4_c1_28", "rand4_c3_32", "close4_c1_28", "const4_c1_28", "ident4_c3_32", "rand3_c3_32", "const3_c1_28",
         "struct4_c1_28")


@pytest.mark.parametrize("name", PAIRS)
def test_gpu_metrics_equal_cpu_metrics(golden, name):
    g = golden("eval")
    x, y = torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"])
    assert abs(psnr(x.to(DEV), y.to(DEV)) - psnr(x, y)) <= 1e-12 * 100
    assert abs(ssim_simple(x.to(DEV), y.to(DEV)) - ssim_simple(x, y)) <= 1e-12
    assert abs(psnr(x.to(DEV), y.to(DEV)) - float(g[f"{name}/psnr"])) <= 1e-4
    assert abs(ssim_simple(x.to(DEV), y.to(DEV)) - float(g[f"{name}/ssim"])) <= 1e-5


def test_gpu_codebook_stats_equal_cpu(golden):
    g = golden("eval")
    for name in ("codes_dead", "codes_kbig", "codes_neg", "codes_allneg"):
        c, K = torch.from_numpy(g[f"{name}/codes"]), int(g[f"{name}/K"])
        assert codebook_stats(c.to(DEV), K) == codebook_stats(c, K)


def test_psnr_of_images_longer_than_the_cap():
    x, y = torch.rand(2, 3, 80, 80), torch.rand(2, 3, 80, 80)
    assert abs(psnr(x.to(DEV), y.to(DEV)) - psnr(x, y)) <= 1e-10
    with pytest.raises(ValueError, match="at most"):
        ssim_simple(x.to(DEV), y.to(DEV))


# ---- the CLIs on the reference's synthetic experiment

def _experiment(tmp_path, g):
    import gzip
    exp = tmp_path / "exp"
    for sub in ("vae/checkpoints", "vae/latents_val", "codebook"):
        (exp / sub).mkdir(parents=True)
    state = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("vae/")}
    torch.save({"model_state_dict": state, "epoch": 3}, exp / "vae/checkpoints/best.pt")
    torch.save(torch.from_numpy(g["exp/z"]), exp / "vae/latents_val/z.pt")
    torch.save(torch.from_numpy(g["exp/mu"]), exp / "vae/latents_val/mu.pt")
    torch.save({"z_medoid": torch.from_numpy(g["exp/z_medoid"])}, exp / "codebook/codebook.pt")
    raw = tmp_path / "data" / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    for fname, arr in (("t10k-images-idx3-ubyte", g["exp/test_images"]), ("t10k-labels-idx1-ubyte", g["exp/test_labels"])):
        head = bytes([0, 0, 0x08, arr.ndim]) + b"".join(int(s).to_bytes(4, "big") for s in arr.shape)
        with gzip.open(raw / (fname + ".gz"), "wb") as f:
            f.write(head + arr.astype(np.uint8).tobytes())
    cfg = tmp_path / "vae.yaml"
    cfg.write_text(yaml.safe_dump(json.loads(str(g["exp/config"]))))
    return exp, cfg


def _compare(got: dict, ref: dict):
    assert list(got) == list(ref)
    for k, v in ref.items():
        if isinstance(v, float):
            tol = 1e-4 if "psnr" in k else 1e-5 if ("ssim" in k or k == "entropy") else 1e-9
            assert abs(got[k] - v) <= tol, (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)


def test_clis_match_reference_json(tmp_path, golden):
    from vqvae_amd.scripts import evaluate_codebook_health, evaluate_quantization_loss, evaluate_vae_quality
    g = golden("eval")
    exp, cfg = _experiment(tmp_path, g)
    n = str(int(g["exp/max_samples"]))
    runs = {
        "vae_quality": (evaluate_vae_quality, ["--experiment", str(exp), "--config", str(cfg), "--max_samples", n,
                                               "--batch_size", "16"], "vae/vae_quality_assessment.json"),
        "quantization_loss": (evaluate_quantization_loss, ["--experiment", str(exp), "--dataset", "fashionmnist",
                                                           "--max_samples", n, "--batch_size", "16", "--data_root",
                                                           str(tmp_path / "data"), "--seed", str(int(g["exp/randperm_seed"]))],
                              "evaluation/quantization_analysis.json"),
        "codebook_health": (evaluate_codebook_health, ["--experiment", str(exp), "--dataset", "fashionmnist", "--batch_size",
                                                       "16"], "evaluation/codebook_health.json"),
    }
    for name, (mod, argv, rel) in runs.items():
        assert mod.main(argv) == int(g[f"cli/{name}/status"]), name
        with open(exp / rel) as f:
            got = json.load(f)
        with open(os.path.join(GOLDEN, f"eval_{name}.json")) as f:
            ref = json.load(f)
        _compare(got, ref)
    assert R.last_assign_path() == "hip"


# ---- spatial extension and assignment paths

def _clustered(n_rows, C, K, seed):
    r = np.random.RandomState(seed)
    zm = (3 * r.randn(K, C)).astype(np.float32)
    rows = (zm[r.randint(0, K, n_rows)] + 0.05 * r.randn(n_rows, C)).astype(np.float32)
    return rows, zm


def test_spatial_quantize_decode_against_fp64_restatement():
    N, C, h, w, K = 24, 8, 4, 4, 16
    rows, zm = _clustered(N * h * w, C, K, 3)
    z = torch.from_numpy(rows).view(N, h, w, C).permute(0, 3, 1, 2).contiguous().to(DEV)
    torch.manual_seed(0)
    dec = SpatialDecoder(1, (64, 32, 16), C, 28, "batch").to(DEV)
    codes, zq = R.quantize(z, torch.from_numpy(zm))
    assert R.last_assign_path() == "hip"
    flat = z.permute(0, 2, 3, 1).reshape(-1, C).double()
    ref_codes = ((flat[:, None, :] - torch.from_numpy(zm).to(DEV).double()[None]) ** 2).sum(-1).argmin(1)
    assert torch.equal(codes.reshape(-1), ref_codes) and codes.shape == (N, h, w)
    ref_zq = torch.from_numpy(zm).to(DEV)[ref_codes].view(N, h, w, C).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(zq, ref_zq)
    mom = R.decode_pair_moments(dec, z, zq, dataset="fashionmnist", apply_sigmoid=True, batch_size=N, return_images=True)
    assert not dec.training
    with torch.no_grad():
        xa = torch.sigmoid(dec(z)).reshape(N, -1)
        xb = torch.sigmoid(dec(ref_zq)).reshape(N, -1)
    assert torch.equal(mom["a"].reshape(N, -1), xa) and torch.equal(mom["b"].reshape(N, -1), xb)
    a, b = xa.double().cpu().numpy(), xb.double().cpu().numpy()
    assert_moments_close(mom["a_b"].cpu().numpy(), moments_ref(a, b), a, b)
    p, s = R.metrics_from_moments(mom["a_b"], mom["n_pix"])
    assert abs(p - psnr(xa.view(N, 1, 28, 28).cpu(), xb.view(N, 1, 28, 28).cpu())) <= 1e-10
    assert abs(s - ssim_simple(xa.view(N, 1, 28, 28).cpu(), xb.view(N, 1, 28, 28).cpu())) <= 1e-12


def test_spatial_codebook_health_cli(tmp_path):
    from vqvae_amd.scripts import evaluate_codebook_health
    N, C, K = 20, 8, 16
    rows, zm = _clustered(N * 16, C, K, 4)
    torch.manual_seed(1)
    dec = SpatialDecoder(1, (64, 32, 16), C, 28, "batch")
    run = tmp_path / "exp" / "vae" / "spatial_vae_fashionmnist"
    (run / "checkpoints").mkdir(parents=True)
    (run / "latents_val").mkdir()
    (tmp_path / "exp" / "codebook").mkdir()
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}, "epoch": 1},
               run / "checkpoints" / "best.pt")
    z = torch.from_numpy(rows).view(N, 4, 4, C).permute(0, 3, 1, 2).contiguous()
    torch.save(z, run / "latents_val" / "z.pt")
    torch.save({"z_medoid": torch.from_numpy(zm), "config": {"in_channels": 1, "output_image_size": 28, "latent_dim": C,
                "dec_channels": [64, 32, 16], "norm_type": "batch", "recon_loss": "mse", "mse_use_sigmoid": True}},
               tmp_path / "exp" / "codebook" / "codebook.pt")
    assert evaluate_codebook_health.main(["--experiment", str(tmp_path / "exp")]) == 0
    got = json.loads((tmp_path / "exp" / "evaluation" / "codebook_health.json").read_text())
    ref_codes = ((torch.from_numpy(rows).double()[:, None] - torch.from_numpy(zm).double()[None]) ** 2).sum(-1).argmin(1)
    st = codebook_stats(ref_codes, K)
    assert got["samples_evaluated"] == N and got["codebook_size"] == K
    assert got["used_codes"] == st["used"] and got["dead_codes"] == st["dead_codes"]
    assert abs(got["entropy"] - st["entropy"]) <= 1e-6


@pytest.mark.parametrize("n,d,K,path", [(500, 16, 32, "hip"), (500, 130, 32, "torch_fp64"), (20, 16, 32, "torch_fp64"),
                                        (5000, 8, 4096, "hip")])
def test_assignment_path_on_both_sides_of_the_envelope(n, d, K, path):
    r = np.random.RandomState(n + d + K)
    z = torch.from_numpy(r.randn(n, d).astype(np.float32)).to(DEV)
    zm = torch.from_numpy(r.randn(K, d).astype(np.float32)).to(DEV)
    codes = R.nearest_medoid_assign(z, zm)
    assert R.last_assign_path() == path
    e = ((z.double()[:, None] - zm.double()[None]) ** 2).sum(-1)
    best = e.gather(1, codes[:, None])[:, 0]
    assert torch.allclose(best, e.min(1).values, rtol=1e-12, atol=0)

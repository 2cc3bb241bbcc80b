"""Writes tests/golden/eval.npz and the three eval_*.json fixtures from the reference's src/eval (metrics and the three
evaluate_* main()s).  Only inputs and outputs are stored; nothing of the reference's code.

  - metrics: psnr, ssim_simple (4-D and 3-D), codebook_stats on fixed random and structured inputs: constant images, identical
    pairs (mse clamped), 1 and 3 channels, 28 and 32 px, codes with -1, dead codes and K above the largest code;
  - CLIs: a tiny synthetic vanilla experiment (random-weight VAE with small channels, validation latents, codebook.pt, a fake
    FashionMNIST test split in idx format).  The reference imports torchvision at module top, which may not be installed, so
    a stub torchvision module serves the fake test split through the one dataset class the scripts construct (and the three
    transforms they compose).  The real-sample permutation is torch.randperm(n, generator=torch.Generator().manual_seed(SEED)),
    which is what `--seed SEED` does in vqvae_amd.scripts.evaluate_quantization_loss.
  - admission: the experiment's seed is admitted only when the reference's float32 a^2 + b^2 - 2ab argmin equals the exact
    fp64 argmin on every validation row, with the fp64 gap between the best and second-best medoid above a bound on the float32
    expansion's error (8 (d + 2) 2^-24 (|a|^2 + max |b|^2), the bound of csrc/kmeans.hip's screen), so the change of
    assignment rule cannot move a code.

    python tools/gen_golden_eval.py /path/to/reference/checkout
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 7
ARCH = {"in_channels": 1, "enc_channels": [8, 16, 32], "dec_channels": [32, 16, 8], "latent_dim": 4, "recon_loss": "mse",
        "norm_type": "batch", "mse_use_sigmoid": True, "output_image_size": 28}
N_VAL, K, N_TEST, MAX_SAMPLES = 48, 12, 80, 32


def metric_inputs():
    """name -> (x, y) float32 arrays, and name -> (codes, K)."""
    r = np.random.RandomState(11)
    pairs = {
        "rand4_c1_28": (r.rand(6, 1, 28, 28), r.rand(6, 1, 28, 28)),
        "rand4_c3_32": (r.rand(5, 3, 32, 32), r.rand(5, 3, 32, 32)),
        "close4_c1_28": None,
        "const4_c1_28": (np.full((3, 1, 28, 28), 0.25), np.full((3, 1, 28, 28), 0.75)),
        "ident4_c3_32": None,
        "rand3_c3_32": (r.rand(3, 32, 32), r.rand(3, 32, 32)),
        "const3_c1_28": (np.full((1, 28, 28), 0.5), np.full((1, 28, 28), 0.5)),
        "struct4_c1_28": None,
    }
    base = r.rand(4, 1, 28, 28)
    pairs["close4_c1_28"] = (base, np.clip(base + 0.01 * r.randn(4, 1, 28, 28), 0, 1))
    same = r.rand(2, 3, 32, 32)
    pairs["ident4_c3_32"] = (same, same.copy())
    g = np.linspace(0, 1, 28)
    ramp = np.broadcast_to(g[None, None, None, :], (3, 1, 28, 28)).copy()
    pairs["struct4_c1_28"] = (ramp, ramp[..., ::-1].copy())
    pairs = {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in pairs.items()}
    codes = {
        "codes_dead": (np.array([0, 1, 1, 3, 3, 3, 7, -1, -1, 2], np.int64), 8),
        "codes_kbig": (r.randint(0, 20, size=500).astype(np.int64), 64),
        "codes_neg": (np.concatenate([r.randint(-1, 5, size=100), [-1, -1]]).astype(np.int64), 5),
        "codes_allneg": (np.full(7, -1, np.int64), 4),
        "codes_uniform": (np.arange(256, dtype=np.int64) % 16, 16),
    }
    return pairs, codes


def stub_torchvision(images: np.ndarray, labels: np.ndarray):
    """A torchvision stand-in: datasets.FashionMNIST over the given arrays, transforms Compose / ToTensor / Lambda."""
    from PIL import Image

    tv = types.ModuleType("torchvision")
    ds = types.ModuleType("torchvision.datasets")
    tr = types.ModuleType("torchvision.transforms")

    class FashionMNIST:
        def __init__(self, root, train=True, download=False, transform=None):
            assert not train
            self.transform = transform

        def __len__(self):
            return len(images)

        def __getitem__(self, i):
            img = Image.fromarray(images[int(i)], mode="L")
            return (self.transform(img) if self.transform else img), int(labels[int(i)])

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class ToTensor:
        def __call__(self, pic):
            t = torch.from_numpy(np.array(pic, copy=True))
            return t.view(pic.size[1], pic.size[0], -1).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Lambda:
        def __init__(self, f):
            self.f = f

        def __call__(self, x):
            return self.f(x)

    ds.FashionMNIST = FashionMNIST
    ds.CIFAR10 = None
    tr.Compose, tr.ToTensor, tr.Lambda = Compose, ToTensor, Lambda
    tv.datasets, tv.transforms = ds, tr
    sys.modules.update({"torchvision": tv, "torchvision.datasets": ds, "torchvision.transforms": tr})


def admitted(z: np.ndarray, zm: np.ndarray) -> bool:
    """float32 expansion argmin == fp64 argmin on every row, with the fp64 gap above the expansion's error bound."""
    zt, mt = torch.from_numpy(z), torch.from_numpy(zm)
    d2 = (zt ** 2).sum(1, keepdim=True) + (mt ** 2).sum(1).view(1, -1) - 2.0 * zt @ mt.t()
    f32 = d2.argmin(1).numpy()
    e = ((z.astype(np.float64)[:, None, :] - zm.astype(np.float64)[None]) ** 2).sum(-1)
    srt = np.sort(e, axis=1)
    bound = 8 * (z.shape[1] + 2) * 2.0 ** -24 * ((z.astype(np.float64) ** 2).sum(1) + (zm.astype(np.float64) ** 2).sum(1).max())
    return bool((f32 == e.argmin(1)).all() and (srt[:, 1] - srt[:, 0] > bound).all())


def main(ref_root: str):
    sys.path.insert(0, ref_root)
    out = {}
    pairs, codes = metric_inputs()
    from src.eval.metrics import codebook_stats, psnr, ssim_simple
    for name, (a, b) in pairs.items():
        x, y = torch.from_numpy(a), torch.from_numpy(b)
        out[f"{name}/x"], out[f"{name}/y"] = a, b
        out[f"{name}/psnr"] = np.float64(psnr(x, y))
        out[f"{name}/ssim"] = np.float64(ssim_simple(x, y))
    for name, (c, k) in codes.items():
        s = codebook_stats(torch.from_numpy(c), k)
        out[f"{name}/codes"], out[f"{name}/K"] = c, np.int64(k)
        out[f"{name}/entropy"], out[f"{name}/dead"], out[f"{name}/used"] = (np.float64(s["entropy"]), np.int64(s["dead_codes"]),
                                                                           np.int64(s["used"]))

    # ---- the synthetic vanilla experiment
    from src.models.vae import VAE
    seed = SEED
    while True:
        torch.manual_seed(seed)
        vae = VAE(in_channels=1, enc_channels=ARCH["enc_channels"], dec_channels=ARCH["dec_channels"],
                  latent_dim=ARCH["latent_dim"], recon_loss="mse", output_image_size=28, norm_type="batch").eval()
        r = np.random.RandomState(seed)
        mu = r.randn(N_VAL, ARCH["latent_dim"]).astype(np.float32)
        z = (mu + 0.3 * r.randn(*mu.shape)).astype(np.float32)
        zm = r.randn(K, ARCH["latent_dim"]).astype(np.float32)
        if admitted(z, zm):
            break
        seed += 1
    imgs = r.randint(0, 256, size=(N_TEST, 28, 28)).astype(np.uint8)
    labels = (np.arange(N_TEST) % 10).astype(np.uint8)
    state = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    for k, v in state.items():
        out[f"vae/{k}"] = v.numpy()
    out.update({"exp/seed": np.int64(seed), "exp/z": z, "exp/mu": mu, "exp/z_medoid": zm, "exp/test_images": imgs,
                "exp/test_labels": labels, "exp/config": np.array(json.dumps({"model": ARCH, "data": {"name": "FashionMNIST"}})),
                "exp/randperm_seed": np.int64(SEED), "exp/max_samples": np.int64(MAX_SAMPLES)})

    stub_torchvision(imgs, labels)
    import yaml
    from src.eval import evaluate_codebook_health, evaluate_quantization_loss, evaluate_vae_quality
    real_randperm = torch.randperm
    with tempfile.TemporaryDirectory() as tmp:
        exp = os.path.join(tmp, "exp")
        for sub in ("vae/checkpoints", "vae/latents_val", "codebook"):
            os.makedirs(os.path.join(exp, sub))
        torch.save({"model_state_dict": state, "epoch": 3}, os.path.join(exp, "vae/checkpoints/best.pt"))
        torch.save(torch.from_numpy(z), os.path.join(exp, "vae/latents_val/z.pt"))
        torch.save(torch.from_numpy(mu), os.path.join(exp, "vae/latents_val/mu.pt"))
        torch.save({"z_medoid": torch.from_numpy(zm)}, os.path.join(exp, "codebook/codebook.pt"))
        cfg = os.path.join(tmp, "vae.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump({"model": ARCH, "data": {"name": "FashionMNIST"}}, f)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            runs = {
                "vae_quality": (evaluate_vae_quality, ["--experiment", exp, "--config", cfg, "--max_samples", str(MAX_SAMPLES),
                                                       "--batch_size", "16"], "vae/vae_quality_assessment.json"),
                "quantization_loss": (evaluate_quantization_loss, ["--experiment", exp, "--dataset", "fashionmnist",
                                                                   "--max_samples", str(MAX_SAMPLES), "--batch_size", "16"],
                                      "evaluation/quantization_analysis.json"),
                "codebook_health": (evaluate_codebook_health, ["--experiment", exp, "--dataset", "fashionmnist",
                                                               "--batch_size", "16"], "evaluation/codebook_health.json"),
            }
            for name, (mod, argv, rel) in runs.items():
                torch.manual_seed(SEED)
                torch.randperm = lambda n, *a, **k: real_randperm(n, generator=torch.Generator().manual_seed(SEED))
                sys.argv = [name] + argv
                try:
                    status = mod.main()
                finally:
                    torch.randperm = real_randperm
                with open(os.path.join(exp, rel)) as f:
                    result = json.load(f)
                out[f"cli/{name}/status"] = np.int64(status)
                with open(os.path.join(GOLDEN, f"eval_{name}.json"), "w") as f:
                    json.dump(result, f, indent=2)
                    f.write("\n")
        finally:
            os.chdir(cwd)
    np.savez_compressed(os.path.join(GOLDEN, "eval.npz"), **out)
    print(f"wrote {len(out)} arrays, experiment seed {seed}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT", "../reference"))

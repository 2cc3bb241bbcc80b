"""Timing of batch assembly and of the spatial-VAE training step, torch batch path against the batch kernel.

    python tools/exp_spatial_vae_train.py --out profiles/spatial_vae_train.json

Synthetic resident uint8 data of the real shapes (FashionMNIST 60 000 x 28 x 28 x 1, CIFAR-10 50 000 x 32 x 32 x 3, batch 256):
neither the loader nor the step depends on pixel values, so no data set files are needed.
  (a) loader: ms per batch of a whole shuffled epoch of ResidentLoader, fused=False (the torch expression) against fused=True
      (geo_batch_assemble), plain for both sets and with crop_flip for CIFAR-10.  The window holds what the trainer waits for
      per batch: the sampler, the random draws, the host-to-device copies and the kernels.
  (b) step: ms per training step (SpatialTrainingEngine.run_epoch over `--steps` batches) of the reference's two spatial
      configurations (fashionmnist and cifar10 spatial/geodesic/vae.yaml: AdamW, clip 1.0, CIFAR-10 with crop_flip) with each loader.
Times are host clocks around windows that end in a device synchronise.  Every variant is warmed up, the variants alternate,
`--repeats` windows each, and the median, minimum and maximum are reported.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vqvae_amd.spatial_vae import SpatialVAE
from vqvae_amd.training.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader, resident_images
from vqvae_amd.training.spatial_engine import SpatialTrainingEngine

SETS = {"fashionmnist": dict(n=60000, size=28, channels=1, normalize=None, crop_flip=False,
                             model=dict(in_channels=1, output_image_size=28, latent_dim=16, enc_channels=[64, 128, 256],
                                        dec_channels=[256, 128, 64], recon_loss="mse", norm_type="batch", mse_use_sigmoid=True)),
        "cifar10": dict(n=50000, size=32, channels=3, normalize=(CIFAR_MEAN, CIFAR_STD), crop_flip=True,
                        model=dict(in_channels=3, output_image_size=32, latent_dim=32, enc_channels=[64, 128, 256],
                                   dec_channels=[256, 128, 64], recon_loss="mse", norm_type="batch", mse_use_sigmoid=False))}


def sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def alternate(variants, repeats):
    """{name: summary of ms per unit}; variants = {name: (fn, units per call)}: one warm-up call each, then alternating windows."""
    for fn, _ in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, units) in variants.items():
            times[k].append(sync_time(fn) / units)
    return {k: summary(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=0, help="images per set; 0 = the real counts")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda")
    B = args.batch
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "steps": args.steps, "repeats": args.repeats, "loader_ms_per_batch": {},
              "train_step_ms": {}}
    for name, cfg in SETS.items():
        n = args.images or cfg["n"]
        r = np.random.RandomState(0)
        shape = (n, cfg["size"], cfg["size"]) + ((cfg["channels"],) if cfg["channels"] > 1 else ())
        data = resident_images(r.randint(0, 256, shape).astype(np.uint8), r.randint(0, 10, n), dev, cfg["normalize"])

        def epoch_of(loader):
            def fn():
                for x, _ in loader:
                    pass
            return fn, len(loader)

        modes = [("plain", False)] + ([("crop_flip", True)] if cfg["crop_flip"] else [])
        variants = {f"{mode}/{'kernel' if fused else 'torch'}": epoch_of(ResidentLoader(data, B, True, cfg["normalize"], crop_flip=cf, fused=fused))
                    for mode, cf in modes for fused in (False, True)}
        result["loader_ms_per_batch"][name] = dict(alternate(variants, args.repeats), batches_per_epoch=(n + B - 1) // B,
                                                   output_bytes_per_batch=4 * B * cfg["channels"] * cfg["size"] ** 2)

        small = resident_images(data.u8[:B * args.steps].cpu().numpy(), np.zeros(B * args.steps, dtype=np.int64), dev, cfg["normalize"])
        steps = {}
        for fused in (False, True):
            torch.manual_seed(0)
            model = SpatialVAE(**cfg["model"]).to(dev)
            engine = SpatialTrainingEngine(model, torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5), dev)
            loader = ResidentLoader(small, B, True, cfg["normalize"], crop_flip=cfg["crop_flip"], fused=fused)
            steps["kernel" if fused else "torch"] = ((lambda e=engine, l=loader: e.run_epoch(l, True, 0, 0, 1.0, 1.0, 0)), len(loader))
        with contextlib.redirect_stdout(io.StringIO()):
            result["train_step_ms"][name] = alternate(steps, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("loader_ms_per_batch", "train_step_ms")}))


if __name__ == "__main__":
    main()

"""Timing of the evaluation stage on one MI355X.  Writes profiles/eval_<name>.json (or --out):
  - geo_image_pair_moments at 10 000 x 3072 and 60 000 x 784: median kernel time (HIP events, 20 launches after 3 warm-ups)
    and the fraction of the HBM model, 2 n_images n_pix 4 bytes at the measured 6.29 TB/s float4 copy rate;
  - evaluate_codebook_health end to end on a 60 000-latent spatial FashionMNIST-shaped experiment (latents 16 x 4 x 4, K 512,
    decoder 256-128-64 with batch norm, random weights) written to a temporary directory, with the stage times of the same
    work: loading, assignment, decode (+ post-processing) and the moments kernel.

    python tools/exp_eval.py [--out profiles/eval_mi355x.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd.eval import reconstruction as R  # noqa: E402
from vqvae_amd.eval.metrics import image_pair_moments  # noqa: E402
from vqvae_amd.scripts import evaluate_codebook_health  # noqa: E402
from vqvae_amd.spatial_decoder import SpatialDecoder  # noqa: E402

HBM_BPS = 6.29e12            # measured float4 copy (MI355X_MICROARCH.md)
DEV = torch.device("cuda", 0)


def kernel_time(B, P, reps=20):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.rand(B, P, device=DEV, generator=g)
    y = torch.rand(B, P, device=DEV, generator=g)
    for _ in range(3):
        image_pair_moments(x, y)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        image_pair_moments(x, y)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    t = float(np.median(ts))
    model = 2 * B * P * 4 / HBM_BPS
    return {"n_images": B, "n_pix": P, "median_s": t, "min_s": float(min(ts)), "hbm_model_s": model,
            "fraction_of_hbm_model": model / t, "bytes": 2 * B * P * 4}


def spatial_experiment(tmp):
    N, C, K = 60_000, 16, 512
    r = np.random.RandomState(0)
    zm = r.randn(K, C).astype(np.float32)
    rows = (zm[r.randint(0, K, N * 16)] + 0.3 * r.randn(N * 16, C)).astype(np.float32)
    torch.manual_seed(0)
    dec = SpatialDecoder(1, (256, 128, 64), C, 28, "batch")
    run = os.path.join(tmp, "exp", "vae", "spatial_vae_fashionmnist")
    os.makedirs(os.path.join(run, "checkpoints"))
    os.makedirs(os.path.join(run, "latents_val"))
    os.makedirs(os.path.join(tmp, "exp", "codebook"))
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}, "epoch": 1},
               os.path.join(run, "checkpoints", "best.pt"))
    z = torch.from_numpy(rows).view(N, 4, 4, C).permute(0, 3, 1, 2).contiguous()
    torch.save(z, os.path.join(run, "latents_val", "z.pt"))
    torch.save({"z_medoid": torch.from_numpy(zm), "config": {"in_channels": 1, "output_image_size": 28, "latent_dim": C,
                "dec_channels": [256, 128, 64], "norm_type": "batch", "recon_loss": "mse", "mse_use_sigmoid": True}},
               os.path.join(tmp, "exp", "codebook", "codebook.pt"))
    return os.path.join(tmp, "exp"), dec, z, torch.from_numpy(zm)


def sync_time(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def end_to_end(reps=3):
    with tempfile.TemporaryDirectory() as tmp:
        exp, dec, z, zm = spatial_experiment(tmp)
        walls = []
        for _ in range(reps):
            with contextlib.redirect_stdout(io.StringIO()):
                _, t = sync_time(lambda: evaluate_codebook_health.main(["--experiment", exp]))
            walls.append(t)
        result = json.load(open(os.path.join(exp, "evaluation", "codebook_health.json")))
    dec = dec.to(DEV).eval()
    zd = z.to(DEV)
    stages = {"assign": [], "decode": [], "moments": []}
    for _ in range(reps):
        (codes, zq), t = sync_time(lambda: R.quantize(zd, zm))
        stages["assign"].append(t)
        imgs = []

        def decode():
            with torch.no_grad():
                for i in range(0, len(zd), 512):
                    imgs.append((torch.sigmoid(dec(zd[i:i + 512])).reshape(-1, 784),
                                 torch.sigmoid(dec(zq[i:i + 512])).reshape(-1, 784)))
        _, t = sync_time(decode)
        stages["decode"].append(t)
        _, t = sync_time(lambda: [image_pair_moments(a, b) for a, b in imgs])
        stages["moments"].append(t)
    med = {k: float(np.median(v)) for k, v in stages.items()}
    wall = float(np.median(walls))
    return {"n_latents": int(z.shape[0]), "positions": int(z.shape[0] * 16), "K": int(zm.shape[0]),
            "assign_path": R.last_assign_path(), "wall_s_median": wall, "wall_s": walls, "stage_s_median": med,
            "decode_share_of_wall": med["decode"] / wall, "result": result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_mi355x.json"))
    args = ap.parse_args()
    rep = {"device": torch.cuda.get_device_name(0), "hbm_bps_model": HBM_BPS,
           "kernel": [kernel_time(10_000, 3072), kernel_time(60_000, 784)], "codebook_health_spatial_60k": end_to_end()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=2)
    print(json.dumps(rep, indent=2))


if __name__ == "__main__":
    main()

"""Native image encode against the torch modules on one MI355X.  Writes profiles/encode_mi355x.json (or --out).

Per shape, three routes, all warmed up three times and then alternating in one process:
  - native: vqvae_amd.encode.encode_latents on a prepared export (the HIP kernels of csrc/encode.hip);
  - encoder_batch512 / encoder_batch4096: the module's encoder alone in eval() under no_grad, in batches of 512 (the size of
    encode_latents' own torch route) and of 4096 (the native pass size), outputs concatenated;
  - model_batch512: whole model(x) in batches of 512, keeping z, mu and logvar as utils/latents.py and
    utils/spatial_latents.py do today (the decoder runs and its output is dropped).
A repetition is the host clock around 10 consecutive encodes ending in a device synchronise, divided by 10; every repetition is
listed.  Inputs are on the device before the clock starts.  Shapes: 10 000 and 60 000 images for each of vanilla 64-128-256
d 128 at 28 px, spatial 64-128-256 d 16 at 28 px, spatial 64-128-256 d 32 at 32 px x 3 channels, all with eval-mode BatchNorm.
Recorded with the times: the multiply-adds of one image (the three convolutions without border savings, and the head; the
rows that pad a 49-pixel output to two 32-row tiles are not counted) and the whole call's share of the f32 matrix peak -- an end-to-end rate over a peak, not a kernel's share
-- and the maximum absolute difference between the native outputs and the module's at the timed size.

    python tools/exp_encode.py [--out profiles/encode_mi355x.json] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd.encode import encode_latents, last_encode_path  # noqa: E402
from vqvae_amd.image_encoder import ImageEncoderExport  # noqa: E402
from vqvae_amd.spatial_vae import SpatialVAE  # noqa: E402
from vqvae_amd.vae import VAE  # noqa: E402

MFMA_F32_FLOPS = 157.3e12        # f32 matrix peak (MI355X_MICROARCH.md)
SIZES, INNER = (10_000, 60_000), 10
ENC, DEC = (64, 128, 256), (256, 128, 64)


def model_macs(kind, d, C, size):
    """Multiply-adds of one image: the three convolutions without border savings, and the head."""
    e1, e2, e3 = ENC
    s1, s2 = size // 2, size // 4
    head = 16 * e3 * 2 * d
    return s1 * s1 * 9 * C * e1 + s2 * s2 * 9 * e1 * e2 + 16 * 9 * e2 * e3 + head


def sync_time(f):
    """Seconds per call of INNER consecutive calls, the clock stopped after a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / INNER


def measure(kind, d, C, size, dev, reps):
    torch.manual_seed(0)
    if kind == "vanilla":
        model = VAE(in_channels=C, enc_channels=ENC, dec_channels=DEC, latent_dim=d, output_image_size=size, norm_type="batch")
    else:
        model = SpatialVAE(C, ENC, DEC, d, "mse", size, "batch")
    model = model.to(dev).eval()
    export = ImageEncoderExport(model.encoder, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for n in SIZES:
        x = torch.rand(n, C, size, size, device=dev, generator=g)

        @torch.no_grad()
        def encoder(batch):
            parts = [model.encoder(x[i:i + batch]) for i in range(0, n, batch)]
            return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

        @torch.no_grad()
        def whole(batch):
            parts = [model(x[i:i + batch])[1:] for i in range(0, n, batch)]
            return tuple(torch.cat([p[k] for p in parts]) for k in range(3))

        contestants = {"native": lambda: encode_latents(export, x), "encoder_batch512": lambda: encoder(512),
                       "encoder_batch4096": lambda: encoder(4096), "model_batch512": lambda: whole(512)}
        for _ in range(3):                                   # warm-up: code objects, convolution set-up, the workspace
            outs = {k: f() for k, f in contestants.items()}
        assert last_encode_path() == "hip"
        diff = max(float((outs["native"][i] - outs[k][i]).abs().max()) for k in outs if k != "native" for i in (0, 1))
        del outs
        times = {k: [] for k in contestants}
        for _ in range(reps):                                # alternating, one process
            for k, f in contestants.items():
                times[k].append(sync_time(f))
        best = min(times["native"])
        macs = model_macs(kind, d, C, size)
        row = {"encoder": kind, "n": n, "enc_channels": list(ENC), "latent_dim": d, "in_channels": C, "in_size": size,
               "encodes_per_timed_window": INNER, "model_multiply_adds_per_image": macs,
               "fraction_of_f32_matrix_peak_whole_call": 2 * macs * n / best / MFMA_F32_FLOPS,
               "max_abs_diff_native_vs_torch": diff}
        for k, ts in times.items():
            row[f"{k}_s"] = ts
            row[f"{k}_s_min"] = min(ts)
            row[f"{k}_s_median"] = float(np.median(ts))
            row[f"{k}_s_max"] = max(ts)
            row[f"{k}_us_per_image_min"] = min(ts) / n * 1e6
            if k != "native":
                row[f"{k}_over_native_min"] = min(ts) / best
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not isinstance(v, list) or k == "enc_channels"}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_mi355x.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_encode.py measures on the MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    rows = []
    for shape in (("vanilla", 128, 1, 28), ("spatial", 16, 1, 28), ("spatial", 32, 3, 32)):
        rows += measure(*shape, dev, args.reps)
    rep = {"device": torch.cuda.get_device_name(0), "f32_matrix_peak_flops": MFMA_F32_FLOPS, "reps": args.reps,
           "timing": "host clock around encodes_per_timed_window consecutive encodes ending in a device synchronise, per encode; "
                     "three warm-ups; routes alternating in one process",
           "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=2)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

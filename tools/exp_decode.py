"""Native image decode against the torch module on one MI355X.  Writes profiles/decode_mi355x.json (or --out).

Per shape, vqvae_amd.decode.decode_logits on a prepared export (the HIP kernels of csrc/vanilla_jvp.hip) and the same
module in eval() under no_grad, in batches of 512 (how eval.reconstruction.decode_pair_moments decodes) and in batches of
4096 (the native pass size; the 512-entry atlas is one batch either way), all warmed up and then alternating in one
process.  A repetition is the host clock around INNER consecutive decodes (10 of 10 000 images, 50 of an atlas), ending in
a device synchronise, divided by INNER; every repetition is listed.  Inputs are on the device before the clock starts.  Shapes:
  - 10 000 vanilla latents, decoder 256-128-64, d 128, 28 px; 10 000 spatial grids, 256-128-64, d 16, 28 px; 10 000 spatial
    grids, 256-128-64, d 32, 32 px, 3 channels; and the K = 512 atlas of each (every codebook entry through the codes path).
Recorded with the times: the model flops of one image (2 per multiply-add of the kernels' formulation, composed first
stage, no border savings) and the whole call's share of the f32 matrix peak -- an end-to-end rate over a peak, not a kernel's share:
the last layer runs on the vector units and the call includes its launches.  The native logits are compared with the module's
at the timed size (maximum absolute difference).

    python tools/exp_decode.py [--out profiles/decode_mi355x.json] [--reps 7]
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

from vqvae_amd.decode import decode_logits, last_decode_path  # noqa: E402
from vqvae_amd.spatial_decoder import SpatialDecoder, SpatialImageDecoderExport  # noqa: E402
from vqvae_amd.vae import Decoder  # noqa: E402
from vqvae_amd.vanilla_decoder import VanillaDecoderExport  # noqa: E402

MFMA_F32_FLOPS = 157.3e12        # f32 matrix peak (MI355X_MICROARCH.md)
N, K, TORCH_BATCHES = 10_000, 512, (512, 4096)
INNER = {"latents": 10, "atlas": 50}


def model_flops(kind, channels, d, C, size):
    """2 x the multiply-adds one image needs in the kernels' formulation (DESIGN.md section 15's count for the vanilla
    decoder): the composed first stage, ConvT2 as 16 taps per input pixel, ConvT3 at 4 taps per output pixel."""
    _, c1, c2 = channels
    s1 = size // 4 if kind == "vanilla" else 8
    front = d * s1 * s1 * c1 if kind == "vanilla" else 64 * 4 * (d + 1) * c1
    return 2 * (front + s1 * s1 * c1 * c2 * 16 + size * size * 4 * c2 * C)


def sync_time(f, inner):
    """Seconds per call of `inner` consecutive calls, the clock stopped after a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def measure(kind, channels, d, C, size, dev, reps):
    torch.manual_seed(0)
    if kind == "vanilla":
        dec = Decoder(C, channels, d, size, "batch").to(dev).eval()
        export = VanillaDecoderExport(dec, dev)
    else:
        dec = SpatialDecoder(C, channels, d, size, "batch").to(dev).eval()
        export = SpatialImageDecoderExport(dec, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn(K, d, device=dev, generator=g)
    if kind == "vanilla":
        z = torch.randn(N, d, device=dev, generator=g)
        atlas = torch.arange(K, device=dev)
        gathered = table
    else:
        z = torch.randn(N, d, 4, 4, device=dev, generator=g)
        atlas = torch.arange(K, device=dev).view(K, 1, 1).expand(K, 4, 4).contiguous()
        gathered = table[:, :, None, None].expand(K, d, 4, 4).contiguous()

    @torch.no_grad()
    def module(x, batch):
        return torch.cat([dec(x[i:i + batch]) for i in range(0, len(x), batch)])

    rows = []
    flops = model_flops(kind, channels, d, C, size)
    for what, native, x, n in (("latents", lambda: decode_logits(export, z), z, N),
                               ("atlas", lambda: decode_logits(export, table=table, codes=atlas), gathered, K)):
        contestants = {"native": native}
        for batch in TORCH_BATCHES:
            contestants[f"torch_batch{batch}"] = lambda x=x, batch=batch: module(x, batch)
        for _ in range(3):                                   # warm-up: code objects, convolution set-up, the workspace
            outs = {k: f() for k, f in contestants.items()}
        assert last_decode_path() == "hip"
        diff = max(float((outs["native"] - outs[k]).abs().max()) for k in outs if k != "native")
        times = {k: [] for k in contestants}
        for _ in range(reps):                                # alternating, one process
            for k, f in contestants.items():
                times[k].append(sync_time(f, INNER[what]))
        best = min(times["native"])
        row = {"decoder": kind, "what": what, "n": n, "dec_channels": list(channels), "latent_dim": d, "out_channels": C,
               "out_size": size, "decodes_per_timed_window": INNER[what], "model_flops_per_image": flops,
               "fraction_of_f32_matrix_peak_whole_call": flops * n / best / MFMA_F32_FLOPS,
               "max_abs_diff_native_vs_torch": diff}
        for k, ts in times.items():
            row[f"{k}_s"] = ts
            row[f"{k}_s_min"] = min(ts)
            row[f"{k}_s_median"] = float(np.median(ts))
            row[f"{k}_us_per_image_min"] = min(ts) / n * 1e6
            if k != "native":
                row[f"{k}_over_native_min"] = min(ts) / best
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not isinstance(v, list) or k == "dec_channels"}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mi355x.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_decode.py measures on the MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    rows = []
    for shape in (("vanilla", (256, 128, 64), 128, 1, 28), ("spatial", (256, 128, 64), 16, 1, 28),
                  ("spatial", (256, 128, 64), 32, 3, 32)):
        rows += measure(*shape, dev, args.reps)
    rep = {"device": torch.cuda.get_device_name(0), "f32_matrix_peak_flops": MFMA_F32_FLOPS, "torch_batches": list(TORCH_BATCHES),
           "reps": args.reps, "timing": "host clock around decodes_per_timed_window consecutive decodes ending in a device synchronise, per decode; alternating", "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=2)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

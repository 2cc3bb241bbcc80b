"""Pull-back metric tensor per latent on one MI355X (geo_decoder_metric_tensor through vqvae_amd.geo.pullback_metric_device):

    fm        60 000 x 16 latents, 28 px, 1 channel  (16 outputs; dec_channels 256-128-64, eval-mode BatchNorm)
    cf        50 000 x 16 latents, 32 px, 3 channels (192 outputs)
    autograd  the generic route (torch.func.jacfwd, float32; Gram and eigvalsh in fp64) on the first 1 024 latents of each shape

Times are host clocks around `--inner` consecutive calls that end in a device synchronise, after a warm-up call of the same shape;
every repetition is reported (the spread is the run-to-run noise).  The native time includes the decoder export.  Nothing is
extrapolated: the autograd route is timed at 1 024 latents only, and no ratio beyond the measured sizes is stated.
Writes profiles/metric_tensor_mi355x.json (or --out).

    python tools/exp_metric_tensor.py [--reps 5] [--inner 5] [--out FILE]
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

from vqvae_amd import _lib  # noqa: E402
from vqvae_amd.geo import riemannian_metric as rm  # noqa: E402
from vqvae_amd.spatial_decoder import DecoderExport, SpatialDecoder  # noqa: E402

SHAPES = {"fm": (60000, 16, 1, 28), "cf": (50000, 16, 3, 32)}
CHANNELS = (256, 128, 64)
N_AUTOGRAD = 1024


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner, out


def make_decoder(d, cout, px, dev):
    torch.manual_seed(0)
    dec = SpatialDecoder(cout, CHANNELS, d, px, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return dec.to(dev).eval()


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--inner", type=int, default=5)
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_tensor_mi355x.json"))
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "dec_channels": CHANNELS, "norm": "batch (eval)", "reps": args.reps,
              "calls_per_rep": args.inner, "shapes": {}}
    for name, (n, d, cout, px) in SHAPES.items():
        dec = make_decoder(d, cout, px, dev)
        assert rm.native_metric_covers(dec)
        z = torch.from_numpy(np.random.RandomState(1).randn(n, d).astype(np.float32)).to(dev)
        z_small = z[:N_AUTOGRAD].contiguous()

        def native():
            return rm.pullback_metric_device(dec, z)

        def native_small():
            return rm.pullback_metric_device(dec, z_small)

        def autograd():
            return rm.PullbackMetric(*rm._generic_metric(dec, z_small, True)[:4], route="autograd")

        native(), native_small(), autograd()                               # warm-up of every timed shape
        t_nat, t_small, t_auto = [], [], []
        for _ in range(args.reps):                                         # alternating
            t, got = timed(native, args.inner)
            t_nat.append(t)
            t, got_small = timed(native_small, args.inner)
            t_small.append(t)
            t, ref = timed(autograd, 1)
            t_auto.append(t)
        assert got.route == "native"
        diag = torch.sqrt(torch.diagonal(ref.G, dim1=1, dim2=2))
        err = ((got_small.G - ref.G).abs() / (diag[:, :, None] * diag[:, None, :])).max()
        ws = lib.geo_metric_tensor_workspace_bytes(DecoderExport(dec, dev).desc, n)
        result["shapes"][name] = {
            "latents": n, "latent_dim": d, "out_channels": cout, "px": px, "outputs": cout * (16 if px == 28 else 64),
            "workspace_bytes": int(ws), "native_s_per_call": t_nat, "native_latents_per_s_best": n / min(t_nat),
            "native_1024_s_per_call": t_small, "autograd_1024_s_per_call": t_auto,
            "rank_deficient": int((got.rank < d).sum()), "logvol_finite": int(torch.isfinite(got.logvol).sum()),
            "max_eig_ratio": float((got.eig[:, -1] / got.eig[:, 0].clamp_min(1e-300)).max()),
            "native_against_autograd_1024_max_normalised_G_difference": float(err)}
        print(name, json.dumps(result["shapes"][name]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

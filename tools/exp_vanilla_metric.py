"""Pull-back metric tensor per latent of the vanilla decoder on one MI355X (geo_vanilla_metric_tensor through
vqvae_amd.geo.pullback_metric_device):

    wide28    60 000 x 128 latents, 28 px, 1 channel  (784 outputs; dec_channels 256-128-64, eval-mode BatchNorm)
    wide32    50 000 x 128 latents, 32 px, 3 channels (3 072 outputs)
    d16       60 000 x 16 latents, 28 px, 1 channel
    autograd  the generic route (torch.func.jacfwd, float32; Gram and eigvalsh in fp64) on the first 1 024 latents of each shape,
              alternating with the native route on the same 1 024

Times are host clocks around calls that end in a device synchronise, after a warm-up call of every timed shape; every repetition
is reported (min - median - max is the run-to-run spread).  The native time includes the decoder export.  Nothing is extrapolated:
the autograd route is timed at 1 024 latents only.  Writes profiles/vanilla_metric_mi355x.json (or --out).

    python tools/exp_vanilla_metric.py [--reps 5] [--out FILE]
    python tools/exp_vanilla_metric.py --single wide32 --latents 4096      # one shape, two calls: for a kernel trace
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
from vqvae_amd.vae import Decoder  # noqa: E402
from vqvae_amd.vanilla_decoder import VanillaDecoderExport  # noqa: E402

SHAPES = {"wide28": (60000, 128, 1, 28), "wide32": (50000, 128, 3, 32), "d16": (60000, 16, 1, 28)}
CHANNELS = (256, 128, 64)
N_AUTOGRAD = 1024


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_decoder(d, cout, px, dev):
    torch.manual_seed(0)
    dec = Decoder(cout, CHANNELS, d, px, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return dec.to(dev).eval()


def spread(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "vanilla_metric_mi355x.json"))
    cli.add_argument("--single", default=None, choices=list(SHAPES), help="two native calls of one shape and nothing else")
    cli.add_argument("--latents", type=int, default=4096, help="latents of --single")
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    if args.single:
        n, d, cout, px = SHAPES[args.single]
        dec = make_decoder(d, cout, px, dev)
        z = torch.from_numpy(np.random.RandomState(1).randn(args.latents, d).astype(np.float32)).to(dev)
        for _ in range(2):
            t, got = timed(lambda: rm.pullback_metric_device(dec, z))
            print(f"{args.single}: {args.latents} latents, route {got.route}, {t:.4f} s")
        return
    result = {"device": torch.cuda.get_device_name(0), "dec_channels": CHANNELS, "norm": "batch (eval)", "reps": args.reps,
              "shapes": {}}
    for name, (n, d, cout, px) in SHAPES.items():
        dec = make_decoder(d, cout, px, dev)
        assert rm.native_vanilla_metric_covers(dec)
        z = torch.from_numpy(np.random.RandomState(1).randn(n, d).astype(np.float32)).to(dev)
        z_small = z[:N_AUTOGRAD].contiguous()

        def native():
            return rm.pullback_metric_device(dec, z)

        def native_no_spectrum():
            return rm.pullback_metric_device(dec, z, spectrum=False)

        def native_small():
            return rm.pullback_metric_device(dec, z_small)

        def autograd():
            return rm.PullbackMetric(*rm._generic_metric(dec, z_small, True)[:4], route="autograd")

        def spectrum_only(G):
            return rm.sym_spectrum_device(G, cout * px * px)

        got = native()                                                     # warm-up of every timed shape
        native_no_spectrum(), native_small(), autograd(), spectrum_only(got.G)
        t_nat, t_bare, t_spec, t_small, t_auto = [], [], [], [], []
        for _ in range(args.reps):                                         # the two routes alternating
            t, got_small = timed(native_small)
            t_small.append(t)
            t, ref = timed(autograd)
            t_auto.append(t)
            t, got = timed(native)
            t_nat.append(t)
            t_spec.append(timed(lambda: spectrum_only(got.G))[0])
            t_bare.append(timed(native_no_spectrum)[0])
        assert got.route == "native" and got_small.route == "native"
        diag = torch.sqrt(torch.diagonal(ref.G, dim1=1, dim2=2))
        err = ((got_small.G - ref.G).abs() / (diag[:, :, None] * diag[:, None, :])).max()
        ws = lib.geo_vanilla_metric_workspace_bytes(VanillaDecoderExport(dec, dev).desc, n)
        nout = cout * px * px
        result["shapes"][name] = {
            "latents": n, "latent_dim": d, "out_channels": cout, "px": px, "outputs": nout, "workspace_bytes": int(ws),
            "native_s_per_call": spread(t_nat), "native_no_spectrum_s_per_call": spread(t_bare),
            "sym_spectrum_s_per_call": spread(t_spec), "native_latents_per_s_best": n / min(t_nat),
            "native_1024_s_per_call": spread(t_small), "autograd_1024_s_per_call": spread(t_auto),
            "autograd_over_native_1024_median": float(np.median(t_auto) / np.median(t_small)),
            "faster_by_more_than_the_combined_spread": bool(min(t_auto) - max(t_small) > 0),
            "fp64_fma_per_latent_gram": d * (d + 1) // 2 * nout, "fp64_fma_per_latent_jacobi_sweep": 2 * d ** 3,
            "rank_deficient": int((got.rank < d).sum()), "logvol_finite": int(torch.isfinite(got.logvol).sum()),
            "max_eig_ratio": float((got.eig[:, -1] / got.eig[:, 0].clamp_min(1e-300)).max()),
            "native_against_autograd_1024_max_normalised_G_difference": float(err)}
        print(name, json.dumps(result["shapes"][name]), flush=True)
        del got, ref, got_small, z
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

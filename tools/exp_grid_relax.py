"""Relaxation of image curves under the whole spatial decoder on one MI355X: the native route
(geo_spatial_curve_relax through vqvae_amd.geo.grid_relaxation) next to the torch route of the same module
(grid_relaxation._torch_relax: the float32 module and torch.autograd.grad over the whole batch) on the same GPU.

    shapes   64 and 1 024 curves x 9 frames of 4x4 grids x `--iters` iterations (default 20), the step left to the call, under
             the (256, 128, 64) eval-BatchNorm decoders at 28 px x 1, d = 16 and at 32 px x 3, d = 32
    native   seconds per relax_grid_curves_device call (decoder export, the probe for the first step and the `--iters` trials
             included), and per geo_spatial_vjp call over the same frames
    torch    seconds per _torch_relax call.  The two routes alternate within a repetition

Times are host clocks around calls that end in a device synchronise, after one warm-up call of every timed shape on both routes;
every repetition is listed with min - median - max.  No number is a target, nothing is extrapolated, and no share of a peak is
claimed.  Writes profiles/grid_relax_mi355x.json (or --out).

    python tools/exp_grid_relax.py [--reps 5] [--iters 20] [--out FILE]
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
from vqvae_amd.geo import grid_relaxation as gr  # noqa: E402
from vqvae_amd.spatial_decoder import SpatialDecoder, SpatialImageDecoderExport  # noqa: E402

SHAPES = {"wide-bn-28-d16": (1, 28, 16), "wide-bn-32x3-d32": (3, 32, 32)}
CHANNELS, F = (256, 128, 64), 9
CURVES = (64, 1024)


def make_decoder(cout, px, d, dev):
    """SpatialDecoder with seeded weights and non-trivial BatchNorm statistics, in eval mode."""
    torch.manual_seed(0)
    dec = SpatialDecoder(cout, CHANNELS, d, px, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return dec.to(dev).eval()


def curves(C, d, dev):
    """Zig-zags of amplitude 4 about random chords over the 16 d coordinates, drawn in one go."""
    rs = np.random.RandomState(1)
    a, b, zig = rs.randn(C, 1, 16 * d), rs.randn(C, 1, 16 * d), rs.randn(C, 1, 16 * d)
    zig /= np.linalg.norm(zig, axis=2, keepdims=True)
    t = (np.arange(F) / (F - 1))[None, :, None]
    sign = np.where(np.arange(F) % 2 == 1, 4.0, -4.0)[None, :, None]
    sign[:, 0], sign[:, -1] = 0.0, 0.0
    return torch.from_numpy((a + t * (b - a) + sign * zig).astype(np.float32)).view(C, F, d, 4, 4).to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(ts):
    return {"reps": ts, "min": min(ts), "median": float(np.median(ts)), "max": max(ts)}


def ratio_fields(energy, energy0):
    r = (energy / energy0).cpu().numpy()
    return {"min": float(r.min()), "median": float(np.median(r)), "max": float(r.max())}


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--iters", type=int, default=20)
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_relax_mi355x.json"))
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "dec_channels": CHANNELS, "norm": "batch (eval)", "frames": F,
              "iters": args.iters, "reps": args.reps, "decoders": {}}
    for name, (cout, px, d) in SHAPES.items():
        dec = make_decoder(cout, px, d, dev)
        assert gr.native_grid_relax_covers(dec)
        ex = SpatialImageDecoderExport(dec, dev)
        shapes = {}
        for C in CURVES:
            x = curves(C, d, dev)
            u = torch.randn(C * F, ex.n_out, device=dev, generator=torch.Generator(dev).manual_seed(2))

            def native():
                return gr.relax_grid_curves_device(dec, x, args.iters)

            def vjp():
                return gr.spatial_grid_vjp_device(ex, x.view(C * F, d, 4, 4), u)

            def torch_route():
                return gr._torch_relax(dec, x, args.iters, torch.full((C,), -1.0, dtype=torch.float64, device=dev))

            native(), vjp(), torch_route()                        # one warm-up per shape
            t_native, t_vjp, t_torch = [], [], []
            for _ in range(args.reps):                            # alternating
                t, got = timed(native)
                t_native.append(t)
                t_vjp.append(timed(vjp)[0])
                t, ref = timed(torch_route)
                t_torch.append(t)
            assert got.route == "native" and bool((got.energy <= got.energy0).all())
            entry = {"curves": C, "frames_total": C * F,
                     "workspace_bytes": int(lib.geo_spatial_curve_workspace_bytes(ex.desc, C, F)),
                     "native_relax_s_per_call": spread(t_native), "native_vjp_s_per_call": spread(t_vjp),
                     "torch_relax_s_per_call": spread(t_torch),
                     "native_energy_ratio": ratio_fields(got.energy, got.energy0),
                     "native_accepted_mean": float(got.accepted.double().mean()),
                     "torch_energy_ratio": ratio_fields(ref[2], ref[1]), "torch_accepted_mean": float(ref[5].double().mean()),
                     "torch_median_over_native_median": float(np.median(t_torch) / np.median(t_native)),
                     "native_slower_than_torch": bool(np.median(t_native) > np.median(t_torch))}
            shapes[str(C)] = entry
            print(name, C, json.dumps(entry), flush=True)
        result["decoders"][name] = {"out_channels": cout, "px": px, "latent_dim": d, "outputs": ex.n_out, "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
